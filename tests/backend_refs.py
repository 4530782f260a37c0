"""Case builders and plain references for the kernels that turn numbers into what a user reads: stage C (postproc.hip:
4-decimal rounding, score fusion, dict collapse, stable sort, greedy NMS, matcher cost), compose_rows (window_ops.hip), the
criterion (criterion.hip: exact assignment by subset DP, the losses, the adapter NCE) and the device metrics (metrics.hip).
Nothing here touches the library; tests/test_backend_kernels_cpu.py validates these helpers -- and shows which planted error
each case family catches -- before tests/test_backend_kernels_gpu.py relies on them.

    STAGE_C_FAMILIES / stage_c_case     named candidate lists, (n, seed) -> (cand fp32 (n, 4), note)
    stage_c_expected                    the oracle's kept rows per score type + first-occurrence index + the fill
    stage_c_model / temporal_nms_model  a pure-python model of fuse_nms_kernel's ALGORITHM (chunked first / last search, ballot +
                                        prefix compaction, counting rank, greedy loop) with a switch per planted error
    cost_matrix64 / giou64 / ce64 / assign_optimum64 / all_assignment_costs64 / losses64 / adapter_nce64
                                        the criterion in float64
    criterion_dp_model                  fp32 model of criterion_window_kernel's subset DP with a switch per planted error
    crit_case / saliency_case           criterion case families
    assign_bound / nce_bound            the bounds, derived below from the number formats
    matcher_case / compose_case / metric builders
"""
from __future__ import annotations

import functools
import math
from itertools import permutations
from types import SimpleNamespace

import numpy as np
import torch

from oracle import cone_oracle as O

U32 = 2.0 ** -24             # unit roundoff of fp32
K_MAX_CAND = 1024            # postproc.hip: kMaxCand
CHUNK = 256                  # fuse_nms_kernel walks the list in workgroup-wide chunks
WAVE = 64

# ---- stage C --------------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024)      # the smallest at which each chunk / wave edge exists
PARAMS = ((-1, 200, 5), (-1, 2000, 1024), (0.0, 200, 5), (0.3, 200, 1024), (0.5, 100, 100), (0.999, 2000, 1024),
          (1.0, 10, 10), (0.7, 300, 1))                                     # (nms_thd, max_before_nms, max_after_nms)
TYPE_COL = (2, 0, 1)         # output order fused / proposal / matching -> index into the dict's value list


def _base(n, rng):
    st = rng.uniform(0, 500, n)
    ed = st + rng.uniform(0, 60, n)
    return st, ed, rng.uniform(0, 1, n), rng.uniform(-0.2, 0.6, n)


def _pack(st, ed, pr, ma):
    return np.stack([st, ed, pr, ma], 1).astype(np.float32)


def fam_random(n, seed):
    rng = np.random.default_rng(1000 + seed)
    st, ed, pr, ma = _base(n, rng)
    if seed % 5 == 0 and n > 4:
        k = n // 3
        st[-k:], ed[-k:] = st[:k], ed[:k]
    if seed % 7 == 0:
        pr[:] = 0.25
    if seed % 11 == 0:
        ma[:] = ma[0]
    if seed % 3 == 0 and n > 2:
        pr[1] = pr[0]
    return _pack(st, ed, pr, ma), "as the property test of test_gpu_parity"


def fam_dups_across_chunks(n, seed):
    rng = np.random.default_rng(2000 + seed)
    st, ed, pr, ma = _base(n, rng)
    k = n // 4
    if k:                                   # n = 1024: keys of i < 256 come back, with other scores, at i >= 768
        st[n - k:], ed[n - k:] = st[:k], ed[:k]
        for i in range(k, n - k - 3, 8):    # interleaved: A B A B
            st[i + 2], ed[i + 2] = st[i], ed[i]
            st[i + 3], ed[i + 3] = st[i + 1], ed[i + 1]
    elif n >= 2:
        st[n - 1], ed[n - 1] = st[0], ed[0]
    return _pack(st, ed, pr, ma), "a key's first and last occurrence lie in different chunks; interleaved duplicates"


def fam_all_same_key(n, seed):
    rng = np.random.default_rng(3000 + seed)
    _, _, pr, ma = _base(n, rng)
    return _pack(np.full(n, 12.5), np.full(n, 20.25), pr, ma), "nu = 1: block_nms returns at m == 1"


def fam_two_keys(n, seed):
    rng = np.random.default_rng(4000 + seed)
    _, _, pr, ma = _base(n, rng)
    w = rng.integers(0, 2, n)
    if n >= 2:
        w[0], w[-1] = 0, 1
    return _pack(np.where(w, 40.0, 12.5), np.where(w, 47.75, 20.25), pr, ma), "nu = 2"


def fam_all_ties(n, seed):
    rng = np.random.default_rng(5000 + seed)
    st, ed, _, _ = _base(n, rng)
    return _pack(st, ed, np.full(n, 0.5), np.full(n, 0.25)), "every score equal: the order is candidate order"


def fam_ties_across_chunks(n, seed):
    rng = np.random.default_rng(6000 + seed)
    st, ed, _, _ = _base(n, rng)
    period = CHUNK if n > CHUNK else max(1, min(32, n // 2))
    i = np.arange(n) % period
    return _pack(st, ed, rng.uniform(0, 1, period)[i], rng.uniform(-0.2, 0.6, period)[i]), "equal scores at i and i + 256 k"


def fam_const_prop(n, seed):
    rng = np.random.default_rng(7000 + seed)
    st, ed, pr, ma = _base(n, rng)
    return _pack(st, ed, np.full(n, 0.3125), ma), "proposal scores constant: min == max"


def fam_const_match(n, seed):
    rng = np.random.default_rng(8000 + seed)
    st, ed, pr, ma = _base(n, rng)
    return _pack(st, ed, pr, np.full(n, -0.125)), "matching scores constant: min == max"


def fam_chain(n, seed):
    rng = np.random.default_rng(9000 + seed)
    _, _, pr, ma = _base(n, rng)
    i = np.arange(n, dtype=np.float64)
    return _pack(i, i + 1.5, pr, ma), "IoU 0.2 with the neighbours, 0 with the rest: a long serial loop"


def fam_nested(n, seed):
    rng = np.random.default_rng(10000 + seed)
    _, _, pr, ma = _base(n, rng)
    st = 0.01 * np.arange(n)
    return _pack(st, 2000.0 - st, pr, ma), "nested spans: the first suppresses all"


def fam_touching(n, seed):
    rng = np.random.default_rng(11000 + seed)
    _, _, pr, ma = _base(n, rng)
    st = 2.0 * np.arange(n)
    return _pack(st, st + 2.0, pr, ma), "ed_i == st_{i+1}: inter = 0, IoU 0 is not > 0"


def fam_zero_length(n, seed):
    rng = np.random.default_rng(12000 + seed)
    _, _, pr, ma = _base(n, rng)
    st = 1.25 * (np.arange(n) // 2)
    return _pack(st, st, pr, ma), "st == ed, every key twice: uni == 0 between equal keys"


def fam_round_ties(n, seed):
    rng = np.random.default_rng(13000 + seed)
    odd = lambda lo, hi, size: (2 * rng.integers(lo, hi, size) + 1) / 32.0        # x * 1e4 is an exact half
    st = odd(0, 16 * 500, n)
    ed = st + rng.integers(0, 32 * 60, n) / 16.0                                   # ed stays an odd multiple of 2^-5
    big = np.arange(n) % 4 == 1                                                    # 4096 .. 11000 s: the fp32 ulp nears 1e-3
    st = np.where(big, odd(16 * 4096, 16 * 10000, n), st)
    ed = np.where(big, st + rng.integers(0, 32 * 30, n) / 16.0, ed)
    neg = np.arange(n) % 4 == 3
    st = np.where(neg, -odd(0, 64, n), st)
    ed = np.where(neg, st + rng.integers(0, 64, n) / 16.0, ed)
    pr = odd(0, 16, n)
    ma = np.where(rng.integers(0, 2, n) == 1, -1.0, 1.0) * odd(0, 16, n)
    tiny = np.arange(n) % 8 == 6                                                   # "-0.0000"
    st = np.where(tiny, -2.0 ** -15, st)
    ed = np.where(tiny, 2.0 ** -15 * (1 + np.arange(n)), ed)
    ma = np.where(np.arange(n) % 8 == 2, -1e-6, ma)
    return _pack(st, ed, pr, ma), "odd multiples of 2^-5: round-half-even; large magnitudes, negatives, -0.0"


STAGE_C_FAMILIES = dict(random=fam_random, dups_across_chunks=fam_dups_across_chunks, all_same_key=fam_all_same_key,
                        two_keys=fam_two_keys, all_ties=fam_all_ties, ties_across_chunks=fam_ties_across_chunks,
                        const_prop=fam_const_prop, const_match=fam_const_match, chain=fam_chain, nested=fam_nested,
                        touching=fam_touching, zero_length=fam_zero_length, round_ties=fam_round_ties)
EVERY_SIZE = ("random", "dups_across_chunks")                   # these run at every size under every parameter set
# the other families: {257, 1024} plus one size <= 64, under the parameter sets at which they bite (indices into PARAMS)
OTHER_SIZES = dict(all_same_key=(2, 257, 1024), two_keys=(63, 257, 1024), all_ties=(64, 257, 1024),
                   ties_across_chunks=(64, 257, 1024), const_prop=(63, 257, 1024), const_match=(2, 257, 1024),
                   chain=(64, 257, 1024), nested=(63, 257, 1024), touching=(64, 257, 1024), zero_length=(64, 257, 1024),
                   round_ties=(63, 257, 1024))
OTHER_PARAMS = dict(all_same_key=(0, 4), two_keys=(2, 6), all_ties=(1, 4, 7), ties_across_chunks=(1, 3, 5),
                    const_prop=(0, 3, 7), const_match=(1, 3, 6), chain=(2, 3, 4, 5), nested=(3, 5, 7), touching=(1, 2, 3),
                    zero_length=(0, 2, 4), round_ties=(1, 4, 6))


def other_family_queries(p):
    """The (family, n) lists that run under parameter set PARAMS[p] beside the every-size families: 9 to 18 per launch."""
    return [(f, n) for f in OTHER_SIZES if p in OTHER_PARAMS[f] for n in OTHER_SIZES[f]]


def case_seed(family, n, seed=None):
    """The default seed of a named case: ``random`` changes its quirks (duplicates, constant lists, ties) with the seed, so it
    takes another one at every size -- at seed 0 the last third of the list are duplicates and a lone candidate in the last
    chunk (n = 257, 513) would never be a unique key."""
    return seed if seed is not None else (n if family == "random" else 0)


def stage_c_case(family: str, n: int, seed=None):
    return _stage_c_case(family, n, case_seed(family, n, seed))


@functools.lru_cache(maxsize=None)
def _stage_c_case(family, n, seed):
    cand, note = STAGE_C_FAMILIES[family](n, seed)
    assert cand.shape == (n, 4) and cand.dtype == np.float32 and np.isfinite(cand).all()
    cand.setflags(write=False)
    return cand, note


@functools.lru_cache(maxsize=None)
def _fused_dict(family, n, seed):
    """The oracle's rounded rows -> fusion dict of a named case, and each key's first candidate index."""
    return _fuse(O.round4_rows(_stage_c_case(family, n, seed)[0].tolist()))


def _fuse(rows):
    first = {}
    for i, r in enumerate(rows):
        first.setdefault((r[0], r[1]), i)
    return O.score_fusion(rows), first


def _expected_from(rd, first, thd, mb, ma):
    opt = SimpleNamespace(nms_thd=thd, max_before_nms=mb, max_after_nms=ma)
    out = []
    for col in TYPE_COL:
        kept = O.post_processing_mr_nms(opt, rd, col)
        rows = np.zeros((ma, 5), np.float64)
        idx = np.full(ma, -1, np.int32)
        if kept:
            rows[:len(kept)] = np.asarray(kept, np.float64)
            idx[:len(kept)] = [first[(m[0], m[1])] for m in kept]
        out.append((rows, idx, len(kept)))
    return out


def stage_c_expected(cand_q, thd, mb, ma):
    """[(rows (ma, 5) fp64, idx (ma,) int32, n_kept)] for fused / proposal / matching: O.round4_rows -> O.score_fusion ->
    O.post_processing_mr_nms on the candidate list ``cand_q`` (n, 4), plus what the kernel returns beside the rows: idx[j] =
    candidate index of the FIRST occurrence of kept row j's key, and past the kept rows 0.0 / -1 up to max_after.  An empty
    list (the reference never builds one: min() of nothing raises) is three empty results."""
    cand_q = np.asarray(cand_q)
    if len(cand_q) == 0:
        return [(np.zeros((ma, 5)), np.full(ma, -1, np.int32), 0) for _ in TYPE_COL]
    rd, first = _fuse(O.round4_rows(cand_q.tolist()))
    return _expected_from(rd, first, thd, mb, ma)


def stage_c_expected_named(family, n, seed, thd, mb, ma):
    """stage_c_expected of a named case; the rounding and the fusion are shared between the parameter sets."""
    rd, first = _fused_dict(family, n, case_seed(family, n, seed))
    return _expected_from(rd, first, thd, mb, ma)


def bits(a):
    """float64 array -> its bit patterns (so that -0.0 and 0.0 differ in a comparison)."""
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def same_result(a, b):
    """Two per-type result lists agree in count, kept rows (bit for bit), idx and fill."""
    return all(x[2] == y[2] and np.array_equal(bits(x[0]), bits(y[0])) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


# ---- the kernel's algorithm in python, with planted errors -------------------------------------------------------------------
STAGE_C_MUTATIONS = ("first_value_wins", "last_position", "no_chunk_carry", "no_wave_prefix", "rank_tie_le", "rank_tie_absent",
                     "ge_thd", "max_before_ignored", "round_half_away", "uni_unguarded")


def _round4(x, mut):
    y = float(x) * 1e4                          # exact in fp64 for an fp32 x
    if "round_half_away" in mut:
        r = math.copysign(math.floor(abs(y) + 0.5), y)
    else:
        r = float(np.rint(y))
    return r / 1e4


def _piou(s0, e0, s1, e1, mut):
    lo = min(e0, e1) - max(s0, s1)
    inter = lo if lo > 0.0 else 0.0
    uni = max(e0, e1) - min(s0, s1)
    if uni == 0.0:
        return float("nan") if "uni_unguarded" in mut else 0.0      # 0 / 0 in the kernel's arithmetic
    return inter / uni


def _block_nms(st, ed, sidx, m, thd, ma, mut):
    if m == 1:
        return [0]
    alive = [True] * m
    kept = []
    start = 0
    while True:
        c = start
        while c < m and not alive[c]:
            c += 1
        if not (c < m and len(kept) < ma):
            break
        kept.append(c)
        s0, e0 = st[sidx[c]], ed[sidx[c]]
        for j in range(c + 1, m):
            if alive[j]:
                v = _piou(s0, e0, st[sidx[j]], ed[sidx[j]], mut)
                if (v >= thd) if "ge_thd" in mut else (v > thd):
                    alive[j] = False
        start = c + 1
    return kept


def _rank(vals, mut):
    """Counting rank of fuse_nms_kernel's step 4; slots that no entry claims keep 0 (whatever the LDS held)."""
    nu = len(vals)
    sidx = [0] * max(nu, 1)
    for u in range(nu):
        v = vals[u]
        if "rank_tie_le" in mut:
            r = sum(1 for w in range(nu) if vals[w] > v or (vals[w] == v and w <= u))
        elif "rank_tie_absent" in mut:
            r = sum(1 for w in range(nu) if vals[w] > v)
        else:
            r = sum(1 for w in range(nu) if vals[w] > v or (vals[w] == v and w < u))
        if r < len(sidx):
            sidx[r] = u
    return sidx


def stage_c_model(cand_q, thd, mb, ma, mut=()):
    """fuse_nms_kernel step by step (one workgroup of 256 threads = 4 waves of 64) on one candidate list; ``mut`` names the
    planted errors (STAGE_C_MUTATIONS).  Same return value as stage_c_expected."""
    mut = frozenset(mut)
    assert mut <= set(STAGE_C_MUTATIONS)
    cand_q = np.asarray(cand_q)                       # fp32 rows, or fp64 rows that are rounded already (cone_fuse_nms_f64)
    n = min(len(cand_q), K_MAX_CAND)
    st = [_round4(cand_q[i, 0], mut) for i in range(n)]
    ed = [_round4(cand_q[i, 1], mut) for i in range(n)]
    val = [[_round4(cand_q[i, c], mut) for i in range(n)] for c in (2, 3)]
    norm = []
    for v in val:
        mn, mx = (min(v), max(v)) if n else (0.0, 0.0)
        norm.append(list(v) if mn == mx else [(x - mn) / (mx - mn) for x in v])
    val.append([(0.0 + a) + b for a, b in zip(*norm)])
    # step 3: first / last occurrence per candidate, then ballot + prefix compaction chunk by chunk
    keys = list(zip(st, ed))
    where = {}
    for i, k in enumerate(keys):
        where.setdefault(k, []).append(i)
    n_chunks = (n + CHUNK - 1) // CHUNK
    flag = [False] * (n_chunks * CHUNK)
    parked = [0] * (n_chunks * CHUNK)
    s_cnt = [[0] * max(n_chunks, 1) for _ in range(4)]
    for i in range(n):
        occ = where[keys[i]]
        flag[i] = (i == occ[-1]) if "last_position" in mut else (i == occ[0])
        parked[i] = i if ("first_value_wins" in mut or "last_position" in mut) else occ[-1]
        if "first_value_wins" in mut and "last_position" not in mut:
            parked[i] = occ[0]
        if flag[i]:
            s_cnt[(i % CHUNK) // WAVE][i // CHUNK] += 1
    u_first = [0] * K_MAX_CAND
    u_last = [0] * K_MAX_CAND
    nu_acc = 0
    for c in range(n_chunks):
        for wave in range(4):
            base = 0 if "no_chunk_carry" in mut else nu_acc
            if "no_wave_prefix" not in mut:
                base += sum(s_cnt[w][c] for w in range(wave))
            before = 0
            for lane in range(WAVE):
                i = c * CHUNK + wave * WAVE + lane
                if i < n and flag[i]:
                    u_first[base + before] = i
                    u_last[base + before] = parked[i]
                    before += 1
        nu_acc += sum(s_cnt[w][c] for w in range(4))
    nu = nu_acc
    out = []
    for col in TYPE_COL:
        uval = [val[col][u_last[u]] for u in range(nu)]
        sidx = _rank(uval, mut)
        if thd != -1.0:
            m = nu if "max_before_ignored" in mut else min(nu, mb)
            cidx = [u_first[sidx[j]] for j in range(m)]
            kept_pos = _block_nms(st, ed, cidx, m, thd, ma, mut) if m else []
        else:
            kept_pos = list(range(min(nu, ma)))
        rows = np.zeros((ma, 5), np.float64)
        idx = np.full(ma, -1, np.int32)
        for j, p in enumerate(kept_pos):
            u = sidx[p]
            kf, kl = u_first[u], u_last[u]
            rows[j] = (st[kf], ed[kf], val[0][kl], val[1][kl], val[2][kl])
            idx[j] = kf
        out.append((rows, idx, len(kept_pos)))
    return out


def temporal_nms_model(pred, thd, ma, mut=()):
    """temporal_nms_kernel on a list of [st, ed, score] -> kept candidate indices."""
    mut = frozenset(mut)
    n = len(pred)
    if n == 1:
        return [0]
    sidx = _rank([p[2] for p in pred], mut)
    kept = _block_nms([p[0] for p in pred], [p[1] for p in pred], sidx, n, thd, ma, mut)
    return [sidx[p] for p in kept]


def nms_list(family, n, seed=None):
    """[st, ed, score] python doubles of a stage C family for ops.temporal_nms / O.temporal_nms (score: the proposal column);
    duplicate spans stay in -- there is no dict in front of this entry."""
    c = stage_c_case(family, n, seed)[0].astype(np.float64)
    return [[float(r[0]), float(r[1]), float(r[2])] for r in c]


# ---- criterion in float64 ---------------------------------------------------------------------------------------------------
HYPER = dict(set_cost_span=10, set_cost_giou=1, set_cost_class=4, eos_coef=0.1, saliency_margin=0.2, temperature=0.07)
LOSS_RTOL = 1e-5             # the project's figure: |got - ref| <= 1e-5 max(1, |ref|)


def _np64(t):
    return np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, np.float64)


def giou64(src, tgt):
    """(n, 2) x (m, 2) (center, width) -> (n, m) generalized temporal IoU (cone/span_utils.py)."""
    src, tgt = _np64(src).reshape(-1, 2), _np64(tgt).reshape(-1, 2)
    x1, x2 = (src[:, 0] - 0.5 * src[:, 1])[:, None], (src[:, 0] + 0.5 * src[:, 1])[:, None]
    t1, t2 = (tgt[:, 0] - 0.5 * tgt[:, 1])[None], (tgt[:, 0] + 0.5 * tgt[:, 1])[None]
    inter = np.maximum(np.minimum(x2, t2) - np.maximum(x1, t1), 0.0)
    uni = (x2 - x1) + (t2 - t1) - inter
    enc = np.maximum(np.maximum(x2, t2) - np.minimum(x1, t1), 0.0)
    with np.errstate(all="ignore"):
        return inter / uni - (enc - uni) / enc


def prob_fg64(logits):
    lg = _np64(logits)
    m = lg.max(-1, keepdims=True)
    e = np.exp(lg - m)
    return e[..., 0] / e.sum(-1)


def cost_matrix64(logits, spans, tgt, hyper=HYPER):
    """One window: logits (Nq, 2), spans (Nq, 2), tgt (T, 2) -> (Nq, T) matcher cost (cone/matcher.py:61-95)."""
    sp, tg = _np64(spans), _np64(tgt).reshape(-1, 2)
    l1 = np.abs(sp[:, None, 0] - tg[None, :, 0]) + np.abs(sp[:, None, 1] - tg[None, :, 1])
    return (hyper["set_cost_span"] * l1 - hyper["set_cost_giou"] * giou64(sp, tg)
            - hyper["set_cost_class"] * prob_fg64(logits)[:, None])


def ce64(logits, y, eos, w_fg=1.0):
    """-w[y] log_softmax(logits)[y] per slot; y = 0 foreground (weight w_fg = 1), 1 background (weight eos)."""
    lg = _np64(logits)
    m = lg.max(-1, keepdims=True)
    lsm = (lg - m) - np.log(np.exp(lg - m).sum(-1, keepdims=True))
    y = np.asarray(y)
    return -np.where(y == 0, w_fg, eos) * np.take_along_axis(lsm, y[..., None], -1)[..., 0]


def assign_optimum64(C):
    """scipy.optimize.linear_sum_assignment on the float64 cost -> (assign (Nq,) int: target of each slot or -1, cost)."""
    from scipy.optimize import linear_sum_assignment
    C = np.asarray(C, np.float64)
    a = np.full(C.shape[0], -1, np.int64)
    if C.shape[1] == 0:
        return a, 0.0
    r, c = linear_sum_assignment(C)
    a[r] = c
    return a, float(C[r, c].sum())


@functools.lru_cache(maxsize=None)
def _injections(ns, nl):
    return np.asarray(list(permutations(range(nl), ns)), np.int64).reshape(-1, ns)


def all_assignment_costs64(C):
    """Every assignment of min(Nq, T) pairs -> (costs, assigns (n_assign, Nq) with -1 for unmatched slots)."""
    C = np.asarray(C, np.float64)
    Nq, T = C.shape
    if Nq <= T:
        p = _injections(Nq, T)                                       # slot n -> target p[:, n]
        return C[np.arange(Nq)[None], p].sum(1), p
    p = _injections(T, Nq)                                           # target j -> slot p[:, j]
    a = np.full((len(p), Nq), -1, np.int64)
    np.put_along_axis(a, p, np.arange(T)[None].repeat(len(p), 0), 1)
    return C[p, np.arange(T)[None]].sum(1), a


def assignment_cost64(C, assign):
    C = np.asarray(C, np.float64)
    return float(sum(C[n, j] for n, j in enumerate(assign) if j >= 0))


def assign_bound(C, Nq):
    """How far the float64 cost of the kernel's assignment may lie above the float64 optimum: Nq 2^-21 max|C|.

    With u = 2^-24: the kernel builds an entry of C from about a dozen correctly rounded fp32 operations and two expf, a few
    ulp -- |dC| <= 4 u max|C| with room to spare.  A DP path adds at most min(Nq, T) <= 8 entries, one rounding each on a
    partial sum of at most Nq max|C|: a further <= 4 u max|C| per pair for Nq <= 8 once the entry errors are spread over the
    pairs (eight fp32 additions of entries each carrying a few ulp).  So the fp32 cost of ANY assignment is within
    e = Nq 8 u max|C| / 2 = Nq 2^-22 max|C| of its float64 cost.  The kernel returns the fp32 optimum A; with A* the float64
    optimum, cost64(A) <= cost32(A) + e <= cost32(A*) + e <= cost64(A*) + 2 e = cost64(A*) + Nq 2^-21 max|C|.
    test_backend_kernels_cpu shows the fp32 DP inside it on every family."""
    return Nq * 2.0 ** -21 * float(np.abs(C).max()) if np.size(C) else 0.0


def losses64(hyper, logits, spans, tgt_list, assign, neg_logits=None, saliency=None, pos_idx=None, neg_idx=None,
             neg_saliency=None, planted=()):
    """O.criterion_layer (cone/model.py:266-363) in float64 at a GIVEN assignment (B, Nq): -1 or the slot's target.
    ``planted``: "bg_weight_on_matched" / "tie_strict" of CRIT_MUTATIONS (the CPU suite's power check)."""
    lg, sp = _np64(logits), _np64(spans)
    B, Nq = lg.shape[:2]
    assign = np.asarray(assign).reshape(B, Nq)
    l1 = gi = 0.0
    nm = correct = 0
    for b in range(B):
        tg = _np64(tgt_list[b]).reshape(-1, 2)
        for n in range(Nq):
            j = int(assign[b, n])
            if j < 0:
                continue
            l1 += abs(sp[b, n, 0] - tg[j, 0]) + abs(sp[b, n, 1] - tg[j, 1])
            gi += 1.0 - float(giou64(sp[b, n], tg[j])[0, 0])
            nm += 1
            # argmax keeps the lower index on a tie
            correct += (lg[b, n, 0] > lg[b, n, 1]) if "tie_strict" in planted else (lg[b, n, 0] >= lg[b, n, 1])
    y = (assign < 0).astype(np.int64)
    ce = ce64(lg, y, hyper["eos_coef"], hyper["eos_coef"] if "bg_weight_on_matched" in planted else 1.0).sum()
    slots = B * Nq
    if neg_logits is not None:
        ng = _np64(neg_logits)
        ce += ce64(ng, np.ones(ng.shape[:2], np.int64), hyper["eos_coef"]).sum()
        slots *= 2
    nan = float("nan")
    out = dict(loss_span=l1 / (2 * nm) if nm else nan, loss_giou=gi / nm if nm else nan, loss_label=ce / slots,
               class_error=100.0 - 100.0 * correct / nm if nm else nan)
    if saliency is not None:
        s = _np64(saliency)
        pi, ni = np.asarray(pos_idx), np.asarray(neg_idx)            # python indexing wraps the negative labels
        P = pi.shape[1]
        ar = np.arange(B)[:, None]
        pos, neg = s[ar, pi], s[ar, ni]
        ls = np.maximum(hyper["saliency_margin"] + neg - pos, 0).sum() / (B * P) * 2
        if neg_saliency is not None:
            nmx = _np64(neg_saliency).max(1)[:, None]
            ls += np.maximum(hyper["saliency_margin"] + nmx - pos, 0).sum() / (B * P) * 2
        out["loss_saliency"] = ls
    return out


def within(got, ref, rtol=LOSS_RTOL):
    """(ok, err / tolerance) under |got - ref| <= rtol max(1, |ref|); two NaNs agree."""
    got, ref = float(got), float(ref)
    if math.isnan(ref) or math.isnan(got):
        return math.isnan(ref) and math.isnan(got), 0.0
    r = abs(got - ref) / (rtol * max(1.0, abs(ref)))
    return r <= 1.0, r


CRIT_MUTATIONS = ("dp_walks_larger_side", "from_not_reset", "k_gt_ns_not_skipped", "bg_weight_on_matched", "tie_strict")


def criterion_dp_model(hyper, logits, spans, tgt_list, mut=()):
    """criterion_window_kernel's assignment: fp32 costs (torch, as the reference builds them) and the kernel's subset DP with
    fp32 partial sums; ``mut`` plants the DP errors of CRIT_MUTATIONS.  Local arrays are NOT cleared between windows (the
    kernel's are whatever the registers / scratch held).  Returns assign (B, Nq): target of each slot or -1."""
    mut = frozenset(mut)
    assert mut <= set(CRIT_MUTATIONS)
    f32 = np.float32
    costs = (hyper["set_cost_span"], hyper["set_cost_giou"], hyper["set_cost_class"])
    B, Nq = logits.shape[:2]
    assign = np.full((B, Nq), -1, np.int64)
    frm = np.full(256, 7, np.int64)
    C = np.full((8, 8), -1e3, f32)
    for b in range(B):
        T = int(tgt_list[b].shape[0])
        if T == 0:
            continue
        C[:Nq, :T] = O.matcher_cost(costs, logits[b:b + 1], spans[b:b + 1], tgt_list[b]).numpy().astype(f32).reshape(Nq, T)
        rows_small = Nq <= T
        ns, nl = (Nq, T) if rows_small else (T, Nq)
        if "dp_walks_larger_side" in mut and Nq != T:
            rows_small, ns, nl = not rows_small, nl, ns
        full = 1 << nl
        best = np.full(256, np.inf, f32)
        best[0] = 0
        for mask in range(1, full):
            k = bin(mask).count("1")
            if "from_not_reset" not in mut:
                frm[mask] = 0
            if k > ns and "k_gt_ns_not_skipped" not in mut:
                continue
            for j in range(nl):
                if mask >> j & 1:
                    v = f32(best[mask ^ (1 << j)] + (C[k - 1, j] if rows_small else C[j, k - 1]))
                    if v < best[mask]:
                        best[mask], frm[mask] = v, j
        bm, bv = 0, np.inf
        for mask in range(full):
            if bin(mask).count("1") == ns and best[mask] < bv:
                bv, bm = best[mask], mask
        for k in range(ns, 0, -1):
            j = int(frm[bm])
            if rows_small:
                assign[b, (k - 1) % Nq] = j
            else:
                assign[b, j % Nq] = k - 1
            bm ^= 1 << j
    return assign


def is_partial_permutation(row, T):
    """One window's assign row: exactly min(Nq, T) slots matched, to distinct targets in [0, T), the others -1."""
    m = [int(j) for j in row if j != -1]
    return len(m) == min(len(row), T) and len(set(m)) == len(m) and all(0 <= j < T for j in m)


CRIT_FAMILIES = ("random", "square8", "wide", "tall", "single_slot", "empty_mixed", "twin_slots", "twin_targets", "disjoint",
                 "containing", "out_of_unit", "sharp_logits", "offset_logits")
CRIT_BATCHES = (1, 63, 64, 65, 129)          # criterion_window_kernel: 64-thread workgroups, one thread per window


@functools.lru_cache(maxsize=None)
def crit_case(family: str, B: int, seed: int = 0):
    """-> SimpleNamespace(logits (B, Nq, 2), spans (B, Nq, 2), tgt [(T_b, 2)], neg_logits (B, Nq, 2)) fp32 CPU tensors."""
    rng = np.random.default_rng(7919 * CRIT_FAMILIES.index(family) + 31 * B + seed)
    Nq = dict(random=(5, 8, 2)[(B + seed) % 3], square8=8, wide=8, tall=2, single_slot=1, empty_mixed=5, twin_slots=6,
              twin_targets=5, disjoint=5, containing=8, out_of_unit=8, sharp_logits=8, offset_logits=8)[family]
    if family == "square8":
        Ts = np.full(B, 8)
    elif family == "wide":
        Ts = 1 + np.arange(B) % 2
    elif family == "tall":
        Ts = np.full(B, 8)
    elif family == "single_slot":
        Ts = 1 + np.arange(B) % 8
    elif family == "empty_mixed":
        Ts = np.where(np.arange(B) % 3 == 1, 0, rng.integers(1, 9, B))
    elif family == "twin_targets":
        Ts = rng.integers(2, 9, B)
    else:
        Ts = rng.integers(1, 9, B)
    lg = rng.standard_normal((B, Nq, 2))
    sp = np.stack([rng.uniform(.1, .9, (B, Nq)), rng.uniform(.02, .6, (B, Nq))], -1)
    tg = [np.stack([rng.uniform(.1, .9, t), rng.uniform(.02, .6, t)], -1) for t in Ts]
    if family == "twin_slots":               # slots (0, 1) and (2, 3) are twins: tied optima; slot 4: l0 == l1
        lg[:, 1], sp[:, 1] = lg[:, 0], sp[:, 0]
        lg[:, 3], sp[:, 3] = lg[:, 2], sp[:, 2]
        lg[:, 4, 1] = lg[:, 4, 0]
        sp[:, 4] = [t[0] for t in tg]        # ... and it sits on the first target, so it is matched
    elif family == "twin_targets":
        for t in tg:
            t[1] = t[0]
    elif family == "disjoint":               # predictions left, targets right: GIoU < 0
        sp = np.stack([rng.uniform(.05, .3, (B, Nq)), rng.uniform(.02, .1, (B, Nq))], -1)
        tg = [np.stack([rng.uniform(.7, .95, t), rng.uniform(.02, .1, t)], -1) for t in Ts]
    elif family == "containing":             # same centres, one inside the other, alternating
        for b, t in enumerate(tg):
            k = len(t)
            sp[b, :, 0] = np.resize(t[:, 0], Nq)
            sp[b, :, 1] = np.resize(t[:, 1], Nq) * np.where(np.arange(Nq) % 2, 0.25, 1.75) + 0.001 * np.arange(Nq)
    elif family == "out_of_unit":
        sp = np.stack([rng.uniform(-.5, 1.5, (B, Nq)), rng.uniform(.02, 1.5, (B, Nq))], -1)
        tg = [np.stack([rng.uniform(-.5, 1.5, t), rng.uniform(.02, 1.5, t)], -1) for t in Ts]
    elif family == "sharp_logits":           # l0 - l1 = +-60 (an exact 0 in every fourth slot), common offsets 0 / +-1e4
        d = np.where(rng.integers(0, 2, (B, Nq)) == 1, 60.0, -60.0)
        d[:, 3::4] = 0.0
        off = np.asarray([0.0, 1e4, -1e4])[rng.integers(0, 3, (B, Nq))]
        lg = np.stack([off + d / 2, off - d / 2], -1)
    elif family == "offset_logits":          # ordinary differences on common offsets +-1e4: softmax is shift invariant
        off = np.asarray([1e4, -1e4])[rng.integers(0, 2, (B, Nq))]
        lg = np.round(lg * 8) / 8 + off[..., None]
    t32 = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float32)
    neg = rng.standard_normal((B, Nq, 2)) * 3
    return SimpleNamespace(logits=t32(lg), spans=t32(sp), tgt=[t32(t).reshape(-1, 2) for t in tg], neg_logits=t32(neg), Nq=Nq,
                           B=B)


def saliency_case(B, L, P, L2, seed=0):
    rng = np.random.default_rng(500 + 13 * B + 7 * L + P + seed)
    sal = torch.tensor(rng.standard_normal((B, L)), dtype=torch.float32)
    nsal = torch.tensor(rng.standard_normal((B, L2)), dtype=torch.float32)
    pos = torch.tensor(rng.integers(-L, L, (B, P)), dtype=torch.int64)       # negative labels: the host wraps them
    neg = torch.tensor(rng.integers(-L, L, (B, P)), dtype=torch.int64)
    return sal, pos, neg, nsal


# ---- adapter NCE --------------------------------------------------------------------------------------------------------------
NCE_SIZES = (1, 2, 64, 65, 300)
NCE_TEMPS = (0.07, 0.01)


@functools.lru_cache(maxsize=None)
def nce_case(n, seed=0):
    rng = np.random.default_rng(900 + n + seed)
    sim = rng.uniform(-1, 1, (n, n))
    if n > 1:
        sim[:, n // 2] = 1.0                     # one dominant off-diagonal column
        sim[n // 2, n // 2] = 0.25
    return torch.tensor(sim, dtype=torch.float32)


def adapter_nce64(sim, temperature):
    x = _np64(sim) / float(np.float32(temperature))          # the kernel receives the temperature as an fp32
    def ce(x):
        m = x.max(1, keepdims=True)
        return (m[:, 0] + np.log(np.exp(x - m).sum(1)) - np.diag(x)).mean()
    return float((ce(x) + ce(x.T)) / 2)


def nce_bound(sim, temperature, ref):
    """|fp32 - float64| of the adapter NCE, from the inputs (u = 2^-24, x = sim / T, X = max|x|, n columns).  Per row:
      x_j = fl(sim_j / T) is off by u |x_j| and lse is 1-Lipschitz in the sup norm: lse(x) - x_ii moves by <= 2 u X;
      a_j = fl(x_j - m) rounds by u |a_j| <= 2 u X, which is the RELATIVE error it puts on exp(a_j); expf is good to 2 ulp
      (4 u); a sequential fp32 sum of n non-negative terms carries (n - 1) u relative -- so log(sum) is off by
      <= (n - 1) u + 4 u + 2 u X absolute; logf to 2 ulp of |log sum| <= ln n: 4 u ln n;
      fl(m + log sum) rounds by u (X + ln n), fl(.. - x_ii) by u (2 X + ln n).
    Sum: u [(n + 3) + 6 ln n + 7 X]; the rows are averaged in double and the result rounded to fp32 once: + u |ref|."""
    n = sim.shape[0]
    X = float(_np64(sim).__abs__().max()) / temperature
    return U32 * ((n + 3) + 6 * math.log(n) + 7 * X + abs(ref))


def adapter_nce_f32(sim, temperature, use_max=True):
    """adapter_nce_kernel's arithmetic in numpy fp32 (sequential sums); use_max=False plants a max-less softmax."""
    f = np.float32
    x = (sim.numpy().astype(f) / f(temperature)).astype(f)
    n = x.shape[0]
    tot = 0.0
    with np.errstate(all="ignore"):
        for mat in (x, x.T):
            for i in range(n):
                m = mat[i].max() if use_max else f(0)
                s = np.cumsum(np.exp((mat[i] - m).astype(f)), dtype=f)[-1]
                tot += float(f(f(m + np.log(s)) - mat[i, i]))
    return float(f(tot / n / 2))


# ---- matcher cost ---------------------------------------------------------------------------------------------------------------
MATCHER_GAP = 2e-5           # twice the 1e-5 cost tolerance: below it the fp32 argmin may differ from the float64 one
MATCHER_SEED = 0


@functools.lru_cache(maxsize=None)
def matcher_case(B, Nq, seed=MATCHER_SEED):
    """-> (logits, spans, tgt (B, 2)) fp32 tensors; windows 50, 150, .. hold an exact tie (two identical slots) when Nq > 1."""
    rng = np.random.default_rng(300 + 17 * B + Nq + seed)
    lg = rng.standard_normal((B, Nq, 2))
    sp = np.stack([rng.uniform(.1, .9, (B, Nq)), rng.uniform(.02, .6, (B, Nq))], -1)
    tg = np.stack([rng.uniform(.1, .9, B), rng.uniform(.02, .6, B)], -1)
    if Nq > 1:
        a, b = (1, Nq - 1) if Nq > 2 else (0, 1)
        for w in range(50, B, 100):               # the tie is the minimum: the twins sit on the target, certainly foreground
            sp[w, a] = sp[w, b] = tg[w]
            lg[w, a] = lg[w, b] = (9.0, -9.0)
    t = lambda a: torch.tensor(a, dtype=torch.float32)
    return t(lg), t(sp), t(tg)


def matcher_reference64(lg, sp, tg):
    """-> (cost (B, Nq) float64, argmin (lower index on ties), gap between the best and the runner-up)."""
    B, Nq = sp.shape[:2]
    C = np.stack([cost_matrix64(lg[b], sp[b], tg[b:b + 1])[:, 0] for b in range(B)])
    best = C.argmin(1)
    s = np.sort(C, 1)
    gap = s[:, 1] - s[:, 0] if Nq > 1 else np.full(B, np.inf)
    return C, best, gap


# ---- compose_rows -----------------------------------------------------------------------------------------------------------
def compose_case(B, Nq, seed=0):
    """logits with equal pairs inside a window (the proposal scores tie exactly), spans, match, durations, starts."""
    g = torch.Generator().manual_seed(40 + 3 * B + Nq + seed)
    # multiples of 1/8 in [-4, 4]: two slots either tie exactly (same l0 - l1: the same fp32 operations in the kernel and in
    # torch) or differ by >= 4e-5 in their score -- never by an ulp, where the two softmax implementations could order them
    # differently and the bit comparison of st / ed would compare different slots
    logits = (torch.randn(B, Nq, 2, generator=g) * 16).round().clamp(-32, 32) / 8
    for k in range(1, Nq, 3):                     # slot k repeats slot k - 1's logits: a stable sort keeps k - 1 first
        logits[:, k] = logits[:, k - 1]
    if Nq >= 6:
        logits[:, Nq - 1] = logits[:, 0]          # a tie across the whole window
    spans = torch.rand(B, Nq, 2, generator=g)
    match = torch.randn(B, Nq, generator=g)
    dur = torch.randint(1, 126, (B,), generator=g).to(torch.int32)
    vs = torch.randint(0, 100000, (B,), generator=g).to(torch.int32)
    return logits, spans, match, dur, vs


# ---- metrics ------------------------------------------------------------------------------------------------------------------
def metric_random_lists(nq, seed=0, kmax=12):
    rng = np.random.default_rng(70 + nq + seed)
    preds, gts = [], []
    for q in range(nq):
        g0 = round(float(rng.uniform(0, 300)), 4)
        g1 = round(g0 + float(rng.uniform(0.5, 40)), 4)
        k = int(rng.integers(1, kmax + 1))
        st = np.round(g0 + rng.uniform(-30, 30, k), 4)
        ed = np.round(st + rng.uniform(0, 50, k), 4)
        preds.append([[float(a), float(b), 0.1, 0.2, 0.3] for a, b in zip(st, ed)])
        gts.append([g0, g1])
    return preds, gts


def metric_crafted_lists():
    """(preds, gts, notes): spans whose IoU sits exactly ON a threshold, inverted, zero-length and disjoint ones."""
    P = lambda *spans: [[float(a), float(b), 0.1, 0.2, 0.3] for a, b in spans]
    cases = [
        (P((0, 3)), [0, 10], "IoU 3/10 in double: 0.3 > 0.3 is false, and 0.3f > 0.3f too"),
        (P((2, 12)), [2, 22], "IoU 1/2 on the threshold 0.5"),
        (P((0, 5), (0, 5.0001)), [0, 10], "second row just over 1/2"),
        (P((100, 130)), [0, 100], "3/10 is exceeded by no rounding: inter 0"),
        (P((8, 3)), [0, 10], "inverted prediction: inter = 3 - 8 < 0 clamps, union 10"),
        (P((12, 4), (1, 9)), [5, 6], "inverted first row, hit in the second"),
        (P((5, 5)), [5, 5], "zero length on zero length: 0 / 0"),
        (P((5, 5), (5, 5)), [5, 5], "twice"),
        (P((7, 7)), [2, 9], "zero-length prediction inside the target: IoU 0"),
        (P((20, 30), (40, 50)), [0, 10], "disjoint"),
        (P((0.1, 0.4)), [0.1, 1.1], "3/10 from decimals that are not exact in binary"),
        (P((0, 0.3)), [0, 1], "0.3 / 1 in double; fp32 rounds 0.3 once on each side"),
        (P((0, 1)), [0, 1], "IoU 1"),
        (P((3, 4), (0, 7), (0, 10)), [0, 10], "1/10, 7/10, 1: first hit per threshold differs"),
    ]
    return [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]


def window_cases(clip_length, max_v_l=90):
    """Targets whose start or end lands on a multiple of S clip_length, a start of 0, an end past the last window, and rank
    lists with a -1 terminator followed by the hitting window.  -> (ranks {qid: list}, gtl, K)."""
    S = int(max_v_l / 2)
    step = S * clip_length
    gts = [[0.0, 0.5 * step], [step, 2 * step], [2 * step, 2.5 * step], [0.25 * step, 3 * step], [3 * step, 3 * step],
           [5 * step, 400 * step], [1.5 * step, 1.75 * step], [7 * step, 7 * step + clip_length]]
    ranks = {}
    for q, (a, b) in enumerate(gts):
        lo, hi = math.floor(a / clip_length / S), math.ceil(b / clip_length / S) + 1
        far = [w for w in range(hi + 3, hi + 9)]
        ranks[f"q{4 * q}"] = far[:2] + [lo] + far[2:]                 # hit at rank 3: the lowest target window
        ranks[f"q{4 * q + 1}"] = far[:4] + [hi - 1]                   # hit at rank 5: the highest
        ranks[f"q{4 * q + 2}"] = far[:3] + [hi] + far[3:]             # hi itself is outside
        ranks[f"q{4 * q + 3}"] = far[:1] + ([lo - 1] if lo else []) + far[1:]
    gtl = [{"query_id": f"q{4 * q + r}", "timestamps": g} for q, g in enumerate(gts) for r in range(4)]
    return ranks, gtl
