"""References, case families and Python models for the bf16 half of prefilter.hip: the bf16 scorers (frame_score_bf16_kernel,
frame_score_mq_bf16_kernel, frame_score_groups_bf16_kernel + win_fill_seg_kernel), pf_index_kernel and the stages of the
certified pre-filter (pf_cand_chunk / pf_cand_merge, pf_rescore, pf_certify, the gated fallback).  Built on prefilter_refs
(poison, guards, the unit / raw families), prefilter_bf16_ref (the bf16 contract in float64) and prefilter_certified_ref (the
bound E).  Nothing here touches the library.

A  bf16 scorers   reference: float64 on bf16-rounded operands; window = max over its frames that are numbers, -inf without one
                  (``windows_of``, vectorised; the CPU suite holds it against prefilter_bf16_ref.window_reduce).
                  Tolerance: prefilter_bf16_ref.accumulation_bound, dv U max_f sum|ab| + 2 U |score|.
                  Families: unit, raw (bound); quantum, quantum x 2^+-20, dictated (the float64 value, bit for bit).
B  index          ``index_rows``: the row contents of the issue, one builder; ``INDEX_INFLATE`` the upper margin.
C  certified      ``dictated_case``: frame f of query q is x[q][f] e_q in the fp32 arena and c[q][f] e_q in the bf16 arena,
                  query q = a_q e_q, so every exact and every coarse frame score is chosen by the case, independently
                  (cone_prefilter_topk_certified cannot check that its three arenas belong together: the instrument);
                  ``stage_model``: windows -> candidate set -> list -> proof -> fallback list, with ONE planted error
                  (STAGE_FAULTS) at a time.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

import prefilter_bf16_ref as R
import prefilter_certified_ref as C
import prefilter_refs as F

NEG = float("-inf")
NAN = float("nan")
EXACT_FAMILIES = ("quantum", "quantum_up", "dictated")
SCORER_FAMILIES = ("unit", "raw") + EXACT_FAMILIES
QUANTUM = 2.0 ** -6
QUANTUM_S = 20
F32_MAX = float(torch.finfo(torch.float32).max)


# ------------------------------------------------------------------------------------------------ windows, vectorised
def windows_of(fs: torch.Tensor, W: int) -> torch.Tensor:
    """(nq, n) frame scores -> (nq, ceil(n / S) + 1) window scores, S = W // 2: window i = the max over the NUMBERS among the
    frames [max((i-1) S, 0), min((i-1) S + W, n)), -inf where there is none.  Computed the way the header states it (half-window
    maxima + the odd-W first-frame term) in whole-tensor operations: 65 536 windows take milliseconds."""
    S, (nq, n) = W // 2, fs.shape
    nh = -(-n // S)
    x = torch.where(torch.isnan(fs), torch.full_like(fs, NEG), fs)
    neg = lambda c: torch.full((nq, c), NEG, dtype=fs.dtype)
    hm = torch.cat([x, neg(nh * S - n)], dim=1).view(nq, nh, S).max(dim=2).values
    win = torch.maximum(torch.cat([neg(1), hm], dim=1), torch.cat([hm, neg(1)], dim=1))
    if W % 2 == 1 and nh >= 2:
        first = x[:, ::S][:, :nh]                                     # frame h S of half window h
        win = torch.maximum(win, torch.cat([first[:, 1:], neg(2)], dim=1))     # window i takes frame (i + 1) S, i + 1 < nh
    return win


def n_windows(n: int, W: int) -> int:
    return F.n_half(n, W) + 1


# ------------------------------------------------------------------------------------------------ A: scorer families
def _case(family, ctx, cls, **kw):
    c = F._case(family, ctx, cls, **kw)
    c.exact_fs = kw.get("exact_fs")
    return c


def unit(n, dv, nq, seed=0):
    return _case("unit", F._unit(n, dv, 1, n, dv, seed), F._unit(nq, dv, 2, nq, dv, seed))


def raw(n, dv, nq, seed=0):
    return _case("raw", torch.randn(n, dv, generator=F._g(3, n, dv, seed)) * 30.0, F._unit(nq, dv, 2, nq, dv, seed))


def quantum(n, dv, nq, seed=0):
    """Rows and queries = multiples of 2^-6 in [-1, 1]: 7 significand bits (bf16 values), products on 2^-12, any partial sum of
    <= 1 024 products below 2^10 on 2^-12 (22 bits): every summation order, in fp32 or inside the matrix cores, is exact."""
    q = lambda r, *key: torch.randint(-64, 65, (r, dv), generator=F._g(*key)).float() * QUANTUM
    return _case("quantum", q(n, 6, n, dv, seed), q(nq, 7, nq, dv, seed))


def quantum_up(n, dv, nq, seed=0):
    """quantum with rows x 2^20 and queries x 2^-20: the same scores, bit for bit."""
    b = quantum(n, dv, nq, seed)
    return _case("quantum_up", b.ctx * 2.0 ** QUANTUM_S, b.cls * 2.0 ** -QUANTUM_S)


DICTATED_SCALES = (1.0, -1.0, 2.0, -0.5)


def dictated_values(n, W, seed=0):
    """bf16 values c_f for the frames of one video: N(0,1) rounded to bf16, then, half window by half window (cyclic),
    a block of all-negative values, -0.0 beside +0.0, a -inf frame, a NaN frame next to numbers, and -- once -- a whole
    window (W frames) of NaN only and a whole window of -inf only."""
    S = W // 2
    nh = F.n_half(n, W)
    c = torch.randn(n, generator=F._g(8, n, W, seed)).bfloat16().float()
    for h in range(nh):
        lo, hi = h * S, min((h + 1) * S, n)
        kind = h % 6
        if kind == 1:
            c[lo:hi] = (-c[lo:hi].abs() - 0.125).bfloat16().float()
        elif kind == 2:
            c[lo:hi] = 0.0
            c[lo + (h // 6) % 2:hi:2] = -0.0                     # (S = 1: -0.0 and +0.0 in turn from one block to the next)
        elif kind == 3:
            c[lo] = NEG
        elif kind == 4:
            c[hi - 1] = NAN
    if nh >= 12:
        i = nh // 2
        c[(i - 1) * S:(i - 1) * S + W] = NAN
        j = nh // 2 + 4
        c[(j - 1) * S:min((j - 1) * S + W, n)] = NEG
    return c


def dictated(n, dv, nq, W, seed=0, channel=0):
    """Row f = c_f e_ch, query q = s_q e_ch with s_q a power of two (1, -1, 2, -1/2, ...): frame score (q, f) = s_q c_f, one
    exact product whatever the form (every other product is 0 x 0)."""
    c = dictated_values(n, W, seed)
    ctx = torch.zeros(n, dv)
    ctx[:, channel] = c
    s = torch.tensor([DICTATED_SCALES[q % 4] * (2.0 ** (q // 4 % 3)) for q in range(nq)])
    cls = torch.zeros(nq, dv)
    cls[:, channel] = s
    case = _case("dictated", ctx, cls)
    case.exact_fs = s.double()[:, None] * c.double()[None, :]
    case.values = c
    return case


def scorer_case(family, n, dv, nq, W, seed=0):
    """One case of a family; dictated: channel 0 (even seeds) or the row's last channel (odd seeds: the last live lane)."""
    if family == "dictated":
        return dictated(n, dv, nq, W, seed, channel=(dv - 1) if seed % 2 else 0)
    return dict(unit=unit, raw=raw, quantum=quantum, quantum_up=quantum_up)[family](n, dv, nq, seed)


def instantiation(nq_launch, dv, nh):
    """frame_score_bf16_kernel<VPL, QG, 4, WPH> as launch_frame_scores_bf16 picks it for a launch of 1 - 4 queries."""
    return f"frame_score_bf16_kernel<{1 if dv <= 512 else 2},{4 if nq_launch >= 3 else nq_launch},4,{4 if nh < 4096 else 1}>"


def sub(case, rows):
    rows = list(rows)
    c = _case(case.family, case.ctx, case.cls[rows])
    c.exact_fs = None if case.exact_fs is None else case.exact_fs[rows].clone()
    return c


_REFS = {}


def scorer_refs(case, W):
    """(wref, bound) float64 (nq, nw), once per (case, W)."""
    key = (id(case), W)
    if key not in _REFS:
        if len(_REFS) > 8:
            _REFS.clear()
        if case.exact_fs is not None:
            fs, ab = case.exact_fs, case.exact_fs.abs()
        else:
            fs, ab = R.frame_scores(case.ctx, case.cls)
        wref = windows_of(fs, W)
        bound = None if case.family in EXACT_FAMILIES else R.accumulation_bound(wref, windows_of(ab, W), case.dv)
        _REFS[key] = (case, wref, bound)
    return _REFS[key][1:]


def scorer_verdict(case, W, win):
    """Failures (empty = pass) and the worst error / bound of one run's window scores (nq, nw) fp32: shape, the poison rule,
    never a NaN, -inf and +inf exactly where the reference has them, and the family's claim -- the float64 value itself
    (EXACT_FAMILIES) or the accumulation bound."""
    wref, bound = scorer_refs(case, W)
    win = win.detach().cpu()
    fails = []
    if tuple(win.shape) != tuple(wref.shape):
        return [f"shape {tuple(win.shape)} != {tuple(wref.shape)}"], 0.0
    if bool(torch.isnan(win).any()):
        fails.append("a NaN window score")
    if bool(((win.abs() >= F.POISON_SEEN) & torch.isfinite(win) & (wref.abs() < F.POISON_SEEN)).any()):
        fails.append("a score of poison size")
    if case.family in EXACT_FAMILIES:
        bad = int((win.double() != wref).sum())
        if bad:
            fails.append(f"{bad} window scores are not the float64 value")
        return fails, 0.0
    worst, bad = F._cmp(win, wref, bound)
    if bad:
        fails.append(f"{bad} non-numbers misplaced")
    if worst > 1.0:
        fails.append(f"{worst:.3g} bounds")
    return fails, worst


# ---- the scorers in fp32 on the CPU, with the two planted errors of the issue that touch them -----------------------------
SCORER_FAULTS = ("half_block_le", "mq_nnxt_long")


def model_scores16(case, fault=None, order=None, pad=F.PAD):
    """fp32 frame scores (nq, n) of the bf16 contract over the case's POISONED bf16 arena, channel sums taken in the order
    ``order`` (a permutation of the channels; None: ascending).  Faults:
      half_block_le  pf16_half_block's ``c * 8 <= dv``: at dv < 512 VPL the lane behind the row's last one loads the 8 values
                     that FOLLOW the row (the next row's first channels, or poison) against a zero query share: x * 0, which
                     is 0 for every number and NaN for NaN / inf.
      mq_nnxt_long   frame_score_mq_bf16_kernel's ``n_nxt = nks - kb``: the next block's loads run up to 8 k-steps past the
                     row into the rows behind it, but the MFMA loop is guarded by ``kb + s < nks``: loaded, never multiplied."""
    arena, _ = F.poisoned(case.ctx.bfloat16().float(), pad)
    n, dv = case.n, case.dv
    q = case.cls.bfloat16().float()
    rows = arena[pad:pad + n]
    perm = torch.arange(dv) if order is None else order
    prod = rows[None, :, perm] * q[:, None, perm]                       # exact in fp32: 8 x 8 significand bits
    s = torch.zeros(case.nq, n)
    for c in range(dv):                                                 # a plain fp32 running sum in the given order
        s = s + prod[:, :, c]
    if fault == "half_block_le" and dv % 512 != 0:
        nxt = arena.flatten()[(pad * dv + dv):][: n * dv].view(n, dv)[:, :8]       # the 8 values behind each row
        s = s + (nxt * 0.0).sum(dim=1)[None, :]
    return s


# ------------------------------------------------------------------------------------------------ B: index rows
INDEX_INFLATE = (1 + 2.0 ** -10) * (1 + 2.0 ** -16)        # the kernel's stated inflation x its stated rounding allowance
INDEX_TINY = 2.0 ** -54                                     # 2^-55 (PF_INDEX_TINY) + the squares lost below fp32 (<= 2^-56), rounded up


def index_rows(n_rows, dim, kind, seed=0):
    """fp32 rows (n_rows, dim) for pf_index_kernel.  kind:
      unit        N(0,1) unit rows x a per-row scale in [0.5, 3]
      midpoints   every element an exact midpoint of two bf16 neighbours, k + 1/2 ulp with k even and odd in turn: round to
                  nearest EVEN goes down for one and up for the other (and x - bf16(x) is exactly half an ulp)
      subnormal   rows of fp32 subnormals and of values just above 2^-126
      negzero     rows of -0.0 with one number
      f32max      one row holds fp32 max: bf16 +inf, so R = N = +inf
      nan         one NaN row followed by finite rows, the last row the largest of all: R and N stay NaN.  The NaN row is
                  row n_rows // 3, or row 0 past 65 536 rows: wave 0 of the capped grid, whose grid-stride then meets the last row"""
    g = F._g(9, n_rows, dim, seed)
    x = torch.randn(n_rows, dim, generator=g)
    x = x / x.norm(dim=1, keepdim=True).clamp_min(1e-20) * torch.linspace(0.5, 3.0, n_rows)[:, None]
    if kind == "unit":
        return x
    if kind == "midpoints":
        b = x.bfloat16().float().view(torch.int32) & ~0xffff
        k = (torch.arange(n_rows * dim, dtype=torch.int32).view(n_rows, dim) % 2) << 16
        return (((b & ~0x10000) | k) | 0x8000).view(torch.float32)          # bit 16 = k's parity, low half = 0x8000: a midpoint
    if kind == "subnormal":
        bits = torch.randint(1, 1 << 23, (n_rows, dim), generator=g, dtype=torch.int32)
        bits[::2] |= 1 << 23                                                 # every other row: smallest normals
        x = bits.view(torch.float32)
        return torch.where(torch.randint(0, 2, (n_rows, dim), generator=g).bool(), -x, x)
    if kind == "negzero":
        x = torch.full((n_rows, dim), -0.0)
        x[:, dim // 2] = torch.linspace(-2.0, 2.0, n_rows)
        return x
    if kind == "f32max":
        x[n_rows // 2, dim - 1] = F32_MAX
        return x
    if kind == "nan":
        x[0 if n_rows > 65536 else n_rows // 3, dim // 3] = NAN
        x[n_rows - 1] *= 10.0
        return x
    raise KeyError(kind)


def index_ref(x):
    """(bf16 bits as int16 (n_rows, dim), R64, N64) -- torch's round-to-nearest-even and prefilter_certified_ref.index_norms."""
    return x.bfloat16().view(torch.int16), *C.index_norms(x)


# ------------------------------------------------------------------------------------------------ C: dictated arenas
def dictated_case(name, coarse, exact, W, k, n_cand, dv=256, R=0.0, N=0.0, a=None, note=""):
    """coarse (nq, n): bf16 VALUES c[q][f]; exact (nq, n): fp32 values x[q][f]; a (nq,): the queries' one non-zero entry
    (default 1.0).  Arenas: vid_f32[f][q] = x[q][f], vid_bf16[f][q] = c[q][f], query q = a_q e_q.  What the device computes,
    exactly: coarse score = bf16(a_q) c (two bf16 factors: exact in fp32), exact score = fl32(a_q x) (one product, the rest
    zeros).  ``coarse_fs`` / ``exact_fs`` hold those, and the model works on them."""
    coarse = torch.as_tensor(coarse, dtype=torch.float32).reshape(-1, torch.as_tensor(coarse).shape[-1])
    exact = torch.as_tensor(exact, dtype=torch.float32).reshape(coarse.shape)
    nq, n = coarse.shape
    assert nq <= dv and torch.equal(torch.where(torch.isnan(coarse), torch.zeros_like(coarse), coarse.bfloat16().float()),
                                    torch.where(torch.isnan(coarse), torch.zeros_like(coarse), coarse)), "coarse: bf16 values only"
    assert nq == 1 or bool(torch.isfinite(coarse).all() and torch.isfinite(exact).all()), \
        "a non-number in one query's channel meets the zeros of every other query: 0 x inf = NaN (one query only)"
    a = torch.ones(nq) if a is None else torch.as_tensor(a, dtype=torch.float32)
    cls = torch.zeros(nq, dv)
    cls[torch.arange(nq), torch.arange(nq)] = a
    return SimpleNamespace(name=name, nq=nq, n=n, dv=dv, W=W, k=k, n_cand=n_cand, R=float(R), N=float(N), cls=cls, a=a,
                           coarse=coarse, exact=exact, coarse_fs=a.bfloat16().float()[:, None] * coarse,
                           exact_fs=a[:, None] * exact, nw=n_windows(n, W), note=note)


def dictated_arenas(case):
    """(vid_f32 (n, dv) fp32, vid_bf16 (n, dv) bf16) of a dictated case."""
    v32 = torch.zeros(case.n, case.dv)
    v16 = torch.zeros(case.n, case.dv)
    v32[:, :case.nq] = case.exact.t()
    v16[:, :case.nq] = case.coarse.t()
    return v32, v16.bfloat16()


def honest_case(vid, cls, W, k, n_cand, name="honest"):
    """The model's input for HONEST arenas (fp32 rows, their bf16 rounding, the measured norms inflated as the device does):
    scores in float64, rounded once to fp32 -- what any fp32 summation gives up to its last bits."""
    v, q = vid.float(), cls.float()
    R_, N_ = C.index_norms(v)
    return SimpleNamespace(name=name, nq=q.shape[0], n=v.shape[0], dv=v.shape[1], W=W, k=k, n_cand=n_cand, cls=q,
                           R=R_ * C.INFLATE + 2.0 ** -55, N=N_ * C.INFLATE + 2.0 ** -55, nw=n_windows(v.shape[0], W),
                           coarse_fs=(C.bf16(q) @ C.bf16(v).t()).float(), exact_fs=(q.double() @ v.double().t()).float())


def rescore_model(fs_row, i, W, le=False, waves=16, rpw=4):
    """pf_rescore_kernel's loop over window i of one row of frame scores (a list): sixteen waves x four row slots, the row
    index clamped to the window's last frame, a slot counted while ``f0 + r < hi`` (``le``: ``<=``, the planted error)."""
    S, n = W // 2, len(fs_row)
    lo, hi = max((i - 1) * S, 0), min((i - 1) * S + W, n)
    m = NEG
    for f0 in range(lo, hi, rpw):                       # (which wave takes f0 does not matter to a max)
        for r in range(rpw):
            s = fs_row[min(f0 + r, hi - 1)]
            if (f0 + r <= hi if le else f0 + r < hi) and s == s:
                m = max(m, s)
    return m


def bound_E(case, q, R=None, N=None):
    """E of query q as pf_certify_kernel evaluates it (prefilter_certified_ref.device_bound on the R and N handed in)."""
    return C.device_bound(case.cls[q], case.R if R is None else R, case.N if N is None else N, case.dv)


def solve_R0(case, q, g):
    """The R at which E(q) == g for the case's N, from the header's formula solved for R:
    E = (R |qh| + N |qh - q| + 2 gamma N max(|q|, |qh|)) (1 + 2^-10) + TINY (1 + |qh| + N)."""
    x, h = case.cls[q].double(), C.bf16(case.cls[q])
    n_q, n_h, n_d = float(x.norm()), float(h.norm()), float((h - x).norm())
    return ((g - C.TINY * (1 + n_h + case.N)) / C.INFLATE - case.N * n_d - 2 * C.gamma(case.dv) * case.N * max(n_q, n_h)) / n_h


# ------------------------------------------------------------------------------------------------ C: the stage model
STAGE_FAULTS = ("key_no_plus_zero", "tie_lt", "tie_bit29", "certify_ge", "cmin_from_exact", "rescore_le")


def pf_key(v, plus_zero=True):
    """pf_key of prefilter.hip on a float32 array: an unsigned that orders like the float, -0 counted as +0 (``v + 0.f``)."""
    v = np.asarray(v, dtype=np.float32)
    if plus_zero:
        v = v + np.float32(0.0)
    b = v.view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def _stable_desc(v):
    """Indices by (value descending, index ascending), -0 == +0; v without NaN."""
    return np.argsort(-np.asarray(v, dtype=np.float64), kind="stable")


def candidate_set(cw, n_cand, fault=None):
    """The first n_cand of the stable (score desc, index asc) order of one row of coarse windows, as the bisection finds them:
    by pf_key.  Returns (sorted window indices, slots left empty)."""
    cw = np.asarray(cw, dtype=np.float32)
    valid = np.flatnonzero(~np.isnan(cw))
    key = pf_key(cw[valid], plus_zero=fault != "key_no_plus_zero").astype(np.int64)
    order = valid[np.lexsort((valid, -key))]
    take = order[:n_cand]
    empty = n_cand - len(take)
    if fault in ("tie_lt", "tie_bit29") and len(order) > n_cand:
        keys = {int(i): int(k) for i, k in zip(valid, key)}
        T = keys[int(take[-1])]
        at = [int(i) for i in order if keys[int(i)] == T]                      # the pairs at the key, ascending index
        r = sum(1 for i in take if keys[int(i)] == T)
        if len(at) > r:                                                        # the tie bisection runs
            if fault == "tie_lt":                                              # `ix < J`: the r-th of them is left out
                take, empty = take[:-1], empty + 1
            elif at[r - 1] >= 1 << 30:                                         # J cannot reach bit 30: out of range here
                take, empty = take[:-1], empty + 1
    return np.sort(take), empty


def stage_model(case, fault=None, R=None, N=None):
    """The pipeline of cone_prefilter_topk_certified on a dictated case: (idx (nq, k) int32, val (nq, k) fp32, certified
    (nq,) int32, cand: list of sorted index arrays).  ONE planted error at a time (STAGE_FAULTS)."""
    W, k, n_cand, nw = case.W, case.k, case.n_cand, case.nw
    cwin = windows_of(case.coarse_fs, W).numpy()
    ewin = windows_of(case.exact_fs, W).numpy()          # (rescore_le: the extra slot re-reads the window's last row -- clamped --
    k_eff = min(k, nw)                                   #  so the max does not move: blind by construction, asserted on the CPU)
    idx = np.full((case.nq, k), -1, dtype=np.int32)
    val = np.full((case.nq, k), NEG, dtype=np.float32)
    cert = np.zeros(case.nq, dtype=np.int32)
    cands = []
    for q in range(case.nq):
        cand, empty = candidate_set(cwin[q], n_cand, fault)
        cands.append(cand)
        ex = ewin[q][cand]
        top = cand[_stable_desc(ex)][:k_eff]
        lst_i, lst_v = top, ewin[q][top]
        t = float(lst_v[k_eff - 1]) if len(lst_v) >= k_eff else NEG
        c_last = NEG if empty else float((ex if fault == "cmin_from_exact" else cwin[q][cand]).min())
        E = bound_E(case, q, R, N)
        finite = np.isfinite(E) and np.isfinite(t) and np.isfinite(c_last)
        with np.errstate(invalid="ignore"):
            gap = np.float64(t) - np.float64(c_last)
        ok = nw <= n_cand or bool(finite and (gap >= E if fault == "certify_ge" else gap > E))
        cert[q] = int(ok)
        if not ok:                                                             # the fallback: every exact window
            lst_i = _stable_desc(ewin[q])[:k_eff]
            lst_v = ewin[q][lst_i]
        idx[q, :len(lst_i)] = lst_i
        val[q, :len(lst_v)] = lst_v
    return torch.from_numpy(idx), torch.from_numpy(val), torch.from_numpy(cert), cands


def brute_topk(ewin_row, k):
    """The first k of (score desc, index asc) of one row by a plain Python sort of (-score, index) pairs, float64."""
    pairs = sorted((-(float(v) + 0.0), i) for i, v in enumerate(ewin_row.tolist()))
    return [i for _, i in pairs[:k]]


# ------------------------------------------------------------------------------------------------ C: the named cases
def _bf(x):
    return torch.as_tensor(x, dtype=torch.float32).bfloat16().float()


def _own_order(n, seed, base=1000.0):
    """fp32 exact frame values above every coarse value used here (|coarse| <= 512), in an order unrelated to the frame index:
    base + a permutation of 0 .. n-1 (integers < 2^24: exact)."""
    return base + torch.randperm(n, generator=F._g(10, n, seed)).float()


COARSE_PATTERNS = ("distinct", "all_equal", "tie_at_ncand", "tie_at_seam", "all_negative", "zeros_mixed", "neg_inf")


def coarse_pattern(pattern, n, n_cand, seed=0):
    """bf16 frame values (n,) for the candidate-set cases at W = 2 (window i = max(frame i - 1, frame i): n + 1 windows).
      distinct       a strictly decreasing ramp shuffled in blocks: no two frames equal (windows tie only in adjacent pairs)
      all_equal      one value: every window ties, the lowest n_cand indices are the set
      tie_at_ncand   a few high frames, then a plateau that starts before the n_cand-th place and ends after it
      tie_at_seam    as tie_at_ncand, the plateau lying across windows 4095 | 4096 (needs n > 4200)
      all_negative   distinct negative values (the ~b branch of pf_key)
      zeros_mixed    positives, then a run of -0.0 / +0.0 in turn across the n_cand-th place, then negatives
      neg_inf        numbers on fewer than n_cand windows, -inf elsewhere: the set has to take -inf windows, lowest index first"""
    g = F._g(11, n, n_cand, seed)
    if pattern == "distinct":
        assert n <= 128 * 100
        steps = torch.arange(n).float()                                           # 128 values per binade, strictly decreasing:
        v = _bf(2.0 ** (8 - (steps // 128)) * (1 + (127 - steps % 128) / 128))   # 1 + j / 128 has 8 significand bits
        blocks = torch.randperm(-(-n // 128), generator=g)
        return torch.cat([v[b * 128:(b + 1) * 128] for b in blocks.tolist()])
    if pattern == "all_equal":
        return torch.full((n,), 0.75)
    if pattern in ("tie_at_ncand", "tie_at_seam"):
        v = torch.full((n,), 0.25)
        if pattern == "tie_at_seam":                                              # half of the set from high frames in front,
            assert n > 4200 + 2 * n_cand                                          # the rest from the plateau: windows
            hi = n_cand // 4                                                      # 4096 - n_cand / 4 .. 4096 + n_cand / 4 are
            v[16 + 3 * torch.arange(hi)] = 2.0 + (torch.arange(hi) % 112).float() / 8 # chosen, the plateau goes on behind them
            lo = 4096 - max(n_cand // 4, 1)
            v[lo:lo + 2 * n_cand + 8] = 1.0
        else:
            hi = max(n_cand // 2 - 1, 0)                                          # high frames (<= 2 windows each) BEHIND the
            v[n - 1 - 3 * torch.arange(hi)] = 2.0 + (torch.arange(hi) % 112).float() / 8  # plateau, which supplies the last 2 - 3
            v[5:5 + 2 * n_cand + 8] = 1.0
        return v
    if pattern == "all_negative":
        return -coarse_pattern("distinct", n, n_cand, seed)
    if pattern == "zeros_mixed":
        v = _bf(-1.0 - torch.rand(n, generator=g))
        hi = max(n_cand // 2 - 1, 0)
        v[n - 1 - 3 * torch.arange(hi)] = 1.0 + (torch.arange(hi) % 56).float() / 8
        z = torch.zeros(2 * n_cand + 8)
        z[::2] = -0.0
        v[5:5 + z.numel()] = z
        return v
    if pattern == "neg_inf":
        v = torch.full((n,), NEG)
        v[3:3 + max(n_cand // 4, 1) * 3:3] = 1.5
        return v
    raise KeyError(pattern)


def visible_case(pattern, nw, n_cand, seed=0, nq=1, dv=256, k=None):
    """"The candidate set made visible": k = n_cand, every exact score above every coarse one and in an order of its own, R =
    N = 0 (E = 2^-113).  Every query whose candidate set holds numbers only certifies, and idx lists exactly the chosen set in
    the exact scores' order; a set that had to take -inf windows never certifies and the list is the fallback's."""
    n = nw - 1                                                                    # W = 2
    co = torch.stack([coarse_pattern(pattern, n, n_cand, seed + q) for q in range(nq)])
    ex = torch.stack([_own_order(n, seed + q) for q in range(nq)])
    return dictated_case(f"visible/{pattern}/nw{nw}/nc{n_cand}" + (f"/q{nq}" if nq > 1 else ""), co, ex, 2, k or n_cand, n_cand, dv=dv)


VISIBLE_NCAND = (1, 2, 63, 64, 65, 128, 255, 256)


def visible_cases_small():
    """The pattern x n_cand grid at num_window = n_cand + 1 .. 4 097: what both suites run (the GPU suite adds the long rows)."""
    out = []
    for nc in VISIBLE_NCAND:
        out.append(visible_case("tie_at_ncand", max(4 * nc + 40, 64), nc, seed=nc))
        out.append(visible_case("distinct", nc + 1, nc, seed=nc))                 # num_window = n_cand + 1
    for p in COARSE_PATTERNS:
        if p != "tie_at_seam":
            out.append(visible_case(p, 700, 64, seed=3))
    for nw in (4095, 4096, 4097):
        out.append(visible_case("tie_at_ncand", nw, 65, seed=nw))
        out.append(visible_case("zeros_mixed", nw, 128, seed=nw))
    return out


def comparison_case(dv=256, a=1.0, N=2.0, name="comparison"):
    """One query, W = 2, 300 frames, n_cand = 8, k = 4.  Coarse: frames 10, 20, 30 at 3.0 and frame 40 at 1.0 (eight candidate
    windows, c_last = 1.0), 0.5 elsewhere.  Exact: frames 10 and 20 at 1.125 (four windows: t = fl32(1.125 a)), 0 elsewhere.
    g = t - c_last is exact in float64; ``solve_R0`` gives the R at which E == g."""
    n = 300
    co = torch.full((n,), 0.5)
    co[[10, 20, 30]] = 3.0
    co[40] = 1.0
    ex = torch.zeros(n)
    ex[[10, 20]] = 1.125
    case = dictated_case(name, co, ex, 2, 4, 8, dv=dv, R=0.0, N=N, a=[a])
    t = float(case.exact_fs[0, 10])
    case.g = t - 1.0 * float(torch.tensor(a).bfloat16())
    return case


def threshold_case(t, c_last=1.0, n=300, n_cand=8, k=4, name="threshold"):
    """As comparison_case with t and c_last dictated and R = N = 0: E = 2^-113 exactly (TINY (1 + |qh|), |qh| = 1)."""
    co = torch.full((n,), float(_bf(c_last)) - 0.5)
    co[[10, 20, 30]] = float(_bf(c_last)) + 2.0
    co[40] = float(_bf(c_last))
    ex = torch.full((n,), -1000.0)
    ex[[10, 20]] = t
    return dictated_case(name, co, ex, 2, k, n_cand)


def mixed_case(flags, nw, k, W=2, seam=False, dv=256, name="mixed"):
    """One query per flag.  Flag 1 (certifies at R = N = 0): exact peaks on the coarse candidates, above every coarse score.
    Flag 0 (does not): the candidates' exact scores all equal c_last, so t == c_last.  In both, a window OUTSIDE the candidate
    set has the largest exact score of all (1e6) -- honest arenas cannot do that --, so the certified list (the candidates')
    and the fallback list (every window's) differ: a fallback that ran for a certified query, or did not run for an
    uncertified one, changes idx.  ``seam``: the peaks lie across windows 4095 | 4096, so the uncertified queries' exact
    ties straddle the fallback's chunk seam (needs nw > 4500)."""
    S = W // 2
    n = (nw - 1) * S
    nq = len(flags)
    co = torch.full((nq, n), 0.25)
    ex = torch.zeros(nq, n)
    n_cand = max(k, 2)
    m = -(-n_cand // 2)                                                           # peaks: each lights >= 2 windows
    for q, f in enumerate(flags):
        start = (4096 - 3 * (m // 2) + q) * S if seam else (50 + 7 * q) * S
        peaks = start + 3 * S * torch.arange(m)
        assert int(peaks[-1]) < n - 5 * nq - 8
        co[q, peaks] = 2.0 + _bf(torch.arange(m).float() / 4)
        ex[q] = _own_order(n, 40 + q, base=0.0) / (4.0 * n)                       # a floor of distinct exact values < 0.25
        ex[q, peaks] = (600.0 + torch.arange(m).float()) if f else 2.0            # 0: t = 2.0 = c_last (the lowest peak)
        ex[q, n - 1 - 5 * q] = 1e6                                                # the outsider
    return dictated_case(f"{name}/{''.join(map(str, flags))}/nw{nw}/k{k}/W{W}", co, ex, W, k, n_cand, dv=dv)


def nan_frames_case(k, name="nanframes"):
    """One query, W = 5 (S = 2), 300 frames, n_cand = 8.  Coarse peaks at frames 22 and 60 (three windows each) and 100 (the
    first two of its three): the candidates.  Exact: NaN on frames 20 .. 24 (window 11 has no number: -inf, it sorts last), a
    NaN beside numbers at frames 59 and 61, high distinct numbers on the other candidates' frames, low ones elsewhere."""
    n = 300
    co = torch.full((n,), 0.25)
    co[[22, 60, 100]] = torch.tensor([3.0, 2.5, 2.0])
    ex = _own_order(n, 5, base=0.0) / 1024.0
    ex[16:30] = 50.0 + torch.arange(14).float()
    ex[56:66] = 70.0 + torch.arange(10).float()
    ex[96:106] = 90.0 + torch.arange(10).float()
    ex[20:25] = NAN
    ex[[59, 61]] = NAN
    return dictated_case(f"{name}/k{k}", co, ex, 5, k, 8)


def cpu_named_cases():
    """Small named cases of every kind, for the CPU suite's planted-error table (and run again on the GPU)."""
    cases = list(visible_cases_small())
    cases.append(comparison_case())
    cases.append(threshold_case(1.0, name="threshold/t==c_last"))
    cases.append(threshold_case(float(np.nextafter(np.float32(1.0), np.float32(2.0))), name="threshold/nextafter"))
    cases.append(threshold_case(2.0 ** -113, c_last=0.0, name="threshold/gap==E"))
    cases += [nan_frames_case(4), nan_frames_case(8)]
    cases.append(mixed_case((1, 0), 700, 8))
    cases.append(mixed_case((0, 1, 1, 0, 1), 700, 1, W=3))
    return cases
