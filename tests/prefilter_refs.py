"""References, case families and planted-error models for the exact-fp32 pre-filter scorers of prefilter.hip
(frame_score_kernel, frame_score_mq_kernel, pf_split_queries_kernel + frame_score_mq3_kernel, frame_score_groups_kernel +
window_max_seg_kernel, window_combine_kernel).  Nothing here touches the library.

Reference      frame score in float64 from the fp32 inputs (``frame_ref``); window = nanmax of its frames, -inf where a window
               holds no number (``window_ref``: prefilter_bf16_ref.window_reduce over the scores with NaN -> -inf).
Bounds         fp32 forms, any summation order:  dv u / (1 - dv u) sum|a b| + u |ref|,  u = 2^-24  (``fp32_bound``);
               split form: row_refs.gemm_delta(mode "split"), the three-piece bound of the six kept products, per score;
               a window's bound is the largest bound among its frames (the error of a max <= the largest error of its members).
Poison         every arena is a slice of a larger buffer whose other rows are POISON (finite: fmaxf would drop a NaN), every
               output and the workspace start as POISON: a score >= POISON_SEEN or a touched guard fails any case.
Model          ``model_run``: the half-window decomposition as the kernels do it -- hm / fr planes, the combine step, tiles of 16
               with clamped spare lanes (form "tile"), row slots of 4 with clamped spare rows (form "stream"), half windows
               handed out ``stride`` at a time to units that keep their state -- with ONE planted error (FAULTS) at a time.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

import prefilter_bf16_ref as R
import row_refs as RR

U = R.U
POISON = 1e30
POISON_SEEN = 1e29
PAD = 64                # poison rows in front of and behind every arena slice (>= the largest S used: 62)
GUARD = 32              # guard elements in front of and behind every output buffer
DVS = (256, 512, 768, 1024)


# ------------------------------------------------------------------------------------------------ reference and bounds
def frame_ref(ctx, cls):
    """(ref (nq, n), ab (nq, n) = sum_c |a b|) in float64 from the fp32 operands."""
    return R.frame_scores(ctx, cls, rounded=False)


def fp32_bound(ref, ab, dv):
    g = dv * U / (1 - dv * U)
    return g * ab + U * ref.abs()


def split_bound(ctx, cls):
    """Three-piece bound of row_refs per score (nq, n): (6 nz + 6) u P + SPLIT_DROP P, nz = the non-zero products."""
    return RR.gemm_delta(cls.double(), ctx.double(), 0.0, "split")


def _no_nan(x, fill):
    return torch.where(torch.isnan(x), torch.full_like(x, fill), x)


def window_ref(fs, W):
    """nanmax over each window's frames, -inf where there is no number."""
    return R.window_reduce(_no_nan(fs, -np.inf), W)


def n_half(ctx_l, W):
    return -(-ctx_l // (W // 2))


# ------------------------------------------------------------------------------------------------ case families
def _g(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def _unit(n, d, *key):
    x = torch.randn(n, d, generator=_g(*key))
    return x / x.norm(dim=1, keepdim=True)


def _case(family, ctx, cls, **kw):
    return SimpleNamespace(family=family, ctx=ctx.float().contiguous(), cls=cls.float().contiguous(), n=ctx.shape[0],
                           dv=ctx.shape[1], nq=cls.shape[0], exact=None, **kw)


def unit(n, dv, nq, seed=0):
    return _case("unit", _unit(n, dv, 1, n, dv, seed), _unit(nq, dv, 2, nq, dv, seed))


def raw(n, dv, nq, seed=0):
    """--no_norm_vfeat: un-normalised rows, N(0,1) x 30."""
    return _case("raw", torch.randn(n, dv, generator=_g(3, n, dv, seed)) * 30.0, _unit(nq, dv, 2, nq, dv, seed))


def offset(n, dv, nq, seed=0):
    """rows = 300 + 0.03 N(0,1) against zero-mean queries: sum|ab| >> |score|."""
    ctx = 300.0 + 0.03 * torch.randn(n, dv, generator=_g(4, n, dv, seed))
    cls = _unit(nq, dv, 2, nq, dv, seed)
    cls = cls - cls.mean(dim=1, keepdim=True)
    return _case("offset", ctx, cls)


POW2_Q = 2.0 ** -10          # operand quantum of the pow2 base case (row_refs.pow2_is_safe: A, bias, R on 2^-10; W on 2^-14)
POW2_S = 20


def pow2_base(n, dv, nq, seed=0):
    """Unit rows and queries rounded to multiples of 2^-10: every product and partial sum is a multiple of 2^-20."""
    qz = lambda x: torch.round(x / POW2_Q) * POW2_Q
    return _case("pow2base", qz(_unit(n, dv, 1, n, dv, seed)), qz(_unit(nq, dv, 2, nq, dv, seed)))


def pow2(n, dv, nq, seed=0):
    """The base case with rows x 2^20 and queries x 2^-20: the same scores, bit for bit."""
    b = pow2_base(n, dv, nq, seed)
    return _case("pow2", b.ctx * 2.0 ** POW2_S, b.cls * 2.0 ** -POW2_S)


def pow2_safe(base):
    """row_refs.pow2_is_safe on both operands: the rows scaled up (as A), the queries scaled down (as A of the transposed
    product) -- no piece of either run is subnormal, nothing overflows."""
    z = lambda r: torch.zeros(r, 1)
    a = SimpleNamespace(A=base.ctx, W=base.cls, bias=z(1), R=z(1))
    b = SimpleNamespace(A=base.cls, W=base.ctx, bias=z(1), R=z(1))
    return RR.pow2_is_safe(a, POW2_S, pieces=True) and RR.pow2_is_safe(b, -POW2_S, pieces=True)


def onehot_channel(f, dv):
    return (7 * f + 3) % dv


ONEHOT2 = 1.0 + 2.0 ** -8 - 2.0 ** -15         # two bf16 pieces: h = 1, m = 2^-8 - 2^-15, l = 0


def onehot(n, dv, nq, seed=0, value=1.0):
    """Frame f = value x the unit vector of channel (7 f + 3) mod dv, dense queries: score[q][f] = value txt[q][c(f)], exactly
    for value 1 (``exact``) -- the only input that pins the channel <-> k-slot permutation of the matrix-core forms."""
    ctx = torch.zeros(n, dv)
    ch = torch.tensor([onehot_channel(f, dv) for f in range(n)])
    ctx[torch.arange(n), ch] = value
    c = _case("onehot" if value == 1.0 else "onehot2", ctx, _unit(nq, dv, 2, nq, dv, seed) * 3.0)
    if value == 1.0:
        c.exact = c.cls[:, ch].clone()
    return c


def onehot_mirror(n, dv, nq, seed=0):
    """One-hot queries (query q: channel (7 q + 3) mod dv) over dense frames: score[q][f] = vid[f][c(q)] exactly."""
    cls = torch.zeros(nq, dv)
    ch = torch.tensor([onehot_channel(q, dv) for q in range(nq)])
    cls[torch.arange(nq), ch] = 1.0
    c = _case("onehot_mirror", _unit(n, dv, 1, n, dv, seed) * 3.0, cls)
    c.exact = c.ctx[:, ch].t().clone()
    return c


def structural_frames(n, W):
    """The frames at which a seam of one of the forms lies, as {name: frame}: half-window first / second / last frames, the
    odd-W extra frame (i+1)S, the tile lanes 16 t - 1 / 16 t of a half window, the last valid lane of its partial tile, the row
    slots on either side of the half window's end, frame 0 and the video's last frame."""
    S, nh = W // 2, n_half(n, W)
    out = {"frame0": 0, "last": n - 1}
    for h in sorted({0, 1, 2, nh // 2, nh - 2, nh - 1}):
        if not 0 <= h < nh:
            continue
        lo, hi = h * S, min((h + 1) * S, n)
        out[f"h{h}.first"] = lo
        out[f"h{h}.last"] = hi - 1
        if lo + 1 < hi:
            out[f"h{h}.second"] = lo + 1
        for t in range(1, (hi - lo + 15) // 16):
            out[f"h{h}.tile{t}.lane15"] = lo + 16 * t - 1
            out[f"h{h}.tile{t}.lane0"] = lo + 16 * t
        for k in range(1, 5):
            if hi - 1 - k >= lo:
                out[f"h{h}.end-{k}"] = hi - 1 - k
    return out


def peak_rounds(n, W, nq):
    """The structural frames, nq at a time: round r places query q's peak at frames[r nq + q]."""
    fr = sorted(set(structural_frames(n, W).values()))
    return [fr[i:i + nq] for i in range(0, len(fr), nq)]


def peaks(n, dv, nq, frames, seed=0):
    """Rows of small scores; query q's frame frames[q % len] raised far above the rest (orthonormal queries)."""
    assert nq <= dv
    qm, _ = torch.linalg.qr(torch.randn(dv, nq, generator=_g(5, dv, nq, seed)).double())
    cls = qm.t().float()
    ctx = 0.01 * _unit(n, dv, 1, n, dv, seed)
    at = [frames[q % len(frames)] for q in range(nq)]
    for q, f in enumerate(at):
        ctx[f] = ctx[f] + cls[q]
    return _case("peaks", ctx, cls, at=at)


def nanrows(n, dv, nq, W, seed=0):
    """The unit case with whole NaN rows at the structural frames, one whole half window and one whole window of them."""
    c = unit(n, dv, nq, seed)
    S, nh = W // 2, n_half(n, W)
    rows = set(structural_frames(n, W).values())
    if nh >= 3:
        rows |= set(range(1 * S, min(2 * S, n)))                          # half window 1
    if nh >= 8:
        i = nh // 2 + 2
        rows |= set(range((i - 1) * S, min((i - 1) * S + W, n)))          # window i
    if n > 1 and len(rows) >= n:
        rows.discard(n // 2)
    c.ctx[sorted(rows)] = float("nan")
    c.family, c.nan_rows = "nanrows", sorted(rows)
    return c


FAMILIES = ("unit", "raw", "offset", "pow2", "onehot", "onehot2", "onehot_mirror", "peaks", "nanrows")


def family_cases(family, n, dv, nq, W, seed=0):
    """Every case of one family at one shape (peaks: one case per round of structural frames)."""
    if family == "peaks":
        return [peaks(n, dv, nq, fr, seed) for fr in peak_rounds(n, W, nq)]
    if family == "nanrows":
        return [nanrows(n, dv, nq, W, seed)]
    if family == "onehot2":
        return [onehot(n, dv, nq, seed, value=ONEHOT2)]
    return [dict(unit=unit, raw=raw, offset=offset, pow2=pow2, onehot=onehot, onehot_mirror=onehot_mirror)[family](n, dv, nq, seed)]


# ------------------------------------------------------------------------------------------------ the verdict on one run
def poisoned(rows, pad=PAD):
    """rows inside a larger buffer of POISON rows; returns (buffer, the slice's first row)."""
    buf = torch.full((pad + rows.shape[0] + pad, rows.shape[1]), POISON, dtype=rows.dtype)
    buf[pad:pad + rows.shape[0]] = rows
    return buf, pad


def guarded(numel, guard=GUARD):
    return torch.full((guard + numel + guard,), POISON, dtype=torch.float32)


def guards_intact(buf, numel, guard=GUARD):
    b = buf.detach().cpu()
    return bool((b[:guard] == np.float32(POISON)).all()) and bool((b[guard + numel:] == np.float32(POISON)).all())


def same(a, b):
    """Bit-for-bit agreement of two score tensors as values: equal numbers, NaN exactly where the other has NaN."""
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _cmp(got, ref, bound):
    """(worst |got - ref| / bound, mismatches of the non-numbers): NaN / -inf must sit exactly where the reference has them."""
    got = got.double()
    special = torch.isnan(ref) | torch.isinf(ref)
    same = (torch.isnan(got) == torch.isnan(ref)) & (torch.where(torch.isinf(ref), got == ref, torch.ones_like(special)))
    bad = int((~same).sum())
    ok = ~special & ~torch.isnan(got)
    if not bool(ok.any()):
        return 0.0, bad
    return RR.worst_ratio(got[ok], ref[ok], bound[ok]), bad


_REFS = {}


def _reduce_rows(rows, W):
    """window_reduce of several (nq, n) float64 matrices in one pass."""
    out = R.window_reduce(torch.cat(rows), W)
    return out.split([r.shape[0] for r in rows])


def refs_of(case, W, split=False):
    """The case's float64 frame / window references and bounds, computed once per (case, W, form)."""
    key = (id(case), W, split)
    if key not in _REFS:
        if len(_REFS) > 8:
            _REFS.clear()
        ref, ab = frame_ref(case.ctx, case.cls)
        bfs = split_bound(case.ctx, case.cls) if split else fp32_bound(ref, ab, case.dv)
        wref, bwin = _reduce_rows([_no_nan(ref, -np.inf), _no_nan(bfs, 0.0)], W)
        _REFS[key] = (case, ref, bfs, wref, bwin)               # (holds the case: its id stays its own)
    return _REFS[key][1:]


def sub(case, rows):
    """The case with a subset of its queries."""
    rows = list(rows)
    c = _case(case.family, case.ctx, case.cls[rows])
    c.exact = None if case.exact is None else case.exact[rows].clone()
    return c


def verdict(case, W, fs, win, split=False, exact=True):
    """Failures (a list of strings, empty = pass) and the worst error / bound of one run.  fs: (nq, n) fp32 or None; win: (nq,
    nh + 1) fp32.  Checks: the poison rule, the bound on frames and windows, the non-numbers, win == window_reduce(fs) bit for
    bit, and the case's exact values (the one-hot families) where ``exact``."""
    ref, bfs, wref, bwin = refs_of(case, W, split)
    fails, worst = [], 0.0
    win = win.detach().cpu()
    fs = None if fs is None else fs.detach().cpu()
    for name, t in (("fs", fs), ("win", win)):
        if t is not None and bool(((_no_nan(t, 0.0).abs() >= POISON_SEEN) & (t != -np.inf)).any()):     # (-inf: see _cmp)
            fails.append(f"{name}: a score of poison size")
    r, bad = _cmp(win, wref, bwin)
    worst = max(worst, r)
    if bad:
        fails.append(f"win: {bad} non-numbers misplaced")
    if r > 1.0:
        fails.append(f"win: {r:.3g} bounds")
    if fs is not None:
        r, bad = _cmp(fs, ref, bfs)
        worst = max(worst, r)
        if bad:
            fails.append(f"fs: {bad} non-numbers misplaced")
        if r > 1.0:
            fails.append(f"fs: {r:.3g} bounds")
        if not torch.equal(window_ref(fs, W), win):
            fails.append("win != window_reduce(fs) bit for bit")
        if exact and case.exact is not None and not same(fs, case.exact):
            fails.append("fs: not the exact one-hot value")
    if exact and case.exact is not None and not torch.equal(win, window_ref(case.exact, W)):
        fails.append("win: not the exact one-hot value")
    return fails, worst


# ------------------------------------------------------------------------------------------------ CPU restatements
def scores_f32(ctx, cls):
    """Plain fp32 restatement of the fp32 forms (torch's own summation order)."""
    return RR.mm32(cls, ctx)


def scores_split(ctx, cls, drop=()):
    """The six kept products of the split form, small terms first (row_refs.mm_split)."""
    return RR.mm_split(cls, ctx, drop=drop)


# ------------------------------------------------------------------------------------------------ the model
FAULTS = ("combine_le", "odd_dropped", "fr_second", "row_clamp_S", "valid_dropped", "hm_not_reset", "kslot_swap",
          "q0_from_zero", "drop_product")
ARITH_FAULTS = ("kslot_swap", "q0_from_zero", "drop_product")
Q0_PASS = 32            # queries per launch of frame_score_mq_kernel at dv > 512


def model_scores(case, fault=None, split=False, pad=PAD):
    """fp32 scores (nq, pad + n + pad) over the case's POISONED arena in the form's arithmetic, with an arithmetic fault."""
    arena, _ = poisoned(case.ctx, pad)
    cls = case.cls.clone()
    if fault == "kslot_swap":                                   # two channels of one 16-channel slab change k slots, on A only
        for s in range(case.dv // 16):
            cls[:, [16 * s + 1, 16 * s + 6]] = cls[:, [16 * s + 6, 16 * s + 1]]
    if fault == "q0_from_zero":
        src = torch.arange(case.nq)
        src[Q0_PASS:] -= Q0_PASS
        cls = cls[src]
    if split:
        return scores_split(arena, cls, drop=("mm",) if fault == "drop_product" else ())
    return scores_f32(arena, cls)


def _fmax(a, b):
    return np.fmax(a, b)            # fmaxf: a NaN operand is dropped


def model_run(sc, n, W, form, fault=None, stride=4, pad=PAD, guard=GUARD):
    """The kernels' decomposition on the scores ``sc`` (nq, pad + n + pad; the columns outside [pad, pad + n) belong to the
    poison rows).  Returns (fs buffer with guards -- flat, GUARD + nq n + GUARD --, win (nq, nh + 1)).  Half windows go to
    ``stride`` units in turn; a unit takes h, h + stride, ... and keeps its registers in between (the grid-stride loop)."""
    sc = np.asarray(sc, dtype=np.float32)
    nq, S = sc.shape[0], W // 2
    nh = -(-n // S)
    fsb = np.full(guard + nq * n + guard, np.float32(POISON), dtype=np.float32)
    planes = np.full(2 * nq * nh + guard, np.float32(POISON), dtype=np.float32)         # hm | fr | what lies behind them
    hm, fr = planes[:nq * nh].reshape(nq, nh), planes[nq * nh:2 * nq * nh].reshape(nq, nh)
    qs = np.arange(nq)
    state = {}
    for h in range(nh):
        lo = h * S
        cnt = min(S, n - lo)
        m = np.full(nq, -np.inf, dtype=np.float32)
        if fault == "hm_not_reset" and (h - stride) in state:
            m = state[h - stride]
        first = 1 if fault == "fr_second" else 0
        step = 4 if form == "stream" else 16
        for j0 in range(0, cnt, step):
            for r in range(step):
                clamp = (S if (fault == "row_clamp_S" and form == "stream") else cnt) - 1
                s = sc[:, pad + lo + min(j0 + r, clamp)]
                valid = j0 + r < cnt or (fault == "valid_dropped" and form == "tile")
                if valid:
                    m = _fmax(m, s)
                    fsb[guard + qs * n + lo + j0 + r] = s
                if j0 == 0 and r == first:
                    fr[:, h] = s
        hm[:, h] = m
        state[h] = m
    win = np.empty((nq, nh + 1), dtype=np.float32)
    frf = planes[nq * nh:]                                              # the fr plane and what follows it, flat
    for i in range(nh + 1):
        m = hm[:, i - 1] if i >= 1 else np.full(nq, -np.inf, dtype=np.float32)
        if i < nh:
            m = _fmax(m, hm[:, i])
        take = (i + 1 <= nh) if fault == "combine_le" else (i + 1 < nh)
        if W % 2 == 1 and take and fault != "odd_dropped":
            m = _fmax(m, frf[qs * nh + i + 1])
        win[:, i] = m
    return torch.from_numpy(fsb), torch.from_numpy(win)


def model_verdict(case, W, form, fault=None, split=False, stride=4):
    """verdict() + the guard check on a model run."""
    sc = model_scores(case, fault if fault in ARITH_FAULTS else None, split)
    fsb, win = model_run(sc.numpy(), case.n, W, form, None if fault in ARITH_FAULTS else fault, stride)
    fs = fsb[GUARD:GUARD + case.nq * case.n].view(case.nq, case.n)
    fails, worst = verdict(case, W, fs, win, split)
    if not guards_intact(fsb, case.nq * case.n):
        fails.append("fs: a guard element was written")
    return fails, worst


def caught(fails, worst):
    """A planted error counts as caught by >= 10 bounds, or by anything that is not a bound (exact mismatch, guard, poison,
    misplaced non-number)."""
    return worst >= 10.0 or any("bounds" not in f for f in fails)


# ------------------------------------------------------------------------------------------------ what the GPU suite runs
STREAM_NH = (2047, 2048, 2049, 4095, 4096, 4097, 8192, 8193)       # around the WPH switch (4096) and the grid cap (2048 / 8192)
STREAM_W = (2, 3, 7)
WIDE_NH = (2049, 4097)
EDGE_W = (90, 125)                                                    # S = 45, 62
EDGE_NH = (1, 2, 3, 17)


def edge_ctx_ls(W, nh):
    """ctx_l with nh half windows whose last one has 0, 1, 2, 3, 4, 5, S - 1 frames past a multiple of S (0 = a full one)."""
    S = W // 2
    return sorted({(nh - 1) * S + (r if r else S) for r in (0, 1, 2, 3, 4, 5, S - 1)})


MQ_NQ = {512: (5, 16, 17, 32, 33, 64, 65, 81, 97), 768: (5, 17, 32, 33, 49, 65), 1024: (5, 17, 32, 33, 49, 65)}
MQ_W = tuple(2 * s + (s % 2) for s in (1, 3, 15, 16, 17, 31, 32, 33, 45, 62))       # S = W // 2; odd S -> odd W
MQ_NH = (1, 11, 12, 13, 25)
SPLIT_NQ = (8, 16, 17, 63, 64, 65, 129)
GROUP_CTX = (1, 3, 4, 5, 15, 16, 17)
GROUP_NQ = (1, 2, 3, 4, 5, 8)
GROUP_STRIDE_CLIPS = 32768 + 9


def mq_grid_nh(n_cu):
    return (12 * n_cu - 1, 12 * n_cu, 12 * n_cu + 1, 24 * n_cu + 5)
