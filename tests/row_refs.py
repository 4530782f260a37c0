"""Hostile value distributions, float64 references and DERIVED elementwise bounds for the row kernels: the fp32 GEMM family
(gemm.hip), the fused layer tails (ffn.hip / ffn_wide.hip, ffn_split.hip, ffn_bf16.hip), gemm_bf16.hip and the row LayerNorm /
L2 normalisation (rowops.hip).  Used by tests/test_row_kernels_cpu.py (the bounds hold for a plain evaluation and every
planted error leaves them), tests/test_row_kernels_gpu.py (the kernels stay inside them) and tests/test_tail_mc_forms_gpu.py
(the matrix-core tails' ride, pre-norm, gather and walk forms: tail_mc_case, the ride's bound in tail_ref_bound, mc_runs).

Nothing here is measured on a kernel.  U = 2^-24 is the unit roundoff of fp32.

Bounds
------
fp32 GEMM + epilogue, y = relu?((A + A2) W^T + bias) + R before any LayerNorm:
    delta = (nz + 6) U (|A + A2| |W|^T + |bias| + |R|)
nz = the number of non-zero products of that element: the forward bound of an fp32 sum of nz terms in ANY order; 6 covers the
A + A2 add, the bias add, the residual add and the store; ReLU is 1-Lipschitz.  An error bound `da` on the activations (an
earlier stage) goes through as da |W|^T.

Three-piece split (ffn_split.hip, tb_split2 in tail_bf16_common.h): x = h + m + l + rho with h = bf16(x), m = bf16(x - h),
l = bf16(x - h - m) (round to nearest even, 8 significant bits each; the subtractions are exact in fp32), so
    |m + l + rho| <= 2^-8 |x|,  |l + rho| <= 2^-16 |x|,  |rho| <= 2^-24 |x|.
The kernel forms (its header and SP_MM6) xl wh + xh wl + xm wm + xh wm + xm wh + xh wh.  Of the full product (h+m+l+rho)(h+m+l+rho)
it therefore leaves out  xm wl,  xl wm,  xl wl  and the terms in rho:
    |xm wl| <= 2^-8 2^-16 |x w| = 2^-24 |x w|, the same for xl wm;  |xl wl| <= 2^-32 |x w|;
    |rho_x w| + |x rho_w| + |rho_x rho_w| <= (2 2^-24 + 2^-48) |x w|
in all (4 + 2^-8 + 2^-24) 2^-24 |x w| <= SPLIT_DROP |x w| with SPLIT_DROP = 4.01 * 2^-24 -- the issue's "about 2^-22".  The six
products of bf16 pairs are exact in fp32 and are accumulated in fp32: 6 nz terms,
    delta_split = ((6 nz + 6) U) (|A||W|^T + |bias| + |R|) + SPLIT_DROP |A||W|^T.

Single piece (ffn_bf16.hip, gemm_bf16.hip): the reference is evaluated on operands rounded once to bf16; the products are then
exact and the fp32 bound above applies to the rounded operands.  Where an operand is itself computed by the kernel (the tail's
LayerNorm output and hidden row) its fp32 value lies within its bound e of the reference's; if no bf16 rounding boundary lies
within e the two round alike, otherwise the rounded values differ by at most e + 1.5 spacings (`flip`).

`tiny` adds 3 nz 2^-126 max|other operand| per output, so that every subnormal operand piece or product may be flushed.

LayerNorm over n channels, c = y - mean(y), s = sqrt(var + 1e-5), first order in the input error delta:
    |d o_i| <= |g_i| / s (delta_i + mean(delta) + |c_i| mean(|c| delta) / s^2) + 16 U (|g_i| |c_i| / s + |b_i|)
doubled for the second order, which is valid while max(delta) / s <= LN_VALID = 0.05.  One LayerNorm behind one GEMM and the
row LayerNorm always lie in that domain (asserted on the CPU).  The worst-case delta of the projecting tails, chained through
|W1| and |W2|, leaves it even on the benign control, so rows outside it take the bound that is not linearised (ln_ref_bound);
the CPU suite asserts that every row of every case has one of the two: no element is exempted.  For the stand-alone
LayerNorm kernel the input is exact (delta = 0) and nothing upstream carries the magnitude of the row, so the rounding of its
own mean is stated separately: the kernel sums a quad, at most four quads per lane and six shuffle steps, then divides -- at
most 13 roundings; LN_OWN_SUM = 16: 16 U mean|y| is added to mean(delta).

L2 normalisation: 8 U |x_i| / norm (the sum of squares, the square root, the eps add and the quotient), for rows whose sum of
squares neither overflows nor underflows in fp32 (L2_DOMAIN).  A zero row with eps = 0 is 0 / 0 = NaN under both clamp values,
as in the float64 evaluation of the same formula; with eps > 0 it is 0."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

U = 2.0 ** -24
SPLIT_DROP = 4.01 * U
LN_VALID = 0.05
LN_RIG_VALID = 0.5
LN_OWN_SUM = 16.0
FLUSH = 3.0 * 2.0 ** -126
L2_DOMAIN = (1e-16, 1e16)       # |x| of every non-zero element: dim * x^2 stays inside fp32's normal range up to dim = 1024
FP32_MIN, FP32_MAX = 2.0 ** -126, 2.0 ** 127

FAMILIES_TAIL = ("benign", "offset300", "offset1e4", "nearconst", "spike", "spike_t", "gains", "dead", "alive", "onehot", "cancel")
FAMILIES_LN = ("benign", "offset300", "offset1e4", "nearconst", "spike", "spike_t", "gains")
POW2_SCALES = (-40, 40)
POW2_SCALES_SPLIT = (-40, 40, -80)
OFFSETS = {"offset300": (300.0, 0.03), "offset1e4": (-1e4, 1.0), "nearconst": (0.5, 2.0 ** -10)}


def bf(t):
    """fp32 -> bf16 (round to nearest even) -> float64: the one rounding of the single-piece kernels."""
    return t.float().bfloat16().double()


def _seed(family, *shape):
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(shape)) + sum(ord(ch) for ch in family) * 104729


# ------------------------------------------------------------------------------------------------ case families
def _student_t(shape, seed):
    """Student-t with 2 degrees of freedom (heavy tails: infinite variance), drawn on the CPU with numpy."""
    return torch.from_numpy(np.random.default_rng(seed).standard_t(2.0, size=shape).astype(np.float32))


def _sparse_rows(M, K, g, nnz=16):
    """N(0, 1) rows with nnz non-zero channels each, at positions that move with the row."""
    A = torch.zeros(M, K)
    for i in range(M):
        idx = (torch.arange(nnz) * (K // nnz) + i) % K
        A[i, idx] = torch.randn(nnz, generator=g)
    return A


def _constant_rows(M, N, g):
    """Exactly constant rows, the value a multiple of 1 / 8 with at most 12 significant bits (so every partial sum of a row's 256
    equal values is exact in fp32 and so is its mean); every fifth row is all zero."""
    v = torch.randint(-2047, 2048, (M, 1), generator=g).float() / 8
    v[::5] = 0
    v[1 % M] = 2047 / 8
    return v.expand(M, N).contiguous()


def _pairs(M, K, N, g):
    """+- pairs: a_(2j) = a_(2j+1), w_(2j+1) = -w_(2j) up to 2^-12: sum a w is about 2^-12 of sum |a w|."""
    a = torch.randn(M, K // 2, generator=g) * 100
    A = a.repeat_interleave(2, dim=1)
    w = torch.randn(N, K // 2, generator=g) / K ** 0.5
    W = torch.stack([w, -w + torch.randn(N, K // 2, generator=g) / K ** 0.5 * 2.0 ** -12], dim=2).reshape(N, K)
    return A.contiguous(), W.contiguous()


def _hostile_gains(n, g):
    lg = torch.rand(n, generator=g) * 16 - 8
    lg[::7] = 0
    lg[1::7] = -lg[1::7].abs()
    lg[3], lg[n - 1] = 8.0, -8.0
    return lg, torch.randn(n, generator=g) * 100


@functools.lru_cache(maxsize=None)
def gemm_case(family, M, N, K, a2=None, scale=None):
    """Operands of C = epi((A [+ A2]) W^T + bias) for one family.  a2: None / "full" / "mod5".  scale: the pow2 family's s
    (family "pow2base" is its control: the benign draw QUANTISED to multiples of 2^-10 (A, bias, R) and 2^-14 (W), so every
    product and every partial sum of any order is a multiple of 2^-24 -- which is what makes the scaled run provably exact)."""
    g = torch.Generator().manual_seed(_seed("pow2base" if family == "pow2" else family, M, N, K))
    c = SimpleNamespace(family=family, M=M, N=N, K=K, a2_mod=0, A2=None, flush=False, kind="gemm")
    c.A = torch.randn(M, K, generator=g)
    c.W = torch.randn(N, K, generator=g) / K ** 0.5
    c.bias = torch.randn(N, generator=g)
    c.R = torch.randn(M, N, generator=g)
    c.lg, c.lb = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
    if a2 == "full":
        c.A2 = torch.randn(M, K, generator=g)
    elif a2 == "mod5":
        c.A2, c.a2_mod = torch.randn(5, K, generator=g), 5
    if family in ("benign",):
        pass
    elif family in ("pow2base", "pow2"):
        q = lambda t, b: torch.round(t * 2.0 ** b) / 2.0 ** b
        c.A, c.W, c.bias, c.R = q(c.A, 10), q(c.W, 14), q(c.bias, 10), q(c.R, 10)
        if family == "pow2":
            f = 2.0 ** scale
            c.A, c.bias, c.R = c.A * f, c.bias * f, c.R * f
            c.scale = scale
    elif family in OFFSETS:
        # the offset sits on the residual; the product is kept below the spread (sparse rows: nz <= 16, which also keeps
        # delta / s inside the LayerNorm bound's domain)
        mean, std = OFFSETS[family]
        c.A = _sparse_rows(M, K, g)
        c.W = c.W * (std / 4) * (K / 16) ** 0.5
        c.bias = c.bias * std
        c.R = mean + std * torch.randn(M, N, generator=g)
    elif family == "constant":
        c.W, c.bias = torch.zeros(N, K), torch.zeros(N)
        c.R = _constant_rows(M, N, g)
    elif family in ("spike", "spike_t"):
        if family == "spike_t":
            c.A = _student_t((M, K), _seed(family, M, K))
            c.R = _student_t((M, N), _seed(family, M, N) + 1)
        rows = torch.arange(M)
        c.A[rows, rows % K] = 1e4
        c.R[rows, (rows * 3 + 1) % N] = 1e4
    elif family == "gains":
        c.lg, c.lb = _hostile_gains(N, g)
    elif family in ("onehot", "onehot1"):
        assert M >= K, "onehot needs a row per k index"
        rows = torch.arange(M)
        amp = torch.ones(M) if family == "onehot1" else torch.randn(M, generator=g) * 3
        c.A = torch.zeros(M, K)
        c.A[rows, rows % K] = amp
    elif family == "cancel":
        c.A, c.W = _pairs(M, K, N, g)
    elif family == "tiny":
        c.A, c.bias, c.R = c.A * 2.0 ** -118, c.bias * 2.0 ** -118, c.R * 2.0 ** -118
        c.W = torch.randn(N, K, generator=g)
        c.flush = True
    else:
        raise KeyError(family)
    return c


@functools.lru_cache(maxsize=None)
def tail_case(family, M, ff):
    """Operands of the layer tail: A (M, 256) attention rows, Wo / bo, R (M, 256) residual (= the block input X of the forms
    without projection), the projection's LayerNorm pg / pb, W1 / b1, W2 / b2, the closing LayerNorm lg / lb; scales and
    generators of the suite's benign tail tests."""
    g = torch.Generator().manual_seed(_seed(family, M, ff))
    c = SimpleNamespace(family=family, M=M, ff=ff, flush=False, kind="tail")
    c.R = torch.randn(M, 256, generator=g) * 1.5
    c.W1 = torch.randn(ff, 256, generator=g) / 16
    c.b1 = torch.randn(ff, generator=g) * 0.2
    c.W2 = torch.randn(256, ff, generator=g) / ff ** 0.5
    c.b2 = torch.randn(256, generator=g) * 0.2
    c.lg, c.lb = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g)
    c.A = torch.randn(M, 256, generator=g)
    c.Wo = torch.randn(256, 256, generator=g) / 16
    c.bo = torch.randn(256, generator=g) * 0.2
    c.pg, c.pb = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g) * 0.3
    if family == "benign":
        pass
    elif family in OFFSETS:
        mean, std = OFFSETS[family]
        c.A = _sparse_rows(M, 256, g, nnz=2)
        c.Wo = c.Wo * std
        c.bo = c.bo * std
        c.R = mean + std * torch.randn(M, 256, generator=g)
        # a near-constant row in fp32 carries 6 U mean / std of relative noise into its LayerNorm's output; the worst-case
        # chain through |W1| |W2| would take that out of every LayerNorm bound's domain, so the hidden units are dead here
        # (and b2 stays below the spread): the case pins the LayerNorms and the residual path
        c.W1 = c.W1 * 2.0 ** -12
        c.b1 = torch.full((ff,), -1e3)
        c.b2 = c.b2 * std
    elif family in ("spike", "spike_t"):
        if family == "spike_t":
            c.A = _student_t((M, 256), _seed(family, M, 1))
            c.R = _student_t((M, 256), _seed(family, M, 2))
        rows = torch.arange(M)
        c.A[rows, rows % 256] = 1e4
        c.R[rows, (rows * 3 + 1) % 256] = 1e4
    elif family == "gains":
        c.pg, c.pb = _hostile_gains(256, g)
        c.lg, c.lb = _hostile_gains(256, g)
    elif family == "dead":
        # (sparse attention rows: the projection's own bound is a few U, so the case is sharp for both LayerNorms)
        c.A = _sparse_rows(M, 256, g, nnz=2)
        c.b1 = torch.full((ff,), -1e3)
    elif family == "alive":
        c.b1 = torch.full((ff,), 1e3)
    elif family == "onehot":
        assert M >= 256
        rows = torch.arange(M)
        amp = torch.randn(M, generator=g) * 3
        c.A = torch.zeros(M, 256)
        c.A[rows, rows % 256] = amp
        c.R = torch.zeros(M, 256)
        c.R[rows, (rows * 5 + 2) % 256] = amp.flip(0)
    elif family == "cancel":
        c.A, c.Wo = _pairs(M, 256, 256, g)
        c.A = c.A / 100
    elif family == "constant":
        # the block contributes nothing (W2 = 0, b2 = 0) and its input rows are exactly constant
        c.W2, c.b2 = torch.zeros(256, ff), torch.zeros(256)
        c.Wo, c.bo = torch.zeros(256, 256), torch.zeros(256)
        c.R = _constant_rows(M, 256, g)
        c.pb = torch.full((256,), 0.75)              # LayerNorm_p of a constant row = pb: constant again
    else:
        raise KeyError(family)
    return c


def gather_rows(c, fault=None):
    """The residual rows as the kernels gather them: row i = Rg[r_idx[i]] where r_idx[i] >= 0, else R2[~r_idx[i]]
    (TB_ADD_RESIDUAL in tail_bf16_common.h).  fault: "gather_sign" reads Rg for the negative indices too, "gather_identity"
    ignores r_idx (row i = Rg[i])."""
    if fault == "gather_identity":
        return c.Rg[:c.M]
    ix = c.r_idx.long()
    neg = ix < 0
    pos_ix = torch.where(neg, ~ix, ix)
    second = c.Rg if fault == "gather_sign" else c.R2
    return torch.where(neg[:, None], second[pos_ix], c.Rg[pos_ix])


@functools.lru_cache(maxsize=None)
def tail_mc_case(family, M, ff, n_qkv):
    """tail_case plus what the matrix-core tails' ride and gather forms read: the NEXT layer's q | k | v projection Wq (n_qkv,
    256) / qb, and the residual R scattered over two (M, 256) source matrices Rg / R2 with the index row r_idx (int32; every
    third row lives in R2 and carries ~position, the others in Rg; positions are a seeded permutation, so no row sits at its own
    index once M > 2): gather_rows(c) == c.R bit for bit, which is why the gathered forms share the references of the plain
    ones.  The rows of Rg / R2 that no index names hold OTHER rows of the same family (decoys a wrong gather would read)."""
    base = tail_case(family, M, ff)
    c = SimpleNamespace(**{k: v for k, v in vars(base).items() if not k.startswith("_")})
    g = torch.Generator().manual_seed(_seed(family + "/mc", M, ff, n_qkv))
    c.n_qkv = n_qkv
    c.Wq = torch.randn(n_qkv, 256, generator=g) / 16
    c.qb = torch.randn(n_qkv, generator=g) * 0.2
    pos = torch.randperm(M, generator=g)
    in2 = torch.arange(M) % 3 == 1
    c.Rg = c.R[(torch.arange(M) + 1) % M].clone()
    c.R2 = c.R.flip(0).roll(2, 0).clone()
    c.Rg[pos[~in2]] = c.R[~in2]
    c.R2[pos[in2]] = c.R[in2]
    c.r_idx = torch.where(in2, ~pos, pos).to(torch.int32)
    return c


@functools.lru_cache(maxsize=None)
def ln_case(family, M, dim):
    g = torch.Generator().manual_seed(_seed(family, M, dim))
    c = SimpleNamespace(family=family, M=M, dim=dim, kind="ln")
    c.x = torch.randn(M, dim, generator=g) * 3 + 1
    c.g, c.b = torch.rand(dim, generator=g) + 0.5, torch.randn(dim, generator=g)
    if family in OFFSETS:
        mean, std = OFFSETS[family]
        c.x = mean + std * torch.randn(M, dim, generator=g)
    elif family == "constant":
        c.x = _constant_rows(M, dim, g)
    elif family in ("spike", "spike_t"):
        c.x = _student_t((M, dim), _seed(family, M, dim)) if family == "spike_t" else torch.randn(M, dim, generator=g)
        rows = torch.arange(M)
        c.x[rows, (rows * 53 + dim - 1) % dim] = 1e4
    elif family == "gains":
        c.g, c.b = _hostile_gains(dim, g)
    elif family != "benign":
        raise KeyError(family)
    return c


@functools.lru_cache(maxsize=None)
def l2_case(family, M, dim):
    g = torch.Generator().manual_seed(_seed(family, M, dim))
    x = torch.randn(M, dim, generator=g)
    if family == "spike":
        rows = torch.arange(M)
        x[rows, (rows * 53 + dim - 1) % dim] = 1e4
    elif family == "zero":
        x[::2] = 0
    elif family == "huge":
        x = x.sign() * (x.abs() + 0.5) * 1e15 / 8
    elif family == "minute":
        x = x.sign() * (x.abs() + 0.5) * 1e-15
    elif family != "benign":
        raise KeyError(family)
    return SimpleNamespace(family=family, M=M, dim=dim, x=x, kind="l2")


# ------------------------------------------------------------------------------------------------ arithmetics
def mm64(a, W):
    return a.double() @ W.double().t()


def mm64_bf(a, W):
    return bf(a) @ bf(W).t()


def mm32(a, W):
    return a.float() @ W.float().t()


def mm32_bf(a, W):
    """The single-piece kernels' arithmetic: operands rounded once to bf16, exact products, fp32 accumulation."""
    return a.float().bfloat16().float() @ W.float().bfloat16().float().t()


def split3(x, flush=False):
    """tb_split2: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), as fp32 tensors.  flush: pieces below 2^-126 (subnormal
    bf16) become 0 -- what a matrix core that flushes subnormal operands would see."""
    x = x.float()
    h = x.bfloat16().float()
    r = x - h
    m = r.bfloat16().float()
    l = (r - m).bfloat16().float()
    if flush:
        h, m, l = (torch.where(p.abs() < FP32_MIN, torch.zeros_like(p), p) for p in (h, m, l))
    return h, m, l


def mm_split(a, W, drop=(), flush=False):
    """The six products the split kernels keep, small terms first, fp32 sums.  drop: planted errors ("mm": that product is
    lost; "l": the third piece is lost, i.e. xl wh and xh wl)."""
    ah, am, al = split3(a, flush)
    wh, wm, wl = split3(W, flush)
    terms = [("l", al, wh), ("l", ah, wl), ("mm", am, wm), ("", ah, wm), ("", am, wh), ("", ah, wh)]
    acc = None
    for tag, x, w in terms:
        if tag and tag in drop:
            continue
        p = x @ w.t()
        acc = p if acc is None else acc + p
    return acc


def ln_plain(y, g, b, eps=1e-5, fault=None):
    """Two-pass LayerNorm in y's dtype; fault plants one of the wrong versions of the issue."""
    n = y.shape[-1]
    g, b = g.to(y.dtype), b.to(y.dtype)
    if fault == "gb_swap":
        g, b = b, g
    if fault == "eps6":
        eps = 1e-6
    mean = y.mean(-1, keepdim=True)
    if fault == "one_pass":
        var = (y * y).mean(-1, keepdim=True) - mean * mean
    else:
        var = ((y - mean) ** 2).sum(-1, keepdim=True) / (n - 1 if fault == "div255" else n)
    return (y - mean) / torch.sqrt(var + eps) * g + b


LN_FAULTS = ("one_pass", "eps6", "div255", "gb_swap")
EPI_FAULTS = ("relu_after_res", "bias_last32", "k_swap", "res_row_m1")
SPLIT_FAULTS = ("drop_mm", "drop_l")
RIDE_FAULTS = ("qkv_row_m1", "qkv_from_prenorm", "qkv_bias_last32")
GATHER_FAULTS = ("gather_sign", "gather_identity")
PRE_FAULTS = ("pre_out_normalised", "pre_res_normalised")


def _a_in(c, dt):
    a = c.A.to(dt)
    if c.A2 is not None:
        a2 = c.A2[torch.arange(c.M) % c.a2_mod] if c.a2_mod else c.A2
        a = a + a2.to(dt)
    return a


def _swap_k(W):
    idx = torch.arange(W.shape[1]) ^ 1
    return W[:, idx]


def eval_gemm(c, flags, mm, dt, fault=None):
    """epi((A + A2) W^T + bias) in dtype dt with GEMM arithmetic mm; flags: 1 relu, 2 residual, 4 LayerNorm."""
    W = _swap_k(c.W) if fault == "k_swap" else c.W
    bias = c.bias.to(dt).clone()
    if fault == "bias_last32":
        bias[-32:] = 0
    y = mm(_a_in(c, dt), W).to(dt) + bias
    R = c.R.roll(1, 0) if fault == "res_row_m1" else c.R
    if fault == "relu_after_res" and flags & 1 and flags & 2:
        y = (y + R.to(dt)).clamp(min=0)
    else:
        if flags & 1:
            y = y.clamp(min=0)
        if flags & 2:
            y = y + R.to(dt)
    if flags & 4:
        y = ln_plain(y, c.lg, c.lb, fault=fault if fault in LN_FAULTS else None)
    return y


def eval_tail(c, mm, dt, proj=True, pre=False, fault=None, ride=False, gather=False):
    """The layer tail in dtype dt.  proj: x0 = R + A Wo^T + bo, x1 = LN(x0; pg, pb); post-norm: OUT = LN(x1 + ffn(x1));
    pre-norm: OUT = x0 + ffn(x1), OUT2 = LN(OUT).  Without proj the block input is R.  gather (a tail_mc_case): the residual
    rows are gathered through r_idx from Rg / R2.  ride (post-norm, a tail_mc_case): QKV = OUT Wq^T + qb.
    -> (OUT, OUT2 or None), with ride (OUT, OUT2, QKV)."""
    assert not ride or (proj and not pre), "the ride belongs to the projecting post-norm tail"
    lnf = fault if fault in LN_FAULTS else None
    W1 = _swap_k(c.W1) if fault == "k_swap" else c.W1
    b2 = c.b2.to(dt).clone()
    if fault == "bias_last32":
        b2[-32:] = 0
    R = (gather_rows(c, fault) if gather else c.R).to(dt)
    if proj:
        x0 = R + mm(c.A.to(dt), c.Wo).to(dt) + c.bo.to(dt)
        x1 = ln_plain(x0, c.pg, c.pb, fault=lnf)
        res = x0 if pre and fault != "pre_res_normalised" else x1
    else:
        x1 = res = R
    if fault == "res_row_m1":
        res = res.roll(1, 0)
    h = (mm(x1, W1).to(dt) + c.b1.to(dt)).clamp(min=0)
    y = res + mm(h, c.W2).to(dt) + b2
    if fault == "relu_after_res":
        y = y.clamp(min=0)
    o = ln_plain(y, c.lg, c.lb, fault=lnf)
    if pre:
        return (o if fault == "pre_out_normalised" else y), o
    if not ride:
        return o, None
    src = y if fault == "qkv_from_prenorm" else o.roll(1, 0) if fault == "qkv_row_m1" else o
    qb = c.qb.to(dt).clone()
    if fault == "qkv_bias_last32":
        qb[-32:] = 0
    return o, None, mm(src, c.Wq).to(dt) + qb


def eval_ln(c, dt, fault=None):
    return ln_plain(c.x.to(dt), c.g, c.b, fault=fault)


def eval_l2(x, eps, clamp, dt):
    x = x.to(dt)
    n = (x * x).sum(-1, keepdim=True).sqrt()
    return x / (torch.clamp(n, min=eps) if clamp else n + eps)


# ------------------------------------------------------------------------------------------------ bounds
def flip(v, e):
    """|bf16(v') - bf16(v)| for any v' within e of v: 0 where no rounding boundary lies within e of v, else e + 1.5 spacings."""
    lo = bf(v)
    ulp = torch.clamp(v.abs(), min=FP32_MIN).log2().floor().exp2() * 2.0 ** -7
    to_mid = ulp / 2 - (v - lo).abs()
    return torch.where(to_mid <= e, e + 1.5 * ulp, torch.zeros_like(ulp))


def gemm_delta(a, W, extra, mode, flush=False, da=None):
    """Bound of the pre-LayerNorm value a W^T + (bias, residual: `extra` = the sum of their magnitudes) for operands a, W as
    the reference uses them (float64; already bf16-rounded in mode "bf16").  da: elementwise bound on an error of a."""
    aa, wa = a.abs(), W.abs()
    P = aa @ wa.t()
    nz = (a != 0).double() @ (W != 0).double().t()
    if mode == "split":
        d = (6 * nz + 6) * U * (P + extra) + SPLIT_DROP * P
    else:
        d = (nz + 6) * U * (P + extra)
    if flush:
        d = d + FLUSH * nz * float(wa.max())
    if da is not None:
        d = d + da @ wa.t()
    return d


def ln_ref_bound(y, delta, g, b, own_sum=0.0):
    """float64 LayerNorm of y, its elementwise bound for an input error delta, and the two domain figures.
    Rows with max(delta) / s <= LN_VALID take the doubled first-order bound of the module docstring.  The chained tails leave
    that domain (their worst-case delta passes through |W1| and |W2|), so the other rows take the bound that is not linearised:
    with dc = delta + mean(delta) and ds = sqrt(mean(dc^2)) (the standard deviation is 1-Lipschitz in the RMS norm),
        |d o_i| <= |g_i| (dc_i / (s - ds) + |c_i| ds / (s (s - ds))) + 32 U (|g_i| |c_i| / s + |b_i|),
    valid for ds < s; it is used up to ds <= LN_RIG_VALID s and a row beyond that has NO bound (inf): the CPU suite asserts
    that no case the suites use has such a row, so no element is exempted.
    -> (o, bound, dict(first = worst max(delta) / s, rig = worst ds / s over the rows outside the first-order domain))."""
    g, b = g.double(), b.double()
    mu = y.mean(-1, keepdim=True)
    c = y - mu
    s = ((c * c).mean(-1, keepdim=True) + 1e-5).sqrt()
    ca, ga = c.abs(), g.abs()
    own = 16 * U * (ga * ca / s + b.abs())
    dmean = delta.mean(-1, keepdim=True) + own_sum * U * y.abs().mean(-1, keepdim=True)
    first = 2 * (ga / s * (delta + dmean + ca * (ca * delta).mean(-1, keepdim=True) / s ** 2) + own)
    v = (delta.max(-1, keepdim=True).values + own_sum * U * y.abs().mean(-1, keepdim=True)) / s
    dc = delta + dmean
    ds = (dc * dc).mean(-1, keepdim=True).sqrt()
    room = torch.clamp(s - ds, min=1e-300)
    rig = ga * (dc / room + ca * ds / (s * room)) + 2 * own
    rig = torch.where(ds <= LN_RIG_VALID * s, rig, torch.full_like(rig, float("inf")))
    in_first = v <= LN_VALID
    bound = torch.where(in_first, first, rig)
    out_rows = ~in_first
    info = dict(first=float(v.max()), rig=float((ds / s)[out_rows].max()) if bool(out_rows.any()) else 0.0)
    return c / s * g + b, bound, info


def _worse(a, b):
    return dict(first=max(a["first"], b["first"]), rig=max(a["rig"], b["rig"]))


NO_LN = dict(first=0.0, rig=0.0)


def _rd(mode):
    return bf if mode == "bf16" else torch.Tensor.double


def gemm_ref_bound(c, flags, mode="f32"):
    """-> (float64 reference, elementwise bound, the LayerNorm bound's domain figures: ln_ref_bound)."""
    rd = _rd(mode)
    a, W = rd(_a_in(c, torch.float32)) if mode == "bf16" else _a_in(c, torch.float64), rd(c.W)
    y = a @ W.t() + c.bias.double()
    extra = c.bias.double().abs().expand_as(y)
    if flags & 1:
        y = y.clamp(min=0)
    if flags & 2:
        y = y + c.R.double()
        extra = extra + c.R.double().abs()
    d = gemm_delta(a, W, extra, mode, c.flush)
    if flags & 4:
        return ln_ref_bound(y, d, c.lg, c.lb)
    return y, d, NO_LN


def tail_ref_bound(c, mode="f32", proj=True, pre=False, ride=False):
    """-> dict(OUT=(ref, bound), OUT2=(ref, bound) or None, QKV=(ref, bound) with ride, valid=the worst domain figures over
    the LayerNorms).  A hidden unit whose pre-activation stays below zero under its own bound (p + dh < 0) is exactly 0 in the
    kernel too: it carries no error into the second GEMM (this is what makes `dead` sharp: nothing of the hidden path may leak).
    pre: the fp32 and the single-piece tails have the form (Mode::HAS_PRE); the three-piece split has none and is refused.
    ride (a tail_mc_case; post-norm with proj): QKV = rd(OUT) rd(Wq)^T + qb; the kernel projects its own OUT, which lies within
    OUT's bound of the reference's, so that bound is carried into the GEMM as `da` exactly as dha is into the second GEMM:
    as it is in mode "split", through the one rounding (`flip`) in mode "bf16".  A gathered residual changes nothing here: the
    gathered rows ARE c.R (tail_mc_case)."""
    if pre and mode == "split":
        raise ValueError("the three-piece split tail has no pre-norm form")
    if ride and (pre or not proj):
        raise ValueError("the ride belongs to the projecting post-norm tail")
    rd = _rd(mode)
    valid = NO_LN
    R = c.R.double()
    if proj:
        a, Wo = rd(c.A), rd(c.Wo)
        x0 = R + a @ Wo.t() + c.bo.double()
        d0 = gemm_delta(a, Wo, c.bo.double().abs() + R.abs(), mode)
        x1, e1, v = ln_ref_bound(x0, d0, c.pg, c.pb)
        valid = _worse(valid, v)
        res, eres = (x0, d0) if pre else (x1, e1)
    else:
        x1, e1 = R, torch.zeros_like(R)
        res, eres = x1, e1
    W1, W2 = rd(c.W1), rd(c.W2)
    xa, dxa = (bf(x1), flip(x1, e1)) if mode == "bf16" else (x1, e1)
    p1 = xa @ W1.t() + c.b1.double()
    dh = gemm_delta(xa, W1, c.b1.double().abs().expand_as(p1), mode, da=dxa)
    h = p1.clamp(min=0)
    dh = torch.where(p1 + dh < 0, torch.zeros_like(dh), dh)
    ha, dha = (bf(h), flip(h, dh)) if mode == "bf16" else (h, dh)
    y = res + ha @ W2.t() + c.b2.double()
    dy = eres + gemm_delta(ha, W2, c.b2.double().abs() + res.abs(), mode, da=dha)
    o, bo_, v = ln_ref_bound(y, dy, c.lg, c.lb)
    valid = _worse(valid, v)
    if pre:
        return dict(OUT=(y, dy), OUT2=(o, bo_), valid=valid)
    rb = dict(OUT=(o, bo_), OUT2=None, valid=valid)
    if ride:
        oa, doa = (bf(o), flip(o, bo_)) if mode == "bf16" else (o, bo_)
        Wq = rd(c.Wq)
        q = oa @ Wq.t() + c.qb.double()
        rb["QKV"] = (q, gemm_delta(oa, Wq, c.qb.double().abs().expand_as(q), mode, da=doa))
    return rb


def ln_kernel_ref_bound(c):
    return ln_ref_bound(c.x.double(), torch.zeros_like(c.x, dtype=torch.float64), c.g, c.b, own_sum=LN_OWN_SUM)


def l2_ref_bound(x, eps, clamp):
    x64 = x.double()
    n = (x64 * x64).sum(-1, keepdim=True).sqrt()
    den = torch.clamp(n, min=eps) if clamp else n + eps
    return x64 / den, 8 * U * x64.abs() / den


def in_l2_domain(x):
    nzv = x[x != 0].abs().double()
    return nzv.numel() == 0 or (float(nzv.min()) >= L2_DOMAIN[0] and float(nzv.max()) <= L2_DOMAIN[1])


def pow2_is_safe(c_base, s, pieces=False):
    """The proof that scaling the pow2base case by 2^s is exact, in float64.  Every operand of the base case is a multiple of
    a quantum (2^-10 for A / bias / R, 2^-14 for W), so every product -- also of bf16 pieces, which are multiples of the
    same quanta -- and every partial sum in any order is a multiple of q = 2^-24 and at most S = max(|A||W|^T + |bias| + |R|):
    nothing is subnormal in either run iff q 2^s and q >= 2^-126 (and the smallest scaled operand / piece quantum 2^(s - 10) is
    a normal bf16 / fp32 number), nothing overflows iff S 2^s, max|A| 2^s < 2^127."""
    qa, qw = 2.0 ** -10, 2.0 ** -14
    for t, q in ((c_base.A, qa), (c_base.bias, qa), (c_base.R, qa), (c_base.W, qw)):
        if not torch.equal(torch.round(t.double() / q) * q, t.double()):
            return False
    S = float((c_base.A.double().abs() @ c_base.W.double().abs().t() + c_base.bias.double().abs() + c_base.R.double().abs()).max())
    f = 2.0 ** s
    small = min(qa * qw, qa * qw * f, qa * f)
    big = max(S, S * f, float(c_base.A.abs().max()) * f, float(c_base.R.abs().max()) * f)
    return small >= FP32_MIN and big < FP32_MAX


def worst_ratio(out, ref, bound):
    """max |out - ref| / bound over the elements (0 / 0 = 0; a non-zero error on a zero bound is inf)."""
    err = (out.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------ what the suites run
GEMM_MS = (1, 17, 130, 257)
GEMM_SHAPES = ((256, 256, (0, 1, 2, 3, 4, 5, 6, 7)), (512, 256, (0, 1, 2, 3)), (256, 1024, (0, 1, 2, 3)), (256, 96, (0, 1, 2, 3)))
TAIL_MS = (17, 130)
TAIL_FFS = {"f32": (128, 1024), "split": (64, 128), "bf16": (64, 128)}
LN_DIMS = (256, 260, 768, 1024)
LN_ROWS = 5
ROWS_SPLIT_NS = (64, 768)
GEMM_BF16_SHAPES = ((256, 256), (128, 96))
L2_DIMS = (256, 512, 1024)
L2_FAMILIES = ("benign", "spike", "zero", "huge", "minute")


# the ride, pre-norm and gather forms of the matrix-core tails (tests/test_tail_mc_forms_gpu.py): 130 rows = two tiles on two
# workgroups (un-walked), 677 = 5 * 128 + 37 rows on a grid sized for 2 CUs = three tiles per workgroup, the last one partial
# with five idle waves.  The walked launches run at the ff where the ring phase moves from tile to tile in every form (slots per
# tile G = 8 + ff / 16 + n_qkv / 32 against a ring of 8 (single piece) or 3 (split) slots: MC_WALK_FF).  MC_EDGE: the shipped
# layout (ff, n_qkv), where the split mode's ride fills 157 of the 160 KiB of LDS.
MC_MS = (130, 677)
MC_NQKV = (96, 768)
MC_WALK_FF = {"split": 128, "bf16": 64}
MC_EDGE = (1024, 768)
# At ff = 1024 the worst-case chain through |W1| |W2| leaves benign and cancel rows without a LayerNorm bound (ds / s = 0.98 /
# 1.14 split, 0.74 / 0.87 single piece), so the edge runs the two families whose bound is finite there in both modes and that
# pin the two halves of the launch: `dead` (nothing of the hidden path may leak: bounds of 4e-5 on OUT, 2e-3 on QKV) and `alive`
# (every hidden unit passes; a coarse bound).  Its sharp checks are the bit identities of the GPU suite.
MC_EDGE_FAMILIES = ("dead", "alive")
# FAMILIES_TAIL left out of the matrix-core form tests, by name: `cancel` in mode "split" -- at ff = 128 and 677 rows one row of
# its projecting tail has ds / s = 0.53 > LN_RIG_VALID under the split's worst-case chain, i.e. NO bound, and no case may carry
# such a row.  Nothing is left out in mode "bf16": the ride's bound is finite wherever OUT's is.
MC_LEFT_OUT = {"split": ("cancel",), "bf16": ()}


def mc_families(mode, M):
    return [f for f in tail_families(M) if f not in MC_LEFT_OUT[mode]]


def mc_forms(mode):
    """The forms of the matrix-core tails beyond the plain ones: (name, pre, ride, gather).  The split has no pre-norm kernel."""
    forms = (("ride", False, True, False), ("gather", False, False, True), ("gather ride", False, True, True))
    return forms + ((("pre", True, False, False),) if mode == "bf16" else ())


def mc_runs(mode):
    """(M, ff, n_qkv) of the float64 checks: every ff and ride width un-walked, the walking ff walked."""
    for ff in TAIL_FFS[mode]:
        for nq in MC_NQKV:
            yield MC_MS[0], ff, nq
    for nq in MC_NQKV:
        yield MC_MS[1], MC_WALK_FF[mode], nq


def gemm_families(M, K, flags):
    """The families that apply to one launch of the GEMM: offsets sit on the residual ahead of a LayerNorm (flags 2 | 4),
    gains need the LayerNorm, tiny and pow2 need its absence, onehot needs a row per k index."""
    fams = ["benign", "spike", "spike_t", "cancel"]
    if flags & 4:
        fams.append("gains")
        if flags & 2:
            fams += list(OFFSETS)
    else:
        fams.append("tiny")
    if M >= K:
        fams.append("onehot")
    return fams


def tail_families(M):
    return [f for f in FAMILIES_TAIL if f != "onehot"] + (["onehot"] if M >= 256 else [])


def tail_cases(M):
    """(family, rows) of one tail test at M rows; the largest M also brings the 257-row cases: onehot (a row per k index) and
    the spikes (the outlier channel walks over all 256)."""
    for fam in tail_families(M):
        yield fam, M
    if M == max(TAIL_MS):
        for fam in ("onehot", "spike", "spike_t"):
            yield fam, 257
