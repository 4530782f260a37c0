"""References, case families and planted-error models for the glue kernels of stage B: the window bookkeeping (scan, compaction,
row index, window table, mask lengths), the packing kernels, the sine position tables and their projected images, the text
position rows, the saliency / memory taps, the 1-2 output heads and the row tilers (window_ops.hip, rowops.hip and their
d-wide copies in general.hip).  Used by tests/test_glue_kernels_cpu.py (the references deserve trust, every planted error is
seen) and tests/test_glue_kernels_gpu.py (the kernels, through the launchers the forward path calls).

Plain numpy on the CPU.  Integer results are exact, float results are float64.  Nothing here is measured on a kernel.

Bounds
------
Integers, gathers, copies: exact (bit compare).
Dots and GEMM rows: tests/row_refs.py (gemm_delta: (nz + 6) U (|a| |w| + |bias|)), no new constant.
Sigmoid of a dot: the sigmoid is 1/4-Lipschitz, so the dot's bound / 4, plus 2 U for exp, the add and the quotient.
LayerNorm(x + E[j]): row_refs.ln_ref_bound with the input error of the one fp32 add, U |x + E[j]|, and the kernel's own mean.
Sine rows: the kernels build the fp32 argument with one IEEE rounding per operation ((p + 1) / (lv + 1e-6f) * 2 pi, / dim_t[c];
__fdiv_rn / __fmul_rn / __fadd_rn), which numpy's float32 scalar arithmetic reproduces bit for bit; sine_rows64 takes sin / cos
of THAT fp32 argument in float64.  What is left to the device is its sinf / cosf.  Their distance to float64 has not been
measured on the device and is not taken from it: the bound is SINE_FACTOR = 8 times the worst distance of the CPU's fp32
sin / cos (torch) to float64 on the table's own arguments (sine_cpu_error: about 3.6e-8 = 0.6 U, so about 2.9e-7) -- a device
math library is allowed a few ulps where the CPU's stays under one.  The CPU suite asserts that the smallest planted error
(a neighbouring lv at equal p: about 6.0e-6) is at least 10 bounds away."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

U = 2.0 ** -24
F = np.float32
SINE_FACTOR = 8.0
SINE_LVS = tuple(range(1, 256)) + (256, 511, 700, 1000, 1023)
LONG_LVS = (256, 511, 1000, 1023)
POISON_BITS = 0x7FC5A5A5            # a quiet NaN with a payload as fp32; 2143659429 as int32: no index, length or offset here


# ------------------------------------------------------------------------------------------------ poison
def poison(*shape, dtype=torch.float32, device="cpu"):
    """A buffer whose every 32-bit element holds POISON_BITS (a NaN pattern for floats)."""
    t = torch.full(tuple(shape), POISON_BITS, dtype=torch.int32, device=device)
    return t if dtype == torch.int32 else t.view(dtype)


def bits(t):
    """The 32-bit patterns of a tensor / array as a numpy int32 array."""
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().contiguous().view(torch.int32).numpy()
    a = np.ascontiguousarray(t)
    return a.view(np.int32)


def untouched(t, written=None):
    """True iff every element of t OUTSIDE the boolean mask `written` (None: nothing was to be written) still holds the poison
    bit for bit."""
    b = bits(t)
    keep = np.ones(b.shape, bool) if written is None else ~np.broadcast_to(np.asarray(written, bool), b.shape)
    return bool((b[keep] == np.int32(POISON_BITS)).all())


def same_bits(a, b):
    return bits(a).shape == bits(b).shape and bool((bits(a) == bits(b)).all())


# ------------------------------------------------------------------------------------------------ integer kernels
def scan_ref(vlen, qlen=None):
    """off[0 .. B]: exclusive prefix sum of vlen (+ qlen)."""
    v = np.asarray(vlen, np.int64) + (0 if qlen is None else np.asarray(qlen, np.int64))
    return np.concatenate([[0], np.cumsum(v)]).astype(np.int32)


def compact_ref(vlen, qlen, Lv_pad, Lq_pad):
    """(voff, toff, vidx, tidx): the offsets are the scans of the lengths, the lists hold the source row b * Lpad + p of every
    valid row in window order (lengths <= the padding, the contract of cone_forward_windows)."""
    vlen, qlen = np.asarray(vlen, np.int64), np.asarray(qlen, np.int64)
    assert (vlen <= Lv_pad).all() and (qlen <= Lq_pad).all()
    vidx = [b * Lv_pad + p for b in range(len(vlen)) for p in range(vlen[b])]
    tidx = [b * Lq_pad + p for b in range(len(qlen)) for p in range(qlen[b])]
    return scan_ref(vlen), scan_ref(qlen), np.asarray(vidx, np.int32).reshape(-1), np.asarray(tidx, np.int32).reshape(-1)


def row_index_ref(vrow0, vlen, trow0, qlen):
    """Source row of every packed token: a clip row r as r, a text row r as ~r."""
    out = []
    for b in range(len(vlen)):
        out += [int(vrow0[b]) + p for p in range(int(vlen[b]))]
        out += [~(int(trow0[b]) + t) for t in range(int(qlen[b]))]
    return np.asarray(out, np.int32).reshape(-1)


def gather_rows(vrow0, vlen, trow0, qlen):
    """(is_clip, source row, position p, window length lv) of every packed token."""
    kind, src, pos, lvs = [], [], [], []
    for b in range(len(vlen)):
        lv, lq = int(vlen[b]), int(qlen[b])
        kind += [True] * lv + [False] * lq
        src += [int(vrow0[b]) + p for p in range(lv)] + [int(trow0[b]) + t for t in range(lq)]
        pos += list(range(lv)) + list(range(lq))
        lvs += [lv] * (lv + lq)
    return np.asarray(kind, bool), np.asarray(src, np.int64), np.asarray(pos, np.int64), np.asarray(lvs, np.int64)


def mask_lengths_ref(mask):
    return np.asarray(mask, np.float64).sum(1).astype(np.int32)


def tile_ref(src, n_rows):
    """rows r of the tiled matrix = row r % period of the `period` source rows."""
    src = np.asarray(src)
    return src[np.arange(n_rows) % src.shape[0]]


def window_table_ref(win_idx, q_ctx_l, q_vid_off, tok_off, tok_len, q_base, eval_bsz, W, n_batches, row_q=None, row_slot=None,
                     batch_pad=None):
    """The eval branch of the dataset + collate, restated row by row: query q's slot-th selected window wi covers clips
    [max((wi - 1) S, 0), min((wi - 1) S + W, ctx_l)) with S = int(W / 2) (window 0 is the half window ahead of the video); the
    reference batches eval_bsz consecutive queries OF THE SPLIT (query q of this view is query q + q_base of the split) and
    pads every window of a batch to the batch's longest.  batch_pad None: derived from the rows given (batches without a row:
    0); otherwise the split's table, which is returned unchanged.  -> dict of the seven columns + batch_pad, int32."""
    win_idx = np.asarray(win_idx)
    nq, K = win_idx.shape
    if row_q is None:
        rows = [(q, s) for q in range(nq) for s in range(K)]
    else:
        rows = list(zip(np.asarray(row_q).tolist(), np.asarray(row_slot).tolist()))
    S = int(W / 2)
    col = {k: [] for k in ("vid_row0", "vid_len", "video_start", "txt_row0", "txt_len", "cls_row")}
    batch_of = []
    for q, s in rows:
        wi = int(win_idx[q, s])
        start, end = max((wi - 1) * S, 0), min((wi - 1) * S + W, int(q_ctx_l[q]))
        col["vid_row0"].append(int(q_vid_off[q]) + start)
        col["vid_len"].append(end - start)
        col["video_start"].append(start)
        col["txt_row0"].append(int(tok_off[q]))
        col["txt_len"].append(int(tok_len[q]))
        col["cls_row"].append(q)
        batch_of.append((q + q_base) // eval_bsz)
    if batch_pad is None:
        pad = [0] * n_batches
        for bid in sorted(set(batch_of)):       # one reference batch at a time
            pad[bid] = max([0] + [v for v, b in zip(col["vid_len"], batch_of) if b == bid])
    else:
        pad = [int(v) for v in batch_pad]
    col["pad_len"] = [pad[b] for b in batch_of]
    out = {k: np.asarray(v, np.int32).reshape(-1) for k, v in col.items()}
    out["batch_pad"] = np.asarray(pad, np.int32)
    return out


# ------------------------------------------------------------------------------------------------ sine rows
def dim_t32(d, temperature=10000.0):
    """temperature ** (2 (i // 2) / d) as the reference states it, in fp32 (torch's arithmetic: the table the model hands the
    library is built by this formula and a wrong one on the handle shows against the rows below)."""
    i = torch.arange(d, dtype=torch.float32)
    return (temperature ** (2 * (i // 2) / d)).numpy()


def sine_args32(lv, d, temperature=10000.0, p_shift=0, lv_shift=0):
    """The fp32 argument of every (p, c), one rounding per operation.  p_shift / lv_shift: planted errors."""
    p = np.arange(lv, dtype=np.float32) + F(1 + p_shift)
    den = F(lv + lv_shift) + F(1e-6)
    xe = (p / den).astype(np.float32) * F(6.283185307179586)
    return (xe[:, None] / dim_t32(d, temperature)[None, :]).astype(np.float32)


def sine_rows64(lv, d, temperature=10000.0, p_shift=0, lv_shift=0):
    """PositionEmbeddingSine(normalize=True) of a window of lv clips: (lv, d) float64, channel c even: sin, odd: cos, of the
    fp32 argument the kernels build."""
    a = sine_args32(lv, d, temperature, p_shift, lv_shift).astype(np.float64)
    out = np.empty_like(a)
    out[:, 0::2] = np.sin(a[:, 0::2])
    out[:, 1::2] = np.cos(a[:, 1::2])
    return out


@functools.lru_cache(maxsize=None)
def table_rows64(max_v_l, d):
    """The sine table: rows (lv, p), p < lv <= max_v_l, at lv (lv - 1) / 2 + p, then the all-zero row."""
    rows = [sine_rows64(lv, d) for lv in range(1, max_v_l + 1)] + [np.zeros((1, d))]
    return np.concatenate(rows, 0)


def table_row_count(max_v_l):
    return max_v_l * (max_v_l + 1) // 2 + 1


def sine_cpu_error(lvs=SINE_LVS, d=256):
    """Worst |fp32 sin / cos of the CPU (torch) - float64| over the arguments of the given window lengths."""
    worst = 0.0
    for lv in lvs:
        a = sine_args32(lv, d)
        t = torch.from_numpy(a)
        got = np.empty(a.shape, np.float64)
        got[:, 0::2] = t[:, 0::2].sin().double().numpy()
        got[:, 1::2] = t[:, 1::2].cos().double().numpy()
        worst = max(worst, float(np.abs(got - sine_rows64(lv, d)).max()))
    return worst


@functools.lru_cache(maxsize=None)
def sine_bound():
    """SINE_FACTOR times the CPU's own fp32 error on the table's arguments (module docstring)."""
    return SINE_FACTOR * sine_cpu_error()


def pos_qk64(rows64, in_proj_weights):
    """rows [W_q | W_k]^T of every encoder layer (the first 2 d rows of its in_proj_weight), no bias: (layers, R, 2 d)."""
    d = rows64.shape[1]
    return np.stack([rows64 @ np.asarray(w, np.float64)[:2 * d].T for w in in_proj_weights])


# ------------------------------------------------------------------------------------------------ float kernels
def txt_index(tok_index, src_row, mod, n_emb, n, n_dev=None, mut=None):
    """(count, j[count]) of the text position kernels: rows below min(n_dev, n), index tok_index[i] or src_row[i] % mod, clamped
    to [0, n_emb - 1].  mut: "div_for_mod", "no_clamp", "n_dev_ignored"."""
    count = n if (n_dev is None or mut == "n_dev_ignored") else min(int(n_dev), n)
    if tok_index is not None:
        j = np.asarray(tok_index, np.int64)[:count]
    elif mut == "div_for_mod":
        j = np.asarray(src_row, np.int64)[:count] // mod
    else:
        j = np.asarray(src_row, np.int64)[:count] % mod
    if mut != "no_clamp":
        j = np.clip(j, 0, n_emb - 1)
    return count, j


def txt_pos64(x, E, j, g, b, eps=1e-5):
    """LayerNorm(x + E[j]) in float64 (j already clamped: txt_index)."""
    y = np.asarray(x, np.float64) + np.asarray(E, np.float64)[j]
    mu = y.mean(-1, keepdims=True)
    c = y - mu
    return c / np.sqrt((c * c).mean(-1, keepdims=True) + eps) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def saliency64(MEM, off, vlen, w, bias, Lv_out):
    """(B, Lv_out) float64: <memory row of clip p, w> + bias for p < vlen[b], 0 in the padding."""
    MEM, w = np.asarray(MEM, np.float64), np.asarray(w, np.float64).reshape(-1)
    out = np.zeros((len(vlen), Lv_out))
    for b in range(len(vlen)):
        lv = int(vlen[b])
        out[b, :lv] = MEM[off[b]:off[b] + lv] @ w + float(np.asarray(bias).reshape(-1)[0])
    return out


def mem_tap_ref(MEM, off, vlen, qlen, Lv_out, Lq_out, mut=None):
    """(B, Lv_out + Lq_out, d) fp32: the window's clip rows, zero rows, its token rows, zero rows.  mut "txt_shift": the text
    half read lv rows too early."""
    MEM = np.asarray(MEM, np.float32)
    out = np.zeros((len(vlen), Lv_out + Lq_out, MEM.shape[1]), np.float32)
    for b in range(len(vlen)):
        lv, lq, o = int(vlen[b]), int(qlen[b]), int(off[b])
        out[b, :lv] = MEM[o:o + lv]
        t0 = o if mut == "txt_shift" else o + lv
        out[b, Lv_out:Lv_out + lq] = MEM[t0:t0 + lq]
    return out


def rowdot64(X, W, b, act):
    """act(X W^T + b) in float64; act 1: the sigmoid.  -> (value, the pre-activation)."""
    s = np.asarray(X, np.float64) @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
    if act == 1:
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(-s)), s
    return s, s


def dot_bound(X, W, b):
    """row_refs.gemm_delta of X W^T + b: (nz + 6) U (|X| |W|^T + |b|)."""
    import row_refs as R
    X, W = torch.as_tensor(np.asarray(X, np.float64)), torch.as_tensor(np.asarray(W, np.float64))
    extra = torch.as_tensor(np.abs(np.asarray(b, np.float64))).expand(X.shape[0], W.shape[0])
    return R.gemm_delta(X, W, extra, "f32").numpy()


def rowdot_bound(X, W, b, act):
    d = dot_bound(X, W, b)
    return d / 4 + 2 * U if act == 1 else d


# ------------------------------------------------------------------------------------------------ python models (planted errors)
def scan_model(vlen, qlen=None, mut=None):
    """scan_lengths_kernel lane by lane: 16 waves, wave w owns windows [w per, (w + 1) per), per = ceil(ceil(B / 16) / 64) 64.
    mut "base_block": a wave's base misses the last 64-window block of the waves before it."""
    v = np.asarray(vlen, np.int64) + (0 if qlen is None else np.asarray(qlen, np.int64))
    B = len(v)
    per = (((B + 15) // 16 + 63) // 64) * 64
    off = np.zeros(B + 1, np.int64)
    wsum = []
    for w in range(16):
        b0 = min(w * per, B)
        wsum.append(int(v[b0:min(b0 + per, B)].sum()))
    for w in range(16):
        b0 = min(w * per, B)
        b1 = min(b0 + per, B)
        run = sum(wsum[:w])
        if mut == "base_block" and w > 0:
            run -= int(v[max(b0 - 64, 0):b0].sum())
        if w == 15:
            off[B] = run + wsum[15]
        for base in range(b0, b1, 64):
            blk = v[base:min(base + 64, b1)]
            off[base:base + len(blk)] = run + np.cumsum(blk) - blk
            run += int(blk.sum())
    return off.astype(np.int32)


def batch_max_model(vid_len, bid, n_batches, mut=None):
    """window_table_kernel's batch maximum wave by wave: every wave of 64 rows visits the reference batches it holds, first lane
    first, and folds one maximum per (wave, batch).  mut "drop_second": the second batch of a wave is skipped (what a ballot
    loop that clears one bit too many does); "clear_lowest": the loop clears only its leader's own bit (todo &= todo - 1), so
    every lane of a batch leads in turn and folds the same maximum again -- more atomics, the same table."""
    pad = [0] * n_batches
    for w0 in range(0, len(bid), 64):
        seen = []
        for b in bid[w0:w0 + 64]:
            if b not in seen:
                seen.append(b)
        if mut == "clear_lowest":           # the loop clears only its leader's bit: every lane leads once, batches repeat
            seen = list(bid[w0:w0 + 64])
        for k, b in enumerate(seen):
            if mut == "drop_second" and k == 1:
                continue
            pad[b] = max(pad[b], max(v for v, bb in zip(vid_len[w0:w0 + 64], bid[w0:w0 + 64]) if bb == b))
    return np.asarray(pad, np.int32)


# ------------------------------------------------------------------------------------------------ case families
def _rng(*key):
    return np.random.default_rng(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) + 12345)


SCAN_BS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 20000)
SCAN_KINDS = ("random", "zero", "max")
COMPACT_PADS = tuple((lv, lq) for lv in (1, 255, 256, 257) for lq in (1, 32))


def scan_case(B, kind):
    """(vlen, qlen) in 0 .. 255: random (zeros and 255s among them), all zero, all 255."""
    rng = _rng(B, len(kind))
    if kind == "zero":
        return np.zeros(B, np.int32), np.zeros(B, np.int32)
    if kind == "max":
        return np.full(B, 255, np.int32), np.full(B, 255, np.int32)
    v, q = rng.integers(0, 256, B).astype(np.int32), rng.integers(0, 256, B).astype(np.int32)
    v[::7], q[::5] = 0, 255
    v[-1] = 255
    return v, q


def compact_case(B, Lv_pad, Lq_pad):
    """Lengths in [0, pad] with windows of length 0 and of length pad on both sides."""
    rng = _rng(B, Lv_pad, Lq_pad)
    v, q = rng.integers(0, Lv_pad + 1, B).astype(np.int32), rng.integers(0, Lq_pad + 1, B).astype(np.int32)
    v[0], q[0] = Lv_pad, 0
    if B > 1:
        v[-1], q[-1] = 0, Lq_pad
    if B > 2:
        v[B // 2], q[B // 2] = Lv_pad, Lq_pad
    return v, q


# windows (lv, lq) of the packing family: one clip + one token, no clips, no tokens, an empty window, lv + lq on both sides of a
# multiple of 4 (tokens per workgroup) and of 256 (row_index: rows per workgroup), the longest one last but one
PACK_WINDOWS = ((1, 1), (0, 3), (4, 0), (0, 0), (2, 1), (2, 2), (3, 2), (90, 20), (200, 55), (200, 56), (255, 2), (17, 20), (6, 1))
PACK_LMAX = 257


def pack_case(d, windows=PACK_WINDOWS, n_clips=300, n_tok=64, seed=0):
    """A packed batch over a clip arena and a token arena of width d (windows overlap in both, like a query's windows)."""
    rng = _rng(d, len(windows), seed)
    g = torch.Generator().manual_seed(1000 + d + seed)
    c = SimpleNamespace(d=d, B=len(windows))
    c.vlen = np.asarray([w[0] for w in windows], np.int32)
    c.qlen = np.asarray([w[1] for w in windows], np.int32)
    n_clips, n_tok = max(n_clips, int(c.vlen.max())), max(n_tok, int(c.qlen.max()))
    c.vrow0 = np.asarray([rng.integers(0, n_clips - lv + 1) for lv in c.vlen], np.int32)
    c.trow0 = np.asarray([rng.integers(0, n_tok - lq + 1) for lq in c.qlen], np.int32)
    c.vproj = torch.randn(n_clips, d, generator=g).numpy()
    c.tproj = torch.randn(n_tok, d, generator=g).numpy()
    c.off = scan_ref(c.vlen, c.qlen)
    c.M = int(c.off[-1])
    c.Lmax = int((c.vlen + c.qlen).max())
    c.kind, c.src, c.pos, c.lv = gather_rows(c.vrow0, c.vlen, c.trow0, c.qlen)
    return c


def pack_x_ref(c):
    """X: a pure gather (fp32 bits)."""
    X = np.empty((c.M, c.d), np.float32)
    X[c.kind] = c.vproj[c.src[c.kind]]
    X[~c.kind] = c.tproj[c.src[~c.kind]]
    return X


def pack_pos64(c):
    """POS without text positions: the sine row of every clip token, zeros for a text token."""
    P = np.zeros((c.M, c.d))
    for b in range(c.B):
        lv = int(c.vlen[b])
        if lv:
            P[c.off[b]:c.off[b] + lv] = sine_rows64(lv, c.d)
    return P


TXT_NS = (1, 3, 4, 5, 257)
TXT_MODS = (1, 7, 32)
TXT_N_EMB = 32


def txt_case(d, n):
    """Projected token rows, an embedding table of TXT_N_EMB rows, LayerNorm gains; the last two rows (n >= 3) are a
    near-constant row and an outlier-channel row of row_refs.ln_case, on embedding row 1, which is tiny."""
    import row_refs as R
    g = torch.Generator().manual_seed(77 + d * 1000 + n)
    c = SimpleNamespace(d=d, n=n, n_emb=TXT_N_EMB)
    c.x = torch.randn(n, d, generator=g) * 1.5
    c.E = torch.randn(TXT_N_EMB, d, generator=g) * 0.5
    c.E[1] = torch.randn(d, generator=g) * 2.0 ** -14
    c.g, c.b = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g)
    rng = _rng(d, n)
    tok = rng.integers(0, TXT_N_EMB, n)
    hostile = [0, TXT_N_EMB - 1, TXT_N_EMB, TXT_N_EMB + 100, -1, -1000]       # the two ends, past the table, below zero
    for i, v in enumerate(hostile[:n]):
        tok[(i * 3) % n] = v
    c.src_row = rng.integers(0, 5000, n).astype(np.int32)
    c.src_row[0] = 0
    if n >= 3:
        c.x[n - 2] = R.ln_case("nearconst", 4, d).x[1]
        c.x[n - 1] = R.ln_case("spike", 4, d).x[2]
        tok[n - 2] = tok[n - 1] = 1
    c.tok = tok.astype(np.int32)
    c.hostile_rows = (n - 2, n - 1) if n >= 3 else ()
    return c


def txt_ref_bound(c, j):
    """float64 LayerNorm(x + E[j]) of the case's first len(j) rows and its elementwise bound (row_refs.ln_ref_bound; the input
    error is the rounding of the one add)."""
    import row_refs as R
    y = c.x[:len(j)].double() + c.E.double()[torch.as_tensor(np.asarray(j, np.int64))]
    return R.ln_ref_bound(y, U * y.abs(), c.g, c.b, own_sum=R.LN_OWN_SUM)


HEAD_ROWS = (1, 3, 4, 5, 1025)
SAT_LOGITS = (30.0, -30.0, 90.0, -90.0)


def head_case(d, n_rows, nout, ldx_extra=8, seed=0):
    """X (n_rows, d + ldx_extra) with poison in the gap columns, W (nout, d), b; the first rows (as many as fit) are scaled so
    that output 0 lands near +-30 and +-90 (the sigmoid's saturation), next to benign rows."""
    g = torch.Generator().manual_seed(31 * d + 7 * n_rows + nout + seed)
    c = SimpleNamespace(d=d, n_rows=n_rows, nout=nout, ldx=d + ldx_extra)
    c.W = (torch.randn(nout, d, generator=g) / d ** 0.5).numpy()
    c.b = (torch.randn(nout, generator=g) * 0.3).numpy()
    x = torch.randn(n_rows, d, generator=g).numpy()
    w0 = c.W[0].astype(np.float64)
    c.sat = []
    for i, t in enumerate(SAT_LOGITS):
        r = 2 * i + 1           # odd rows: benign neighbours on both sides
        if r < n_rows:
            x[r] = ((t - float(c.b[0])) * w0 / (w0 @ w0)).astype(np.float32)
            c.sat.append((r, t))
    c.x = x
    buf = np.full((n_rows, c.ldx), np.int32(POISON_BITS), np.int32).view(np.float32)
    buf[:, :d] = x
    c.xbuf = buf
    return c


TILE_PERIODS = (1, 5, 10, 16)


def tile_rows_of(period):
    return (period, period + 1, 4 * period + 3, 1000)


MASK_LS = (1, 63, 64, 65, 255)
MASK_BS = (1, 4, 5, 257)


def mask_case(B, L, kind):
    rng = _rng(B, L, len(kind))
    n = {"ones": np.full(B, L), "zeros": np.zeros(B, np.int64), "prefix": rng.integers(0, L + 1, B)}[kind]
    return (np.arange(L)[None, :] < n[:, None]).astype(np.float32)


# --- window table
WT_WS = (90, 125)
WT_BATCHING = ((1, 1), (4, 4), (3, 5), (100, 20))
WT_NQ = 70


def wt_video_lengths(W):
    """One clip, around the stride, around the window, 3 S + 1, and one video long enough to own 20 windows."""
    S = int(W / 2)
    return [1, S - 1, S, S + 1, W - 1, W, W + 1, 3 * S + 1, 19 * S + 1]


def wt_q_bases(eval_bsz):
    return sorted({0, 1, eval_bsz - 1, eval_bsz})


def wt_case(W, eval_bsz, K, nq=WT_NQ, sparse=False):
    """Crafted metadata of nq queries over the video-length family; every query selects window 0, the last window and the one
    before it first, then the rest in a shuffled order (dense: K entries per query, drawn with repetition where the video
    owns fewer windows; sparse: the row_q / row_slot list of min(K, windows of the video) rows per query)."""
    S = int(W / 2)
    rng = _rng(W, eval_bsz, K, int(sparse))
    lens = wt_video_lengths(W)
    c = SimpleNamespace(W=W, eval_bsz=eval_bsz, K=K, nq=nq)
    ctx = np.asarray([lens[(q * 3 + q // len(lens)) % len(lens)] for q in range(nq)], np.int32)
    c.q_ctx_l = ctx
    c.q_vid_off = (np.concatenate([[0], np.cumsum(ctx)[:-1]]) + 11).astype(np.int32)
    c.tok_len = rng.integers(1, 26, nq).astype(np.int32)
    c.tok_off = (np.concatenate([[0], np.cumsum(c.tok_len)[:-1]]) + 5).astype(np.int32)
    nwin = -(-ctx.astype(np.int64) // S) + 1
    win = np.full((nq, K), -1, np.int32)
    rq, rs = [], []
    for q in range(nq):
        n = int(nwin[q])
        first = [0, n - 1, max(n - 2, 0)]
        rest = [w for w in rng.permutation(n).tolist() if w not in first]
        order = (list(dict.fromkeys(first)) + rest)
        order = order[q % 3:] + order[:q % 3]       # the edge windows do not always sit in slot 0
        own = min(K, n)
        if sparse:
            win[q, :own] = order[:own]
            rq += [q] * own
            rs += list(range(own))
        else:
            win[q] = [order[i % n] for i in range(K)]
    c.win_idx = win
    c.row_q = np.asarray(rq, np.int32) if sparse else None
    c.row_slot = np.asarray(rs, np.int32) if sparse else None
    c.n_rows = len(rq) if sparse else nq * K
    c.nwin = nwin
    return c


def wt_view(c, q_base, n_split_extra=0):
    """(n_batches of the split, kwargs of window_table_ref) for the view that starts at split query q_base."""
    nb = (q_base + c.nq + c.eval_bsz - 1) // c.eval_bsz + n_split_extra
    return nb, dict(win_idx=c.win_idx, q_ctx_l=c.q_ctx_l, q_vid_off=c.q_vid_off, tok_off=c.tok_off, tok_len=c.tok_len, q_base=q_base,
                    eval_bsz=c.eval_bsz, W=c.W, n_batches=nb, row_q=c.row_q, row_slot=c.row_slot)


# --- saliency
SAL_WINDOWS = ((5, 3), (0, 4), (7, 0), (0, 0), (1, 1), (64, 20), (33, 7), (4, 4))


def sal_case(d, windows=SAL_WINDOWS):
    g = torch.Generator().manual_seed(500 + d)
    c = SimpleNamespace(d=d, B=len(windows))
    c.vlen = np.asarray([w[0] for w in windows], np.int32)
    c.qlen = np.asarray([w[1] for w in windows], np.int32)
    c.off = scan_ref(c.vlen, c.qlen)
    c.M = int(c.off[-1])
    # (lv_max + 8 rows behind the batch that no window owns: a kernel that forgets a guard then reads defined memory)
    c.MEM = torch.randn(c.M + int(c.vlen.max()) + 8, d, generator=g).numpy()
    c.w = (torch.randn(1, d, generator=g) / d ** 0.5).numpy()
    c.bias = np.asarray([0.37], np.float32)
    c.lv_max, c.lq_max = int(c.vlen.max()), int(c.qlen.max())
    return c
