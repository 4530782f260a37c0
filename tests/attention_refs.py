"""Plain float64 references and case builders for the attention cores of the shipped 256 / 8-head model (attention.hip,
dec_cross.hip, dec_cross_mfma.hip).  Nothing here imports the library: tests/test_attention_cores_cpu.py validates these
references and proves that the cases can fail, tests/test_attention_cores_gpu.py holds the kernels against them.

Conventions (cone_hip.h): a window b owns the packed tokens off[b] .. off[b + 1], its lv = vlen[b] clips first, then its text
tokens; the position table holds the row of clip p of a window with lv clips at lv (lv - 1) / 2 + p and one all-zero row (the
last); rows are q | k | v of 3 x 256 channels, 8 heads of 32."""
import functools
import math
import types

import numpy as np
import torch

TOL = 2e-5          # the bound of every kernel-level attention test of this project (tests/test_gpu_parity.py)
HEADS, HD, D = 8, 32, 256
MODES = (0, 1, 2, 1 | 4, 2 | 4)         # packed, gather, pos-add, and the two text-position forms
MAX_V_L = 255                           # the largest clip count a 256-token window's table is built for here


def mha64(q, k, v):
    """softmax(q k^T / sqrt(32)) v per head in float64: q (nq, 256), k / v (L, 256) -> (nq, 256)."""
    q, k, v = (torch.as_tensor(t).double() for t in (q, k, v))
    nq, L = q.shape[0], k.shape[0]
    qh = q.reshape(nq, HEADS, HD).transpose(0, 1) / math.sqrt(HD)
    kh = k.reshape(L, HEADS, HD).transpose(0, 1)
    vh = v.reshape(L, HEADS, HD).transpose(0, 1)
    p = torch.softmax(qh @ kh.transpose(1, 2), dim=2)
    return (p @ vh).transpose(0, 1).reshape(nq, D)


def scores64(q, k, head=0):
    """The scaled scores of one head in float64 (what the saturated construction is checked on)."""
    sl = slice(HD * head, HD * head + HD)
    return (torch.as_tensor(q).double()[:, sl] / math.sqrt(HD)) @ torch.as_tensor(k).double()[:, sl].t()


def pos_base(lv):
    return lv * (lv - 1) // 2


def _table(g, lvs, width):
    """A position table for the clip counts ``lvs`` and their neighbours lv +- 1 (the wrong rows of the power test): rows
    of every other clip count stay zero (they are never addressed), the all-zero row is the last one."""
    wmax = min(max(list(lvs) + [1]) + 1, MAX_V_L)
    zrow = pos_base(wmax) + wmax
    pos = torch.zeros(zrow + 1, width)
    for lv in sorted({x for l in lvs for x in (l - 1, l, l + 1) if 1 <= x <= wmax}):
        pos[pos_base(lv):pos_base(lv) + lv] = torch.randn(lv, width, generator=g)
    return pos, zrow


def _scatter_rows(lens, first, gap):
    """Row bases of per-window blocks laid out in REVERSED window order from row ``first`` with ``gap`` spare rows between
    blocks: non-zero and not in window order.  -> (bases, total rows)."""
    bases, at = [0] * len(lens), first
    for b in reversed(range(len(lens))):
        bases[b] = at
        at += lens[b] + gap
    return bases, at


# ------------------------------------------------------------------------------------------------ encoder core
def enc_lengths(n):
    """(clips, text tokens) of the windows of the batch that pins tile count n (Lmax = 16 n exactly): the full window, one
    and three short of it (the second: clips only), one key into the last tile, two into the one before, a window more than
    two tiles short (P.V skips key quads only in the last two tiles), 1 / 4 / 5 / 16 / 17 tokens, text only, clips only and
    clip / text boundaries inside a key quad (lv % 4 != 0)."""
    T = 16 * n
    w = [(T - 25, 25),                       # 16 n; lv = 16 n - 25 is odd: the boundary falls inside a key quad
         (T - 1, 0),                         # 16 n - 1, clips only
         (T - 11, 8),                        # 16 n - 3
         (T - 15 - 20, 20),                  # 16 (n - 1) + 1: one key in the last tile
         (T - 30 - 7, 7),                    # 16 (n - 2) + 2
         (T - 43 - 13, 13),                  # 16 (n - 3) + 5: both last tiles empty
         (1, 0), (0, 1), (0, 4), (3, 2), (16, 0), (12, 5), (8, 9)]
    assert [a + b for a, b in w[:6]] == [T, T - 1, T - 3, T - 15, T - 30, T - 43]
    assert max(a for a, _ in w) <= MAX_V_L
    return w


def _enc_case_from(vl, tl, g):
    B = len(vl)
    L = [a + b for a, b in zip(vl, tl)]
    off = np.concatenate([[0], np.cumsum(L)]).astype(np.int32)
    M = int(off[-1])
    pos, zrow = _table(g, vl, 512)
    vrow0, n_vid = _scatter_rows(vl, 3, 2)
    trow0, n_txt = _scatter_rows(tl, 5, 1)
    return types.SimpleNamespace(
        vl=list(vl), tl=list(tl), L=L, B=B, off=off, M=M, Lmax=max(L), pos=pos, zrow=zrow, vrow0=vrow0, trow0=trow0,
        QKV=torch.randn(M, 768, generator=g), qkv_vid=torch.randn(n_vid, 768, generator=g),
        qkv_txt=torch.randn(n_txt, 768, generator=g), txt_pos=torch.randn(n_txt, 512, generator=g))


@functools.lru_cache(maxsize=3)
def enc_case(n, short=False):
    """The batch of tile count n (``short``: eight one-token windows, Lmax = 1 -- the short-batch ride on the 6-wave build)."""
    g = torch.Generator().manual_seed(1000 + n + (500 if short else 0))
    w = [(1, 0), (0, 1)] * 4 if short else enc_lengths(n)
    c = _enc_case_from([a for a, _ in w], [b for _, b in w], g)
    assert c.Lmax == (1 if short else 16 * n) and 8 <= c.B <= 40
    return c


def enc_rows(mode, c, lv_table=None, p_shift=0):
    """Effective q | k | v rows (M, 768) in float64 of every packed token of case ``c`` in ``mode``: 0 the packed rows as
    they are; 2 the packed rows, 1 rows gathered from the per-clip / per-text-token caches; in both table modes clip p of a
    window with lv clips adds table row lv (lv - 1) / 2 + p to q | k and a text token j adds the zero row -- or, with | 4, its
    own row txt_pos[trow0[b] + j].  ``lv_table`` (per window) / ``p_shift``: the WRONG table rows of the power test -- another
    clip count's, or clip p + p_shift's (clamped to the table)."""
    rows = torch.empty(c.M, 768, dtype=torch.float64)
    for b in range(c.B):
        lv, lt, t0 = c.vl[b], c.tl[b], int(c.off[b])
        if mode & 3 == 1:
            rows[t0:t0 + lv] = c.qkv_vid[c.vrow0[b]:c.vrow0[b] + lv].double()
            rows[t0 + lv:t0 + lv + lt] = c.qkv_txt[c.trow0[b]:c.trow0[b] + lt].double()
        else:
            rows[t0:t0 + lv + lt] = c.QKV[t0:t0 + lv + lt].double()
        if mode & 3:
            base = pos_base(lv if lv_table is None else lv_table[b])
            idx = (base + torch.arange(lv) + p_shift).clamp(0, c.zrow - 1)
            rows[t0:t0 + lv, :512] += c.pos[idx].double()
            rows[t0 + lv:t0 + lv + lt, :512] += (c.txt_pos[c.trow0[b]:c.trow0[b] + lt] if mode & 4
                                                 else c.pos[c.zrow].expand(lt, 512)).double()
    return rows


def enc_window64(r, extra_last=0):
    """Self-attention of one window's effective rows r (L, 768); extra_last = +1: the last key duplicated (the padded copy
    leaking through the mask), -1: the last key dropped."""
    k, v = r[:, 256:512], r[:, 512:]
    if extra_last > 0:
        k, v = torch.cat([k, k[-1:]]), torch.cat([v, v[-1:]])
    elif extra_last < 0:
        k, v = k[:-1], v[:-1]
    return mha64(r[:, :256], k, v)


def enc_ref64(rows, off):
    return torch.cat([enc_window64(rows[off[b]:off[b + 1]]) for b in range(len(off) - 1)])


# ------------------------------------------------------------------------------------------------ saturated scores
SAT_WINDOWS = ((90, 20), (125, 25), (150, 42), (231, 25))       # 110 / 150 / 192 / 256 tokens: NKT 7, 10, 12, 16


@functools.lru_cache(maxsize=4)
def enc_saturated_case(lv, lt):
    """One-window-length batch (eight windows of lv + lt tokens) with the construction of test_streaming_core_saturated_scores
    at head_dim 32: per head a unit direction u, q = a u + noise, k_j = a ramp_j u + noise with ramp rising to 0.9, the last
    key's 1 and the first key's -1, a = sqrt(60 sqrt(32)): scores reach about +-60 and every row's maximum is the last key.
    The rows are the EFFECTIVE ones; the packed rows of the table modes have the table row subtracted (enc_rows adds it
    back, in float64 on the rounded difference -- which the reference follows)."""
    n = lv + lt
    rng = np.random.default_rng(7000 + n)
    B = 8
    eff = np.zeros((B * n, 768), np.float32)
    eff[:, 512:] = (rng.standard_normal((B * n, D)) * 2).astype(np.float32)
    a = np.sqrt(60.0 * np.sqrt(HD))
    ramp = 0.9 * (np.arange(n) + 1.0) / n
    ramp[0], ramp[-1] = -1.0, 1.0
    for h in range(HEADS):
        u = rng.standard_normal(HD)
        u /= np.linalg.norm(u)
        for b in range(B):
            r = slice(b * n, (b + 1) * n)
            eff[r, h * HD:(h + 1) * HD] = a * u + 0.3 * rng.standard_normal((n, HD))
            eff[r, D + h * HD:D + (h + 1) * HD] = a * ramp[:, None] * u + 0.3 * rng.standard_normal((n, HD))
    g = torch.Generator().manual_seed(7000 + n)
    c = _enc_case_from([lv] * B, [lt] * B, g)
    c.QKV = torch.from_numpy(eff)
    c.QKV_table = c.QKV.clone()                   # what mode 2 is handed: effective rows minus the clip rows' table row
    for b in range(B):
        c.QKV_table[b * n:b * n + lv, :512] -= c.pos[pos_base(lv):pos_base(lv) + lv]
    return c


def saturated_rows(mode, c):
    """Effective float64 rows of a saturated case in mode 0 (packed) or 2 (pos-add, on the pre-subtracted rows)."""
    if mode == 0:
        return enc_rows(0, c)
    d = types.SimpleNamespace(**vars(c))
    d.QKV = c.QKV_table
    return enc_rows(2, d)


# ------------------------------------------------------------------------------------------------ folded decoder cross-attention
DEC_LENGTHS = (1, 16, 17, 128, 129, 143, 144, 145, 240, 241, 2, 33, 64, 65, 100, 111, 127, 191)


@functools.lru_cache(maxsize=4)
def dec_case(Lmax, nq=5, shared=False):
    """A batch whose longest window has Lmax tokens, mixing the lengths around the key-tile structure of the matrix-core
    kernels (wave w owns key tiles w and w + 8: 128 | 129, 143 | 144 | 145, 240 | 241, one-key tiles) that fit; text only,
    clips only and mixed windows.  ``shared``: every window has the same query rows (first decoder layer)."""
    g = torch.Generator().manual_seed(9000 + 10 * Lmax + nq + (5 if shared else 0))
    L = [Lmax] + [x for x in DEC_LENGTHS if x < Lmax]
    txt = [20, 0, 1, 3, 0, 25, 7]
    tl = [min(L[i], txt[i % len(txt)]) for i in range(len(L))]
    tl[2] = L[2]                                                   # a window with text only
    vl = [min(a - b, MAX_V_L) for a, b in zip(L, tl)]
    tl = [a - b for a, b in zip(L, vl)]
    B = len(L)
    assert 8 <= B <= 40 and 0 in vl and 0 in tl
    off = np.concatenate([[0], np.cumsum(L)]).astype(np.int32)
    M = int(off[-1])
    pos, zrow = _table(g, vl, D)
    X = torch.randn(M, D, generator=g)
    XP = X + 0.5 * torch.randn(M, D, generator=g)                  # memory + table rows + a perturbation: not derivable from X
    for b in range(B):
        XP[off[b]:off[b] + vl[b]] += pos[pos_base(vl[b]):pos_base(vl[b]) + vl[b]]
    DQ = torch.randn(nq, D, generator=g).repeat(B, 1) if shared else torch.randn(B * nq, D, generator=g)
    return types.SimpleNamespace(
        vl=vl, tl=tl, L=L, B=B, nq=nq, off=off, M=M, Lmax=Lmax, pos=pos, zrow=zrow, X=X, XP=XP, DQ=DQ,
        Wk=torch.randn(D, D, generator=g) / 16, Wv=torch.randn(D, D, generator=g) / 16, bv=torch.randn(D, generator=g),
        sal_w=torch.randn(D, generator=g) / 16, sal_b=torch.randn(1, generator=g))


def dec_window64(c, b, use_xp=False, lv_table=None, extra_last=0):
    """The fold written out for window b: K = (mem + pos) Wk^T -- with ``use_xp`` K = XP Wk^T --, V = mem Wv^T + bv, then the
    plain attention of the window's nq query rows.  lv_table / extra_last: the wrong versions of the power test."""
    mem = c.X[c.off[b]:c.off[b + 1]].double()
    lv = c.vl[b]
    if use_xp:
        keys = c.XP[c.off[b]:c.off[b + 1]].double()
    else:
        keys = mem.clone()
        base = pos_base(lv if lv_table is None else lv_table)
        keys[:lv] += c.pos[base:base + lv].double()
    K = keys @ c.Wk.double().t()
    V = mem @ c.Wv.double().t() + c.bv.double()
    if extra_last > 0:
        K, V = torch.cat([K, K[-1:]]), torch.cat([V, V[-1:]])
    elif extra_last < 0:
        K, V = K[:-1], V[:-1]
    return mha64(c.DQ[b * c.nq:(b + 1) * c.nq], K, V)


def dec_cross64(c, use_xp=False):
    """-> (OUT (B nq, 256), sal): sal[b] (lv,) = mem[p] . sal_w + sal_b on the RAW memory rows of the window's clips."""
    out = torch.cat([dec_window64(c, b, use_xp) for b in range(c.B)])
    sal = [c.X[c.off[b]:c.off[b] + c.vl[b]].double() @ c.sal_w.double() + c.sal_b.double() for b in range(c.B)]
    return out, sal


# ------------------------------------------------------------------------------------------------ the decoder's small attentions
SMALL_KEYS = (1, 63, 64, 65, 127, 128, 129, 191, 192)
SMALL_ND = 2                    # decoder layers: K / V of every layer side by side, ld = 256 nd; the second layer's slice is used


@functools.lru_cache(maxsize=8)
def small_cross_case(nq):
    g = torch.Generator().manual_seed(8000 + nq)
    L = list(SMALL_KEYS)
    off = np.concatenate([[0], np.cumsum(L)]).astype(np.int32)
    M = int(off[-1])
    return types.SimpleNamespace(L=L, B=len(L), nq=nq, off=off, M=M, Lmax=max(L), Q=torch.randn(len(L) * nq, D, generator=g),
                                 KD=torch.randn(M, D * SMALL_ND, generator=g), VD=torch.randn(M, D * SMALL_ND, generator=g))


def small_cross_window64(c, b, extra_last=0):
    k = c.KD[c.off[b]:c.off[b + 1], D:2 * D]
    v = c.VD[c.off[b]:c.off[b + 1], D:2 * D]
    if extra_last > 0:
        k, v = torch.cat([k, k[-1:]]), torch.cat([v, v[-1:]])
    elif extra_last < 0:
        k, v = k[:-1], v[:-1]
    return mha64(c.Q[b * c.nq:(b + 1) * c.nq], k, v)


SMALL_SELF_B = (1, 3, 4, 5, 9)  # four windows per workgroup of dec_self_attn_kernel: partial last workgroups


@functools.lru_cache(maxsize=16)
def small_self_case(nq):
    """Packed q | k | v slot rows (9 nq, 768): window b owns rows b nq .. (b + 1) nq; a batch of B windows is its first B nq."""
    g = torch.Generator().manual_seed(8500 + nq)
    return torch.randn(max(SMALL_SELF_B) * nq, 768, generator=g)


def small_self_window64(qkv, nq, b, extra_last=0):
    return enc_window64(qkv[b * nq:(b + 1) * nq].double(), extra_last)
