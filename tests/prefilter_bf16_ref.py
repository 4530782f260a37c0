"""CPU restatement of the opt-in bf16 pre-filter's contract (include/cone_hip.h, "OPT-IN bf16 pre-filter"), in float64.

    score[q][f] = sum_c bf16(ctx[f][c]) * bf16(cls[q][c])        both operands rounded once, to nearest even
    win[q][i]   = max of score[q][f] over frames [max((i-1)S, 0), min((i-1)S + W, ctx_l)),  S = W // 2,
                  i = 0 .. ceil(ctx_l / S)          (num_window = ceil(ctx_l / S) + 1)

The window rule is written out twice: over the frame range (``window_scores``) and the way the header states the kernels
compute it -- half-window maxima hm[h] over frames [hS, (h+1)S), win[i] = max(hm[i-1], hm[i], W odd ? score[(i+1)S] : -inf)
over the half windows that exist (``window_scores_by_halves``).  Nothing here touches the library or the oracle.
"""
from __future__ import annotations

import numpy as np
import torch

U = 2.0 ** -24                                              # unit roundoff of fp32
# |bf16 score - fp32 score| for unit-norm rows: each operand carries a relative error <= 2^-9, so every product
# a b (1 + d1)(1 + d2) is off by <= |a b| (2^-8 + 2^-18) = |a b| 2^-8 (1 + 2^-10) <= |a b| 2^-8 (1 + 2^-9); sum |a b| <= 1
# (Cauchy-Schwarz); plus the fp32 accumulation of either side, dv U sum |a b| each: 2 * 256 * 2^-24 = 256 * 2^-23 at dv = 256
EPS_UNIT = 2.0 ** -8 * (1 + 2.0 ** -9) + 256 * 2.0 ** -23


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """The contract's operand rounding: fp32 -> bf16 (round to nearest even) -> float64."""
    return x.float().bfloat16().double()


def frame_scores(ctx: torch.Tensor, cls: torch.Tensor, rounded: bool = True):
    """(scores (nq, ctx_l), abs_sums (nq, ctx_l) = sum_c |a b|) in float64; ``rounded=False``: the unrounded fp32 operands."""
    a = bf16_round(ctx) if rounded else ctx.double()
    b = bf16_round(cls) if rounded else cls.double()
    return b @ a.t(), b.abs() @ a.abs().t()


def num_windows(ctx_l: int, W: int) -> int:
    S = W // 2
    return -(-ctx_l // S) + 1


def window_reduce(fs: torch.Tensor, W: int) -> torch.Tensor:
    """Max of each row of fs (nq, ctx_l) over the frame range of every window."""
    S, ctx_l = W // 2, fs.shape[1]
    nw = num_windows(ctx_l, W)
    out = torch.empty(fs.shape[0], nw, dtype=fs.dtype)
    for i in range(nw):
        lo, hi = max((i - 1) * S, 0), min((i - 1) * S + W, ctx_l)
        out[:, i] = fs[:, lo:hi].max(dim=1).values
    return out


def window_scores(ctx, cls, W: int, rounded: bool = True):
    """(win (nq, nw) float64, abs (nq, nw) = the largest sum_c |a b| among the window's frames)."""
    fs, ab = frame_scores(ctx, cls, rounded)
    return window_reduce(fs, W), window_reduce(ab, W)


def window_scores_by_halves(fs: torch.Tensor, W: int) -> torch.Tensor:
    """The header's statement of how the kernels combine: half-window maxima + the odd-W first-frame term."""
    S, ctx_l = W // 2, fs.shape[1]
    nh = -(-ctx_l // S)
    neg = torch.full((fs.shape[0],), -np.inf, dtype=fs.dtype)
    hm = [fs[:, h * S:min((h + 1) * S, ctx_l)].max(dim=1).values for h in range(nh)]
    out = torch.empty(fs.shape[0], nh + 1, dtype=fs.dtype)
    for i in range(nh + 1):
        m = hm[i - 1] if i >= 1 else neg
        if i < nh:
            m = torch.maximum(m, hm[i])
        if W % 2 == 1 and i + 1 < nh:
            m = torch.maximum(m, fs[:, (i + 1) * S])
        out[:, i] = m
    return out


def accumulation_bound(win: torch.Tensor, ab: torch.Tensor, dv: int) -> torch.Tensor:
    """Worst-case fp32 accumulation error of a window score: dv U max_f sum_c |a b| + 2 U |score| (products are exact)."""
    return dv * U * ab + 2 * U * win.abs()


def stable_topk(win_row: torch.Tensor, k: int):
    """First k window indices of the stable descending sort of one score row, -1 padded."""
    order = torch.sort(win_row, descending=True, stable=True).indices.tolist()[:k]
    return order + [-1] * (k - len(order))


# ---- planted inputs for the pipeline test: a few clips of each query's video along the query's direction ---------------------
def plant(opt, ann, video_feats, query_feats, n_clips: int = 3):
    """Copies of video_feats with, for the j-th query of a video, clips [j S + 10, j S + 10 + n_clips) set to the query's cls
    vector (times the row scale of the synthetic clips): half window j, hence windows j and j + 1, stand out for that query."""
    S = int(opt.max_v_l / 2)
    vf = {k: v.copy() for k, v in video_feats.items()}
    seen = {}
    for row in ann:
        j = seen.get(row["clip_id"], 0)
        seen[row["clip_id"]] = j + 1
        lo = j * S + 10
        v = vf[row["clip_id"]]
        if lo + n_clips <= v.shape[0]:
            v[lo:lo + n_clips] = query_feats[row["query_id"]]["cls_features"][None, :]
    return vf


def adapted_rows_f64(sd, x: np.ndarray, eps: float = 1e-5) -> np.ndarray:
    """cone/inference.py:254-258 on l2-normalised rows, float64: y = adapter(x) + x, y / ||y||."""
    x = x.astype(np.float64)
    x = x / (np.linalg.norm(x, axis=1, keepdims=True) + eps)
    h = np.maximum(x @ sd["adapter_layer.layers.0.weight"].astype(np.float64).T + sd["adapter_layer.layers.0.bias"], 0.0)
    y = h @ sd["adapter_layer.layers.1.weight"].astype(np.float64).T + sd["adapter_layer.layers.1.bias"] + x
    return y / np.linalg.norm(y, axis=1, keepdims=True)


def covered_top1(win_f32_row: torch.Tensor, K: int, eps: float = EPS_UNIT) -> bool:
    """Rule 1 covers the query's top-1 window: its fp32 score exceeds the fp32 (K+1)-th by more than 2 eps (a video with at
    most K windows: every window is in any top-K)."""
    s = torch.sort(win_f32_row, descending=True).values
    return bool(s.numel() <= K or s[0] - s[K] > 2 * eps)


def check_rank_rule(win_f32_row: torch.Tensor, top_bf16, K: int, eps: float = EPS_UNIT):
    """The derived rule on one query: (missing, intruders) -- fp32 top-K windows whose score clears the fp32 (K+1)-th by more
    than 2 eps and are NOT in the bf16 top-K; bf16 top-K windows whose fp32 score is below the fp32 K-th minus 2 eps."""
    s, order = torch.sort(win_f32_row, descending=True, stable=True)
    n = s.numel()
    got = [i for i in top_bf16 if i >= 0]
    kk = min(K, n)
    kth = float(s[kk - 1])
    nxt = float(s[K]) if n > K else -np.inf
    must = [int(i) for i, v in zip(order[:kk].tolist(), s[:kk].tolist()) if v - nxt > 2 * eps]
    missing = [i for i in must if i not in got]
    intruders = [i for i in got if float(win_f32_row[i]) < kth - 2 * eps]
    return missing, intruders
