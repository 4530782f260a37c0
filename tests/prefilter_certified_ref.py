"""Float64 restatement of the certified pre-filter's bound (include/cone_hip.h): R, N, E(q), and the margin a
query has against it.  Plain torch on the CPU: no library call, no oracle.

    R  = max over rows of |v - bf16(v)|                (2-norms; bf16 = round to nearest even, 8 significand bits)
    N  = max over rows of max(|v|, |bf16(v)|)
    E  = (R |qh| + N |qh - q| + 2 g N max(|q|, |qh|)) (1 + 2^-10),   qh = bf16(q), g = (dv+1) u / (1 - (dv+1) u), u = 2^-24

E bounds |coarse - exact| of every frame, hence of every window: coarse = any fp32 summation of the exact products of the
rounded operands, exact = any fp32 summation of the fp32 products of the originals.  The device adds TINY (1 + |qh| + N) for
operands, products and sums below 2^-126 (``device_bound``); R and N as the device reports them lie in [1, 1 + 2^-10] times
these plus 2^-55.  The worst relative error of one rounding is 2^-8 / (1 + 2^-8) (``U_BF16``), not 2^-9: 1 + 2^-8 -> 1.0."""
import torch

U_BF16 = 2.0 ** -8 / (1 + 2.0 ** -8)
TINY = 2.0 ** -114
INFLATE = 1 + 2.0 ** -10


def bf16(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 (round to nearest even) -> float64."""
    return x.to(torch.float32).bfloat16().to(torch.float64)


def index_norms(vid: torch.Tensor):
    """(R, N) of the rows of vid (ctx_l, dv), float64."""
    v, vh = vid.to(torch.float32).to(torch.float64), bf16(vid)
    R = (v - vh).norm(dim=1).max()
    N = torch.maximum(v.norm(dim=1), vh.norm(dim=1)).max()
    return float(R), float(N)


def gamma(dv: int) -> float:
    du = (dv + 1) * 2.0 ** -24
    return du / (1 - du)


def cert_bound(q: torch.Tensor, R: float, N: float, dv: int) -> float:
    """E(q) for one query vector (dv,)."""
    x, h = q.to(torch.float32).to(torch.float64), bf16(q)
    nq, nh, nd = float(x.norm()), float(h.norm()), float((h - x).norm())
    return (R * nh + N * nd + 2 * gamma(dv) * N * max(nq, nh)) * INFLATE


def device_bound(q: torch.Tensor, R: float, N: float, dv: int) -> float:
    """What pf_certify_kernel compares against, given the R and N it is handed."""
    return cert_bound(q, R, N, dv) + TINY * (1 + float(bf16(q).norm()) + N)


def num_windows(ctx_l: int, W: int) -> int:
    S = W // 2
    return -(-ctx_l // S) + 1


def window_scores(fs: torch.Tensor, W: int) -> torch.Tensor:
    """fs (nq, ctx_l) -> (nq, num_window): window i = max over frames [max((i-1)S, 0), min((i-1)S + W, ctx_l))."""
    nq, ctx_l = fs.shape
    S = W // 2
    out = torch.empty(nq, num_windows(ctx_l, W), dtype=fs.dtype)
    for i in range(out.shape[1]):
        out[:, i] = fs[:, max((i - 1) * S, 0):min((i - 1) * S + W, ctx_l)].max(dim=1).values
    return out


def stable_desc(row: torch.Tensor) -> torch.Tensor:
    """Window indices by (score descending, index ascending)."""
    return torch.sort(row, descending=True, stable=True).indices


def margin(vid: torch.Tensor, q: torch.Tensor, W: int, k: int, n_cand: int):
    """(t - c_last, E) for one query in float64: what the proof sees up to the fp32 rounding of the scores (< E / 50 for unit
    rows).  A query whose margin is far above E certifies, one far below does not; nothing is claimed in between."""
    v, x = vid.to(torch.float32).to(torch.float64), q.to(torch.float32).to(torch.float64)
    exact = window_scores((v @ x)[None, :], W)[0]
    coarse = window_scores((bf16(vid) @ bf16(q))[None, :], W)[0]
    cand = stable_desc(coarse)[:n_cand]
    t = exact[cand].sort(descending=True).values[min(k, cand.numel()) - 1]
    R, N = index_norms(vid)
    return float(t - coarse[cand[-1]]), device_bound(q, R * INFLATE + 2.0 ** -55, N * INFLATE + 2.0 ** -55, vid.shape[1])
