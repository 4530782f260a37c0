#!/usr/bin/env python3
"""The row-GEMM shapes of the step that matter, the shipped form against the tall form (gemm_tall.hip) IN ALTERNATION in one
process: q|k|v of encoder layer 2 (2.08 M rows x N 768 x K 256, bias), the 40-query chunk's q|k|v (96 000 x 768), a decoder-side
192 000 x 256 x 256 with bias + ReLU, the same with a residual, and a sweep of M at N = 768 and N = 256 for the tall form's row
threshold.  Per shape and form: the median over the rounds of the mean launch time, its spread (max - min over the rounds) and
TFLOP/s.  "shipped" = what an automatic launch runs with the tall form off (the 8-wave row tile, its small forms below their
thresholds); "tall" = family 4.  The last line is the decoder-side N 256 GEMM with residual + LayerNorm (no tall form).

    python tools/gemm_qkv_bench.py [--rounds 5] [--launches 10] [--no-sweep]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cone_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--launches", type=int, default=10)
ap.add_argument("--no-sweep", action="store_true")
args = ap.parse_args()

dev = torch.device("cuda", 0)
lib, P = _lib.load(), _lib.ptr
K = 256
SHIPPED, TALL = 1 << 11, 4 << 8       # cone_test_gemm_tall: automatic with the tall form off / the tall form forced
HEAD = [(2_079_985, 768, 0), (96_000, 768, 0), (192_000, 256, 1), (192_000, 256, 2)]
SWEEP = [(M, N, 0) for N in (768, 256) for M in (4096, 8192, 16384, 32768, 65536, 131072, 262144, 524288)]


def timed(call, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


print(f"rounds {args.rounds}, launches per round {args.launches}; ms = median over the rounds, spread = max - min")
for M, N, flags in HEAD + ([] if args.no_sweep else SWEEP):
    A = torch.randn(M, K, device=dev)
    W = torch.randn(N, K, device=dev) / K ** 0.5
    bias, R = torch.randn(N, device=dev), torch.randn(M, N, device=dev) if flags & 2 else None
    Cs = {name: torch.empty(M, N, device=dev) for name in ("shipped", "tall")}
    form = dict(shipped=SHIPPED, tall=TALL)
    calls = {name: (lambda name=name: _lib.check(lib.cone_test_gemm_tall(
        P(A), None, 0, P(W), P(bias), P(R) if R is not None else None, None, None, P(Cs[name]), None, None, M, N, K,
        flags | form[name], 0, 0, None, 0, _lib.stream()))) for name in Cs}
    for c in calls.values():
        c(), c()
    ms = {name: [] for name in calls}
    for _ in range(args.rounds):
        for name, c in calls.items():
            ms[name].append(timed(c, args.launches))
    same = torch.equal(Cs["shipped"], Cs["tall"])
    line = f"M={M} N={N} K={K} flags={flags}:"
    for name, v in ms.items():
        med = statistics.median(v)
        line += f"  {name} {med:.4f} ms (spread {max(v) - min(v):.4f}, {2.0 * M * N * K / med / 1e9:.1f} TFLOP/s)"
    line += f"  tall/shipped {statistics.median(ms['tall']) / statistics.median(ms['shipped']):.3f}  equal {same}"
    print(line, flush=True)
    del A, W, R, Cs, calls

M, N, flags = 163_840, 256, 2 | 4
A, W = torch.randn(M, K, device=dev), torch.randn(N, K, device=dev) / K ** 0.5
bias, R = torch.randn(N, device=dev), torch.randn(M, N, device=dev)
lg, lb, C = torch.rand(N, device=dev) + 0.5, torch.randn(N, device=dev), torch.empty(M, N, device=dev)
call = lambda: _lib.check(lib.cone_test_gemm(P(A), None, 0, P(W), P(bias), P(R), P(lg), P(lb), P(C), None, None, M, N, K, flags,
                                             _lib.stream()))
call(), call()
ms = timed(call, 20)
print(f"M={M} N={N} K={K} flags={flags}: {ms:.3f} ms  {2.0 * M * N * K / ms / 1e9:.1f} TFLOP/s  checksum {float(C[::4097].double().sum()):.6f}")
