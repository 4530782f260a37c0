#!/usr/bin/env python3
"""The two weight-ring kernels streaming their weights from the packed slab image (tail_pack.hip) against the same kernels
gathering them from the row-major matrices (both forms issue their pieces as saddr + voffset: the A/B isolates the image),
IN ALTERNATION in one process, on random operands: the projecting layer tail's
persistent 128-row kernel (ffn.hip, cone_test_tail_packed) at the step's row counts and the tall row GEMM (gemm_tall.hip,
cone_test_gemm_tall_packed) at its.  Per shape and form: the median over the rounds of the mean launch time, its spread
(max - min over the rounds) and TFLOP/s -- the procedure of tools/gemm_qkv_bench.py; the outputs of the two forms must be equal.

    python tools/tail_packed_bench.py [--rounds 5] [--launches 10] [--ff 1024]"""
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
ap.add_argument("--ff", type=int, default=1024)
ap.add_argument("--tail-rows", type=int, nargs="*", default=[677_111, 1_950_000, 96_000])
ap.add_argument("--tall-rows", type=int, nargs="*", default=[2_079_985, 262_144])
args = ap.parse_args()

dev = torch.device("cuda", 0)
lib, P = _lib.load(), _lib.ptr
FORMS = ("row-major", "packed")


def timed(call, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def ab(label, calls, outs, flop):
    for c in calls.values():
        c(), c()
    ms = {name: [] for name in calls}
    for _ in range(args.rounds):
        for name, c in calls.items():
            ms[name].append(timed(c, args.launches))
    line = f"{label}:"
    for name, v in ms.items():
        med = statistics.median(v)
        line += f"  {name} {med:.4f} ms (spread {max(v) - min(v):.4f}, {flop / med / 1e9:.1f} TFLOP/s)"
    a, b = (statistics.median(ms[f]) for f in FORMS)
    line += f"  packed - row-major {b - a:+.4f} ms ({(b / a - 1) * 100:+.2f} %)  equal {torch.equal(*outs)}"
    print(line, flush=True)


print(f"rounds {args.rounds}, launches per round {args.launches}; ms = median over the rounds, spread = max - min")
ff = args.ff
mk = lambda *s: torch.randn(*s, device=dev)
Wo, bo, W1, b1 = mk(256, 256) / 16, mk(256) * 0.1, mk(ff, 256) / 16, mk(ff) * 0.1
W2, b2 = mk(256, ff) / ff ** 0.5, mk(256) * 0.1
pg, pb, lg, lb = torch.rand(256, device=dev) + 0.5, mk(256), torch.rand(256, device=dev) + 0.5, mk(256)
img = torch.empty(lib.cone_test_f32_pack_tail_bytes(ff, 1, 0), dtype=torch.uint8, device=dev)
_lib.check(lib.cone_test_f32_pack_tail(P(Wo), P(W1), P(W2), ff, None, 0, P(img), _lib.stream()))
for M in args.tail_rows:
    A, R = mk(M, 256), mk(M, 256)
    outs = [torch.empty(M, 256, device=dev) for _ in FORMS]
    calls = {name: (lambda o=o, im=im: _lib.check(lib.cone_test_tail_packed(
        P(A), P(Wo), P(bo), P(R), P(pg), P(pb), P(W1), P(b1), P(W2), P(b2), P(lg), P(lb), P(o), M, ff, 0, None, None, None, None, 0,
        8, 0, P(im) if im is not None else None, _lib.stream()))) for name, o, im in zip(FORMS, outs, (None, img))}
    ab(f"tail M={M} ff={ff}", calls, outs, 4.0 * M * ff * 256 + 2.0 * M * 256 * 256)
    del A, R, outs, calls

for N in (768,):
    W, bias = mk(N, 256) / 16, mk(N)
    wimg = torch.empty(lib.cone_test_f32_pack_rows_bytes(N), dtype=torch.uint8, device=dev)
    _lib.check(lib.cone_test_f32_pack_rows(P(W), N, P(wimg), _lib.stream()))
    for M in args.tall_rows:
        A = mk(M, 256)
        outs = [torch.empty(M, N, device=dev) for _ in FORMS]
        calls = {name: (lambda o=o, im=im: _lib.check(lib.cone_test_gemm_tall_packed(
            P(A), P(W), P(bias), None, P(o), M, N, 0, None, 0, P(im) if im is not None else None, _lib.stream())))
            for name, o, im in zip(FORMS, outs, (None, wimg))}
        ab(f"tall M={M} N={N} K=256", calls, outs, 2.0 * M * N * 256)
        del A, outs, calls
