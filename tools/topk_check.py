#!/usr/bin/env python3
"""Stable top-k (cone_topk_windows_ws) against tests/index_refs.topk_reference at MAD-scale sizes, on the adversarial rows of
tests/index_refs.topk_rows -- the patterns live there, and tests/test_index_kernels_gpu.py runs them at the sizes where the
kernel forms change; this script only adds rows of up to 300 000 windows.  Run on the GPU box."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import index_refs as R  # noqa: E402
from cone_amd import ops  # noqa: E402

dev = torch.device("cuda", 0)
n_ok = 0
for nq, n, k in ((3, 100001, 30), (2, 9000, 256), (2, 9000, 300), (5, 50000, 1), (4, 70000, 200), (2, 300000, 30),
                 (2, 20000, 64), (2, 20000, 65), (3, 12345, 20)):
    rows = [R.topk_rows(n, k, seed) for seed in range(nq)]
    for name in rows[0]:
        x = torch.stack([r[name] for r in rows])
        idx, val = ops.topk_windows(x.to(dev).contiguous(), k)
        for q in range(nq):
            want_i, want_v = R.topk_reference(x[q], k)
            assert torch.equal(idx[q].cpu(), want_i) and torch.equal(val[q].cpu(), want_v), (name, nq, n, k, q)
        n_ok += 1
print(f"topk ok: {n_ok} cases")
