#!/usr/bin/env python3
"""Windows of more than 256 tokens: the streaming attention core against the resident one, and the step time of a
256 / 8 handle at several window lengths.

    python tools/long_window_bench.py core  [--windows 20000] [--head_dim 32] [--heads 8] [--keys 256] [--iters 5]
    python tools/long_window_bench.py steps [--only 90g 256 400 992] [--steps 3] [--warmup 1] [--queries 1000] [--out f.json]

``core``: both kernels on the same packed q | k | v rows through cone_test_gen_attn, every window ``--keys`` (<= 256) keys
long, the resident kernel with kcap = 256 and the streaming kernel with kcap = 257 (the capacity only selects the kernel);
encoder form (queries = keys) and decoder cross form (5 slot queries).  One JSON line: ms per launch each, the ratio.

``steps``: predict_split one step at a time on a synthetic Ego4D-style split, as tools/shape_bench.py: ``90g`` = window_len 90
with the handle forced onto the general path (option general_shape = 1: shape_bench's 256x8g row), ``256`` / ``400`` /
``992`` = max_v_l 256 / 400 / 992 with max_q_l 32 / 20 / 32 (long-window handles).  Top-20 windows per query everywhere and
``--queries`` * 90 / max_v_l queries on videos of ~10 windows' length, so that every configuration covers the same number
of clips per step.  One JSON line per configuration: ms per step, windows, tokens per step.  The attention core's share:

    rocprofv3 --kernel-trace --stats -d out -- python tools/long_window_bench.py steps --only 400 --steps 1 --warmup 1
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cone_amd import _lib  # noqa: E402
from cone_amd import inference as inf  # noqa: E402
from cone_amd import synth  # noqa: E402
from cone_amd.config import make_opt  # noqa: E402
from cone_amd.model import build_model  # noqa: E402

CONFIGS = {"90g": (90, 20, 1), "256": (256, 32, 0), "400": (400, 20, 0), "992": (992, 32, 0)}


def bench_core(a):
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    hd, heads, n, B = a.head_dim, a.heads, a.keys, a.windows
    d = hd * heads
    torch.manual_seed(0)
    qkv = torch.randn(B * n, 3 * d, device=dev) * 2
    dq = torch.randn(B * 5, 3 * d, device=dev) * 2
    off = torch.arange(0, (B + 1) * n, n, dtype=torch.int32, device=dev)
    p = lambda x: x.data_ptr()

    def run(kcap, cross):
        out = torch.empty((B * 5 if cross else B * n, d), device=dev)
        call = lambda: _lib.check(lib.cone_test_gen_attn(
            p(dq) if cross else p(qkv), 3 * d, p(qkv) + 4 * d, 3 * d, p(qkv) + 8 * d, 3 * d, p(out), d,
            None if cross else p(off), p(off), B, 5 if cross else 0, heads, hd, kcap, _lib.stream()))
        call()
        torch.cuda.synchronize()
        best = float("inf")
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1))
        return best, out

    row = dict(windows=B, keys=n, head_dim=hd, heads=heads)
    for cross in (False, True):
        r_ms, r_out = run(256, cross)
        s_ms, s_out = run(257, cross)
        k = "cross5" if cross else "encoder"
        row[k] = dict(resident_ms=round(r_ms, 3), streaming_ms=round(s_ms, 3), streaming_over_resident=round(s_ms / r_ms, 3),
                      max_abs_diff=float((r_out - s_out).abs().max()))
    print(json.dumps(row), flush=True)
    return [row]


def bench_steps(a):
    rows = []
    for name in a.only:
        W, Lq, forced = CONFIGS[name]
        nq = max(4, round(a.queries * 90 / W))
        videos = max(2, min(a.videos, nq // 4))
        opt = make_opt("ego4d", nms_thd=0.5, eval_split_name="test", topk_window=20, eval_bsz=32, max_v_l=W, max_q_l=Lq)
        sd = synth.make_state_dict(opt, 0)
        model, _ = build_model(opt)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        if forced:
            model.set_option("general_shape", 1)
        ctx = (850, 950) if W == 90 else (int(9.5 * W), int(10.5 * W))
        ann, vf, qf = synth.make_dataset(opt, nq, videos, seed=0, ctx_range=ctx, lq_range=(5, min(Lq, 18) + 1))
        store = inf.FeatureStore(opt, ann, vf, qf)
        for _ in range(a.warmup):
            _, info = inf.predict_split(model, store, opt)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            _, info = inf.predict_split(model, store, opt)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.steps
        nw = int(info["n_windows"])
        row = dict(config=name, max_v_l=W, max_q_l=Lq, max_window_tokens=getattr(model, "max_window_tokens", 256), queries=nq,
                   videos=videos, ms_per_step=round(dt * 1e3, 2), windows=nw, clips_per_step=nw * W,
                   windows_per_s=round(nw / dt, 1))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del model, store
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["core", "steps"])
    ap.add_argument("--windows", type=int, default=20000)
    ap.add_argument("--head_dim", type=int, default=32)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--keys", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--videos", type=int, default=50)
    ap.add_argument("--only", nargs="*", default=list(CONFIGS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = bench_core(a) if a.mode == "core" else bench_steps(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
