#!/usr/bin/env python3
"""Step time of BASELINE configs[1] (Ego4D-NLQ val-scale synthetic split: 1 000 queries x 50 videos, window_len 90, top-20,
NMS 0.5; predict_split one step at a time) in the three arithmetic modes of the transformer layer tails: the default
(exact-fp32 MFMA), ``split_bf16`` (six bf16 products per fp32 product, fp32-accurate) and ``bf16`` (operands rounded once,
one product).  One model, one store, the same seeded inputs; the modes are timed in ``--rounds`` interleaved rounds so
that clock drift hits all three alike.

    python tools/bf16_bench.py [--steps 5] [--warmup 2] [--rounds 3] [--queries 1000] [--videos 50]

ONE JSON line: per mode the median, min and max ms per step over the rounds, and the ratios.  Kernel times behind a figure:
``rocprofv3 --kernel-trace --stats -d out -- python tools/bf16_bench.py --only bf16 --rounds 1 --steps 2 --warmup 1``.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cone_amd import inference as inf  # noqa: E402
from cone_amd import synth  # noqa: E402
from cone_amd.config import make_opt  # noqa: E402
from cone_amd.model import build_model  # noqa: E402

MODES = ("default", "split_bf16", "bf16")


def set_mode(model, mode):
    model.set_option("split_bf16", 0)
    model.set_option("bf16", 0)
    if mode != "default":
        model.set_option(mode, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--videos", type=int, default=50)
    ap.add_argument("--only", nargs="*", default=list(MODES), choices=MODES)
    a = ap.parse_args()
    opt = make_opt("ego4d", nms_thd=0.5, eval_split_name="test", topk_window=20, eval_bsz=32)
    sd = synth.make_state_dict(opt, 0)
    model, _ = build_model(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    ann, vf, qf = synth.make_dataset(opt, a.queries, a.videos, seed=0)
    store = inf.FeatureStore(opt, ann, vf, qf)
    ms = {m: [] for m in a.only}
    n_windows = 0
    for _ in range(a.rounds):
        for mode in a.only:
            set_mode(model, mode)
            for _ in range(a.warmup):
                inf.predict_split(model, store, opt)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                _, info = inf.predict_split(model, store, opt)
            torch.cuda.synchronize()
            ms[mode].append((time.perf_counter() - t0) / a.steps * 1e3)
            n_windows = int(info["n_windows"])
    row = dict(workload="configs[1]", windows=n_windows, steps=a.steps, rounds=a.rounds)
    for mode in a.only:
        row[mode] = dict(ms_per_step=round(statistics.median(ms[mode]), 3), min=round(min(ms[mode]), 3),
                         max=round(max(ms[mode]), 3))
    med = lambda m: statistics.median(ms[m])
    if "bf16" in ms and "split_bf16" in ms:
        row["bf16_vs_split_bf16"] = round(med("split_bf16") / med("bf16"), 3)
    if "bf16" in ms and "default" in ms:
        row["bf16_vs_default"] = round(med("default") / med("bf16"), 3)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
