#!/usr/bin/env python3
"""Step time of BASELINE configs[1] (Ego4D-NLQ val-scale synthetic split: 1 000 queries x 50 videos, window_len 90, top-20,
NMS 0.5; predict_split one step at a time) at several model shapes: 256 / 8 on the shipped path, 256 / 8 forced onto the
general-shape path (cone_model_set_option "general_shape"), and the general path at 128 / 4, 256 / 16, 512 / 8.

    python tools/shape_bench.py [--steps 3] [--warmup 1] [--queries 1000] [--videos 50] [--out shape_bench.json]

One JSON line per shape: ms per step, windows / s.  Kernel names behind a figure: run under
``rocprofv3 --kernel-trace --stats -d out -- python tools/shape_bench.py --only 256x8g --steps 1 --warmup 1``.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cone_amd import inference as inf  # noqa: E402
from cone_amd import synth  # noqa: E402
from cone_amd.config import make_opt  # noqa: E402
from cone_amd.model import build_model  # noqa: E402

SHAPES = {"256x8": (256, 8, 0), "256x8g": (256, 8, 1), "128x4": (128, 4, 0), "256x16": (256, 16, 0), "512x8": (512, 8, 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--videos", type=int, default=50)
    ap.add_argument("--only", nargs="*", default=list(SHAPES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for name in a.only:
        d, h, forced = SHAPES[name]
        opt = make_opt("ego4d", nms_thd=0.5, eval_split_name="test", topk_window=20, eval_bsz=32, hidden_dim=d, nheads=h)
        sd = synth.make_state_dict(opt, 0)
        model, _ = build_model(opt)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        if forced:
            model.set_option("general_shape", 1)
        ann, vf, qf = synth.make_dataset(opt, a.queries, a.videos, seed=0)
        store = inf.FeatureStore(opt, ann, vf, qf)
        for _ in range(a.warmup):
            _, info = inf.predict_split(model, store, opt)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            _, info = inf.predict_split(model, store, opt)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.steps
        row = dict(shape=name, hidden_dim=d, nheads=h, path="general" if forced or (d, h) != (256, 8) else "shipped",
                   ms_per_step=round(dt * 1e3, 2), windows=int(info["n_windows"]),
                   windows_per_s=round(info["n_windows"] / dt, 1))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del model, store
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
