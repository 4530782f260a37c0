#!/usr/bin/env python3
"""Option ``general_bf16`` against the exact-fp32 general path, on the SAME handle in ONE session.

The step configurations of tools/shape_bench.py (window_len 90 + 20 words, 1 000 queries x 50 videos, top-20) at the general
path's shapes -- 128 / 4, 256 / 16, 512 / 8 and 256 / 8 forced onto it (``256x8g``) -- and of tools/long_window_bench.py at
256 / 8 with windows of 256 + 32, 400 + 20 and 992 + 32 tokens (``--queries`` * 90 / max_v_l queries: the same clips per
step).  Per configuration ``--rounds`` INTERLEAVED rounds of (option off, option on), each the median of ``--steps``
device-timed ``predict_split`` calls; one JSON line per configuration: ms per step off / on (rounds and medians), on / off.

    python tools/general_bf16_bench.py [--only 128x4 256x16 512x8 256x8g w256 w400 w992] [--steps 3] [--rounds 3] [--queries 1000]
    python tools/general_bf16_bench.py --kernels [--only 256x8g w400]

``--kernels``: per configuration and mode ONE step under ``rocprofv3 --kernel-trace --stats`` in a fresh child process of its
own (this file with ``--child``), and a per-kernel table from its statistics: the new kernel's time (gemm_bf16_kernel) next
to gemm_rows16_kernel + gemm_f32_kernel<128,128,true> of the option-off step on the same rows, and every kernel above 2 % of
either step.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (hidden_dim, nheads, general_shape forced, max_v_l, max_q_l)
CONFIGS = {"128x4": (128, 4, 0, 90, 20), "256x16": (256, 16, 0, 90, 20), "512x8": (512, 8, 0, 90, 20),
           "256x8g": (256, 8, 1, 90, 20), "w256": (256, 8, 0, 256, 32), "w400": (256, 8, 0, 400, 20),
           "w992": (256, 8, 0, 992, 32)}


def setup(name, queries, videos):
    import torch
    from cone_amd import inference as inf, synth
    from cone_amd.config import make_opt
    from cone_amd.model import build_model
    d, h, forced, W, Lq = CONFIGS[name]
    long_cfg = W != 90
    nq = max(4, round(queries * 90 / W))
    nv = max(2, min(videos, nq // 4)) if long_cfg else videos
    opt = make_opt("ego4d", nms_thd=0.5, eval_split_name="test", topk_window=20, eval_bsz=32, hidden_dim=d, nheads=h,
                   max_v_l=W, max_q_l=Lq)
    model, _ = build_model(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(opt, 0).items()})
    if forced:
        model.set_option("general_shape", 1)
    kw = dict(ctx_range=(int(9.5 * W), int(10.5 * W)), lq_range=(5, min(Lq, 18) + 1)) if long_cfg else {}
    ann, vf, qf = synth.make_dataset(opt, nq, nv, seed=0, **kw)
    return model, opt, inf.FeatureStore(opt, ann, vf, qf), inf


def timed(fn, steps):
    """Median device time of fn() in ms (events around each call)."""
    import torch
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def bench(a):
    import torch
    for name in a.only:
        model, opt, store, inf = setup(name, a.queries, a.videos)
        info = {}

        def step():
            info.update(n=int(inf.predict_split(model, store, opt)[1]["n_windows"]))
        for on in (0, 1):                                   # warm-up of both modes (allocations, weight images)
            model.set_option("general_bf16", on)
            step()
        torch.cuda.synchronize()
        ms = {0: [], 1: []}
        for _ in range(a.rounds):                           # interleaved: every round times both modes once
            for on in (0, 1):
                model.set_option("general_bf16", on)
                ms[on].append(round(timed(step, a.steps), 2))
        off, on = statistics.median(ms[0]), statistics.median(ms[1])
        d, h, forced, W, Lq = CONFIGS[name]
        print(json.dumps(dict(config=name, hidden_dim=d, nheads=h, max_v_l=W, max_q_l=Lq, windows=info["n"],
                              ms_per_step_off=off, ms_per_step_on=on, on_over_off=round(on / off, 3),
                              off_rounds=ms[0], on_rounds=ms[1])), flush=True)
        del model, store
        torch.cuda.empty_cache()


def child(a):
    """One configuration, one mode, one warm-up and one step: what the profiler's child process runs."""
    import torch
    model, opt, store, inf = setup(a.only[0], a.queries, a.videos)
    model.set_option("general_bf16", a.child)
    for _ in range(2):
        inf.predict_split(model, store, opt)
    torch.cuda.synchronize()


def kernel_stats(name, on, a):
    """{kernel name: total us} of one child run (both of its steps) under rocprofv3 --kernel-trace --stats."""
    with tempfile.TemporaryDirectory() as out:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
               os.path.abspath(__file__), "--child", str(on), "--only", name, "--queries", str(a.queries), "--videos", str(a.videos)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 failed for {name}:\n{r.stderr[-2000:]}")
        tot = {}
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    tot[row["Name"]] = tot.get(row["Name"], 0.0) + float(row["TotalDurationNs"]) / 1e3
        return tot


def short(k):
    return k.split("(")[0].replace("void ", "").replace("cone::", "")


def kernels(a):
    for name in a.only:
        off, on = kernel_stats(name, 0, a), kernel_stats(name, 1, a)
        s_off, s_on = sum(off.values()), sum(on.values())
        pick = lambda t, pat: sum(v for k, v in t.items() if pat in k)
        fp32_gemm = pick(off, "gemm_rows16_kernel") + sum(v for k, v in off.items() if "gemm_f32_kernel<128,128,true" in k.replace(" ", ""))
        print(json.dumps(dict(config=name, kernel_us_off=round(s_off, 1), kernel_us_on=round(s_on, 1),
                              gemm_bf16_kernel_us_on=round(pick(on, "gemm_bf16_kernel"), 1),
                              gemm_rows16_plus_f32_128x128_a2_us_off=round(fp32_gemm, 1),
                              same_fp32_kernels_left_on_us=round(pick(on, "gemm_rows16_kernel"), 1))), flush=True)
        print(f"# {name}: kernels above 2 % of either run (two steps each; us off | us on)")
        for k in sorted(set(off) | set(on), key=lambda k: -(off.get(k, 0) + on.get(k, 0))):
            if off.get(k, 0) > 0.02 * s_off or on.get(k, 0) > 0.02 * s_on:
                print(f"#   {short(k)[:70]:70s} {off.get(k, 0):12.1f} | {on.get(k, 0):12.1f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=list(CONFIGS))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--videos", type=int, default=50)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        child(a)
    elif a.kernels:
        kernels(a)
    else:
        bench(a)


if __name__ == "__main__":
    main()
