#!/usr/bin/env python3
"""The opt-in bf16 pre-filter against the fp32 forms, in ONE session: BASELINE.json configs[2]'s MAD-scale video (ctx_l =
6.2 M clips x 512: 12.7 GB fp32, 6.3 GB bf16; `--ctx_l 1500000` for a short slot -- both sides then use that video).

Per query count (default 1, 2, 4, 5, 8, 16, 64), three INTERLEAVED rounds of
    fp32          ops.prefilter_scores(fp32 arena)                      (tools/prefilter_bench.py's default figure)
    split_bf16    ... split_bf16=True, from 8 queries on                (tools/prefilter_bench.py --split_bf16)
    bf16          ops.prefilter_scores(bf16 arena)                      (cone_prefilter_scores_bf16)
each the median of `--steps` device-timed calls (window scores, no frame-score matrix, no top-k: the stream alone).  Reported:
ms, GB/s of the bytes the form actually streams (4 or 2 B per arena element + the query vectors + the window scores) and the
fraction of the 8 TB/s HBM3E peak.  One JSON line per (query count, form), and a last line for the config-2 step
(`predict_split`, 1 000 queries x 50 videos) with and without `opt.prefilter_bf16` (`--no_step` skips it).

Which bf16 FORM serves a query count is CONE_PF16_MQ_MIN (prefilter.hip); the other side of the threshold is measured by
building the library with another value (`CONE_HIPCC_FLAGS=-DCONE_PF16_MQ_MIN=1` or `=99`, python -m cone_amd.build) and running
this tool with `--tag`.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cone_amd import ops  # noqa: E402


def timed(fn, steps):
    """Median device time of fn() in ms (events around each call; one warm-up)."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def config2_step(steps):
    from cone_amd import inference as inf, synth
    from cone_amd.config import make_opt
    from cone_amd.model import build_model
    opt = make_opt("ego4d", nms_thd=0.5, eval_split_name="val")
    model, _ = build_model(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(opt, 0).items()})
    ann, vf, qf = synth.make_dataset(opt, 1000, 50, seed=0)
    store = inf.FeatureStore(opt, ann, vf, qf)
    res = {}
    for rnd in range(3):
        for flag in (False, True):
            opt.prefilter_bf16 = flag

            def step():
                inf.predict_split(model, store, opt)
            ms = timed(step, steps)
            res.setdefault("prefilter_bf16" if flag else "default", []).append(round(ms, 2))
    return {"workload": "config-2 step: predict_split, 1000 queries x 50 videos (ego4d preset)",
            "ms_per_step_rounds": res, "ms_per_step": {k: statistics.median(v) for k, v in res.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctx_l", type=int, default=6_200_000)
    ap.add_argument("--dv", type=int, default=512)
    ap.add_argument("--W", type=int, default=125)
    ap.add_argument("--queries", type=str, default="1,2,4,5,8,16,64")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no_step", action="store_true")
    ap.add_argument("--only_bf16", action="store_true", help="skip the fp32 arena (a threshold A/B build)")
    ap.add_argument("--tag", type=str, default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    vid = ops.l2_normalize(torch.randn(args.ctx_l, args.dv, device=dev, generator=g), 0.0)
    vid16 = ops.rows_to_bf16(vid)
    if args.only_bf16:
        vid = None
    nw = ops.num_windows(args.ctx_l, args.W)
    for nq in [int(x) for x in args.queries.split(",")]:
        txt = ops.l2_normalize(torch.randn(nq, args.dv, device=dev, generator=g), 0.0)
        forms = {"bf16": lambda: ops.prefilter_scores(vid16, txt, args.W, frame_scores=False)}
        if vid is not None:
            forms["fp32"] = lambda: ops.prefilter_scores(vid, txt, args.W, frame_scores=False)
            if nq >= 8:
                forms["split_bf16"] = lambda: ops.prefilter_scores(vid, txt, args.W, frame_scores=False, split_bf16=True)
        ms = {k: [] for k in forms}
        for _ in range(args.rounds):                    # interleaved: every round times every form once
            for k in sorted(forms):
                ms[k].append(timed(forms[k], args.steps))
        for k in sorted(forms):
            m = statistics.median(ms[k])
            elt = 2.0 if k == "bf16" else 4.0
            nbytes = elt * args.ctx_l * args.dv + nq * 4.0 * (args.dv + nw)
            print(json.dumps({"tag": args.tag, "ctx_l": args.ctx_l, "dv": args.dv, "W": args.W, "queries": nq, "form": k,
                              "ms": round(m, 3), "ms_rounds": [round(x, 3) for x in ms[k]],
                              "GB_streamed": round(nbytes / 1e9, 3), "GB_per_s": round(nbytes / (m * 1e-3) / 1e9, 1),
                              "frac_of_8TBps": round(nbytes / (m * 1e-3) / 8e12, 4)}), flush=True)
        if vid is not None:       # what the rounding costs: the largest score difference between the modes, for the record
            a = ops.prefilter_scores(vid, txt, args.W, frame_scores=False)[1]
            b = ops.prefilter_scores(vid16, txt, args.W, frame_scores=False)[1]
            print(json.dumps({"tag": args.tag, "queries": nq, "max_abs_window_score_diff_bf16_vs_fp32": float((a - b).abs().max())}),
                  flush=True)
    del vid, vid16
    torch.cuda.empty_cache()
    if not args.no_step:
        print(json.dumps(config2_step(args.steps)), flush=True)


if __name__ == "__main__":
    main()
