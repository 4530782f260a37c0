#!/usr/bin/env python3
"""The certified pre-filter against the two paths it sits between, in ONE session: BASELINE.json configs[2]'s MAD-scale video
(ctx_l = 6.2 M clips x 512: 12.7 GB fp32 + 6.3 GB bf16 shadow = the 1.5 x the index keeps resident; `--ctx_l 1500000` for a
short slot), N(0,1) unit rows, top-k windows per query (default k = 30).

Per query count (default 1, 4, 16, 64), `--rounds` INTERLEAVED rounds of
    fp32       ops.prefilter_scores(fp32 rows) + ops.topk_windows          (the exact path: what the certified call returns)
    bf16       ops.prefilter_scores(bf16 shadow) + ops.topk_windows        (cone_prefilter_scores_bf16: NOT fp32-accurate)
    certified  ops.PrefilterIndex.topk                                     (cone_prefilter_topk_certified)
each the median of `--steps` device-timed calls.  One JSON line per query count: the three times, certified / bf16 (the
overhead of the rescore, the proof and the gated launches: accepted up to 1.10 at 1 query with every query certified),
certified / fp32 (reported, not judged: the bf16 stream's own HBM fraction is a measurement of this tool, too), the share of
certified queries, and whether the certified rows equal the fp32 path's.  `--out FILE` also appends the lines there
(profiles/prefilter_certified.txt).

(The fp32 and bf16 forms score all queries of a call together -- from 5 queries on, on the matrix cores -- while the certified
call's contract is the streaming form's bits; its equality column is therefore checked per query, against the streaming form.)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctx_l", type=int, default=6_200_000)
    ap.add_argument("--dv", type=int, default=512)
    ap.add_argument("--W", type=int, default=125)
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--n_cand", type=int, default=0, help="0 = the entry's default min(num_window, max(4 k, 128))")
    ap.add_argument("--queries", type=str, default="1,4,16,64")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--check_queries", type=int, default=4, help="queries per count whose rows are compared with the fp32 path")
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--tag", type=str, default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    vid = ops.l2_normalize(torch.randn(args.ctx_l, args.dv, device=dev, generator=g), 0.0)
    index = ops.PrefilterIndex(vid)                         # holds `vid` itself (already fp32, contiguous) + the shadow
    torch.cuda.synchronize()
    lines = [{"tag": args.tag, "ctx_l": args.ctx_l, "dv": args.dv, "W": args.W, "k": args.k, "n_cand": args.n_cand,
              "num_window": ops.num_windows(args.ctx_l, args.W), "R": float(index.err[0]), "N": float(index.err[1]),
              "GB_fp32": round(vid.numel() * 4 / 1e9, 3), "GB_bf16": round(vid.numel() * 2 / 1e9, 3)}]
    print(json.dumps(lines[0]), flush=True)
    for nq in [int(x) for x in args.queries.split(",")]:
        txt = ops.l2_normalize(torch.randn(nq, args.dv, device=dev, generator=g), 0.0)
        forms = {
            "fp32": lambda: ops.topk_windows(ops.prefilter_scores(vid, txt, args.W, frame_scores=False)[1], args.k),
            "bf16": lambda: ops.topk_windows(ops.prefilter_scores(index.vid16, txt, args.W, frame_scores=False)[1], args.k),
            "certified": lambda: index.topk(txt, args.W, args.k, args.n_cand or None),
        }
        ms = {f: [] for f in forms}
        for _ in range(args.rounds):                        # interleaved: every round times every form once
            for f in sorted(forms):
                ms[f].append(timed(forms[f], args.steps))
        med = {f: statistics.median(v) for f, v in ms.items()}
        idx, val, cert = index.topk(txt, args.W, args.k, args.n_cand or None)
        same = True
        for q in range(min(nq, args.check_queries)):        # the contract: the streaming form with the query alone
            e_idx, e_val = ops.topk_windows(ops.prefilter_scores(vid, txt[q:q + 1].contiguous(), args.W, frame_scores=False)[1], args.k)
            same = same and torch.equal(e_idx[0], idx[q]) and torch.equal(e_val[0], val[q])
        line = {"tag": args.tag, "queries": nq, "ms": {f: round(m, 3) for f, m in med.items()},
                "ms_rounds": {f: [round(x, 3) for x in v] for f, v in ms.items()},
                "certified_over_bf16": round(med["certified"] / med["bf16"], 4),
                "certified_over_fp32": round(med["certified"] / med["fp32"], 4),
                "certified_share": round(float(cert.float().mean()), 4), "rows_equal_fp32_path": bool(same),
                "bf16_frac_of_8TBps": round(vid.numel() * 2 / (med["bf16"] * 1e-3) / 8e12, 4)}
        lines.append(line)
        print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
