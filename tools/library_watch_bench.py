"""Latency of standing queries on a live video: ``w.poll()`` next to the parent's way to the same lists, ``lib.predict_moments`` on
the same pairs after the same ``extend`` -- in ONE process and one session of the card, both on THIS build (``predict_moments``
is the untouched entry of the parent commit).

usage: python tools/library_watch_bench.py [--calls 200] [--rounds 3] [--sizes 900,33000] [--out profiles/library_watch_latency.txt]

A resident video of 900 and of 33 000 clips, 1, 16 and 64 standing queries.  One STEP is ``lib.extend(vid, 8 clips)`` followed by
the answer; only the answer is timed (the extend is the same on both sides), on the host from its start to the host lists it
returns, queries resident on the device.  Per round and side the video starts again at its size and grows by 8 clips a step, so
both sides answer the same sequence of videos.  Per round the median over --calls steps of:
  poll                  w.poll(): scan, plan, the window model on the missing windows only, stage C on the cache; 2 read-backs
  predict_moments       lib.predict_moments([(vid, q) for q in queries]): the window model on all K windows; 1 read-back
and, once per round, outside the steps:
  cold poll             the first poll of a new watcher (every listed window runs) next to one predict_moments at that state
  idle poll             the median over --calls polls with no extend in between (no window runs)
The expectation: at 16 and 64 queries ``poll`` is below ``predict_moments`` in every round pairing; the tool says whether it holds
and exits non-zero otherwise.  At 1 query both sides are launch-bound and nothing is gated.
"""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cone_amd import synth  # noqa: E402
from cone_amd.localizator import CONELocalizator, LOCALIZER_OPT  # noqa: E402
from session_bench import median_ms, verdict  # noqa: E402

STEP = 8


def row(name, v, extra=""):
    return f"{name:36s} " + "  ".join(f"{x:9.4f}" for x in v) + f"   median {statistics.median(v):9.4f}" + extra


def steps(lib, vid, more, answer, calls, warmup, after=None):
    """extend by STEP clips, then ``answer`` (timed): the median in ms over the last ``calls`` of ``warmup + calls`` steps."""
    ts = []
    for i in range(warmup + calls):
        lib.extend(vid, more[i * STEP:(i + 1) * STEP])
        torch.cuda.synchronize()
        t = time.perf_counter()
        answer()
        ts.append(time.perf_counter() - t)
        if after is not None and i >= warmup:
            after()
    return statistics.median(ts[warmup:]) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="900,33000")
    ap.add_argument("--queries", default="1,16,64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(SimpleNamespace(**LOCALIZER_OPT), 0).items()}
    loc = CONELocalizator(state_dict=sd)
    g = torch.Generator().manual_seed(0)
    lens = [12, 7, 20, 3, 16, 9, 12, 1, 20, 5, 14, 8, 11, 19, 6, 12, 4, 13, 2, 17, 10]
    queries = [(torch.randn(lens[i % len(lens)], 768, generator=g).cuda(), torch.randn(256, generator=g).cuda()) for i in range(64)]
    n_steps = a.warmup + a.calls
    more = (torch.randn(n_steps * STEP, 256, generator=g) * 2).cuda()
    lines = [f"library_watch_bench: {a.calls} steps per median (one step = extend by {STEP} clips, then the timed answer), {a.rounds} "
             f"rounds, warm-up {a.warmup} steps; ms per ANSWER; both sides on this build; {torch.cuda.get_device_name(0)}",
             f"topk_window = {loc.args.topk_window}, max_v_l = {loc.args.max_v_l}, num_queries = {loc.args.num_queries}"]
    ok = True
    for clips in (int(s) for s in a.sizes.split(",")):
        base = torch.randn(clips, 256, generator=g) * 2
        lib = loc.open_library(clips + n_steps * STEP + 64)
        lines.append(f"--- a video of {clips} clips growing to {clips + n_steps * STEP} (library arena {lib.nbytes / 2**20:.1f} MiB)")
        for nq in (int(s) for s in a.queries.split(",")):
            qs = queries[:nq]
            res = {k: [] for k in ("poll", "predict_moments", "cold poll", "predict_moments (cold state)", "idle poll")}
            run, listed, nbytes = [], 0, 0
            for r in range(a.rounds):
                vid = lib.add(base)
                pairs = [(vid, q) for q in qs]
                w = lib.watch(vid, qs)
                torch.cuda.synchronize()
                t = time.perf_counter()
                first = w.poll()
                res["cold poll"].append((time.perf_counter() - t) * 1e3)
                assert first == lib.predict_moments(pairs)
                torch.cuda.synchronize()
                t = time.perf_counter()
                lib.predict_moments(pairs)
                res["predict_moments (cold state)"].append((time.perf_counter() - t) * 1e3)
                res["idle poll"].append(median_ms(w.poll, a.calls, 5))
                assert w.windows_run == [0] * nq
                res["poll"].append(steps(lib, vid, more, w.poll, a.calls, a.warmup, lambda: run.append(sum(w.windows_run) / nq)))
                assert w.poll() == lib.predict_moments(pairs)                   # the same lists at the end of the round
                listed, nbytes = w.windows_listed[0], w.nbytes
                w.close()
                lib.remove(vid)
                vid = lib.add(base)
                pairs = [(vid, q) for q in qs]
                res["predict_moments"].append(steps(lib, vid, more, lambda: lib.predict_moments(pairs), a.calls, a.warmup))
                lib.remove(vid)
            tag = f", {clips} clips, {nq}q"
            lines += [row(k + tag, v) for k, v in res.items()]
            p, m = statistics.median(res["poll"]), statistics.median(res["predict_moments"])
            lines.append(f"    mean windows_run per poll and query {statistics.mean(run):.3f} of {listed} listed; predict_moments / poll = "
                         f"{m / p:.2f}x on the medians; watcher cache {nbytes / 1e6:.2f} MB")
            v = verdict("poll", res["poll"], "predict_moments", res["predict_moments"])
            lines.append(f"    {v}")
            if nq >= 16 and "below" not in v:
                ok = False
        lib.close()
        del lib
        torch.cuda.empty_cache()
    lines.append("expectation poll below predict_moments in every round pairing at 16 and 64 queries: " + ("holds" if ok else "DOES NOT HOLD"))
    lines.append("Not measured: peaked features where the list changes often, other topk_window, other window lengths.")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
