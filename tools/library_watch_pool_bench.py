"""Latency of standing queries over a library: ``w.poll()`` of a ``lib.watch_moments`` watcher next to the parent's way to the same
lists, ``lib.search_moments`` with the same arguments after the same ``extend`` -- in ONE process and one session of the card,
both on THIS build (``search_moments`` returns what the parent commit's returns).

usage: python tools/library_watch_pool_bench.py [--calls 200] [--rounds 3] [--videos 16,256] [--queries 1,16,64]
                                                [--out profiles/library_watch_pool_latency.txt]

A library of 16 and of 256 videos of 900 clips, 1, 16 and 64 standing queries, ``n_windows = 20``.  One STEP is
``lib.extend(<the next video, round robin>, 8 clips)`` followed by the answer; only the answer is timed (the extend is the same on
both sides), on the host from its start to the host lists it returns.  Per round and side the library is built again, so both
sides answer the same sequence of libraries.  Per round the median over --calls steps of:
  poll                  w.poll(): scan, budget, plan, the window model on the missing windows only, stage C on the cache; 2 read-backs
  search_moments        lib.search_moments(queries, 20): the window model on all 20 windows of every query; 2 read-backs
and, once per round, outside the steps:
  cold poll             the first poll of a new watcher (every chosen window runs) next to one search_moments at that state
  idle poll             the median over --calls polls with no extend in between (no window runs)
The expectation: ``poll`` is below ``search_moments`` in every round pairing; the tool says whether it holds and exits non-zero
otherwise.  The cold poll is expected above ``search_moments``.
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

STEP, CLIPS, N_WINDOWS = 8, 900, 20


def row(name, v, extra=""):
    return f"{name:40s} " + "  ".join(f"{x:9.4f}" for x in v) + f"   median {statistics.median(v):9.4f}" + extra


def steps(lib, ids, more, answer, calls, warmup, after=None):
    """extend the next video by STEP clips, then ``answer`` (timed): the median in ms over the last ``calls`` steps."""
    ts = []
    for i in range(warmup + calls):
        lib.extend(ids[i % len(ids)], more[i * STEP:(i + 1) * STEP], compact=True)
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
    ap.add_argument("--videos", default="16,256")
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
    lines = [f"library_watch_pool_bench: {a.calls} steps per median (one step = extend one video by {STEP} clips, then the timed "
             f"answer), {a.rounds} rounds, warm-up {a.warmup} steps; ms per ANSWER; both sides on this build; "
             f"{torch.cuda.get_device_name(0)}",
             f"n_windows = {N_WINDOWS}, topk_window = {loc.args.topk_window}, max_v_l = {loc.args.max_v_l}, num_queries = "
             f"{loc.args.num_queries}"]
    ok = True
    for V in (int(s) for s in a.videos.split(",")):
        base = list((torch.randn(V * CLIPS, 256, generator=g) * 2).cuda().split(CLIPS))
        capacity = V * CLIPS + n_steps * STEP + 2 * (CLIPS + n_steps * STEP)     # (a video that is not the last relocates)
        lines.append(f"--- {V} videos of {CLIPS} clips, one of them growing by {STEP} a step")
        for nq in (int(s) for s in a.queries.split(",")):
            qs = queries[:nq]
            res = {k: [] for k in ("poll", "search_moments", "cold poll", "search_moments (cold state)", "idle poll")}
            share, nbytes = [], 0
            for r in range(a.rounds):
                with loc.open_library(capacity) as lib:
                    ids = lib.add_many(base)
                    w = lib.watch_moments(qs, n_windows=N_WINDOWS)
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    first = w.poll()
                    res["cold poll"].append((time.perf_counter() - t) * 1e3)
                    assert first == lib.search_moments(qs, N_WINDOWS)
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    lib.search_moments(qs, N_WINDOWS)
                    res["search_moments (cold state)"].append((time.perf_counter() - t) * 1e3)
                    res["idle poll"].append(median_ms(w.poll, a.calls, 5))
                    assert w.windows_run == [0] * nq
                    res["poll"].append(steps(lib, ids, more, w.poll, a.calls, a.warmup,
                                             lambda: share.append(sum(w.windows_run) / max(sum(w.windows_listed), 1))))
                    assert w.poll() == lib.search_moments(qs, N_WINDOWS)        # the same lists at the end of the round
                    nbytes = w.nbytes
                    w.close()
                with loc.open_library(capacity) as lib:
                    ids = lib.add_many(base)
                    res["search_moments"].append(steps(lib, ids, more, lambda: lib.search_moments(qs, N_WINDOWS), a.calls, a.warmup))
                torch.cuda.empty_cache()
            tag = f", {V} videos, {nq}q"
            lines += [row(k + tag, v) for k, v in res.items()]
            p, m = statistics.median(res["poll"]), statistics.median(res["search_moments"])
            lines.append(f"    mean windows_run / windows_listed per poll {statistics.mean(share):.4f}; search_moments / poll = "
                         f"{m / p:.2f}x on the medians; watcher cache {nbytes / 1e6:.2f} MB")
            v = verdict("poll", res["poll"], "search_moments", res["search_moments"])
            lines.append(f"    {v}")
            if "below" not in v:
                ok = False
        del base
        torch.cuda.empty_cache()
    lines.append("expectation poll below search_moments in every round pairing: " + ("holds" if ok else "DOES NOT HOLD"))
    lines.append("Not measured: peaked features where the budget moves often, other n_windows, trims between polls.")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
