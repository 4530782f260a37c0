"""Per-query latency of a video session against CONELocalizator.predict_moment, in ONE process and one session of the card.

usage: python tools/session_bench.py [--calls 200] [--rounds 3] [--sizes 900,33000] [--out profiles/session_latency.txt]

Per video size (900 clips = BASELINE configs[0]: one query, 20 windows of 90 clips; 33 000 clips = a MAD-length video) and per
round, the median over --calls timed calls -- each call timed on the host from its start to the moments it returns, inputs
resident on the device -- of:
  parent eager      CONELocalizator.predict_moment(video, query)
  parent hip_graph  the same with hip_graph=True (replays of a captured shape)
  session python    open_video(video, step="python").predict_moment(query)
  session c         open_video(video, step="c").predict_moment(query)
  batch16 python/c  predict_moments(16 queries of ragged lengths), per query
The variants of a round run back to back, so that every comparison is between figures of the same minutes of the card.  A
comparison "holds" when the slower side's BEST round is still below the faster side's WORST round (beyond the spread of the
rounds); otherwise it is reported as within the spread.
"""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cone_amd import synth  # noqa: E402
from cone_amd.localizator import CONELocalizator, LOCALIZER_OPT  # noqa: E402


def median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts) * 1e3


def verdict(name_a, a, name_b, b):
    """a should not be above b."""
    if max(a) < min(b):
        return f"{name_a} below {name_b} in every round pairing (holds beyond the spread of the rounds)"
    if min(a) > max(b):
        return f"{name_a} ABOVE {name_b} in every round pairing"
    return f"{name_a} vs {name_b}: within the spread of the rounds (no claim)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--sizes", default="900,33000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(SimpleNamespace(**LOCALIZER_OPT), 0).items()}
    eager, graph = CONELocalizator(state_dict=sd), CONELocalizator(state_dict=sd, hip_graph=True)
    g = torch.Generator().manual_seed(0)
    lines = [f"session_bench: {a.calls} calls per median, {a.rounds} rounds, warm-up {a.warmup}; ms per QUERY; "
             f"{torch.cuda.get_device_name(0)}"]
    for ctx_l in (int(s) for s in a.sizes.split(",")):
        vid = (torch.randn(ctx_l, 256, generator=g) * 2).cuda()
        lens = [12, 7, 20, 3, 16, 9, 12, 1, 20, 5, 14, 8, 11, 19, 6, 12]
        queries = [(torch.randn(n, 768, generator=g).cuda(), torch.randn(256, generator=g).cuda()) for n in lens]
        q = queries[0]
        t0 = time.perf_counter()
        s_py, s_c = eager.open_video(vid, step="python"), eager.open_video(vid, step="c")
        torch.cuda.synchronize()
        t_open = (time.perf_counter() - t0) / 2 * 1e3
        want = eager.predict_moment(vid, q)
        assert graph.predict_moment(vid, q) == want and s_py.predict_moment(q) == want and s_c.predict_moment(q) == want
        assert s_py.predict_moments(queries) == s_c.predict_moments(queries) == [eager.predict_moment(vid, x) for x in queries]
        variants = {
            "parent eager": (lambda: eager.predict_moment(vid, q), 1),
            "parent hip_graph": (lambda: graph.predict_moment(vid, q), 1),
            "session python": (lambda: s_py.predict_moment(q), 1),
            "session c": (lambda: s_c.predict_moment(q), 1),
            "batch16 python": (lambda: s_py.predict_moments(queries), 16),
            "batch16 c": (lambda: s_c.predict_moments(queries), 16),
        }
        res = {k: [] for k in variants}
        for r in range(a.rounds):
            for k, (fn, per) in variants.items():
                res[k].append(median_ms(fn, a.calls, a.warmup if r == 0 else 5) / per)
        lines.append(f"--- {ctx_l} clips ({s_py.K} windows per query; resident {s_py.nbytes / 2**20:.1f} MiB = "
                     f"{s_py.nbytes / ctx_l:.0f} B per clip; open_video {t_open:.2f} ms first call)")
        for k, v in res.items():
            lines.append(f"{k:18s} " + "  ".join(f"{x:8.4f}" for x in v) + f"   median {statistics.median(v):8.4f}")
        lines.append("  " + verdict("session python", res["session python"], "parent eager", res["parent eager"]))
        lines.append("  " + verdict("session c", res["session c"], "parent eager", res["parent eager"]))
        lines.append("  " + verdict("session c", res["session c"], "session python", res["session python"]))
        lines.append("  " + verdict("batch16 c", res["batch16 c"], "batch16 python", res["batch16 python"]))
        s_py.close(); s_c.close()
        del vid
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
