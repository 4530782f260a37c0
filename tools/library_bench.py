"""Per-pair latency of a video library against what the parent offers for queries on DIFFERENT videos -- one call per video on
its own session --, in ONE process and one session of the card.

usage: python tools/library_bench.py [--calls 200] [--rounds 3] [--clips 900] [--out profiles/library_latency.txt]

16 videos of --clips clips each are resident twice: in one VideoLibrary, and as 16 VideoSession(step="c").  Per round, the
median over --calls timed calls -- each timed on the host from its start to the moments it returns, inputs resident on the
device -- of:
  (a) library 16 videos    lib.predict_moments(16 pairs on 16 different videos), per pair
  (b) 16 sessions          16 x session[v].predict_moment(query), per call (what the parent offers for such a list)
  (c) library one video    lib.predict_moments(16 pairs on ONE video), per pair
      session batch16      session[0].predict_moments(the same 16 queries), per query
  (d) the device half of (c) alone -- the queries concatenated, ONE C call, the read-back; no validation, planning or parsing --
      through lib._enqueue and through session[0].enqueue: tells the C entries' cost from the wrappers'
The variants of a round run back to back, so that every comparison is between figures of the same minutes of the card.  A
comparison "holds" when the slower side's BEST round is still below the faster side's WORST round (beyond the spread of the
rounds); otherwise it is reported as within the spread.
"""
import argparse
import os
import statistics
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cone_amd import synth  # noqa: E402
from cone_amd.localizator import CONELocalizator, LOCALIZER_OPT  # noqa: E402
from session_bench import median_ms, verdict  # noqa: E402

N_VIDEOS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--clips", type=int, default=900)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(SimpleNamespace(**LOCALIZER_OPT), 0).items()}
    loc = CONELocalizator(state_dict=sd)
    g = torch.Generator().manual_seed(0)
    videos = [(torch.randn(a.clips, 256, generator=g) * 2).cuda() for _ in range(N_VIDEOS)]
    lens = [12, 7, 20, 3, 16, 9, 12, 1, 20, 5, 14, 8, 11, 19, 6, 12]
    queries = [(torch.randn(n, 768, generator=g).cuda(), torch.randn(256, generator=g).cuda()) for n in lens]
    lib = loc.open_library(N_VIDEOS * a.clips)
    ids = [lib.add(v) for v in videos]
    sessions = [loc.open_video(v, step="c") for v in videos]
    spread = [(ids[i], q) for i, q in enumerate(queries)]
    one = [(ids[0], q) for q in queries]
    want = [loc.predict_moment(videos[i], q) for i, q in enumerate(queries)]
    assert lib.predict_moments(spread) == want == [sessions[i].predict_moment(q) for i, q in enumerate(queries)]
    assert lib.predict_moments(one) == sessions[0].predict_moments(queries) == [loc.predict_moment(videos[0], q) for q in queries]

    def per_video_calls():
        for s, q in zip(sessions, queries):
            s.predict_moment(q)

    chunk = [(lib._videos[ids[0]][:2], q) for q in queries]

    def session_device_half():
        dev = loc.device                                         # (the conversions lib._enqueue makes, no-ops here)
        tok_cat = torch.cat([t.to(dev, torch.float32).contiguous() for t, _ in queries])
        cls = torch.stack([c.to(dev, torch.float32).reshape(-1) for _, c in queries]).contiguous()
        return sessions[0].enqueue(tok_cat, lens, cls).cpu()

    assert torch.equal(lib._enqueue(sessions[0].K, chunk).cpu(), session_device_half())
    variants = {
        "(a) library 16 videos": (lambda: lib.predict_moments(spread), 16),
        "(b) 16 sessions": (per_video_calls, 16),
        "(c) library one video": (lambda: lib.predict_moments(one), 16),
        "(c) session batch16": (lambda: sessions[0].predict_moments(queries), 16),
        "(d) library device half": (lambda: lib._enqueue(sessions[0].K, chunk).cpu(), 16),
        "(d) session device half": (session_device_half, 16),
    }
    res = {k: [] for k in variants}
    for r in range(a.rounds):
        for k, (fn, per) in variants.items():
            res[k].append(median_ms(fn, a.calls, a.warmup if r == 0 else 5) / per)
    lines = [f"library_bench: {a.calls} calls per median, {a.rounds} rounds, warm-up {a.warmup}; ms per PAIR (video, query); "
             f"{torch.cuda.get_device_name(0)}",
             f"--- {N_VIDEOS} videos of {a.clips} clips ({sessions[0].K} windows per query; library arena {lib.nbytes / 2**20:.1f} MiB)"]
    for k, v in res.items():
        lines.append(f"{k:24s} " + "  ".join(f"{x:8.4f}" for x in v) + f"   median {statistics.median(v):8.4f}")
    lines.append("  " + verdict("(a) library 16 videos", res["(a) library 16 videos"], "(b) 16 sessions", res["(b) 16 sessions"]))
    lines.append("  " + verdict("(c) library one video", res["(c) library one video"], "(c) session batch16", res["(c) session batch16"]))
    lines.append("  " + verdict("(c) session batch16", res["(c) session batch16"], "(a) library 16 videos", res["(a) library 16 videos"]))
    lines.append("  " + verdict("(d) library device half", res["(d) library device half"], "(d) session device half", res["(d) session device half"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
