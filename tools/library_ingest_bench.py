"""Latency of loading and growing a video library against the only ways there were before ``add_many`` / ``extend``: one ``add``
per video, and ``remove`` + ``add`` of the whole grown video from its raw clip features; ONE process, one session of the card.

usage: python tools/library_ingest_bench.py [--calls 200] [--rounds 3] [--videos 128] [--clips 900] [--more 8]
                                            [--out profiles/library_ingest_latency.txt]

Per round, the median over --calls timed calls -- each timed on the host from its start until the device has finished, raw
features resident on the device in every arm; the library's bookkeeping is put back between calls, outside the timed part -- of:
  (a) add_many                  --videos videos of --clips clips into an empty library: one concatenation, one launch chain
      add x N                   the same videos, one ``add`` each
  (b) extend, in place          --more clips behind a resident video of --clips clips, the rows behind it free
      remove + add              the grown video indexed again from its raw features
  (c) extend, relocating        the same, a neighbour directly behind: the resident rows move into a hole, the new ones follow
(a) and (b) must be below their baseline in every round pairing; the tool exits non-zero otherwise.  (c) is recorded and
compared with the baseline of (b), not gated.
"""
import argparse
import copy
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
from session_bench import verdict  # noqa: E402


def snapshot(lib):
    return copy.deepcopy(lib._rows), dict(lib._videos), lib._next_id


def restore(lib, snap):
    """Puts the bookkeeping back (the rows keep whatever the last call wrote: every arm writes all the rows it reads)."""
    lib._rows, lib._videos, lib._next_id = copy.deepcopy(snap[0]), dict(snap[1]), snap[2]
    lib._scan_cache = None


def timed(fn, reset, calls, warmup):
    """Median ms of fn() + synchronize, with reset() (synchronized) before every call and outside the clock."""
    ts = []
    for i in range(warmup + calls):
        reset()
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(time.perf_counter() - t)
    return statistics.median(ts) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--videos", type=int, default=128)
    ap.add_argument("--clips", type=int, default=900)
    ap.add_argument("--more", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(SimpleNamespace(**LOCALIZER_OPT), 0).items()}
    loc = CONELocalizator(state_dict=sd)
    g = torch.Generator().manual_seed(0)
    V, n, m = a.videos, a.clips, a.more
    raw = [(torch.randn(n, 256, generator=g) * 2).cuda() for _ in range(V)]
    grown = (torch.randn(n + m, 256, generator=g) * 2).cuda()
    first, more = grown[:n].contiguous(), grown[n:].contiguous()
    small = (torch.randn(10, 256, generator=g) * 2).cuda()
    query = (torch.randn(12, 768, generator=g).cuda(), torch.randn(256, generator=g).cuda())

    # (a) an empty library of exactly the videos' clips
    cat = loc.open_library(V * n)
    empty = snapshot(cat)
    probe = (0, V // 2, V - 1)
    ids = cat.add_many(raw)
    want = cat.predict_moments([(ids[i], query) for i in probe])
    assert want == [loc.predict_moment(raw[i], query) for i in probe]
    restore(cat, empty)
    ids = [cat.add(v) for v in raw]
    assert cat.predict_moments([(ids[i], query) for i in probe]) == want            # the ways agree before they are timed

    def add_each():
        for v in raw:
            cat.add(v)

    # (b) / (c) one resident video with free rows behind it / with a neighbour directly behind
    want_grown = loc.predict_moment(grown, query)
    free, blocked = loc.open_library(2 * (n + m) + 100), loc.open_library(2 * (n + m) + 100)
    vf, vb = free.add(first), blocked.add(first)
    blocked.add(small)
    s_free, s_blocked = snapshot(free), snapshot(blocked)
    assert free.extend(vf, more) == n + m and free._videos[vf][0] == 0 and free.predict_moment(vf, query) == want_grown
    assert blocked.extend(vb, more) == n + m and blocked._videos[vb][0] == n + 10 and blocked.predict_moment(vb, query) == want_grown
    restore(free, s_free)
    free.remove(vf)
    assert free.predict_moment(free.add(grown), query) == want_grown

    def readd():
        free.remove(vf)
        free.add(grown)

    variants = {
        f"(a) add_many, {V} x {n} clips": (lambda: cat.add_many(raw), lambda: restore(cat, empty)),
        f"(a) add x {V}": (add_each, lambda: restore(cat, empty)),
        f"(b) extend by {m}, in place": (lambda: free.extend(vf, more), lambda: restore(free, s_free)),
        f"(b) remove + add of {n + m} clips": (readd, lambda: restore(free, s_free)),
        f"(c) extend by {m}, relocating": (lambda: blocked.extend(vb, more), lambda: restore(blocked, s_blocked)),
    }
    res = {k: [] for k in variants}
    for r in range(a.rounds):
        for k, (fn, reset) in variants.items():
            res[k].append(timed(fn, reset, a.calls, a.warmup if r == 0 else 3))
    lines = [f"library_ingest_bench: {a.calls} calls per median, {a.rounds} rounds, warm-up {a.warmup}; ms per CALL, host clock, "
             f"device finished; raw features resident on the device; {torch.cuda.get_device_name(0)}",
             f"--- (a) {V} videos of {n} clips = {V * n} clips into an empty library (arena {cat.nbytes / 2**20:.1f} MiB); "
             f"(b) / (c) {m} clips behind a resident video of {n}"]
    for k, v in res.items():
        lines.append(f"{k:36s} " + "  ".join(f"{x:9.4f}" for x in v) + f"   median {statistics.median(v):9.4f}   "
                     f"spread {min(v):.4f} .. {max(v):.4f}")
    names, ok = list(variants), True
    for new, old in ((names[0], names[1]), (names[2], names[3])):
        lines.append("  " + verdict(new, res[new], old, res[old]) + f": {statistics.median(res[old]) / statistics.median(res[new]):.2f} x")
        ok = ok and max(res[new]) < min(res[old])
    lines.append("  " + verdict(names[4], res[names[4]], names[3], res[names[3]])
                 + f": {statistics.median(res[names[3]]) / statistics.median(res[names[4]]):.2f} x (recorded, not gated)")
    lines.append("(add_many's time includes the one concatenation of the raw rows on the device; an extend that relocates is one "
                 "table upload, one copy of the resident rows and the index chain of the new ones)")
    lines.append("not measured: raw features on the host, prefilter_bf16 libraries, long-window and 128 / 4 handles, other lengths, "
                 "fragmented arenas (several runs), chunk_clips cuts")
    lines.append("condition add_many / extend in place below the parent's way in every round pairing: " + ("holds" if ok else "DOES NOT HOLD"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
