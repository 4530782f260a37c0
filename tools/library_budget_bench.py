"""Latency of the ragged library call against the grouped plan, and of a budgeted search against the per-video search -- in ONE
process and one session of the card.

usage: python tools/library_budget_bench.py [--calls 200] [--rounds 3] [--clips 900] [--out profiles/library_budget_latency.txt]

Per round, the median over --calls timed calls -- each timed on the host from its start to the host lists it returns, inputs
resident on the device -- of:
  (a) ragged                lib.predict_moments(pairs, ragged=True): the seven MIXED videos (1 .. 6 000 clips, K = 2, 2, 3, 4, 9, 20,
                            20) x 3 queries in ONE cone_library_localize_ragged call
      grouped               the same list with ragged=False: the parent's plan, one cone_library_localize call per K (five)
      The expectation is ragged < grouped in every round pairing; the tool says whether it holds and exits non-zero otherwise.
  (b) search_windows W=20   lib.search_windows(queries, n_windows=20) for V = 16 and 256 resident videos of --clips clips, 1 and 16
                            queries: scan + budget + the ragged calls on at most 20 windows per query
      search n_videos=4     lib.search(queries, n_videos=4): 80 windows per query
      predict_moment        lib.predict_moments on ONE pair per query: 20 windows per query without any search -- the price the
                            budget is meant to come near (plus the scan).  Recorded, not gated.
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

MIXED_CLIPS = (1, 45, 46, 91, 333, 900, 6000)


def rows_of(res, width=32):
    return [f"{k:{width}s} " + "  ".join(f"{x:9.4f}" for x in v) + f"   median {statistics.median(v):9.4f}" for k, v in res.items()]


def timed(variants, a):
    res = {k: [] for k in variants}
    for r in range(a.rounds):
        for k, fn in variants.items():
            res[k].append(median_ms(fn, a.calls, a.warmup if r == 0 else 5))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--clips", type=int, default=900)
    ap.add_argument("--sizes", default="16,256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(SimpleNamespace(**LOCALIZER_OPT), 0).items()}
    loc = CONELocalizator(state_dict=sd)
    g = torch.Generator().manual_seed(0)
    lens = [12, 7, 20, 3, 16, 9, 12, 1, 20, 5, 14, 8, 11, 19, 6, 12, 4, 13, 2, 17, 10]
    queries = [(torch.randn(n, 768, generator=g).cuda(), torch.randn(256, generator=g).cuda()) for n in lens]
    lines = [f"library_budget_bench: {a.calls} calls per median, {a.rounds} rounds, warm-up {a.warmup}; ms per CALL; "
             f"{torch.cuda.get_device_name(0)}"]
    # (a) one ragged call against one call per K
    lib = loc.open_library(sum(MIXED_CLIPS))
    ids = [lib.add((torch.randn(n, 256, generator=g) * 2).cuda()) for n in MIXED_CLIPS]
    pairs = [(ids[i % 7], q) for i, q in enumerate(queries)]
    assert lib.predict_moments(pairs, ragged=True) == lib.predict_moments(pairs)          # the two plans agree before they are timed
    lines.append(f"--- (a) {len(pairs)} pairs on {len(ids)} videos of {MIXED_CLIPS} clips, K = {[lib._videos[v][2] for v in ids]}")
    res = timed({"(a) ragged, one call": lambda: lib.predict_moments(pairs, ragged=True),
                 "(a) grouped, one call per K": lambda: lib.predict_moments(pairs)}, a)
    lines += rows_of(res)
    new, old = list(res)
    lines.append("  " + verdict(new, res[new], old, res[old]))
    ok = max(res[new]) < min(res[old])
    lib.close()
    # (b) a budget of 20 windows per query against 4 videos x 20 windows
    for V in (int(s) for s in a.sizes.split(",")):
        lib = loc.open_library(V * a.clips)
        ids = lib.add_many([torch.randn(a.clips, 256, generator=g) * 2 for _ in range(V)])
        lines.append(f"--- (b) {V} videos of {a.clips} clips (library arena {lib.nbytes / 2**20:.1f} MiB)")
        for qs in (queries[:1], queries[:16]):
            nq = len(qs)
            found = lib.search_windows(qs, n_windows=20)
            assert all(sum(k for _, _, k, _ in row) == 20 for row in found)
            again = lib.predict_moments([(v, q) for row, q in zip(found, qs) for v, _, _, _ in row],
                                        windows=[k for row in found for _, _, k, _ in row])
            assert [m for row in found for _, _, _, m in row] == again                      # the budgeted answers are the pairs' own
            shares = sorted((k for _, _, k, _ in found[0]), reverse=True)
            lines.append(f"    query 0 of {nq}: 20 windows over {len(shares)} videos, shares {shares}")
            res = timed({f"(b) search_windows W=20, {nq}q": lambda: lib.search_windows(qs, n_windows=20),
                         f"(b) search n_videos=4, {nq}q": lambda: lib.search(qs, n_videos=4),
                         f"(b) predict_moment x {nq}": lambda: lib.predict_moments([(ids[i % V], q) for i, q in enumerate(qs)])}, a)
            lines += rows_of(res)
            names = list(res)
            lines.append("  " + verdict(names[0], res[names[0]], names[1], res[names[1]]))
        lib.close()
        del lib
        torch.cuda.empty_cache()
    lines.append("expectation (a) ragged below grouped in every round pairing: " + ("holds" if ok else "DOES NOT HOLD"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
