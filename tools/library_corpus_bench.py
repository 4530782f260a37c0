"""Latency of the library moment search next to the budgeted search it is built on -- in ONE process and one session of the card.

usage: python tools/library_corpus_bench.py [--calls 200] [--rounds 3] [--clips 900] [--parent FILE] [--windows-only]
                                            [--out profiles/library_corpus_latency.txt]

Per round, the median over --calls timed calls -- each timed on the host from its start to the host lists it returns, inputs
resident on the device -- on the library of tools/library_budget_bench.py (V = 16 and 256 resident videos of --clips clips, 1 and
16 queries) of:
  search_moments W=20   lib.search_moments(queries, n_windows=20): scan + budget + the candidates calls + the pooled stage C
  search_windows W=20   lib.search_windows(queries, n_windows=20): the same windows, one stage C per (video, query) pair
  unit                  a bare 16-KiB host-to-device copy plus an empty launch: what the new plan adds twice over (the table's
                        upload and the pooled launch)

--windows-only measures search_windows and the unit alone: it runs on a build of the PARENT commit too (copy this file there).
--parent FILE takes such a run's output: the expectation is then
  search_moments <= the parent's search_windows + 2 x unit + the spread of the rounds (max - min, both rows)
for every (V, queries), on the medians of the rounds; the tool says whether it holds and exits non-zero otherwise.  Without
--parent the parent's figures are "Not measured" and nothing is gated: this is a capability, not a speed-up.
"""
import argparse
import os
import re
import statistics
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cone_amd import synth  # noqa: E402
from cone_amd.localizator import CONELocalizator, LOCALIZER_OPT  # noqa: E402
from session_bench import median_ms  # noqa: E402

ROW = re.compile(r"^(search_windows W=20, V=\d+, \d+q|unit, V=\d+, \d+q)\s+(.*?)\s+median")


def row(name, v):
    return f"{name:36s} " + "  ".join(f"{x:9.4f}" for x in v) + f"   median {statistics.median(v):9.4f}"


def parent_rows(path):
    out = {}
    with open(path) as f:
        for line in f:
            m = ROW.match(line)
            if m:
                out[m.group(1)] = [float(x) for x in m.group(2).split()]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--clips", type=int, default=900)
    ap.add_argument("--sizes", default="16,256")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--windows-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(SimpleNamespace(**LOCALIZER_OPT), 0).items()}
    loc = CONELocalizator(state_dict=sd)
    g = torch.Generator().manual_seed(0)
    lens = [12, 7, 20, 3, 16, 9, 12, 1, 20, 5, 14, 8, 11, 19, 6, 12, 4, 13, 2, 17, 10]
    queries = [(torch.randn(n, 768, generator=g).cuda(), torch.randn(256, generator=g).cuda()) for n in lens]
    parent = parent_rows(a.parent) if a.parent else {}
    lines = [f"library_corpus_bench: {a.calls} calls per median, {a.rounds} rounds, warm-up {a.warmup}; ms per CALL; "
             f"{torch.cuda.get_device_name(0)}" + ("; search_windows and the unit only" if a.windows_only else "")]
    table_16k, one = np.zeros(4096, np.int32), torch.zeros(1, device="cuda")

    def unit():
        torch.from_numpy(table_16k).to("cuda")
        one.fill_(0)

    ok = True
    for V in (int(s) for s in a.sizes.split(",")):
        lib = loc.open_library(V * a.clips)
        lib.add_many([torch.randn(a.clips, 256, generator=g) * 2 for _ in range(V)])
        lines.append(f"--- {V} videos of {a.clips} clips (library arena {lib.nbytes / 2**20:.1f} MiB)")
        for qs in (queries[:1], queries[:16]):
            nq = len(qs)
            tag = f"V={V}, {nq}q"
            variants = {f"search_windows W=20, {tag}": lambda: lib.search_windows(qs, n_windows=20), f"unit, {tag}": unit}
            if not a.windows_only:
                found = lib.search_moments(qs, n_windows=20)
                pairs = lib.search_windows(qs, n_windows=20)
                assert all(1 <= len(m) <= 5 and {v for v, _ in m} <= {v for v, _, _, _ in r_} for m, r_ in zip(found, pairs))
                lines.append(f"    query 0 of {nq}: {len(found[0])} moments from {len({v for v, _ in found[0]})} of the "
                             f"{len(pairs[0])} videos that received windows")
                variants = {f"search_moments W=20, {tag}": lambda: lib.search_moments(qs, n_windows=20), **variants}
            res = {k: [] for k in variants}
            for r in range(a.rounds):
                for k, fn in variants.items():
                    res[k].append(median_ms(fn, a.calls, a.warmup if r == 0 else 5))
            lines += [row(k, v) for k, v in res.items()]
            if a.windows_only:
                continue
            was = parent.get(f"search_windows W=20, {tag}")
            if was is None:
                lines.append(f"parent's search_windows W=20, {tag}: Not measured")
                continue
            new, u = res[f"search_moments W=20, {tag}"], statistics.median(res[f"unit, {tag}"])
            spread = (max(new) - min(new)) + (max(was) - min(was))
            bound = statistics.median(was) + 2 * u + spread
            holds = statistics.median(new) <= bound
            ok = ok and holds
            lines.append(row(f"parent's search_windows W=20, {tag}", was))
            lines.append(f"  search_moments {statistics.median(new):.4f} <= parent's search_windows {statistics.median(was):.4f} + 2 x unit "
                         f"{u:.4f} + spread {spread:.4f} = {bound:.4f}: " + ("holds" if holds else "DOES NOT HOLD"))
        lib.close()
        del lib
        torch.cuda.empty_cache()
    if not a.windows_only:
        lines.append("expectation search_moments <= parent's search_windows + 2 x unit + spread: "
                     + ("Not measured (no --parent)" if not parent else "holds" if ok else "DOES NOT HOLD"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
