"""Latency of a library search against the parent's way to the same answers, and the scan's bandwidth next to the single-video
stream -- in ONE process and one session of the card.

usage: python tools/library_search_bench.py [--calls 200] [--rounds 3] [--clips 900] [--out profiles/library_search_latency.txt]

V = 16 and V = 256 videos of --clips clips are resident in one VideoLibrary; 1 query and 16.  Per round, the median over --calls
timed calls -- each timed on the host from its start to the host lists it returns, inputs resident on the device -- of:
  (a) rank_videos           lib.rank_videos(queries): one scan, one read-back
      per-video stage A     the parent's way to the same lists: per video cone_prefilter_scores (launches of at most 4 queries)
                            + cone_topk_windows_ws on its rows -- the stage A a library call runs per run --, the best scores
                            stacked, one read-back, the videos sorted on the host
  (b) search n_videos=4     lib.search(queries, n_videos=4)
      rank + predict        the per-video ranking of (a), then lib.predict_moments on the 4 chosen pairs of every query
(a) and (b) must be below their parent form at both sizes, beyond the spread of the rounds (the slower side's best round above
the faster side's worst); the tool exits non-zero otherwise.
  (c) the scan of one arena of ~1 M clips as 1 100 videos of 900 (cone_library_scan, device time by events, the two planes and
      the lists included), next to cone_prefilter_scores on ONE contiguous video of the same clips (the stream's ceiling), 1 and
      4 queries: both as GB/s of the adapted rows.  Recorded, not gated.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cone_amd import _lib, ops, synth  # noqa: E402
from cone_amd.library import scan_table  # noqa: E402
from cone_amd.localizator import CONELocalizator, LOCALIZER_OPT  # noqa: E402
from session_bench import median_ms, verdict  # noqa: E402


def adapted_rows(lib):
    """The library's adapted rows (capacity, v_dim) as a tensor over its arena."""
    cl = lib._cl
    at = (cl.adapted - lib._arena.data_ptr()) // 4
    return lib._arena.view(torch.float32)[at:at + lib._rows.capacity * cl.v_dim].view(-1, cl.v_dim)


def parent_ranking(lib, ids, rows, queries, n):
    """Per query [(video id, score), ...], the n best: stage A per video as a library call runs it, ranked on the host."""
    W = lib._loc.args.max_v_l
    cls = torch.stack([c.reshape(-1) for _, c in queries]).contiguous()
    best = []
    for v in ids:
        row0, ctx_l, K = lib._videos[v]
        vid = rows[row0:row0 + ctx_l]
        win = [ops.prefilter_scores(vid, cls[g:g + 4], W, frame_scores=False)[1] for g in range(0, cls.shape[0], 4)]
        best.append(ops.topk_windows(win[0] if len(win) == 1 else torch.cat(win), K)[1][:, 0])
    host = torch.stack(best, dim=1).cpu().tolist()                                    # (nq, V): the one read-back
    return [sorted(zip(ids, row), key=lambda e: -e[1])[:n] for row in host]           # (stable: ties to the earlier video)


def device_median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def stream_section(a, lines):
    """(c): a dictated arena of unit rows behind a hand-made cone_library -- the scan reads nothing but the adapted rows."""
    lib = _lib.load()
    V, n, dv, W, K = 1100, a.clips, 256, 90, 20
    rows = torch.nn.functional.normalize(torch.randn(V * n, dv, device="cuda"), dim=1)
    _, row0, ctx, hb_off = scan_table([(i * n, n) for i in range(V)], W // 2)
    t = [torch.from_numpy(x).cuda() for x in (row0, ctx, hb_off)]
    handle = _lib.Library(0x1000, V * n, 0, dv, 256, None, rows.data_ptr(), None, None, None)
    p = _lib.SessionParams(W, 20, 0.5333, 0.5, 100, 5)
    gb = rows.numel() * 4 / 1e9
    lines.append(f"--- (c) {V} videos of {n} clips = {V * n} clips, {gb:.3f} GB of adapted rows; device ms by events, GB/s of those rows")
    for nq in (1, 4):
        cls = torch.nn.functional.normalize(torch.randn(nq, dv, device="cuda"), dim=1)
        n_ws = lib.cone_library_scan_workspace(C.byref(handle), V, int(hb_off[-1]), nq, K, 10)
        ws = torch.empty(n_ws, dtype=torch.uint8, device="cuda")
        widx, wval = torch.empty(nq * V * K, dtype=torch.int32, device="cuda"), torch.empty(nq * V * K, device="cuda")
        rs, rv = torch.empty(nq * 10, dtype=torch.int32, device="cuda"), torch.empty(nq * 10, device="cuda")

        def scan():
            _lib.check(lib.cone_library_scan(C.c_void_p(0x1000), C.byref(handle), _lib.ptr(t[0]), _lib.ptr(t[1]), _lib.ptr(t[2]), V,
                                             int(hb_off[-1]), _lib.ptr(cls), nq, K, 10, C.byref(p), _lib.ptr(widx), _lib.ptr(wval),
                                             _lib.ptr(rs), _lib.ptr(rv), _lib.ptr(ws), n_ws, _lib.stream()))

        def single():
            ops.prefilter_scores(rows, cls, W, frame_scores=False)

        res = {"library scan": [], "one video": []}
        for r in range(a.rounds):
            res["library scan"].append(device_median_ms(scan, a.calls, a.warmup if r == 0 else 5))
            res["one video"].append(device_median_ms(single, a.calls, a.warmup if r == 0 else 5))
        for k, v in res.items():
            m = statistics.median(v)
            lines.append(f"(c) {nq} quer{'y' if nq == 1 else 'ies'} {k:14s} " + "  ".join(f"{x:8.4f}" for x in v)
                         + f"   median {m:8.4f} ms = {gb / m * 1e3:7.1f} GB/s")
        lines.append(f"    scan / one video: {statistics.median(res['library scan']) / statistics.median(res['one video']):.3f} x the time")


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
    lens = [12, 7, 20, 3, 16, 9, 12, 1, 20, 5, 14, 8, 11, 19, 6, 12]
    queries16 = [(torch.randn(n, 768, generator=g).cuda(), torch.randn(256, generator=g).cuda()) for n in lens]
    lines = [f"library_search_bench: {a.calls} calls per median, {a.rounds} rounds, warm-up {a.warmup}; ms per CALL; "
             f"{torch.cuda.get_device_name(0)}"]
    ok = True
    for V in (int(s) for s in a.sizes.split(",")):
        lib = loc.open_library(V * a.clips)
        ids = [lib.add((torch.randn(a.clips, 256, generator=g) * 2).cuda()) for _ in range(V)]
        rows = adapted_rows(lib)
        lines.append(f"--- {V} videos of {a.clips} clips (library arena {lib.nbytes / 2**20:.1f} MiB)")
        for queries in (queries16[:1], queries16):
            nq = len(queries)
            # the two ways agree before they are timed: the same ranking, the same moments
            want = parent_ranking(lib, ids, rows, queries, 4)
            assert lib.rank_videos(queries, n_videos=4) == want
            found = lib.search(queries, n_videos=4)
            pairs = [(v, q) for row, q in zip(want, queries) for v, _ in row]
            assert [m for row in found for _, _, m in row] == lib.predict_moments(pairs)

            def parent_search():
                ranked = parent_ranking(lib, ids, rows, queries, 4)
                return lib.predict_moments([(v, q) for row, q in zip(ranked, queries) for v, _ in row])

            variants = {
                f"(a) rank_videos, {nq}q": lambda: lib.rank_videos(queries, n_videos=4),
                f"(a) per-video stage A, {nq}q": lambda: parent_ranking(lib, ids, rows, queries, 4),
                f"(b) search n_videos=4, {nq}q": lambda: lib.search(queries, n_videos=4),
                f"(b) rank + predict, {nq}q": parent_search,
            }
            res = {k: [] for k in variants}
            for r in range(a.rounds):
                for k, fn in variants.items():
                    res[k].append(median_ms(fn, a.calls, a.warmup if r == 0 else 5))
            for k, v in res.items():
                lines.append(f"{k:32s} " + "  ".join(f"{x:9.4f}" for x in v) + f"   median {statistics.median(v):9.4f}")
            names = list(variants)
            for new, old in ((names[0], names[1]), (names[2], names[3])):
                lines.append("  " + verdict(new, res[new], old, res[old]))
                ok = ok and max(res[new]) < min(res[old])
        lib.close()
        del lib, rows
        torch.cuda.empty_cache()
    stream_section(a, lines)
    lines.append("conditions (a), (b) below their parent form at both sizes: " + ("hold" if ok else "DO NOT HOLD"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
