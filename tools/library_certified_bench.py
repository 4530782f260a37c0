"""Latency of the budgeted searches on a certified library against the same calls on a plain library holding the same videos --
in ONE process and one session of the card.

usage: python tools/library_certified_bench.py [--calls 200] [--rounds 3] [--clips 900] [--sizes 16,256,1100,6900]
                                               [--queries 1,16,64] [--out profiles/library_certified_latency.txt]

Per size V (videos of --clips clips, filled on the device in chunks by add_many, the same rows in both libraries) and query
count, per round the median over --calls timed calls -- each timed on the host from its start to the host lists it returns --
of lib.search_windows(queries, n_windows=20) and lib.search_moments(queries, n_windows=20), certified against plain.  The answers
are compared with == before anything is timed, and the certified flags are recorded.  Every row is a median of --calls calls.
The scans are timed twice by device events: the two SCAN KERNELS alone -- library_scan_bf16_kernel and library_scan_kernel, by the
library's own per-launch event pairs (cone_prof_enable: one pair around each scan launch, a launch covers all passes), with the
TB/s of the rows they stream --, and the whole C entries around them (cone_library_scan: + the per-video top-k and the ranking;
cone_library_scan_certified: + the five small stages).  At the largest size the certified entry is also timed at n_cand = 128,
1 024 and 4 096: the walk ranks its candidates by counting, O(n_cand^2) per query.
REQUIRED (the tool says whether it holds and exits non-zero otherwise): at the largest size, with 1 query, the certified call is
below the plain one in every round pairing, for both calls.  Everything else is recorded, not gated."""
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
from library_budget_bench import rows_of, timed  # noqa: E402
from session_bench import verdict  # noqa: E402


def device_ms(fn, calls):
    """Median device time of ``fn`` by events, one pair per call."""
    for _ in range(5):
        fn()
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def kernel_ms(fn, calls):
    """Median device time of the scan-kernel launch inside ``fn`` (the library's launch records of kind PK_FRAME_SCORE = 4: one
    per call, the scan's only launch of that kind)."""
    import numpy as np
    from cone_amd import _lib
    lib = _lib.load()
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    lib.cone_prof_enable(1)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    buf = np.zeros((4 * calls + 16, 5))
    n = lib.cone_prof_collect(buf.ctypes.data, len(buf))
    lib.cone_prof_enable(0)
    ms = buf[:n][buf[:n, 0] == 4][:, 4]
    assert len(ms) == calls, (len(ms), calls)
    return statistics.median(ms.tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--clips", type=int, default=900)
    ap.add_argument("--sizes", default="16,256,1100,6900")
    ap.add_argument("--queries", default="1,16,64")
    ap.add_argument("--chunk", type=int, default=100, help="videos per add_many call")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(SimpleNamespace(**LOCALIZER_OPT), 0).items()}
    loc = CONELocalizator(state_dict=sd)
    g = torch.Generator().manual_seed(0)
    lens = [12, 7, 20, 3, 16, 9, 12, 1, 20, 5, 14, 8, 11, 19, 6, 12, 4, 13, 2, 17, 10] * 4
    queries = [(torch.randn(n, 768, generator=g).cuda(), torch.randn(256, generator=g).cuda()) for n in lens[:64]]
    lines = [f"library_certified_bench: {a.calls} calls per median, {a.rounds} rounds, warm-up {a.warmup}; ms per CALL; "
             f"{torch.cuda.get_device_name(0)}"]
    sizes, ok = [int(s) for s in a.sizes.split(",")], True
    gd = torch.Generator(device="cuda").manual_seed(1)
    for V in sizes:
        plain, cert = loc.open_library(V * a.clips), loc.open_library(V * a.clips, certified=True)
        for c in range(0, V, a.chunk):
            vids = list((torch.randn(min(a.chunk, V - c) * a.clips, 256, generator=gd, device="cuda") * 2).split(a.clips))
            plain.add_many(vids)
            cert.add_many(vids)
        del vids
        dv, n_clips = 256, V * a.clips
        lines.append(f"--- {V} videos of {a.clips} clips = {n_clips} clips: plain arena {plain.nbytes / 2**30:.2f} GiB, certified "
                     f"{cert.nbytes / 2**30:.2f} GiB (+{100 * (cert.nbytes - plain.nbytes) / plain.nbytes:.1f} %)")
        table = cert._table(None, list(cert._videos))
        ptable = plain._table(None, list(plain._videos))
        for nq in (int(s) for s in a.queries.split(",")):
            qs = queries[:nq]
            assert cert.search_windows(qs, 20) == plain.search_windows(qs, 20)           # equal before they are timed
            flags = list(cert.last_certified)
            assert cert.search_moments(qs, 20) == plain.search_moments(qs, 20)
            lines.append(f"    {nq} queries: certified flags {sum(flags)} of {nq}")
            res = timed({f"search_windows W=20, {nq}q, certified": lambda: cert.search_windows(qs, 20),
                         f"search_windows W=20, {nq}q, plain": lambda: plain.search_windows(qs, 20),
                         f"search_moments W=20, {nq}q, certified": lambda: cert.search_moments(qs, 20),
                         f"search_moments W=20, {nq}q, plain": lambda: plain.search_moments(qs, 20)}, a)
            lines += rows_of(res, 44)
            names = list(res)
            for new, old in ((names[0], names[1]), (names[2], names[3])):
                lines.append("  " + verdict(new, res[new], old, res[old]))
                if V == sizes[-1] and nq == 1:
                    ok = ok and max(res[new]) < min(res[old])
            cert_scan, plain_scan = (lambda: cert._scan_certified(table, qs, 20)), (lambda: plain._scan(ptable, qs, 1))
            k16, k32 = kernel_ms(cert_scan, 50), kernel_ms(plain_scan, 50)
            t16, t32 = device_ms(cert_scan, 50), device_ms(plain_scan, 50)
            passes = (nq + 3) // 4
            b16 = passes * n_clips * 2 * dv + n_clips * 8                   # (the measures ride pass 0 only)
            lines.append(f"    scan kernels, {nq}q ({passes} pass{'es' if passes > 1 else ''}, medians of 50 launches): library_scan_bf16_kernel "
                         f"{k16:8.4f} ms = {b16 / k16 / 1e9:6.3f} TB/s of bf16 rows + measures; library_scan_kernel {k32:8.4f} ms = "
                         f"{passes * n_clips * 4 * dv / k32 / 1e9:6.3f} TB/s of fp32 rows")
            lines.append(f"    whole entries, {nq}q: cone_library_scan_certified {t16:8.4f} ms (the five small stages: {t16 - k16:7.4f} ms), "
                         f"cone_library_scan {t32:8.4f} ms (top-k and ranking: {t32 - k32:7.4f} ms)")
            if V == sizes[-1] and nq == 1:
                keep, row = cert.n_cand, []
                for n_cand in (128, 1024, 4096):
                    cert.n_cand = n_cand
                    row.append(f"n_cand = {n_cand}: {device_ms(cert_scan, 50):7.4f} ms")
                cert.n_cand = keep
                lines.append("    cone_library_scan_certified, 1q, by n_cand (the default is 128 at W = 20): " + ", ".join(row))
        plain.close(), cert.close()
        del plain, cert, table, ptable
        torch.cuda.empty_cache()
    lines.append(f"REQUIRED at {sizes[-1]} videos, 1 query: certified below plain in every round pairing, both calls: "
                 + ("holds" if ok else "DOES NOT HOLD"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
