"""Latency of compacting / resizing a video library against the parent's only way to the same state -- a fresh library and an
``add`` of every remaining video from its raw clip features --, and the mover's achieved HBM rate; ONE process, one session of
the card.

usage: python tools/library_compact_bench.py [--calls 200] [--rounds 3] [--videos 256] [--clips 900]
                                             [--out profiles/library_compact_latency.txt]

A library of --videos videos of --clips clips with every second one removed (the first, third, ...), so every remaining video
moves and the plan is staged steps followed by direct ones.  Per round, the median over --calls timed calls -- each timed on the
host from its start until the device has finished, inputs resident on the device; the fragmented state is put back between
calls, outside the timed part -- of:
  (a) compact()                 the default 256 MiB staging buffer
      compact(small stage)      --small-stage-mib: no step fits the buffer's rows below its gap, so every step is direct
      re-add                    the parent: open_library(capacity) + add(raw features) per remaining video
  (b) resize(2 x capacity)      one direct call into the new arena
      re-add, 2 x capacity      the parent into a library of that size
compact (both) and resize must not take longer than their re-add in any round pairing; the tool exits non-zero otherwise.
Recorded next to it: launches per call, and bytes read + written (2 x the moved bytes for a direct step, 4 x for a staged one)
over the call's time, next to the 8 TB/s HBM peak.
  (c) the cone_library_move_rows calls of the three plans alone -- table and staging buffer resident --, device time by
      events: the same bytes over the mover's own time.  Recorded, not gated.
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
from cone_amd import _lib, synth  # noqa: E402
from cone_amd.library import compaction_moves, plan_steps  # noqa: E402
from cone_amd.localizator import CONELocalizator, LOCALIZER_OPT  # noqa: E402
from session_bench import verdict  # noqa: E402

HBM_PEAK = 8.0e12


def snapshot(lib):
    return lib._arena, lib._cl, copy.deepcopy(lib._rows), dict(lib._videos)


def restore(lib, snap, pristine=None):
    """Puts the fragmented state back: the bookkeeping, the arena tensor and (after a compaction in place) its bytes."""
    lib._arena, lib._cl, lib._rows, lib._videos = snap[0], snap[1], copy.deepcopy(snap[2]), dict(snap[3])
    lib._scan_cache = None
    if pristine is not None:
        lib._arena.copy_(pristine)


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


def device_ms(lib, dst_cl, moving, steps, reset, calls, warmup):
    """Median device ms (events) of the steps' cone_library_move_rows calls alone: the table and the staging buffer are
    resident, reset() is enqueued ahead of the first event."""
    import ctypes as C
    import numpy as np
    clib, h, n = _lib.load(), lib._loc.localizator._h(), len(moving)
    table = np.zeros(3 * n + 1, dtype=np.int64)
    table[:n], table[n:2 * n] = [m[0] for m in moving], [m[1] for m in moving]
    np.cumsum([m[2] for m in moving], out=table[2 * n + 1:])
    dev, total = torch.from_numpy(table).cuda(), int(table[-1])
    at = lambda k: C.c_void_p(dev.data_ptr() + 8 * k)
    rows = max((e - b for b, e, s in steps if s), default=0)
    need = clib.cone_library_move_stage_bytes(C.byref(lib._cl), rows) if rows else 0
    stage = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    ts = []
    for i in range(warmup + calls):
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for begin, end, staged in steps:
            _lib.check(clib.cone_library_move_rows(h, C.byref(lib._cl), C.byref(dst_cl), at(0), at(n), at(2 * n), n, total, begin, end,
                                                   _lib.ptr(stage) if staged else None, need if staged else 0, _lib.stream()))
        b.record()
        b.synchronize()
        if i >= warmup:
            ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--videos", type=int, default=256)
    ap.add_argument("--clips", type=int, default=900)
    ap.add_argument("--small-stage-mib", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(SimpleNamespace(**LOCALIZER_OPT), 0).items()}
    loc = CONELocalizator(state_dict=sd)
    g = torch.Generator().manual_seed(0)
    V, n = a.videos, a.clips
    capacity = V * n
    raw = [(torch.randn(n, 256, generator=g) * 2).cuda() for _ in range(V)]
    query = (torch.randn(12, 768, generator=g).cuda(), torch.randn(256, generator=g).cuda())
    lib = loc.open_library(capacity)
    ids = [lib.add(v) for v in raw]
    for i in range(0, V, 2):
        lib.remove(ids[i])
    kept = list(range(1, V, 2))
    probe = [(ids[i], query) for i in (kept[0], kept[len(kept) // 2], kept[-1])]
    want = lib.predict_moments(probe)
    frag = snapshot(lib)
    pristine = lib._arena.clone()
    row_bytes = lib._cl.v_dim * 8 + lib._cl.hidden_dim * 16
    small = a.small_stage_mib << 20

    # what a call launches and moves (the plan is a function of the layout alone)
    moves = compaction_moves([lib._videos[ids[i]][:2] for i in kept])
    moved = sum(m[2] for m in moves if m[0] != m[1])
    plans = {"default": plan_steps(moves, min(moved, (256 << 20) // row_bytes)), "small": plan_steps(moves, small // row_bytes)}
    launches = {k: sum(2 if s else 1 for _, _, s in p) for k, p in plans.items()}
    traffic = {k: sum((e - b) * row_bytes * (4 if s else 2) for b, e, s in p) for k, p in plans.items()}
    launches["resize"], traffic["resize"] = 1, 2 * len(kept) * n * row_bytes

    # the ways agree before they are timed
    assert lib.compact() == moved and lib.predict_moments(probe) == want and lib.free_clips == capacity - len(kept) * n
    restore(lib, frag, pristine)
    assert lib.compact(stage_bytes=small) == moved and lib.predict_moments(probe) == want
    restore(lib, frag, pristine)
    lib.resize(2 * capacity)
    assert lib.predict_moments(probe) == want and lib.free_clips == 2 * capacity - len(kept) * n
    restore(lib, frag)

    def readd(cap):
        fresh = loc.open_library(cap)
        for i in kept:
            fresh.add(raw[i])
        return fresh
    fresh = readd(capacity)
    assert fresh.predict_moments([(1 + k, query) for k in (0, len(kept) // 2, len(kept) - 1)]) == want
    fresh.close()

    lines = [f"library_compact_bench: {a.calls} calls per median, {a.rounds} rounds, warm-up {a.warmup}; ms per CALL, host clock, "
             f"device finished; {torch.cuda.get_device_name(0)}",
             f"--- {V} videos of {n} clips, every second one removed: {len(kept)} videos = {moved} clips = {moved * row_bytes / 2**20:.1f} MiB "
             f"move (library arena {lib.nbytes / 2**20:.1f} MiB)"]
    nothing = lambda: None
    variants = {
        "(a) compact()": (lambda: lib.compact(), lambda: restore(lib, frag, pristine), "default"),
        f"(a) compact({a.small_stage_mib} MiB stage)": (lambda: lib.compact(stage_bytes=small), lambda: restore(lib, frag, pristine), "small"),
        "(a) re-add": (lambda: readd(capacity).close(), nothing, None),
        "(b) resize(2 x capacity)": (lambda: lib.resize(2 * capacity), lambda: restore(lib, frag), "resize"),
        "(b) re-add, 2 x capacity": (lambda: readd(2 * capacity).close(), nothing, None),
    }
    res = {k: [] for k in variants}
    for r in range(a.rounds):
        for k, (fn, reset, _) in variants.items():
            res[k].append(timed(fn, reset, a.calls, a.warmup if r == 0 else 3))
    for k, v in res.items():
        m, plan = statistics.median(v), variants[k][2]
        line = f"{k:30s} " + "  ".join(f"{x:9.4f}" for x in v) + f"   median {m:9.4f}"
        if plan:
            rate = traffic[plan] / (m * 1e-3)
            line += f"   {launches[plan]:3d} launches, {traffic[plan] / 1e9:6.3f} GB read + written = {rate / 1e12:5.2f} TB/s = " \
                    f"{100 * rate / HBM_PEAK:4.1f} % of the 8 TB/s peak"
        lines.append(line)
    for k, p in plans.items():
        lines.append(f"    plan ({k} stage): " + ", ".join(f"{'staged' if s else 'direct'} {e - b}" for b, e, s in p[:12])
                     + (f", ... ({len(p)} steps)" if len(p) > 12 else ""))
    # (c) the mover's calls alone, by device events
    import ctypes as C
    restore(lib, frag, pristine)
    moving = [m for m in moves if m[0] != m[1]]
    clib, h = _lib.load(), loc.localizator._h()
    n2 = clib.cone_library_arena_bytes(h, 2 * capacity, 0)
    arena2, cl2 = torch.empty(n2, dtype=torch.uint8, device="cuda"), _lib.Library()
    _lib.check(clib.cone_library_open(h, 2 * capacity, 0, _lib.ptr(arena2), n2, C.byref(cl2)))
    back = lambda: lib._arena.copy_(pristine)
    lines.append("--- (c) the cone_library_move_rows calls alone (table and staging buffer resident), device ms by events")
    for k, dst, steps, reset in (("default", lib._cl, plans["default"], back), ("small", lib._cl, plans["small"], back),
                                 ("resize", cl2, [(0, moved, False)], nothing)):
        v = [device_ms(lib, dst, moving, steps, reset, a.calls, a.warmup if r == 0 else 3) for r in range(a.rounds)]
        m = statistics.median(v)
        rate = traffic[k] / (m * 1e-3)
        lines.append(f"(c) {k:28s} " + "  ".join(f"{x:9.4f}" for x in v) + f"   median {m:9.4f}   {launches[k]:3d} launches, "
                     f"{traffic[k] / 1e9:6.3f} GB = {rate / 1e12:5.2f} TB/s = {100 * rate / HBM_PEAK:4.1f} % of the 8 TB/s peak")
    names, ok = list(variants), True
    for new, old in ((names[0], names[2]), (names[1], names[2]), (names[3], names[4])):
        lines.append("  " + verdict(new, res[new], old, res[old]))
        ok = ok and max(res[new]) <= min(res[old])
    lines.append("(the rates of (a) / (b) include the host's part of a call: planning, one table upload, the staging buffer's allocation)")
    lines.append("not measured: prefilter_bf16 libraries, long-window and 128 / 4 handles, other video lengths, arenas beyond this one")
    lines.append("condition compact / resize no longer than the re-add in every round pairing: " + ("holds" if ok else "DOES NOT HOLD"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
