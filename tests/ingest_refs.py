"""Shared by tests/test_library_ingest_cpu.py and tests/test_library_ingest_gpu.py: the row model of tests/library_refs.py with
exact claims (``take_at``), first-principles models of what sequential ``add`` calls, ``extend`` and ``plan_runs`` must decide,
a library object without a GPU, and the row counts at which the video half's launchers change form.  numpy only, no GPU."""
import os
import re
from types import SimpleNamespace

import numpy as np

import library_refs as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ row ownership
class RowModel(L.RowModel):
    """One flag per row; an exact claim succeeds when every row asked for is free (free neighbours are one hole by construction)."""

    def take_at(self, start, n):
        if n < 1 or start < 0 or start + n > len(self.used) or self.used[start:start + n].any():
            return None
        self.used[start:start + n] = True
        return start


# (op, start or name, n) on 100 rows.  Holes after the set-up: [10, 40) and [60, 100)
TAKE_AT_CAPACITY = 100
TAKE_AT_SCRIPT = [
    ("take", "a", 10), ("take", "b", 30), ("take", "c", 20), ("release", "b", 0),   # holes [10, 40), [60, 100)
    ("take_at", 10, 5),             # a hole's start
    ("take_at", 20, 5),             # a hole's middle: [15, 20) and [25, 40) remain
    ("take_at", 35, 5),             # a hole's end: [25, 35) remains
    ("take_at", 15, 5),             # a whole hole
    ("refuse_at", 30, 35),          # straddles two holes (and the owned rows between them)
    ("refuse_at", 34, 2),           # one owned row at its end
    ("refuse_at", 45, 1),           # an owned row
    ("refuse_at", 24, 3),           # one owned row at its start
    ("refuse_at", 95, 6),           # past the capacity
    ("refuse_at", -1, 2),
    ("refuse_at", 70, 0),
    ("take_at", 60, 40),            # a whole hole up to the capacity
    ("release", "c", 0),            # [40, 60) free again, between owned rows
    ("take_at", 25, 10),
    ("refuse_at", 39, 2), ("take_at", 40, 20),
]


# ------------------------------------------------------------------------------------------------ placement models
def model_of(capacity, owned):
    m = RowModel(capacity)
    for row0, n in owned:
        assert not m.used[row0:row0 + n].any()
        m.used[row0:row0 + n] = True
    return m


def sequential_add(capacity, owned, lens):
    """What ``[lib.add(v) for v in videos]`` decides on an arena whose rows ``owned`` are taken: (placements, holes), or
    (index of the first video that finds no hole, None)."""
    m = model_of(capacity, owned)
    placed = []
    for i, n in enumerate(lens):
        start = m.take(n)
        if start is None:
            return i, None
        placed.append((start, n))
    return placed, m.holes()


def runs_model(placements):
    """First principles: walk the list, a video continues the run when it starts where the one before ends."""
    runs = []
    for i, (row0, n) in enumerate(placements):
        if i and placements[i - 1][0] + placements[i - 1][1] == row0:
            runs[-1][1] += n
            runs[-1][3] = i + 1
        else:
            runs.append([row0, n, i, i + 1])
    return [tuple(r) for r in runs]


def extend_model(capacity, owned, row0, n, m):
    """The decision of ``extend`` for the video (row0, n) of ``owned``: in place when the m rows behind it are free; else the
    lowest start whose n + m rows are all free; else no room."""
    model = model_of(capacity, owned)
    end = row0 + n
    if end + m <= capacity and not model.used[end:end + m].any():
        return "in_place", row0
    for start, length in model.holes():
        if length >= n + m:
            return "relocate", start
    return "no_room", None


# ------------------------------------------------------------------------------------------------ a library without a GPU
def stub_library(capacity, videos, max_v_l=90, topk_window=20):
    """tests/test_library_compact_cpu.py's stub with the model's own width check: no handle, no arena, no GPU.  ``videos`` =
    [(row0, n), ...] taken with ``take_at`` (any layout); ``lib.launched`` records what ``_index`` / ``_move`` / ``compact``
    were asked to do instead of doing it."""
    from cone_amd.library import RowRanges, VideoLibrary, compaction_moves
    from cone_amd.model import CONE
    from cone_amd import ops
    handle = SimpleNamespace(value=1)
    model = SimpleNamespace(_handle=handle, _h=lambda: handle, _check_dim=CONE._check_dim)
    lib = object.__new__(VideoLibrary)
    lib._loc = SimpleNamespace(args=SimpleNamespace(v_appear_feat_dim=256, v_motion_feat_dim=256, max_v_l=max_v_l, topk_window=topk_window),
                               localizator=model, device="cpu")
    lib._handle_obj, lib._handle_value, lib._open = handle, 1, True
    lib.max_q_l, lib._rows, lib._videos, lib._next_id, lib._scan_cache = 20, RowRanges(capacity), {}, 1, "stale"
    for row0, n in videos:
        lib._rows.take_at(row0, n)
        lib._videos[lib._next_id] = (row0, n, min(topk_window, ops.num_windows(n, max_v_l)))
        lib._next_id += 1
    lib.launched = []
    lib._index = lambda raw, launches: lib.launched.append(("index", tuple(raw.shape), list(launches)))
    lib._move = lambda src, dst, moves, steps, stage: lib.launched.append(("move", list(moves), list(steps)))
    lib._cl = None

    def compact():
        ids = sorted(lib._videos, key=lambda v: lib._videos[v][0])
        moves = compaction_moves([lib._videos[v][:2] for v in ids])
        for v, (_, dst, _) in zip(ids, moves):
            lib._videos[v] = (dst,) + lib._videos[v][1:]
        lib._rows.compacted()
        lib._scan_cache = None
        lib.launched.append(("compact",))
    lib.compact = compact
    return lib


def state(lib):
    return dict(lib._videos), list(lib._rows.holes), lib._next_id


# ------------------------------------------------------------------------------------------------ form thresholds of the chain
def gemm_constants():
    """The constants of csrc/gemm.hip and csrc/gemm_tall.h that the row counts below are derived from."""
    with open(os.path.join(ROOT, "cone_amd", "csrc", "gemm.hip")) as f:
        src = f.read()
    with open(os.path.join(ROOT, "cone_amd", "csrc", "gemm_tall.h")) as f:
        tall = f.read()
    return dict(RSP_MAX_GROUPS=int(re.search(r"constexpr int RSP_MAX_GROUPS = (\d+);", src).group(1)),
                RSP_MAX_TILES=int(re.search(r"constexpr int RSP_MAX_TILES = (\d+);", src).group(1)),
                RS_MAX_WGS=int(re.search(r"#define CONE_RS_MAX_WGS (\d+)", src).group(1)),
                TALL_MIN_ROWS=int(re.search(r"#define CONE_GEMM_TALL_MIN_ROWS (\d+)", tall).group(1)))


def threshold_rows(c=None):
    """Last row count of the spread form and of the small form at N = 768 and N = 256 (16-row groups; the spread form holds at
    most RSP_MAX_GROUPS groups and RSP_MAX_TILES 16 x 16 tiles, the small form RS_MAX_WGS workgroups of 16 rows x 256 columns)."""
    c = c or gemm_constants()
    spread = lambda N: 16 * min(c["RSP_MAX_GROUPS"], c["RSP_MAX_TILES"] // (N // 16))
    small = lambda N: 16 * (c["RS_MAX_WGS"] // (N // 256))
    return dict(spread_768=spread(768), spread_256=spread(256), small_768=small(768), small_256=small(256))


def pin_row_counts(c=None):
    """Tile edges, then either side of every form threshold."""
    t = threshold_rows(c)
    counts = [1, 15, 16, 17, 127, 128, 129]
    for k in ("spread_768", "spread_256", "small_768", "small_256"):
        counts += [t[k], t[k] + 1]
    return counts


REDUCED_KEYS = ("spread_768", "spread_256", "small_768")


def reduced_row_counts(c=None):
    t = threshold_rows(c)
    return [1, 17] + [t[k] + 1 for k in REDUCED_KEYS]
