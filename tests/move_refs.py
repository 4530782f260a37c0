"""Models, named cases and planted errors for library maintenance (cone_library_move_rows; compaction_moves / plan_steps of
cone_amd/library.py).  numpy only, no GPU.

The arena model: a list of planes, plane p an int32 array (capacity, words per row) whose word w of row r holds
``encode(p, r, w)`` -- every word of the arena is unique, so a row that lands in the wrong place, a plane that is left out or a
row that is overwritten before it is read shows in the bits.  The truth of a move list is a sequential ``memmove`` in arena
order.  A step (one C call) is modelled as the call promises to behave: a DIRECT step copies in no particular order, so its
model first asserts that the rows it writes and the rows it reads are disjoint (``Overlap`` otherwise) -- that is what makes
the launch's internal order irrelevant --; a STAGED step is a gather of all its rows followed by a scatter.

Which named case catches which planted error (``CATCHES``; tests/test_library_compact_cpu.py holds the table to it):
    seam_off_by_one         a step ends one row early: the row at every seam is never moved      stage_below_video, stage_video_minus_1
    direct_where_overlap    overlapping rows copied directly (modelled back to front)            shift_700_by_1, one_row_shift_1 is NOT enough
    steps_reversed          the plan's steps run last to first                                   three_chained, mixed_plan
    plane_skipped           the last plane is not moved                                          every case that moves a row
"""
import numpy as np

TILE = 16                   # flat rows per workgroup of library_move_kernel (csrc/library_move.hip: MOVE_TILE)
NEW_SYMBOLS = ("cone_library_move_stage_bytes", "cone_library_move_rows")
CPU_WORDS = (2, 2, 1, 3)    # words per row of the CPU tests' small planes (the GPU tests take the handle's widths)


class Overlap(AssertionError):
    """A direct step whose destination rows and source rows are not disjoint."""


# ------------------------------------------------------------------------------------------------ the arena
def encode(p, r, w):
    return (np.int64(p) << 28 | np.asarray(r, dtype=np.int64) << 10 | np.asarray(w, dtype=np.int64)).astype(np.int32)


def fill(planes):
    """Writes the pattern into every row of every plane (views are written in place)."""
    for p, plane in enumerate(planes):
        cap, words = plane.shape
        assert words < 1024 and cap < (1 << 18) and p < 8
        plane[:] = encode(p, np.arange(cap)[:, None], np.arange(words)[None, :])
    return planes


def arena(capacity, words=CPU_WORDS):
    return fill([np.empty((capacity, w), dtype=np.int32) for w in words])


def plane_words(v_dim, hidden_dim, bf16, has_qkv):
    """int32 words per row of the planes a library holds, in arena order (arena_layout of csrc/session.hip)."""
    words = [v_dim] + ([v_dim // 2] if bf16 else [v_dim]) + [hidden_dim] + ([3 * hidden_dim] if has_qkv else [])
    return tuple(words)


# ------------------------------------------------------------------------------------------------ the truth and the steps
def truth_moves(videos):
    """First principles: the videos in arena order, each at the end of its predecessor."""
    out, at = [], 0
    for row0, n in sorted(videos):
        out.append((row0, at, n))
        at += n
    return out


def memmove_truth(planes, moves):
    """Sequential memmove in arena order on copies of the planes."""
    out = [p.copy() for p in planes]
    for s, d, n in moves:
        for p in out:
            p[d:d + n] = p[s:s + n].copy()
    return out


def flat_rows(moving):
    """(src row, dst row) of every flat row of the move list."""
    return [(s + k, d + k) for s, d, n in moving for k in range(n)]


def apply_step(planes, moving, begin, end, staged, planted=None):
    rows = flat_rows(moving)[begin:end - 1 if planted == "seam_off_by_one" and end < sum(m[2] for m in moving) else end]
    n_planes = len(planes) - (planted == "plane_skipped")
    if staged and planted != "direct_where_overlap":
        for p in planes[:n_planes]:
            stage = np.stack([p[s] for s, _ in rows]) if rows else None         # gather ...
            for k, (_, d) in enumerate(rows):                                   # ... then scatter
                p[d] = stage[k]
        return
    if planted != "direct_where_overlap" and {d for _, d in rows} & {s for s, _ in rows}:
        raise Overlap(f"direct step [{begin}, {end}) writes rows it reads")
    for p in planes[:n_planes]:
        for s, d in reversed(rows):             # (no order is promised: back to front is the one a downward memmove must not take)
            p[d] = p[s]


def run_plan(planes, moves, steps, planted=None):
    """The steps of a plan on copies of the planes: what the C calls leave behind."""
    out = [p.copy() for p in planes]
    moving = [m for m in moves if m[0] != m[1]]
    for begin, end, staged in (reversed(steps) if planted == "steps_reversed" else steps):
        apply_step(out, moving, begin, end, staged, planted)
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def step_sets(moving, begin, end):
    rows = flat_rows(moving)[begin:end]
    return {s for s, _ in rows}, {d for _, d in rows}


# ------------------------------------------------------------------------------------------------ named cases
# name -> (capacity, [(row0, n), ...], stage_rows)
CASES = {
    f"tile_{n}": (n + 8, [(5, n)], 64) for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
}
CASES.update({
    "one_row_shift_1": (4, [(1, 1)], 8),
    "shift_700_by_1": (702, [(1, 700)], 1000),                         # heavy self-overlap: one staged step
    "three_chained": (170, [(20, 100), (120, 20), (140, 20)], 50),     # each video's dst lies inside its predecessor's src
    "stage_below_video": (110, [(7, 100)], 30),                        # step seams inside a move
    "stage_video_minus_1": (140, [(3, 64), (70, 64)], 63),
    "stage_video_plus_1": (140, [(3, 64), (70, 64)], 65),
    "hole_front": (90, [(9, 40), (49, 30)], 16),
    "hole_middle": (90, [(0, 40), (52, 30)], 16),
    "hole_end": (90, [(0, 40), (40, 30)], 16),                         # nothing moves
    "mixed_plan": (320, [(2, 30), (100, 200)], 16),                    # staged steps (one across the videos' seam), then direct ones
})

PLANTED = ("seam_off_by_one", "direct_where_overlap", "steps_reversed", "plane_skipped")
CATCHES = {
    "seam_off_by_one": ("stage_below_video", "stage_video_minus_1", "mixed_plan"),
    "direct_where_overlap": ("shift_700_by_1", "three_chained", "stage_below_video"),
    "steps_reversed": ("three_chained", "mixed_plan", "stage_below_video"),
    "plane_skipped": tuple(k for k in CASES if k != "hole_end"),
}


def history(rng, capacity=400, steps=40):
    """A random add / remove history on a first-fit free list (the library's RowRanges): the surviving (row0, n)."""
    from cone_amd.library import RowRanges
    rows, videos = RowRanges(capacity), []
    for _ in range(steps):
        if videos and rng.random() < 0.45:
            rows.release(*videos.pop(int(rng.integers(len(videos)))))
        else:
            n = int(rng.integers(1, 60))
            if rows.largest >= n:
                videos.append((rows.take(n), n))
    return rows, videos
