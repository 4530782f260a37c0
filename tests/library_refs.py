"""Shared by tests/test_library_cpu.py and tests/test_library_gpu.py: the numpy model of a library call's index metadata
(tests/session_refs.py's, with a video per query), a first-principles model of first-fit row ownership, and the cases both
files walk."""
import numpy as np

import session_refs as S

NEW_SYMBOLS = ("cone_library_arena_bytes", "cone_library_open", "cone_library_add_workspace", "cone_library_add",
               "cone_library_query_layout", "cone_library_localize_workspace", "cone_library_localize")

MAX_Q_L, MAX_V_L, NUM_QUERIES, TOPK_WINDOW = S.MAX_Q_L, S.MAX_V_L, S.NUM_QUERIES, 20
OUTPUTS = S.OUTPUTS
INT32_MAX = 2 ** 31 - 1


def num_windows(ctx_l, max_v_l=MAX_V_L):
    """cone/ego4d_mad_dataloader.py:146: ceil(ctx_l / slide) + 1 windows, slide = max_v_l / 2."""
    slide = max_v_l // 2
    return -(-ctx_l // slide) + 1


def layout_model(tok_len, ctx_l, row0, K, num_queries=NUM_QUERIES, max_v_l=MAX_V_L):
    """session_refs.layout_model with q_ctx_l / q_vid_off per query."""
    out = S.layout_model(tok_len, 0, K, num_queries, max_v_l)
    out["q_ctx_l"] = np.asarray(ctx_l, dtype=np.int32)
    out["q_vid_off"] = np.asarray(row0, dtype=np.int32)
    assert len(out["q_ctx_l"]) == len(out["q_vid_off"]) == len(tok_len)
    return out


def _ragged(nq, seed, lo, hi):
    return [int(v) for v in np.random.default_rng(seed).integers(lo, hi + 1, nq)]


def _stacked(ctx):
    """Videos back to back from row 0."""
    return [int(v) for v in np.concatenate([[0], np.cumsum(ctx)[:-1]])]


_C64 = _ragged(64, 7, 900, 7000)
# (token lengths, q_ctx_l, q_row0, K): nq 1 / 2 / 64; token sums 255 / 256 / 257 (the layout kernel's 256 threads); one video
# for all, a video per query, runs; row offsets up to the last one an int32 row index can address
LAYOUT_CASES = [
    ([1], [1], [0], 2), ([20], [900], [5000], 20), ([7], [333], [INT32_MAX - 333], 9),
    ([1, 1], [46, 46], [10, 10], 3), ([20, 20], [6000, 900], [0, 6000], 20), ([3, 17], [91, 333], [333, 0], 4),
    ([1] * 64, [900] * 64, [123] * 64, 20), ([20] * 64, _C64, _stacked(_C64), 20),
    (S._mixed(64, 3), [900] * 30 + [33000] * 34, [0] * 30 + [INT32_MAX - 33000] * 34, 20),
    ([20] * 12 + [15], [900] * 13, _stacked([900] * 13), 20), ([20] * 12 + [16], [900] * 6 + [1000] * 7, [0] * 6 + [900] * 7, 20),
    ([20] * 12 + [17], _ragged(13, 9, 45, 46), _stacked([46] * 13), 2),
    (S._mixed(17, 5), _ragged(17, 11, 1, 45), _ragged(17, 13, 0, 10 ** 9), 2),
]


class RowModel:
    """First-fit with coalescing from first principles: one flag per row.  A request of n rows gets the lowest start whose n
    rows are all free; freeing clears the flags (so neighbouring holes are one hole by construction)."""

    def __init__(self, capacity):
        self.used = np.zeros(capacity, dtype=bool)

    def holes(self):
        out, start = [], None
        for i, u in enumerate(list(self.used) + [True]):
            if not u and start is None:
                start = i
            if u and start is not None:
                out.append((start, i - start))
                start = None
        return out

    def take(self, n):
        for start, length in self.holes():
            if length >= n:
                self.used[start:start + n] = True
                return start
        return None

    def release(self, start, n):
        assert self.used[start:start + n].all()
        self.used[start:start + n] = False


# (op, name, clips): the scripted sequence of the issue on 100 rows -- fill; remove the middle, refill smaller; remove
# neighbours so they coalesce; exact fit; a refusal that names the largest hole
ROW_CAPACITY = 100
ROW_SCRIPT = [
    ("add", "a", 30), ("add", "b", 30), ("add", "c", 30), ("add", "d", 10),         # full
    ("refuse", "x", 1),
    ("remove", "b", 0), ("add", "e", 20),                                           # into b's hole, 10 left behind it
    ("refuse", "x", 11),                                                            # largest hole: 10
    ("remove", "c", 0),                                                             # 10 + 30 coalesce -> 40
    ("refuse", "x", 41), ("add", "f", 40),                                          # exact fit
    ("remove", "a", 0), ("remove", "e", 0),                                         # neighbours: [0, 50) is one hole
    ("refuse", "x", 51), ("add", "g", 50),
    ("remove", "d", 0), ("remove", "f", 0),                                         # tail hole [50, 100)
    ("add", "h", 7), ("add", "i", 43), ("refuse", "x", 1),
    ("remove", "g", 0), ("remove", "i", 0), ("remove", "h", 0),                     # out of order: everything is one hole again
    ("add", "j", 100),
]
