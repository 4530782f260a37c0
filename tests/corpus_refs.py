"""Library moment search: the model of ``cone_corpus_fuse_nms`` and the tables the kernel tests dictate.

``pool_ref`` restates run_on_video/cone_localizator.py:187-221 (and utils/temporal_nms.py:25-74) for ONE query whose candidates
are a pool of segments, each segment the rows of one (video, query) pair: the dict key carries the segment's tag (its video) and
a kept moment suppresses only moments of its own tag.  Plain Python floats, ``float(f"{e:.4f}")``, ``sorted(reverse=True)``, a
dict -- the kernel runs the same operations in fp64, so every comparison is bit for bit.  ``mut`` plants one error at a time
(``MUTATIONS``): each is caught by a named case of tests/test_library_corpus_cpu.py."""
import functools

import numpy as np

NEW_SYMBOLS = ("cone_corpus_fuse_nms", "cone_library_localize_candidates_workspace", "cone_library_localize_candidates")
N_ARGS = {"cone_corpus_fuse_nms": 14, "cone_library_localize_candidates_workspace": 9, "cone_library_localize_candidates": 21}
MAX_POOL = 1024
MUTATIONS = ("norm_per_segment", "key_without_tag", "nms_across_tags", "first_value_wins", "unstable_sort", "cut_after_nms")


def _normalize(values):
    lo, hi = min(values), max(values)
    return list(values) if lo == hi else [(v - lo) / (hi - lo) for v in values]


def _iou(a, b):
    inter = max(0, min(a[1], b[1]) - max(a[0], b[0]))
    union = max(a[1], b[1]) - min(a[0], b[0])
    return 0 if union == 0 else 1.0 * inter / union


def _nms(moments, thd, max_after, across_tags=False):
    """``moments`` = [[tag, st, ed, score], ...] in score order; a list of one is returned untouched."""
    if len(moments) == 1:
        return moments
    rest, kept = list(moments), []
    while len(rest) > 1 and len(kept) < max_after:
        head = rest[0]
        rest = [head] + [m for m in rest[1:] if not ((across_tags or m[0] == head[0]) and _iou(head[1:3], m[1:3]) > thd)]
        kept.append(rest.pop(0))
    if len(kept) < max_after and len(rest) >= 1:
        kept.append(rest.pop(0))
    return kept


def pool_ref(cand, segments, thd, max_before, max_after, mut=()):
    """``cand`` (rows, 4) fp32 [st, ed, prop, match]; ``segments`` = [(first row, rows, tag), ...] of one query, in table order.
    Returns (rows (max_after, 5) fp64 [st, ed, prop, match, fused], seg (max_after,) int32, n): the kept moments, the ordinal
    of the segment each one's key first occurred in, their number; 0.0 / -1 past them.  At most MAX_POOL candidates are taken,
    the segment that crosses the cap truncated (the kernel's clamp; the wrapper never builds such a table)."""
    mut = frozenset(mut)
    assert mut <= set(MUTATIONS)
    cand = np.asarray(cand)
    total, seg_of = [], []
    for s, (row0, n, tag) in enumerate(segments):
        for r in range(max(int(n), 0)):
            if len(total) == MAX_POOL:
                break
            total.append([int(tag)] + [float(f"{e:.4f}") for e in cand[row0 + r].tolist()])
            seg_of.append(s)
    rows, seg = np.zeros((max_after, 5), np.float64), np.full(max_after, -1, np.int32)
    if not total:
        return rows, seg, 0
    if "norm_per_segment" in mut:
        prop, match = [], []
        for s in range(len(segments)):
            mine = [item for item, so in zip(total, seg_of) if so == s]
            if mine:
                prop += _normalize([item[3] for item in mine])
                match += _normalize([item[4] for item in mine])
    else:
        prop, match = _normalize([item[3] for item in total]), _normalize([item[4] for item in total])
    fusion = [sum(x) for x in zip(prop, match)]
    table, first = {}, {}
    for i, (item, score) in enumerate(zip(total, fusion)):
        key = (item[1], item[2]) if "key_without_tag" in mut else (item[0], item[1], item[2])
        if "first_value_wins" in mut and key in table:
            continue
        if key not in first:
            first[key] = (i, item[0])
        table[key] = [item[3], item[4], score]
    moments = [[first[k][1], k[-2], k[-1], v[2]] for k, v in table.items()]
    if "unstable_sort" in mut:
        moments = sorted(moments, key=lambda x: x[3])[::-1]
    else:
        moments = sorted(moments, key=lambda x: x[3], reverse=True)
    if thd == -1:
        kept = moments[:max_after]
    elif "cut_after_nms" in mut:
        kept = _nms(moments, thd, len(moments), "nms_across_tags" in mut)[:max_before][:max_after]
    else:
        kept = _nms(moments[:max_before], thd, max_after, "nms_across_tags" in mut)
    for j, m in enumerate(kept):
        key = (m[1], m[2]) if "key_without_tag" in mut else (m[0], m[1], m[2])
        rows[j] = (m[1], m[2], table[key][0], table[key][1], table[key][2])
        seg[j] = seg_of[first[key][0]]
    return rows, seg, len(kept)


def moments_of(rows, seg, n, tags):
    """What ``search_moments`` returns for a query from the kernel's outputs: [(tag, [st, ed, fused]), ...]."""
    return [(tags[int(seg[j])], [float(rows[j, 0]), float(rows[j, 1]), float(rows[j, 4])]) for j in range(n)]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


# ---- hand-made tables ---------------------------------------------------------------------------------------------------------
def _rows(*r):
    return np.asarray(r, dtype=np.float32)


def two_videos():
    """A: props 0.9 / 0.1, B: 0.3 / 0.2, every match 0.5: per pair both tops fuse to 1.5; pooled A 1.5, B 0.75."""
    cand = _rows([0, 10, .9, .5], [20, 30, .1, .5], [0, 10, .3, .5], [20, 30, .2, .5])
    return cand, [(0, 2, 7), (2, 2, 9)]


def same_span_two_tags():
    cand = _rows([5, 15, .9, .2], [40, 50, .1, .1], [5, 15, .4, .6], [70, 80, .3, .3])
    return cand, [(0, 2, 1), (2, 2, 2)]


def identical_spans_two_videos():
    """The second video's moment lies on the first's: IoU 1 across tags, both kept; the third row overlaps inside video 1."""
    cand = _rows([0, 10, .9, .9], [1, 10, .5, .5], [0, 10, .8, .8], [100, 110, .1, .1])
    return cand, [(0, 2, 1), (2, 2, 2)]


def dup_in_segment():
    """(5, 15) three times in one segment with other scores: position of the first, values of the last."""
    cand = _rows([5, 15, .2, .1], [40, 50, .6, .5], [5, 15, .9, .9], [70, 80, .5, .6], [5, 15, .7, .3])
    return cand, [(0, 5, 3)]


def ties_across_segments():
    cand = _rows([0, 10, .5, .5], [20, 30, .9, .1], [40, 50, .5, .5], [60, 70, .1, .9], [80, 90, .5, .5], [100, 110, .5, .5])
    return cand, [(0, 2, 4), (2, 2, 2), (4, 2, 4)]


def cut_then_nms():
    """Rows 2 and 3 lie on row 1: with max_before = 3 the cut leaves one moment; NMS first would let the fourth through."""
    cand = _rows([0, 10, .9, .9], [0, 10.5, .8, .8], [0, 11, .7, .7], [50, 60, .6, .6], [80, 90, .1, .1])
    return cand, [(0, 5, 1)]


def iou_edges():
    """Same tag: [0, 20] against [0, 10] is exactly 0.5 (kept), [0, 19.9] is just above (suppressed); tag 2 repeats [0, 19.9]."""
    cand = _rows([0, 10, .9, .9], [0, 20, .8, .8], [0, 19.9, .7, .7], [0, 19.9, .6, .6], [300, 310, .1, .1])
    return cand, [(0, 3, 1), (3, 2, 2)]


def two_segments_one_tag():
    """Segments 0 and 2 are one video: their equal span collapses (values of the last) and their moments suppress each other."""
    cand = _rows([5, 15, .3, .3], [40, 50, .9, .8], [5, 15, .5, .5], [5, 15, .7, .9], [41, 50, .6, .6])
    return cand, [(0, 2, 1), (2, 1, 2), (3, 2, 1)]


HAND_MADE = dict(two_videos=two_videos, same_span_two_tags=same_span_two_tags, identical_spans_two_videos=identical_spans_two_videos,
                 dup_in_segment=dup_in_segment, ties_across_segments=ties_across_segments, cut_then_nms=cut_then_nms,
                 iou_edges=iou_edges, two_segments_one_tag=two_segments_one_tag)
# the planted error -> (the hand-made table that catches it, (thd, max_before, max_after))
CAUGHT_BY = dict(norm_per_segment=("two_videos", (0.5, 100, 5)), key_without_tag=("same_span_two_tags", (0.5, 100, 5)),
                 nms_across_tags=("identical_spans_two_videos", (0.5, 100, 5)), first_value_wins=("dup_in_segment", (0.5, 100, 5)),
                 unstable_sort=("ties_across_segments", (0.5, 100, 5)), cut_after_nms=("cut_then_nms", (0.5, 3, 5)))


# ---- dictated pools -----------------------------------------------------------------------------------------------------------
POOL_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024)
FAMILIES = ("distinct", "all_equal", "dup_in_segment", "span_under_every_tag", "fused_ties", "cut_in_ties", "past_fourth")


def split(n, n_seg, seed):
    """``n`` rows over ``n_seg`` segments of at least one row (as even as the seed's shuffle leaves it)."""
    assert 1 <= n_seg <= n
    rng = np.random.default_rng(seed)
    sizes = np.full(n_seg, n // n_seg)
    sizes[:n % n_seg] += 1
    return rng.permutation(sizes).tolist()


def pool_case(family, sizes, seed=0, n_tags=3):
    """One query's pool: (cand (n, 4) fp32, [(first row, rows, tag), ...]) for the segment sizes given.  Tags repeat (segment s
    is video s % n_tags, so two segments of one tag are one video) and the segments lie in the buffer in ANOTHER order than in
    the table, so seg_cand is what finds them."""
    return _pool_case(family, tuple(int(s) for s in sizes), seed, n_tags)


@functools.lru_cache(maxsize=None)
def _pool_case(family, sizes, seed, n_tags):
    rng = np.random.default_rng(50000 + 1000 * FAMILIES.index(family) + seed + sum(sizes))
    n = sum(sizes)
    st = np.round(rng.uniform(0, 500, n), 2)
    ed = st + np.round(rng.uniform(1, 60, n), 2)
    pr, ma = rng.uniform(0, 1, n), rng.uniform(-0.2, 0.6, n)
    start = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(int)
    tags = [100 + s % n_tags for s in range(len(sizes))]
    if family == "all_equal":
        pr[:], ma[:] = 0.3125, -0.125
    elif family == "dup_in_segment":
        for a, k in zip(start, sizes):
            if k >= 2:
                st[a + k - 1], ed[a + k - 1] = st[a], ed[a]
    elif family == "span_under_every_tag":
        st[start], ed[start] = 10.0, 20.0           # every segment's first row: equal tags collapse, different tags do not
    elif family == "fused_ties":
        pr, ma = rng.choice([0.25, 0.5, 0.75], n), rng.choice([0.0, 0.5], n)
    elif family == "cut_in_ties":                   # disjoint spans: nothing is suppressed, the cut at max_before decides
        st = 100.0 * np.arange(n)
        ed = st + 10
        hi = min(n, 90)
        pr[:hi], ma[:hi] = np.linspace(1.0, 0.6, hi), 0.5
        pr[hi:], ma[hi:] = 0.25, 0.5
    elif family == "past_fourth":                   # three spans and two scores, blurred past the fourth decimal
        j = rng.integers(0, 3, n)
        st = 12.5 * j + rng.uniform(-4e-5, 4e-5, n)
        ed = 12.5 * j + 30 + rng.uniform(-4e-5, 4e-5, n)
        pr = 0.25 * (1 + rng.integers(0, 2, n)) + rng.uniform(-4e-5, 4e-5, n)
        ma = 0.5 + rng.uniform(-4e-5, 4e-5, n)
    cand = np.stack([st, ed, pr, ma], 1).astype(np.float32)
    place = rng.permutation(len(sizes))             # where each segment lies in the buffer
    out, segs, at = np.zeros((n, 4), np.float32), [None] * len(sizes), 0
    for s in place:
        out[at:at + sizes[s]] = cand[start[s]:start[s] + sizes[s]]
        segs[s] = (at, sizes[s], tags[s])
        at += sizes[s]
    out.setflags(write=False)
    return out, segs


def assemble(cases):
    """Queries ``[(cand, segments), ...]`` -> one flat buffer and table: (cand (rows, 4) fp32, seg_off (nq + 1) int32, seg_cand
    int64, seg_n int32, seg_tag int32, per query [(first row, rows, tag), ...] in the flat buffer)."""
    rows, seg_off, seg_cand, seg_n, seg_tag, per_q, at = [], [0], [], [], [], [], 0
    for cand, segs in cases:
        mine = [(at + r0, n, tag) for r0, n, tag in segs]
        per_q.append(mine)
        for r0, n, tag in mine:
            seg_cand.append(r0); seg_n.append(n); seg_tag.append(tag)
        seg_off.append(len(seg_cand))
        rows.append(np.asarray(cand, np.float32).reshape(-1, 4))
        at += len(rows[-1])
    flat = np.concatenate(rows) if rows else np.zeros((0, 4), np.float32)
    return (flat, np.asarray(seg_off, np.int32), np.asarray(seg_cand, np.int64), np.asarray(seg_n, np.int32),
            np.asarray(seg_tag, np.int32), per_q)
