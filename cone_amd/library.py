"""Video libraries: many resident videos in one arena, one call for queries on any mix of them
(``CONELocalizator.open_library``).

A ``VideoSession`` batches the queries of ONE video; a process that keeps many videos resident (a user's recordings, a
catalogue of episodes) receives queries for different videos and would pay the single-query price -- almost all of it launch
latency -- for each.  A ``VideoLibrary`` keeps the video half of ``predict_moment`` (run_on_video/cone_localizator.py:121-221)
of MANY videos in the rows of one arena and answers a list of ``(video, query)`` pairs in one C call per 64 pairs
(``cone_library_localize``, csrc/session.hip).  Nothing new is computed: the window ranking runs per video exactly as in a
session, everything after it is one launch over all windows of all pairs, and every answer equals the localizer's
``predict_moment(video_feats, query)`` with ``==``.

``rank_videos`` / ``search`` answer the question that comes before a pair: which of the resident videos shows this, and where.
One ``cone_library_scan`` (csrc/prefilter.hip) runs the pre-filter over the rows of EVERY video in one pass over the arena --
windows restart at each video's first row, the window lists are the per-video pre-filter's bit for bit -- and ranks the videos
by their best window score (a cosine in the adapter's space: comparable across videos); ``search`` then localizes on the
chosen (video, query) pairs through ``cone_library_localize_ranked``, which takes its window lists from the scan, so the
moments still equal ``predict_moment``'s with ``==``.  ``scan_table`` lays the videos out for the scan (slots by first row,
prefix sums of half-blocks).  fp32 libraries only: a ``prefilter_bf16`` library's search is refused by name.

``search_windows`` spends a BUDGET of windows per query instead of K windows on each of n videos: ``cone_library_budget``
(csrc/library_budget.hip) picks the W best windows over every list of the scan and counts them per video, one small read-back
brings the (video, count) pairs to the host, and ``cone_library_localize_ragged`` -- the library call with a window count PER
PAIR -- runs them (``plan_ragged_calls``: sorted by video, cut at 64 pairs, whatever their counts).  The windows chosen from a
video are a prefix of its stable list, so a video that receives k windows answers with ``predict_moment`` at ``topk_window = k``,
``==``.  ``predict_moments(..., ragged=True)`` / ``windows=[k, ...]`` reach the same call for a caller's own pairs.

``search_moments`` answers what a library is for: the n best moments for a query in everything it holds.  The lists above are
each normalised over the candidates of ONE pair (every pair's best proposal becomes 1.0), so they cannot be merged; here the
budget's pairs run through ``cone_library_localize_candidates`` -- the ragged call stopped before its stage C -- into one
candidate buffer, and ``cone_corpus_fuse_nms`` (csrc/library_corpus.hip) runs the reference's stage C over the whole pool of a
query: both score lists normalised over the pool, the dict keyed by (video, st, ed), NMS inside each video only.
Every budgeted call is built from the same pieces: ``_budget_args`` (the refusals), ``_scan_budget`` (scan + budget per 64
queries), ``decode_budget`` (the read-back's words), ``place_calls`` (the calls' rows in the one candidate buffer) and ``FuseOut``
(stage C's output layout, its launch and its read-back).

Rows are handed out first-fit from a free list and coalesce when a video is removed, so ``add`` / ``remove`` traffic
fragments the arena: by default ``add`` raises when no hole fits, however many clips are free in total.  ``compact`` closes the
holes in place and ``resize`` moves every video into an arena of another size (``add(..., compact=True)`` compacts when that is
what it takes; ``largest_free`` tells a caller when).  Neither recomputes anything: everything the library holds per clip is a
row in four or five planes, a row's bits do not depend on where it lives, so ``cone_library_move_rows``
(csrc/library_move.hip) copies the rows and every answer keeps its bits.  ``compaction_moves`` lays the videos out in arena
order (ids, rankings and their tie order do not change); ``plan_steps`` cuts the moves into calls that never overwrite a row a
later call has yet to read -- staged through a buffer where a call's source and destination rows overlap, direct where they
cannot.

Ingest.  Every launcher of the video half works row by row and a row's bits do not depend on its launch's row count either
(every form of the row GEMM runs the same chains per row; tests/test_library_ingest_gpu.py pins it at the forms' thresholds),
so rows indexed in ANY launch equal the rows of the video's own launch.  ``add_many`` therefore indexes a list of videos with
one upload and one ``cone_library_add`` per run of adjacent ranges (``plan_runs``) and leaves exactly the state sequential
``add`` calls leave; ``extend`` appends clips to a resident video -- in place when the rows behind it are free
(``RowRanges.take_at``), else by moving it into a hole that holds all of it (``plan_extend``) -- indexing only the new rows;
``trim`` drops a video's oldest clips without a launch.  ``extend`` + ``trim`` are the sliding window of a live recording.

``watch`` is what a live recording is for: a fixed set of queries asked again after every few new clips.  A ``VideoWatcher``
(cone_amd/watch.py) keeps the candidate rows of every (query, window) it has computed; its ``poll`` runs the window model only on
the listed windows it has not seen, or saw while they were still growing, and stage C on the cache -- the answer is still
``predict_moment``'s, ``==``.  A ``trim`` resets the video's watchers (``_trimmed``); moves change nothing.
``watch_moments`` is the same economy under ``search_moments``' contract: a ``LibraryWatcher`` keeps one slab of cached windows per
resident video, its ``poll`` answers ``== search_moments`` and runs the window model only on the budget's windows the cache does
not hold (``cone_watch_pool_plan`` / ``cone_watch_pool_store``, csrc/library_watch_pool.hip).

Certified budgets (``open_library(..., certified=True)``).  The scan is the one part of a budgeted search that grows with the
library; a certified library keeps, beside its fp32 arena, a bf16 SHADOW of the adapted rows and two fp32 measures per row
(``cone_library_shadow_index``: a pure function of the adapted rows, so whoever writes or moves rows re-indexes them -- ``add``,
``add_many``, ``extend``, ``compact``, ``resize``; ``remove`` / ``trim`` do nothing).  ``_budgeted`` then takes the lists of
``search_windows`` / ``search_moments`` from ``cone_library_scan_certified`` (csrc/prefilter.hip): the shadow scanned at half
the bytes, the ``n_cand`` best coarse windows of the whole table rescored in fp32 with the scan's own bits, and a proof per
query that the budget's choice is the fp32 scan's.  The flags ride in the budget's read-back; a chunk with an uncertified query
runs the fp32 scan again, so the answers ``==`` a plain library's whatever ``last_certified`` says.  ``certified_table`` adds the
windows' prefix sums to ``scan_table``'s arrays.  Everything else -- ``predict_moments``, ``rank_videos``, ``search``, the
watchers -- runs its fp32 path unchanged.
Out of scope here: certified ``rank_videos`` / ``search`` / watcher polls, headroom reserved behind a video, capturing the call
in a graph.
"""
from __future__ import annotations

import ctypes as C
import operator
import struct
import weakref

import torch

from . import _lib, ops
from .session import (CERTIFIED_WITH_BF16, MAX_QUERIES, NMS_THD, MAX_BEFORE, MAX_AFTER, VideoSession, _kept_bytes, _pack_queries,
                      check_queries)
from .watch import LibraryWatcher, VideoWatcher

MAX_POOL = 1024     # candidates of one query in cone_corpus_fuse_nms (csrc/stage_c.h: kMaxCand)


class RowRanges:
    """Who owns which rows of ``[0, capacity)``: a first-fit free list, holes sorted by start and coalesced on release.
    Pure Python, no GPU."""

    def __init__(self, capacity: int):
        if capacity < 1:
            raise ValueError(f"capacity must be at least one clip, got {capacity}")
        self.capacity = int(capacity)
        self.holes = [(0, self.capacity)]          # (start, length), sorted by start, no two adjacent

    @property
    def free(self) -> int:
        return sum(n for _, n in self.holes)

    @property
    def largest(self) -> int:
        return max((n for _, n in self.holes), default=0)

    def take(self, n: int) -> int:
        """First row of the first hole that holds ``n`` rows."""
        if n < 1:
            raise ValueError(f"a range needs at least one row, got {n}")
        for i, (start, length) in enumerate(self.holes):
            if length >= n:
                if length == n:
                    del self.holes[i]
                else:
                    self.holes[i] = (start + n, length - n)
                return start
        raise ValueError(f"no free range of {n} clips: the largest free hole has {self.largest} "
                         f"({self.free} of {self.capacity} clips are free; a library does not compact)")

    def take_at(self, start: int, n: int) -> int:
        """Claims exactly rows ``[start, start + n)`` when they lie inside ONE hole (the hole is split around them); raises
        ``ValueError`` and changes nothing otherwise."""
        start, n = int(start), int(n)
        if n < 1:
            raise ValueError(f"a range needs at least one row, got {n}")
        for i, (h0, length) in enumerate(self.holes):
            if h0 <= start and start + n <= h0 + length:
                left = [(h0, start - h0)] if start > h0 else []
                right = [(start + n, h0 + length - start - n)] if start + n < h0 + length else []
                self.holes[i:i + 1] = left + right
                return start
        raise ValueError(f"rows [{start}, {start + n}) do not lie inside one free hole")

    def release(self, start: int, n: int):
        i = 0
        while i < len(self.holes) and self.holes[i][0] < start:
            i += 1
        before_end = sum(self.holes[i - 1]) if i else -1
        after_start = self.holes[i][0] if i < len(self.holes) else -1
        if n < 1 or start < 0 or start + n > self.capacity or (i and before_end > start) or (after_start != -1 and after_start < start + n):
            raise ValueError(f"rows [{start}, {start + n}) are not an owned range")
        if before_end == start:                    # coalesce with the hole before, the hole after, or both
            start, n = self.holes[i - 1][0], n + self.holes[i - 1][1]
            i -= 1
            del self.holes[i]
        if after_start == start + n:
            n += self.holes[i][1]
            del self.holes[i]
        self.holes.insert(i, (start, n))

    def grow(self, capacity: int):
        """The range becomes ``[0, capacity)``: the new rows are one hole behind the old ones (coalesced with a hole that ended
        there).  Owned ranges stay where they are."""
        capacity = int(capacity)
        if capacity <= self.capacity:
            raise ValueError(f"grow: capacity={capacity} is not above the {self.capacity} rows there are")
        old, self.capacity = self.capacity, capacity
        self.release(old, capacity - old)

    def compacted(self):
        """After a compaction the owned rows are ``[0, capacity - free)``: one hole at the end (none in a full arena)."""
        free = self.free
        self.holes = [(self.capacity - free, free)] if free else []


def compaction_moves(videos):
    """``[(row0, n), ...]`` in any order -> ``[(src, dst, n), ...]`` in ARENA order, ``dst`` = the running sum of the lengths:
    the videos packed to the front, none overtaking another (``rank_videos`` breaks ties to the video that lies first in the
    arena: the order must not change).  Videos already in place come out with ``src == dst``.  Pure Python, no GPU;
    overlapping ranges are refused."""
    videos = sorted((int(r), int(n)) for r, n in videos)
    moves, at, end = [], 0, 0
    for row0, n in videos:
        if n < 1 or row0 < end:
            raise ValueError("compaction_moves: a video needs at least one clip and rows of its own")
        moves.append((row0, at, n))
        at, end = at + n, row0 + n
    return moves


def plan_steps(moves, stage_rows: int):
    """The ``cone_library_move_rows`` calls of a compaction: ``moves`` = ``compaction_moves``' list, ``stage_rows`` = rows the
    staging buffer holds.  Returns ``[(row_begin, row_end, staged), ...]`` over the flat row list of the moves with
    ``src != dst`` (the table the calls get).  At flat row p let g = src(p) - dst(p), the rows freed below it.  g >= stage_rows:
    a DIRECT step of min(g, remaining) rows -- the destinations are contiguous, so they end at or below the step's first source
    row: disjoint.  Otherwise a STAGED step of min(stage_rows, remaining) rows.  g never decreases along the arena, so a plan is
    a staged prefix and a direct suffix.  Every step's destination rows lie at or below its own source rows and every later
    step's source rows above them: no step overwrites a row a later step has yet to read."""
    if stage_rows < 1:
        raise ValueError(f"plan_steps: stage_rows={stage_rows} < 1")
    moving = [(int(s), int(d), int(n)) for s, d, n in moves if s != d]
    at = moving[0][1] if moving else 0
    gap = 1
    for s, d, n in moving:
        if n < 1 or d != at or s - d < gap:
            raise ValueError("plan_steps: not the moves of a compaction (downward, in arena order, destinations contiguous)")
        at, gap = d + n, s - d
    total = sum(n for _, _, n in moving)
    steps, p, i, first = [], 0, 0, 0            # first = flat row of move i
    while p < total:
        while p >= first + moving[i][2]:
            first += moving[i][2]
            i += 1
        g = moving[i][0] - moving[i][1]
        staged = g < stage_rows
        n = min(stage_rows if staged else g, total - p)
        steps.append((p, p + n, staged))
        p += n
    return steps


def plan_runs(placements):
    """The launches of one ``add_many``: ``placements`` = ``[(row0, n), ...]`` of the call's videos in LIST order.  Consecutive
    videos whose ranges are adjacent and ascending (``row0`` of the next = the end of the one before) become one run.  Returns
    ``[(row0, n, first, end), ...]``: videos ``[first, end)`` of the list lie back to back in the ``n`` rows from ``row0``, as
    their raw rows do in the list's concatenation.  A fresh or compact library yields one run.  Pure Python, no GPU."""
    runs = []
    for i, (row0, n) in enumerate(placements):
        row0, n = int(row0), int(n)
        if n < 1 or row0 < 0:
            raise ValueError("plan_runs: a video needs row0 >= 0 and at least one clip")
        if runs and runs[-1][0] + runs[-1][1] == row0:
            r = runs[-1]
            runs[-1] = (r[0], r[1] + n, r[2], i + 1)
        else:
            runs.append((row0, n, i, i + 1))
    return runs


def plan_extend(rows: RowRanges, row0: int, n: int, m: int):
    """Where a resident video ``(row0, n)`` grows by ``m`` clips, decided on the free list alone (``rows`` is not changed):
    ``("in_place", row0)`` when the ``m`` rows right behind it lie in one hole; else ``("relocate", dst)`` with ``dst`` the first
    hole that holds ``n + m`` rows (first-fit, as ``take`` would); else ``("no_room", None)``.  Pure Python, no GPU."""
    row0, n, m = int(row0), int(n), int(m)
    if n < 1 or m < 1:
        raise ValueError(f"plan_extend: a video of {n} clips cannot grow by {m}")
    end = row0 + n
    for h0, length in rows.holes:
        if h0 <= end and end + m <= h0 + length:        # (holes never overlap an owned row: h0 == end)
            return "in_place", row0
    for h0, length in rows.holes:
        if length >= n + m:
            return "relocate", h0
    return "no_room", None


def plan_calls(video_of, k_of, limit: int = MAX_QUERIES):
    """The calls of one ``predict_moments``: ``video_of[i]`` / ``k_of[i]`` = video id and window count K of pair i.  Pairs are
    grouped by K (one K per ``cone_library_localize`` call), a group is sorted by video (stable: a video's queries become one
    run, in the caller's order) and cut into calls of at most ``limit``.  Returns ``[(K, [pair index, ...]), ...]``."""
    groups = {}
    for i, k in enumerate(k_of):
        groups.setdefault(int(k), []).append(i)
    calls = []
    for k in sorted(groups):
        idx = sorted(groups[k], key=lambda i: video_of[i])
        calls += [(k, idx[g:g + limit]) for g in range(0, len(idx), limit)]
    return calls


def plan_ragged_calls(video_of, k_of, limit: int = MAX_QUERIES, max_windows: int = 64 * 256):
    """The calls of a ragged ``predict_moments`` / ``search_windows``: ``cone_library_localize_ragged`` takes a window count per
    pair, so nothing is grouped by K.  The pairs are sorted by video (stable: a video's pairs become one run, in the caller's
    order, whatever their k) and cut into calls of at most ``limit`` pairs and ``max_windows`` windows.  Returns
    ``[[pair index, ...], ...]``; ``inverse_order`` takes it as ``[(None, idx) for idx in calls]``.  Pure Python, no GPU."""
    limit, max_windows = int(limit), int(max_windows)
    if limit < 1 or max_windows < 1:
        raise ValueError(f"plan_ragged_calls: limit={limit} / max_windows={max_windows} < 1")
    if len(video_of) != len(k_of):
        raise ValueError(f"plan_ragged_calls: {len(video_of)} videos for {len(k_of)} window counts")
    calls, cur, windows = [], [], 0
    for i in sorted(range(len(k_of)), key=lambda i: video_of[i]):
        k = int(k_of[i])
        if not 1 <= k <= max_windows:
            raise ValueError(f"plan_ragged_calls: pair {i} asks for {k} windows, not in [1, max_windows={max_windows}]")
        if cur and (len(cur) == limit or windows + k > max_windows):
            calls.append(cur)
            cur, windows = [], 0
        cur.append(i)
        windows += k
    if cur:
        calls.append(cur)
    return calls


def inverse_order(calls, n: int):
    """``where[i]`` = position of pair i in the concatenation of the calls' index lists (each pair exactly once)."""
    where = [-1] * n
    at = 0
    for _, idx in calls:
        for i in idx:
            if where[i] != -1:
                raise ValueError(f"pair {i} is planned twice")
            where[i] = at
            at += 1
    if at != n or -1 in where:
        raise ValueError("the plan does not cover every pair")
    return where


def pooled_moments(rows, seg, n, seg_video):
    """One query's answer from a ``cone_corpus_fuse_nms`` launch: ``rows`` = its kept rows ``[st, ed, prop, match, fused]``,
    ``seg`` = their segment ordinals within the query, ``n`` = how many were kept, ``seg_video[s]`` = the video id behind the
    query's segment ``s`` (a pair in ``search_moments``, a window in a ``LibraryWatcher``).  Returns
    ``[(video id, [st, ed, score]), ...]``.  Pure Python, no GPU."""
    return [(seg_video[seg[j]], [rows[j][0], rows[j][1], rows[j][4]]) for j in range(n)]


def _as_int(value, refusal):
    try:
        return operator.index(value)
    except TypeError:
        raise ValueError(refusal) from None


def _chunked(queries):
    return [queries[g:g + MAX_QUERIES] for g in range(0, len(queries), MAX_QUERIES)]


def decode_budget(words, at, nq, W, best=False, miss_at=None):
    """One chunk of the budget's read-back, ``words`` = the int32 words as a flat list, ``at`` = the chunk's first word: ``n_pairs
    (nq) | pair_slot | pair_k | pair_best (nq x W each)``.  Returns ``(pairs, the next chunk's first word)``; ``pairs[q]`` = the
    query's pairs in the budget's order, ``(slot, k)`` each -- ``(slot, k, best score)`` with ``best``, the score decoded from its
    float32 bits; ``(slot, k, miss)`` with ``miss_at`` = the first word of the chunk's ``pair_miss`` plane ``(nq, W)`` that a
    ``LibraryWatcher`` appends to the read-back.  Pure Python, no GPU."""
    pairs = []
    for q in range(nq):
        n, row = words[at + q], at + nq + q * W
        if not 0 <= n <= W:
            raise IndexError(f"decode_budget: query {q} of the chunk has n_pairs={n}, not in [0, {W}]")
        cols = [words[row:row + n], words[row + nq * W:row + nq * W + n]]
        if best:
            bits = words[row + 2 * nq * W:row + 2 * nq * W + n]
            cols.append(struct.unpack(f"{n}f", struct.pack(f"{n}i", *bits)))
        if miss_at is not None:
            cols.append(words[miss_at + q * W:miss_at + q * W + n])
        pairs.append(list(zip(*cols)))
    return pairs, at + nq + 3 * nq * W


def merge_ranges(ranges):
    """``[(row0, n), ...]`` -> the same rows as sorted ranges with adjacent and overlapping ones merged: the destinations of a
    compaction, or the launches of one ``add_many`` run, become one ``cone_library_shadow_index`` launch.  Pure Python, no GPU."""
    out = []
    for row0, n in sorted((int(r), int(n)) for r, n in ranges):
        if n < 1:
            raise ValueError(f"merge_ranges: a range needs at least one row, got {n}")
        if out and row0 <= out[-1][0] + out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], row0 + n - out[-1][0]))
        else:
            out.append((row0, n))
    return out


def splice_budgets(host, nqs, W, redo, words):
    """``host`` = the budgets' words of chunks of ``nqs[i]`` queries back to back (``decode_budget``'s layout: ``nq + 3 nq W`` words
    a chunk); ``words`` = the budgets of the chunks ``redo`` (ascending indices) run again, back to back.  Overwrites those chunks'
    words in ``host``, in place.  Pure Python, no GPU."""
    first = [0]
    for nq in nqs:
        first.append(first[-1] + nq * (1 + 3 * W))
    at = 0
    for i in redo:
        n = first[i + 1] - first[i]
        host[first[i]:first[i + 1]] = words[at:at + n]
        at += n
    if at != len(words) or first[-1] != len(host):
        raise ValueError("splice_budgets: the words do not match the chunks")


def place_calls(calls, counts, Nq: int, first: int = 0):
    """Where the candidate rows of ragged calls lie in ONE buffer: ``calls`` = ``plan_ragged_calls``' index lists over pairs of
    ``counts[i]`` windows, ``Nq`` rows a window.  The calls follow each other from row ``first``, inside a call the pairs lie in
    the call's order (a call writes from its first pair's row).  Returns ``(row_of, end)``: pair i's first row, and the row behind
    the last.  Pure Python, no GPU."""
    row_of, at = [0] * len(counts), first
    for idx in calls:
        for i in idx:
            row_of[i] = at
            at += counts[i] * Nq
    return row_of, at


class FuseOut:
    """The outputs of the ``cone_corpus_fuse_nms`` launches of one call in ONE float64 tensor, one read-back: per chunk of ``nq``
    queries ``out_rows (nq, M, 5) float64 | out_seg (nq, M) int32 | out_n (nq) int32``, the int32 words padded to a whole 8-byte
    word so that the next chunk's rows stay aligned.  ``regions[i]`` = chunk i's three outputs, ``(byte offset, bytes)`` each.
    A watcher keeps one for its life: the sizes never change, and a poll has read the buffer back before the next writes it."""

    def __init__(self, nqs, M, device):
        self.nqs, self.M, self.regions = list(nqs), int(M), []
        at = 0
        for nq in self.nqs:
            seg = at + 8 * nq * M * 5
            self.regions.append(((at, seg - at), (seg, 4 * nq * M), (seg + 4 * nq * M, 4 * nq)))
            at += 8 * (nq * M * 5 + (nq * M + nq + 1) // 2)
        self.buf = torch.empty(at // 8, dtype=torch.float64, device=device)

    def launch(self, i, cand, seg_off, seg_cand, seg_n, seg_tag, n_seg):
        """Stage C of chunk i over the candidate rows at ``cand`` and a table of ``n_seg`` segments (five device pointers)."""
        out = [C.c_void_p(self.buf.data_ptr() + off) for off, _ in self.regions[i]]
        _lib.check(_lib.load().cone_corpus_fuse_nms(cand, seg_off, seg_cand, seg_n, seg_tag, self.nqs[i], n_seg, NMS_THD, MAX_BEFORE,
                                                    self.M, *out, _lib.stream()))

    def read(self, seg=True):
        """The one read-back: per chunk ``(rows, seg, kept)`` as lists -- per query ``M`` rows ``[st, ed, prop, match, fused]``,
        their ``M`` segment ordinals (``None`` without ``seg``: a caller with one video does not ask), and how many were kept."""
        host, M, out = self.buf.cpu(), self.M, []
        for nq, ((r, n_r), (s, _), (k, n_k)) in zip(self.nqs, self.regions):
            ints = host[s // 8:(k + n_k + 7) // 8].view(torch.int32).tolist()
            out.append((host[r // 8:s // 8].view(nq, M, 5).tolist(), [ints[q * M:(q + 1) * M] for q in range(nq)] if seg else None,
                        ints[nq * M:nq * M + nq]))
        return out


def scan_table(videos, S: int):
    """The table of one ``cone_library_scan``: ``videos`` = ``[(row0, ctx_l), ...]`` in any order, ``S`` = max_v_l // 2 clips
    per half-block.  Slots are ordered by ``row0`` (the scan walks the arena front to back).  Returns ``(order, v_row0, v_ctx_l,
    v_hb_off)``: ``order[slot]`` = index into ``videos``; ``v_row0`` int64 / ``v_ctx_l`` int32 per slot; ``v_hb_off`` int64
    (V + 1) = exclusive prefix sums of ``ceil(ctx_l / S)``, so slot s owns units ``[v_hb_off[s], v_hb_off[s + 1])`` of the flat
    half-block list and ``v_hb_off[-1]`` is its length.  Pure numpy, no GPU; overlapping ranges are refused."""
    import numpy as np
    if S < 1:
        raise ValueError(f"scan_table: S={S} < 1")
    videos = [(int(r), int(n)) for r, n in videos]
    order = sorted(range(len(videos)), key=lambda i: videos[i][0])
    row0 = np.asarray([videos[i][0] for i in order], dtype=np.int64)
    ctx = np.asarray([videos[i][1] for i in order], dtype=np.int64)
    if (ctx < 1).any() or (row0 < 0).any():
        raise ValueError("scan_table: a video needs row0 >= 0 and at least one clip")
    if (row0[1:] < row0[:-1] + ctx[:-1]).any():
        raise ValueError("scan_table: two videos share arena rows")
    hb_off = np.zeros(len(order) + 1, dtype=np.int64)
    np.cumsum((ctx + S - 1) // S, out=hb_off[1:])
    return order, row0, ctx.astype(np.int32), hb_off


def certified_table(videos, S: int, max_v_l: int):
    """The table of one ``cone_library_scan_certified``: ``scan_table``'s ``(order, v_row0, v_ctx_l, v_hb_off)`` plus ``v_win_off``
    int64 (V + 1) = exclusive prefix sums of ``cone_num_windows(ctx_l, max_v_l)`` = ``ceil(ctx_l / S) + 1``, so window j of slot
    s is entry ``v_win_off[s] + j`` of the flat window row and ``v_win_off[-1]`` is its length.  ``S`` must be ``max_v_l // 2``.
    Pure numpy, no GPU."""
    import numpy as np
    if int(S) != int(max_v_l) // 2:
        raise ValueError(f"certified_table: S={S} is not max_v_l // 2 = {int(max_v_l) // 2}")
    order, row0, ctx, hb_off = scan_table(videos, S)
    win_off = np.zeros(len(order) + 1, dtype=np.int64)
    np.cumsum((ctx.astype(np.int64) + S - 1) // S + 1, out=win_off[1:])
    return order, row0, ctx, hb_off, win_off


class VideoLibrary:
    """Many resident videos of a ``CONELocalizator`` (``open_library``).  ``add`` indexes a video into free rows and returns its
    id (never reused); ``predict_moments([(id, (tok, cls)), ...])`` returns, per pair and in the order given, what the
    localizer's ``predict_moment`` returns for that video and query, ``==``.  ``rank_videos`` / ``search`` answer "which video,
    and where" without the caller naming one.  ``compact`` / ``resize`` move the resident rows bit for bit: see the module text."""

    _watchers = None                        # a weak set of the VideoWatchers ``watch`` has handed out (none yet)
    certified, n_cand, last_certified = False, 0, None      # a plain library: no shadow, no certified scans
    _shadow = _sh = _cert_cache = None

    def __init__(self, localizer, capacity_clips: int, certified: bool = False, n_cand=None):
        if certified and localizer.prefilter_bf16:
            raise ValueError(CERTIFIED_WITH_BF16)
        from .model import Workspace
        self._loc = localizer
        a, m = localizer.args, localizer.localizator
        self.max_q_l = int(a.max_q_l)
        self._rows = RowRanges(int(capacity_clips))
        self._videos = {}                   # id -> (row0, ctx_l, K)
        self._next_id = 1
        self._handle_obj, self._handle_value = m._handle, m._h().value
        lib, h = _lib.load(), m._h()
        self._flags = _lib.SESSION_BF16 if localizer.prefilter_bf16 else 0
        n_arena = _lib.sized(lib.cone_library_arena_bytes(h, self._rows.capacity, self._flags))
        self._arena = torch.empty(n_arena, dtype=torch.uint8, device=localizer.device)
        self._cl = _lib.Library()
        _lib.check(lib.cone_library_open(h, self._rows.capacity, self._flags, _lib.ptr(self._arena), n_arena, C.byref(self._cl)))
        self._params = _lib.SessionParams(int(a.max_v_l), int(a.max_q_l), float(a.clip_length), NMS_THD, MAX_BEFORE, MAX_AFTER)
        self._ws = Workspace()              # the per-call workspace (grow-only)
        self._scan_ws = Workspace()         # the scan's planes and ranking scratch (grow-only)
        self._scan_cache = None             # the device table of ALL resident videos; rebuilt lazily after add / remove
        self.certified, self.n_cand = bool(certified), int(n_cand or 0)
        self.last_certified = None          # the flags of the last budgeted call on a certified library, one per query
        self._cert_cache = None             # (the scan table it belongs to, device v_win_off, total_win)
        self._shadow, self._sh = self._open_shadow(self._cl) if self.certified else (None, None)
        self._open = True

    # ---- the certified shadow --------------------------------------------------------------------
    def _open_shadow(self, cl):
        """A shadow arena for the library handle ``cl`` and its layout: (tensor, ``cone_library_shadow``)."""
        lib = _lib.load()
        n = _lib.sized(lib.cone_library_shadow_bytes(C.byref(cl)))
        arena, sh = torch.empty(n, dtype=torch.uint8, device=self._loc.device), _lib.LibraryShadow()
        _lib.check(lib.cone_library_shadow_open(C.byref(cl), _lib.ptr(arena), n, C.byref(sh)))
        return arena, sh

    def _shadow_index(self, ranges, cl=None, sh=None):
        """Re-indexes the shadow rows of ``ranges`` = ``[(row0, n), ...]`` from the adapted rows there (the stream's order: after
        the launches that wrote them); nothing on a plain library."""
        if not self.certified:
            return
        lib, h = _lib.load(), self._loc.localizator._h()
        cl, sh = (self._cl, self._sh) if cl is None else (cl, sh)
        for row0, n in merge_ranges(ranges):
            _lib.check(lib.cone_library_shadow_index(h, C.byref(cl), C.byref(sh), int(row0), int(n), _lib.stream()))

    # ---- lifetime ------------------------------------------------------------------------------
    @property
    def nbytes(self) -> int:
        """Bytes that stay resident for the library (its arena, whatever it holds; a certified library's shadow too)."""
        return int(self._arena.numel()) + (int(self._shadow.numel()) if self.certified else 0) if self._open else 0

    @property
    def free_clips(self) -> int:
        return self._rows.free if self._open else 0

    def close(self):
        self._open = False              # (the ids stay known: a call on a closed library says "closed", not "unknown id")
        self._arena = self._cl = self._ws = self._scan_ws = self._scan_cache = self._shadow = self._sh = self._cert_cache = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _check_live(self):
        if not self._open:
            raise RuntimeError("VideoLibrary: the library is closed")
        m = self._loc.localizator
        if m._handle is not self._handle_obj or m._handle is None or m._handle.value != self._handle_value:
            raise RuntimeError("VideoLibrary: load_state_dict replaced the model handle these videos were indexed with; the "
                               "resident rows belong to the old weights -- open a new library")

    # ---- videos --------------------------------------------------------------------------------
    @torch.no_grad()
    def add(self, video_feats, compact=False):
        """Index ``video_feats`` (clips, dim) into the first free row range that holds it; returns the video's id.  Raises
        ``ValueError`` when no hole fits (the message names the clips asked for and the largest free hole) -- unless
        ``compact=True`` and the free clips together hold it: then the library compacts first (``compact``)."""
        self._check_live()
        a, m = self._loc.args, self._loc.localizator
        vid = video_feats.to(self._loc.device, torch.float32).contiguous()
        if vid.dim() != 2 or vid.shape[0] < 1:
            raise ValueError(f"add: video_feats must be (clips >= 1, dim), got {tuple(vid.shape)}")
        m._check_dim(vid, a.v_appear_feat_dim, "appearance clip features")
        m._check_dim(vid, a.v_motion_feat_dim, "motion clip features")
        n = int(vid.shape[0])
        if compact and self._rows.largest < n <= self._rows.free:
            self.compact()
        row0 = self._rows.take(n)
        try:
            lib, h = _lib.load(), m._h()
            n_ws = lib.cone_library_add_workspace(h, n)
            ws = torch.empty(max(n_ws, 1), dtype=torch.uint8, device=vid.device)
            _lib.check(lib.cone_library_add(h, C.byref(self._cl), row0, _lib.ptr(vid), n, _lib.ptr(ws), n_ws, _lib.stream()))
            self._shadow_index([(row0, n)])
        except Exception:
            self._rows.release(row0, n)
            raise
        self._scan_cache = None
        vid_id, self._next_id = self._next_id, self._next_id + 1
        self._videos[vid_id] = (row0, n, min(int(a.topk_window), ops.num_windows(n, a.max_v_l)))
        return vid_id

    def remove(self, vid_id):
        """The video's rows become free (queries already enqueued on the stream have read them by the time a later ``add``
        overwrites them: one stream).  Its id is never handed out again."""
        row0, n, _ = self._video(vid_id)
        del self._videos[vid_id]
        self._scan_cache = None
        self._rows.release(row0, n)

    # ---- ingest: many videos a call, growing and trimming resident ones --------------------------
    def _checked(self, who, feats):
        """The checks of ``add`` on the tensor as the caller holds it (nothing is uploaded for a refusal); returns its clips."""
        a, m = self._loc.args, self._loc.localizator
        try:
            if not hasattr(feats, "dim") or feats.dim() != 2 or feats.shape[0] < 1:
                raise ValueError(f"video_feats must be (clips >= 1, dim), got {tuple(getattr(feats, 'shape', ()))}")
            m._check_dim(feats, a.v_appear_feat_dim, "appearance clip features")
            m._check_dim(feats, a.v_motion_feat_dim, "motion clip features")
        except ValueError as e:
            raise ValueError(f"{who}: {e}") from None
        return int(feats.shape[0])

    def _k(self, n):
        a = self._loc.args
        return min(int(a.topk_window), ops.num_windows(n, a.max_v_l))

    def _index(self, raw, launches):
        """``launches`` = ``[(arena row, first row of raw, rows), ...]``: one ``cone_library_add`` each, on one workspace sized for
        the largest (the launches follow each other on one stream)."""
        lib, h = _lib.load(), self._loc.localizator._h()
        n_ws = max(lib.cone_library_add_workspace(h, n) for n in {n for _, _, n in launches})
        ws = torch.empty(max(n_ws, 1), dtype=torch.uint8, device=raw.device)
        base, row_bytes = _lib.ptr(raw, torch.float32).value, raw.shape[1] * 4
        for row0, at, n in launches:
            _lib.check(lib.cone_library_add(h, C.byref(self._cl), row0, C.c_void_p(base + at * row_bytes), n, _lib.ptr(ws), ws.numel(),
                                            _lib.stream()))
        self._shadow_index([(row0, n) for row0, _, n in launches])

    def _place(self, lens):
        """Sequential first-fit of the call's videos; on a failure every range taken so far is released again."""
        taken = []
        try:
            for n in lens:
                taken.append((self._rows.take(n), n))
        except ValueError as e:
            for r in reversed(taken):
                self._rows.release(*r)
            raise ValueError(f"add_many: video {len(taken)}: {e}") from None
        return taken

    @torch.no_grad()
    def add_many(self, videos, compact=False, chunk_clips=262144):
        """Indexes a list of videos and returns their ids: the library ends in exactly the state ``[lib.add(v) for v in videos]``
        leaves it in -- consecutive ids, the same first-fit ``(row0, n, K)`` per id, the same holes, the same bits in every
        plane -- with ONE concatenation and ONE upload of the raw rows and one ``cone_library_add`` per run of ``plan_runs``
        (one run on a fresh or compact library), cut at ``chunk_clips`` rows so that the workspace stays bounded: a row's bits do
        not depend on the launch it is indexed in.  Every video is checked before any row is taken and before any GPU work;
        all or nothing: when some video finds no hole, every range taken for the call is released and the ``ValueError`` names
        that video's index -- unless ``compact=True`` and ``free_clips`` holds them all: then the library compacts once and places
        them behind the resident videos.  An empty list returns ``[]`` and launches nothing."""
        videos = list(videos)
        lens = [self._checked(f"add_many: video {i}", v) for i, v in enumerate(videos)]
        if int(chunk_clips) < 1:
            raise ValueError(f"add_many: chunk_clips={chunk_clips} < 1")
        if not videos:
            return []
        self._check_live()
        try:
            placed = self._place(lens)
        except ValueError:
            if not (compact and sum(lens) <= self._rows.free):
                raise
            self.compact()
            placed = self._place(lens)              # (one hole at the end that holds them all)
        try:
            dev, chunk = self._loc.device, int(chunk_clips)
            parts = [v.to(torch.float32) for v in videos]
            if len({p.device for p in parts}) > 1:
                parts = [p.to(dev) for p in parts]
            raw = (parts[0] if len(parts) == 1 else torch.cat(parts)).to(dev).contiguous()        # the call's one upload
            launches, at = [], 0
            for row0, n, _, _ in plan_runs(placed):
                launches += [(row0 + c, at + c, min(chunk, n - c)) for c in range(0, n, chunk)]
                at += n
            self._index(raw, launches)
        except Exception:
            for r in reversed(placed):
                self._rows.release(*r)
            raise
        self._scan_cache = None
        ids = list(range(self._next_id, self._next_id + len(videos)))
        self._next_id += len(videos)
        for vid_id, (row0, n) in zip(ids, placed):
            self._videos[vid_id] = (row0, n, self._k(n))
        return ids

    @torch.no_grad()
    def extend(self, vid_id, more_feats, compact=False) -> int:
        """Appends the clips ``more_feats`` (clips, dim) to the resident video ``vid_id`` and returns its new clip count; the id
        stays, and every later answer for it ``==`` ``predict_moment(torch.cat([video, more_feats]), query)``.  ``plan_extend``
        decides where.  IN PLACE when the rows right behind the video are free: one ``cone_library_add`` of the new rows, nothing
        else is touched.  Otherwise the video RELOCATES into the first hole that holds all of it: one direct
        ``cone_library_move_rows`` copies the resident rows (the hole was free: source and destination are disjoint), the new
        rows are indexed behind them, the old range becomes free.  A relocation changes the arena order and with it the order
        ``rank_videos`` breaks exact ties in.  ``compact=True`` compacts first when no hole fits but the free clips suffice.
        Queries enqueued earlier on the stream have read their rows (``remove``'s rule).  Unknown ids, a closed library, a wrong
        width, no clips and no room are refused before any GPU work, and the free list is then unchanged."""
        row0, n, _ = self._video(vid_id)
        m = self._checked("extend", more_feats)
        self._check_live()
        where, dst = plan_extend(self._rows, row0, n, m)
        if where == "no_room":
            last = row0 == max(v[0] for v in self._videos.values())         # behind the last video a compaction leaves every free clip
            if compact and self._rows.free >= (m if last else n + m):
                self.compact()
                row0 = self._videos[vid_id][0]
                where, dst = plan_extend(self._rows, row0, n, m)
            else:
                try:
                    self._rows.take(n + m)              # (raises: take's message, the free list unchanged)
                except ValueError as e:
                    raise ValueError(f"extend: the {m} rows behind video {vid_id!r} are not free and {e}") from None
        more = more_feats.to(self._loc.device, torch.float32).contiguous()
        if where == "in_place":
            self._rows.take_at(row0 + n, m)
            try:
                self._index(more, [(row0 + n, 0, m)])
            except Exception:
                self._rows.release(row0 + n, m)
                raise
        else:
            dst = self._rows.take(n + m)                # (first-fit: the hole plan_extend named)
            try:
                self._move(self._cl, self._cl, [(row0, dst, n)], [(0, n, False)], None)
                self._shadow_index([(dst, n)])
                self._index(more, [(dst + n, 0, m)])
            except Exception:
                self._rows.release(dst, n + m)
                raise
            self._rows.release(row0, n)
        self._scan_cache = None
        self._videos[vid_id] = (dst, n + m, self._k(n + m))
        return n + m

    def trim(self, vid_id, n_front) -> int:
        """Drops the video's oldest ``n_front`` clips and returns the clips that remain: their rows become free, nothing is
        launched (``remove``'s stream rule), and every later answer ``==`` ``predict_moment(video[n_front:], query)`` -- seconds
        count from the new first clip.  ``0 <= n_front < clips`` (0 changes nothing; dropping every clip is ``remove``)."""
        row0, n, _ = self._video(vid_id)
        n_front = _as_int(n_front, f"trim: n_front must be an integer, got {n_front!r}")
        if not 0 <= n_front < n:
            raise ValueError(f"trim: n_front={n_front} not in [0, {n}) for video {vid_id!r} (remove drops a whole video)")
        if n_front:
            self._rows.release(row0, n_front)
            self._videos[vid_id] = (row0 + n_front, n - n_front, self._k(n - n_front))
            self._scan_cache = None
            for w in list(self._watchers or ()):        # seconds and window indices shift: what a watcher has cached is stale
                w._trimmed(vid_id)
        return n - n_front

    # ---- maintenance ---------------------------------------------------------------------------
    @property
    def largest_free(self) -> int:
        """Clips of the largest hole: what one ``add`` can take without a compaction (``free_clips`` is what it can take
        with one)."""
        return self._rows.largest if self._open else 0

    def _move(self, src_cl, dst_cl, moves, steps, stage):
        """Uploads the table of ``moves`` once and enqueues one ``cone_library_move_rows`` per step."""
        import numpy as np
        lib, h, n = _lib.load(), self._loc.localizator._h(), len(moves)
        table = np.zeros(3 * n + 1, dtype=np.int64)                  # mv_src | mv_dst | mv_off: one upload
        table[:n], table[n:2 * n] = [m[0] for m in moves], [m[1] for m in moves]
        np.cumsum([m[2] for m in moves], out=table[2 * n + 1:])
        total = int(table[-1])
        dev = torch.from_numpy(table).to(self._loc.device)
        at = lambda k: C.c_void_p(dev.data_ptr() + 8 * k)
        for begin, end, staged in steps:
            _lib.check(lib.cone_library_move_rows(h, C.byref(src_cl), C.byref(dst_cl), at(0), at(n), at(2 * n), n, total, begin, end,
                                                  _lib.ptr(stage) if staged else None, stage.numel() if staged else 0, _lib.stream()))
        return total

    @torch.no_grad()
    def compact(self, stage_bytes: int = 256 << 20) -> int:
        """Closes the holes in place: every video slides down to the end of its predecessor, in arena order; returns the clips
        moved (0, and nothing is launched, on a compact library).  Ids, answers and rankings do not change -- the rows are
        copied bit for bit --, the free list becomes one hole at the end, the scan's table is rebuilt on the next search.  The
        moves run as ``plan_steps`` lays them out, on the library's one stream (queries enqueued earlier have read their
        rows): steps whose source and destination rows can overlap go through a staging buffer of at most ``stage_bytes``
        (allocated for the call, released after it; two launches a step), the others are one launch each."""
        self._check_live()
        ids = sorted(self._videos, key=lambda v: self._videos[v][0])
        moves = compaction_moves([self._videos[v][:2] for v in ids])
        moving = [m for m in moves if m[0] != m[1]]
        if not moving:
            self._rows.compacted()              # (already one hole at the end: unchanged)
            return 0
        lib = _lib.load()
        need = lambda rows: lib.cone_library_move_stage_bytes(C.byref(self._cl), rows)
        cl = self._cl
        row_bytes = cl.v_dim * (4 + 4 * bool(cl.adapted) + 2 * bool(cl.adapted_bf16)) + cl.hidden_dim * (4 + 12 * bool(cl.qkv_vid))
        stage_rows = min(sum(m[2] for m in moving), int(stage_bytes) // row_bytes)
        while stage_rows >= 1 and need(stage_rows) > stage_bytes:     # (every plane of the buffer is rounded up to 256 B)
            stage_rows -= 1
        if stage_rows < 1:
            raise ValueError(f"compact: stage_bytes={stage_bytes} holds no clip (one clip takes {need(1)} bytes)")
        steps = plan_steps(moving, stage_rows)
        largest = max((e - b for b, e, staged in steps if staged), default=0)
        stage = torch.empty(need(largest), dtype=torch.uint8, device=self._loc.device) if largest else None
        moved = self._move(self._cl, self._cl, moving, steps, stage)
        self._shadow_index([(dst, n) for _, dst, n in moving])
        for v, (_, dst, _) in zip(ids, moves):
            self._videos[v] = (dst,) + self._videos[v][1:]
        self._rows.compacted()
        self._scan_cache = None
        return moved

    @torch.no_grad()
    def resize(self, capacity_clips: int):
        """Moves the library into a new arena of ``capacity_clips`` clips, larger or smaller, compacting on the way: ONE
        direct ``cone_library_move_rows`` call copies every video, in arena order, to the front of the new arena; then the
        arenas are swapped.  Ids and answers do not change.  BOTH arenas live during the call (the old one is released when
        the copy has run).  Raises ``ValueError`` when ``capacity_clips`` is smaller than the resident clips."""
        capacity = int(capacity_clips)
        resident = sum(v[1] for v in self._videos.values())
        if capacity < resident:
            raise ValueError(f"resize: capacity_clips={capacity} is smaller than the {resident} resident clips")
        if capacity < 1:
            raise ValueError(f"capacity must be at least one clip, got {capacity}")
        self._check_live()
        lib, h = _lib.load(), self._loc.localizator._h()
        n_arena = _lib.sized(lib.cone_library_arena_bytes(h, capacity, self._flags))
        arena, cl = torch.empty(n_arena, dtype=torch.uint8, device=self._loc.device), _lib.Library()
        _lib.check(lib.cone_library_open(h, capacity, self._flags, _lib.ptr(arena), n_arena, C.byref(cl)))
        ids = sorted(self._videos, key=lambda v: self._videos[v][0])
        moves = compaction_moves([self._videos[v][:2] for v in ids])
        shadow, sh = self._open_shadow(cl) if self.certified else (None, None)
        if moves:
            self._move(self._cl, cl, moves, [(0, resident, False)], None)
            self._shadow_index([(0, resident)], cl, sh)             # (the videos lie packed at the front of the new arena)
        for v, (_, dst, _) in zip(ids, moves):
            self._videos[v] = (dst,) + self._videos[v][1:]
        self._shadow, self._sh = shadow, sh
        self._arena, self._cl = arena, cl       # (the old arena goes back to the allocator of this stream: the copy has read it by
        self._rows = RowRanges(capacity)        #  the time anything enqueued later writes there)
        if resident:
            self._rows.take(resident)
        self._scan_cache = None

    def _video(self, vid_id):
        try:
            return self._videos[vid_id]
        except (KeyError, TypeError):
            raise ValueError(f"VideoLibrary: unknown or removed video id {vid_id!r}") from None

    # ---- queries -------------------------------------------------------------------------------
    def _localize(self, chunk, K=None, ks=None, scan=None, V=0, cand=None):
        """One C call of the query half: ``chunk`` = [((row0, ctx_l), (tok, cls), scan query, slot), ...], at most MAX_QUERIES
        (the last two entries of a pair are read only with ``scan``).  ``K``: that many windows for every pair --
        ``cone_library_localize``, or ``cone_library_localize_ranked`` when ``scan`` = the scan whose lists (of ``V`` videos) the
        pairs take their windows from.  ``ks``: a window count per pair -- ``cone_library_localize_ragged``; ``scan`` as above
        (``None``: the call's own stage A).  ``cand`` (fp32, on the device, only with ``ks``):
        ``cone_library_localize_candidates`` -- the call's ``sum(ks) * num_queries`` candidate rows are written there, no stage C
        runs, nothing is returned.  Otherwise returns the kept rows and their counts as one byte buffer on the device."""
        lib, dev = _lib.load(), self._loc.device
        nq = len(chunk)
        tok_cat, cls, lens = _pack_queries([c[1] for c in chunk], dev)
        i32 = C.c_int32 * nq
        head = (self._loc.localizator._h(), C.byref(self._cl), i32(*(c[0][0] for c in chunk)), i32(*(c[0][1] for c in chunk)))
        lens, count, params = i32(*lens), K if ks is None else i32(*ks), C.byref(self._params)
        name = "cone_library_localize" + ("_candidates" if cand is not None else "_ragged" if ks is not None else
                                          "_ranked" if scan is not None else "")
        if scan is not None:
            _, sq, widx, wval = scan
            lists = (i32(*(c[2] for c in chunk)), i32(*(c[3] for c in chunk)), _lib.ptr(widx), _lib.ptr(wval), len(sq), V,
                     int(self._loc.args.topk_window))
        else:
            lists = () if ks is None else (None, None, None, None, 0, 0, 0)
        ranked = () if ks is None else (int(scan is not None),)
        ws = self._ws.get(_lib.sized(getattr(lib, name + "_workspace")(*head, lens, nq, count, params, *ranked)), dev)
        if cand is None:
            R, N = _kept_bytes(nq)
            buf = torch.empty(R + N, dtype=torch.uint8, device=dev)
            out = (C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + R))
        else:
            buf, out = None, (_lib.ptr(cand, torch.float32),)
        _lib.check(getattr(lib, name)(*head, _lib.ptr(tok_cat, torch.float32), lens, nq, _lib.ptr(cls, torch.float32), count, params,
                                      *lists, *out, _lib.ptr(ws), ws.numel(), _lib.stream()))
        return buf

    def _enqueue(self, K, chunk):
        """One ``cone_library_localize`` call: ``chunk`` = [((row0, ctx_l), (tok, cls)), ...], at most MAX_QUERIES."""
        return self._localize(chunk, K=K)

    def _enqueue_ragged(self, chunk, ks, scan=None, V=0, cand=None):
        """One ``cone_library_localize_ragged`` / ``_candidates`` call with ``ks`` windows per pair: ``_localize``'s arguments."""
        return self._localize(chunk, ks=ks, scan=scan, V=V, cand=cand)

    @torch.no_grad()
    def predict_moments(self, pairs, ragged=False, windows=None):
        """``[(video id, (text_token_feats, text_cls_feat)), ...]`` for any mix of the library's videos -> a list of moment
        lists in the order given, each ``==`` the localizer's ``predict_moment(video_feats, query)``.  Every pair is checked
        before any GPU work; the pairs are grouped by window count K (long videos all share ``topk_window``: usually one
        group), sorted by video inside a group, cut into calls of at most ``MAX_QUERIES``; every call is enqueued, then ONE
        read-back.
        ``ragged=True``: the same answers through ``cone_library_localize_ragged``, which takes a window count per pair -- the
        pairs are only sorted by video and cut at 64 (``plan_ragged_calls``), so videos of different K share a call.
        ``windows=[k, ...]``, one per pair (implies ragged): pair i runs on its ``k_i`` best windows only and answers with the
        localizer's ``predict_moment`` at ``topk_window = k_i``; a k outside ``[1, K of the video]`` is refused before any GPU
        work."""
        pairs = list(pairs)
        videos = [self._video(v) for v, _ in pairs]
        check_queries([int(q[0].shape[0]) for _, q in pairs], self.max_q_l)
        if windows is not None:
            windows = list(windows)
            if len(windows) != len(pairs):
                raise ValueError(f"VideoLibrary: {len(windows)} window counts for {len(pairs)} pairs")
            for i, (k, v) in enumerate(zip(windows, videos)):
                windows[i] = _as_int(k, f"VideoLibrary: windows[{i}] must be an integer, got {k!r}")
                if not 1 <= windows[i] <= v[2]:
                    raise ValueError(f"VideoLibrary: windows[{i}]={k} not in [1, {v[2]}] for video {pairs[i][0]!r}")
        if not pairs:
            return []
        self._check_live()
        if ragged or windows is not None:
            ks = windows if windows is not None else [v[2] for v in videos]
            calls = plan_ragged_calls([v[0] for v in videos], ks)
            where = inverse_order([(None, idx) for idx in calls], len(pairs))
            bufs = [self._enqueue_ragged([(videos[i][:2], pairs[i][1], 0, 0) for i in idx], [ks[i] for i in idx]) for idx in calls]
            out = VideoSession._read_calls(bufs, [len(idx) for idx in calls])   # the call's one read-back
            return [out[w] for w in where]
        calls = plan_calls([v[0] for v in videos], [v[2] for v in videos])        # (a video is its first row: unique while it lives)
        where = inverse_order(calls, len(pairs))
        bufs = [self._enqueue(K, [(videos[i][:2], pairs[i][1]) for i in idx]) for K, idx in calls]
        out = VideoSession._read_calls(bufs, [len(idx) for _, idx in calls])      # the call's one read-back
        return [out[w] for w in where]

    def predict_moment(self, vid_id, text_feats):
        """``localizer.predict_moment(video_feats, text_feats)`` for the resident video ``vid_id``."""
        return self.predict_moments([(vid_id, text_feats)])[0]

    # ---- standing queries ----------------------------------------------------------------------
    def watch(self, vid_id, queries):
        """A ``VideoWatcher`` for the standing ``queries`` = ``[(tok, cls), ...]`` (any count >= 1, 64 a call) on the resident
        video ``vid_id``: ``w.poll()`` returns one moment list per query, each ``==`` ``predict_moment(<the video's current
        clips>, query)`` after any sequence of ``extend`` / ``trim`` / ``compact`` / ``resize`` and ``add`` / ``remove`` of other
        videos, and runs the window model only on the listed windows it has not answered from before (``w.windows_run``, of
        ``w.windows_listed``); a ``trim`` makes the next poll run them all.  ``remove(vid_id)`` makes later polls raise.  The
        watcher keeps ``num_queries`` rows of 16 B and a 4-B stamp per query and window of the video (``w.nbytes``; 7.7 MB for
        64 queries on 33 000 clips).  fp32 libraries only; ``topk_window * num_queries`` may not exceed 1 024 candidates."""
        self._video(vid_id)
        queries = list(queries)
        if not queries:
            raise ValueError("VideoLibrary: watch: an empty query list (a watcher needs at least one standing query)")
        check_queries([int(q[0].shape[0]) for q in queries], self.max_q_l)
        self._check_pool("topk_window", int(self._loc.args.topk_window))
        return self._watcher("watch", VideoWatcher, vid_id, queries)

    def _watcher(self, call, cls, *args):
        """The tail of ``watch`` / ``watch_moments``: a live fp32 library, the watcher built and registered for ``trim``'s word."""
        self._check_live()
        if self._flags & _lib.SESSION_BF16:
            raise _lib.ConeHipError(f"{call}: CONE_SESSION_BF16 libraries are not supported (prefilter_bf16): the scan that lists a "
                                    "poll's windows does not serve them")
        w = cls(self, *args)
        if self._watchers is None:
            self._watchers = weakref.WeakSet()
        self._watchers.add(w)
        return w

    def watch_moments(self, queries, n_windows=None, n_moments=5, videos=None):
        """A ``LibraryWatcher`` for the standing ``queries`` = ``[(tok, cls), ...]`` (any count >= 1, 64 a call) over every
        resident video -- or over ``videos``: ``w.poll() == lib.search_moments(queries, n_windows, n_moments, videos)`` on the
        library as it is now, after any sequence of ``extend`` / ``trim`` / ``add`` / ``add_many`` / ``remove`` / ``compact`` /
        ``resize``, and runs the window model only on the budget's windows it has not answered from before (``w.windows_run``,
        of ``w.windows_listed``, per query).  ``videos=None`` follows the resident set: added videos join at the next poll,
        removed ones drop out and their cache is freed; with an explicit list a later ``remove`` of a listed video makes
        ``poll()`` raise what ``search_moments`` raises for that id.  A ``trim`` makes that video's cached windows stale, no
        other's.  The watcher keeps ``num_queries`` rows of 16 B and a 4-B stamp per query and per window of every watched video
        plus a quarter of headroom (``w.nbytes``).  fp32 libraries only; the limits are ``search_moments``'."""
        queries = list(queries)
        if not queries:
            raise ValueError("VideoLibrary: watch_moments: an empty query list (a watcher needs at least one standing query)")
        check_queries([int(q[0].shape[0]) for q in queries], self.max_q_l)
        W, M = self._budget_args(n_windows, n_moments)
        subset, _ = self._search_ids(videos)
        return self._watcher("watch_moments", LibraryWatcher, queries, W, M, subset)

    # ---- search --------------------------------------------------------------------------------
    def _search_ids(self, videos):
        """The ids a search runs over: every resident video, or the caller's (unknown ids and duplicates are refused)."""
        if videos is None:
            return None, list(self._videos)
        ids = list(videos)
        for v in ids:
            self._video(v)
        if len(set(ids)) != len(ids):
            dup = sorted({v for v in ids if ids.count(v) > 1})
            raise ValueError(f"VideoLibrary: video id {dup[0]!r} is listed more than once")
        return ids, ids

    def _table(self, subset, ids):
        """``scan_table`` of the videos on the device: (ids by slot, device v_row0 / v_ctx_l / v_hb_off, total_hb).  The table of
        ALL resident videos is kept until the next ``add`` / ``remove``; a subset's is built per call."""
        if subset is None and self._scan_cache is not None:
            return self._scan_cache
        order, row0, ctx, hb_off = scan_table([self._videos[v][:2] for v in ids], int(self._loc.args.max_v_l) // 2)
        dev = self._loc.device
        t = ([ids[i] for i in order], torch.from_numpy(row0).to(dev), torch.from_numpy(ctx).to(dev), torch.from_numpy(hb_off).to(dev),
             int(hb_off[-1]))
        if subset is None:
            self._scan_cache = t
        return t

    def _scan(self, table, queries, n_rank):
        """One ``cone_library_scan`` of at most MAX_QUERIES queries: (widx, wval, rank) on the device, K = topk_window; rank =
        (2, nq, n_rank) int32 words: the slots, then the scores' bits (one tensor: one read-back)."""
        lib, m, dev = _lib.load(), self._loc.localizator, self._loc.device
        _, row0, ctx, hb_off, total_hb = table
        V, nq, K = int(ctx.numel()), len(queries), int(self._loc.args.topk_window)
        cls = torch.stack([c.to(dev, torch.float32).reshape(-1) for _, c in queries]).contiguous()
        ws = self._scan_ws.get(_lib.sized(lib.cone_library_scan_workspace(C.byref(self._cl), V, total_hb, nq, K, n_rank)), dev)
        widx = torch.empty(nq * V * K, dtype=torch.int32, device=dev)
        wval = torch.empty(nq * V * K, dtype=torch.float32, device=dev)
        rank = torch.empty(2, nq, n_rank, dtype=torch.int32, device=dev)
        _lib.check(lib.cone_library_scan(m._h(), C.byref(self._cl), _lib.ptr(row0), _lib.ptr(ctx), _lib.ptr(hb_off), V, total_hb,
                                         _lib.ptr(cls, torch.float32), nq, K, n_rank, C.byref(self._params), _lib.ptr(widx),
                                         _lib.ptr(wval), C.c_void_p(rank[0].data_ptr()), C.c_void_p(rank[1].data_ptr()),
                                         _lib.ptr(ws), ws.numel(), _lib.stream()))
        return widx, wval, rank

    def _ranked(self, queries, n_videos, videos):
        """The scans of one ``rank_videos`` / ``search`` and their ONE read-back: (table, [(first query, queries, widx, wval)],
        per query [(slot, score), ...]); ``None`` where nothing is to be searched."""
        queries = list(queries)
        check_queries([int(q[0].shape[0]) for q in queries], self.max_q_l)
        subset, ids = self._search_ids(videos)
        if n_videos is not None and int(n_videos) < 1:
            raise ValueError(f"VideoLibrary: n_videos={n_videos} < 1")
        if not queries or not ids:
            return None, [], [[] for _ in queries]
        self._check_live()
        n_rank = len(ids) if n_videos is None else min(int(n_videos), len(ids))
        table = self._table(subset, ids)
        scans, ranks = [], []
        for chunk in _chunked(queries):
            widx, wval, rank = self._scan(table, chunk, n_rank)
            scans.append((MAX_QUERIES * len(scans), chunk, widx, wval))
            ranks.append(rank.reshape(2, -1))
        host = (ranks[0] if len(ranks) == 1 else torch.cat(ranks, dim=1)).cpu()       # the one small read-back
        slots = host[0].reshape(len(queries), n_rank).tolist()
        vals = host[1].contiguous().view(torch.float32).reshape(len(queries), n_rank).tolist()
        return table, scans, [list(zip(s, v)) for s, v in zip(slots, vals)]

    @torch.no_grad()
    def rank_videos(self, queries, n_videos=None, videos=None):
        """``[(tok, cls), ...]`` -> per query ``[(video id, score), ...]``: the ``n_videos`` best (all when ``None``) of the
        resident videos -- or of ``videos``, an iterable of ids -- by their best window score for the query (the pre-filter's
        cosine in the adapter's space, cone/inference.py:276-299), descending; ties to the video that lies first in the arena.
        One scan of the arena per 64 queries, one read-back; no window model runs."""
        table, _, ranked = self._ranked(queries, n_videos, videos)
        return [[(table[0][s], v) for s, v in row] for row in ranked]

    @torch.no_grad()
    def search(self, queries, n_videos=5, videos=None):
        """``[(tok, cls), ...]`` -> per query ``[(video id, score, moments), ...]`` for its ``n_videos`` best videos (clamped to
        the videos searched), in ``rank_videos``' order; ``moments == localizer.predict_moment(video_feats, query)``: the scan's
        window lists are the per-video pre-filter's, bit for bit, and everything after them is ``predict_moments``' call.  One
        scan per 64 queries, ONE small read-back (the chosen slots and scores), the ``cone_library_localize_ranked`` calls that
        ``plan_calls`` lays out (one K per call, pairs sorted by video, at most 64), one read-back of the kept rows."""
        table, scans, ranked = self._ranked(queries, n_videos, videos)
        if table is None:
            return ranked
        ids, V = table[0], len(table[0])
        bufs, sizes, plans = [], [], []
        for scan in scans:
            g, chunk = scan[0], scan[1]
            pairs = [(q, slot) for q in range(len(chunk)) for slot, _ in ranked[g + q]]
            vids = [self._videos[ids[slot]] for _, slot in pairs]
            calls = plan_calls([v[0] for v in vids], [v[2] for v in vids])
            where = inverse_order(calls, len(pairs))
            bufs += [self._localize([(vids[i][:2], chunk[pairs[i][0]], pairs[i][0], pairs[i][1]) for i in idx], K=K, scan=scan, V=V)
                     for K, idx in calls]
            sizes += [len(idx) for _, idx in calls]
            plans.append(where)
        moments = VideoSession._read_calls(bufs, sizes)                           # the kept rows' one read-back
        out, base = [], 0
        for (g, chunk, _, _), where in zip(scans, plans):
            it = iter(where)
            for q in range(len(chunk)):
                out.append([(ids[slot], val, moments[base + next(it)]) for slot, val in ranked[g + q]])
            base += len(where)
        return out

    # ---- window budgets ------------------------------------------------------------------------
    def _budget(self, scan, V, W):
        """``cone_library_budget`` on one scan's lists: (nq, 1 + 3 W) int32 words on the device -- n_pairs, then the slots, the
        counts and the best scores' bits (one tensor: one read-back)."""
        lib, dev = _lib.load(), self._loc.device
        _, chunk, _, wval = scan
        nq, K = len(chunk), int(self._loc.args.topk_window)
        ws = self._scan_ws.get(_lib.sized(lib.cone_library_budget_workspace(nq, V, K, W)), dev)     # (the scan has run: stream order)
        out = torch.empty(nq + 3 * nq * W, dtype=torch.int32, device=dev)
        at = lambda k: C.c_void_p(out.data_ptr() + 4 * (nq + k * nq * W))
        _lib.check(lib.cone_library_budget(_lib.ptr(wval), nq, V, K, W, C.c_void_p(out.data_ptr()), at(0), at(1), at(2), _lib.ptr(ws),
                                           ws.numel(), _lib.stream()))
        return out

    def _budget_args(self, n_windows, n_moments, pool=True):
        """``(W, M)`` of a budgeted call, or its refusal: ``n_windows`` (``None``: ``topk_window``) an integer in [1, 256], then
        -- with ``pool``; ``search_windows`` has none and gets ``(W, None)`` -- ``n_moments`` an integer in [1, 100] and at most
        ``MAX_POOL`` candidates in a query's pool."""
        a = self._loc.args
        W = _as_int(int(a.topk_window) if n_windows is None else n_windows,
                    f"VideoLibrary: n_windows must be an integer, got {n_windows!r}")
        if not 1 <= W <= 256:
            raise ValueError(f"VideoLibrary: n_windows={W} not in [1, 256]")
        if not pool:
            return W, None
        M = _as_int(n_moments, f"VideoLibrary: n_moments must be an integer, got {n_moments!r}")
        if not 1 <= M <= MAX_BEFORE:
            raise ValueError(f"VideoLibrary: n_moments={M} not in [1, {MAX_BEFORE}]")
        self._check_pool("n_windows", W)
        return W, M

    def _check_pool(self, name, n):
        """``n`` windows of ``num_queries`` candidates each must fit the pool of one ``cone_corpus_fuse_nms`` query."""
        Nq = int(self._loc.args.num_queries)
        if n * Nq > MAX_POOL:
            raise ValueError(f"VideoLibrary: {name}={n} x num_queries={Nq} = {n * Nq} candidates > {MAX_POOL} in one pool")

    def _scan_budget(self, table, chunks, W):
        """One ``_scan`` and one ``_budget`` of ``W`` windows per chunk of at most MAX_QUERIES queries (a watcher's chunks are on the
        device already and stay there).  Yields, chunk by chunk, ``((first query, chunk, widx, wval), the budget's words)``, all on
        the device -- a watcher plans a chunk before the next is scanned --; the caller reads the words back in one copy."""
        V, g = len(table[0]), 0
        for chunk in chunks:
            widx, wval, _ = self._scan(table, chunk, 1)
            scan = (g, chunk, widx, wval)
            yield scan, self._budget(scan, V, W)
            g += len(chunk)

    def _cert_table(self, table):
        """``certified_table``'s ``v_win_off`` for a ``_table``: (device int64 (V + 1), total_win); the one of ALL resident videos is
        kept as long as its scan table is."""
        if self._cert_cache is not None and self._cert_cache[0] is table:
            return self._cert_cache[1:]
        W = int(self._loc.args.max_v_l)
        win_off = certified_table([self._videos[v][:2] for v in table[0]], W // 2, W)[4]
        t = (table, torch.from_numpy(win_off).to(self._loc.device), int(win_off[-1]))
        if table is self._scan_cache:
            self._cert_cache = t
        return t[1:]

    def _scan_certified(self, table, queries, W):
        """One ``cone_library_scan_certified`` of at most MAX_QUERIES queries for a budget of ``W`` windows: (widx, wval,
        certified) on the device, ``_scan``'s lists where a query's flag is 1."""
        lib, m, dev = _lib.load(), self._loc.localizator, self._loc.device
        _, row0, ctx, hb_off, total_hb = table
        win_off, total_win = self._cert_table(table)
        V, nq, K = int(ctx.numel()), len(queries), int(self._loc.args.topk_window)
        n_cand = min(max(self.n_cand, min(W, total_win)), total_win, 4096) if self.n_cand else 0
        cls = torch.stack([c.to(dev, torch.float32).reshape(-1) for _, c in queries]).contiguous()
        ws = self._scan_ws.get(_lib.sized(lib.cone_library_scan_certified_workspace(C.byref(self._cl), V, total_hb, total_win, nq, K, W,
                                                                                    n_cand)), dev)
        widx = torch.empty(nq * V * K, dtype=torch.int32, device=dev)
        wval = torch.empty(nq * V * K, dtype=torch.float32, device=dev)
        cert = torch.empty(nq, dtype=torch.int32, device=dev)
        _lib.check(lib.cone_library_scan_certified(m._h(), C.byref(self._cl), C.byref(self._sh), _lib.ptr(row0), _lib.ptr(ctx),
                                                   _lib.ptr(hb_off), _lib.ptr(win_off), V, total_hb, total_win,
                                                   _lib.ptr(cls, torch.float32), nq, K, W, n_cand, C.byref(self._params), _lib.ptr(widx),
                                                   _lib.ptr(wval), _lib.ptr(cert), _lib.ptr(ws), ws.numel(), _lib.stream()))
        return widx, wval, cert

    def _budgeted_certified(self, table, chunks, W):
        """``_budgeted``'s scans and budgets on a certified library: ``cone_library_scan_certified`` + ``cone_library_budget`` per
        chunk, the flags behind the budgets' words in the ONE read-back; a chunk with an uncertified query is run again, whole,
        through ``_scan`` + ``_budget`` and those budgets are read back in a second copy (in that case only)."""
        V, scans, budgets, flags, g = len(table[0]), [], [], [], 0
        for chunk in chunks:
            widx, wval, cert = self._scan_certified(table, chunk, W)
            scans.append((g, chunk, widx, wval))
            budgets.append(self._budget(scans[-1], V, W))
            flags.append(cert)
            g += len(chunk)
        host = torch.cat(budgets + flags).cpu().tolist()                # the one small read-back
        host, self.last_certified = host[:-g], host[-g:]
        redo = [i for i, s in enumerate(scans) if not all(self.last_certified[s[0]:s[0] + len(s[1])])]
        if redo:
            again = []
            for i in redo:
                widx, wval, _ = self._scan(table, scans[i][1], 1)
                scans[i] = scans[i][:2] + (widx, wval)
                again.append(self._budget(scans[i], V, W))
            splice_budgets(host, [len(s[1]) for s in scans], W, redo, torch.cat(again).cpu().tolist())     # the fallback's read-back
        return scans, host

    def _budgeted(self, call, queries, videos, W):
        """What ``search_windows`` / ``search_moments`` do between their budget's refusals and their plans: the queries' and the
        videos' refusals, then -- on a live fp32 library -- the scans and budgets of ``W`` windows and their ONE read-back (a
        certified library: ``_budgeted_certified``).
        Returns ``(ids by table slot, scans, the budgets' words as a flat list)``; no scans where nothing is to be searched."""
        check_queries([int(q[0].shape[0]) for q in queries], self.max_q_l)
        subset, ids = self._search_ids(videos)
        if self.certified:
            self.last_certified = []                # (nothing searched: no flags; a search that runs fills them in)
        if not queries or not ids:
            return ids, [], []
        self._check_live()
        if self._flags & _lib.SESSION_BF16:
            raise _lib.ConeHipError(f"VideoLibrary: {call}: CONE_SESSION_BF16 libraries are not supported (prefilter_bf16)")
        table = self._table(subset, ids)
        if self.certified:
            scans, host = self._budgeted_certified(table, _chunked(queries), W)
            return table[0], scans, host
        scans, budgets = zip(*self._scan_budget(table, _chunked(queries), W))
        return table[0], scans, (budgets[0] if len(budgets) == 1 else torch.cat(budgets)).cpu().tolist()

    @torch.no_grad()
    def search_windows(self, queries, n_windows=None, videos=None):
        """``[(tok, cls), ...]`` -> per query ``[(video id, best score, k, moments), ...]``: a budget of ``n_windows`` windows per
        query (``None``: ``topk_window``, the price of ONE ``predict_moment``) spent on the best windows of the whole library --
        or of ``videos`` --, wherever they lie: twelve may go to one video, one each to three more.  The entries are the videos
        that receive a window, in ``rank_videos``' order, with its score; ``k`` is the video's share and ``moments ==`` a
        localizer of the same weights with ``topk_window = k``, ``.predict_moment(video_feats, query)`` (the windows chosen from a
        video are a prefix of its stable list).  A window of score -inf is never chosen: a library with fewer windows than the
        budget spends it short, every video then at its own K, as in ``search``.
        One scan and one ``cone_library_budget`` per 64 queries, ONE small read-back (pairs, counts, scores), the
        ``cone_library_localize_ragged`` calls that ``plan_ragged_calls`` lays out, one read-back of the kept rows.  fp32
        libraries only (a ``prefilter_bf16`` library is refused by name); ``n_windows`` in [1, 256].
        The scores inside ``moments`` are normalised per pair and are not comparable across videos: ``search_moments`` is the call
        that ranks the moments of different videos against each other."""
        queries = list(queries)
        W, _ = self._budget_args(n_windows, None, pool=False)
        ids, scans, host = self._budgeted("search_windows", queries, videos, W)                 # the one small read-back
        if not scans:
            return [[] for _ in queries]
        V = len(ids)
        bufs, sizes, plans, at = [], [], [], 0
        for scan in scans:
            chunk = scan[1]
            pairs, at = decode_budget(host, at, len(chunk), W, best=True)
            chosen = [(q, slot, k, score) for q in range(len(chunk)) for slot, k, score in pairs[q]]
            vids = [self._videos[ids[slot]] for _, slot, _, _ in chosen]
            calls = plan_ragged_calls([v[0] for v in vids], [c[2] for c in chosen])
            bufs += [self._enqueue_ragged([(vids[i][:2], chunk[chosen[i][0]], chosen[i][0], chosen[i][1]) for i in idx],
                                          [chosen[i][2] for i in idx], scan, V) for idx in calls]
            sizes += [len(idx) for idx in calls]
            plans.append((chosen, inverse_order([(None, idx) for idx in calls], len(chosen))))
        moments = VideoSession._read_calls(bufs, sizes) if bufs else []              # the kept rows' one read-back
        out, base = [], 0
        for (g, chunk, _, _), (chosen, where) in zip(scans, plans):
            rows = [[] for _ in chunk]
            for i, (q, slot, k, score) in enumerate(chosen):
                rows[q].append((ids[slot], score, k, moments[base + where[i]]))
            out += rows
            base += len(chosen)
        return out

    # ---- moment search -------------------------------------------------------------------------
    @torch.no_grad()
    def search_moments(self, queries, n_windows=None, n_moments=5, videos=None):
        """``[(tok, cls), ...]`` -> per query ``[(video id, [st, ed, score]), ...]``: the at most ``n_moments`` best moments of
        the whole library -- or of ``videos`` -- for the query, fused score descending; seconds from each video's first clip,
        4-decimal doubles like ``predict_moment``'s.  ``search_windows``' budget of ``n_windows`` windows (``None``:
        ``topk_window``) picks where to look; everything that comes out of those windows is ONE candidate pool per query and
        run_on_video/cone_localizator.py:187-221 runs on the pool: both score lists are normalised over all of it, so a score
        means the same in every video, the dict is keyed by (video, st, ed) and a moment suppresses only moments of its own
        video.  On a one-video library the answer is the localizer's ``predict_moment`` at ``topk_window = `` the video's share.
        One scan and one ``cone_library_budget`` per 64 queries, ONE small read-back (pairs, counts), the
        ``cone_library_localize_candidates`` calls that ``plan_ragged_calls`` lays out -- all writing into one candidate buffer
        --, the segment table built on the host and uploaded once, one ``cone_corpus_fuse_nms`` per 64 queries, ONE read-back.
        ``n_windows * num_queries`` (the decoder's slots) may not exceed 1 024 candidates; ``n_moments`` in [1, 100]; fp32
        libraries only."""
        import numpy as np
        queries = list(queries)
        W, M = self._budget_args(n_windows, n_moments)
        ids, scans, host = self._budgeted("search_moments", queries, videos, W)                 # the one small read-back
        if not scans:
            return [[] for _ in queries]
        V, Nq, dev = len(ids), int(self._loc.args.num_queries), self._loc.device
        # the plan of every scan: its pairs in the budget's order (per query: best score descending, ties to the lower slot) and
        # where each pair's candidates lie in the ONE buffer of the search
        plans, at, n_rows = [], 0, 0
        for scan in scans:
            pairs, at = decode_budget(host, at, len(scan[1]), W)
            chosen = [(q, slot, k) for q, row in enumerate(pairs) for slot, k in row]
            vids = [self._videos[ids[slot]] for _, slot, _ in chosen]
            calls = plan_ragged_calls([v[0] for v in vids], [c[2] for c in chosen])
            row_of, n_rows = place_calls(calls, [c[2] for c in chosen], Nq, n_rows)
            plans.append((chosen, vids, calls, row_of, pairs))
        cand = torch.empty(max(n_rows, 1), 4, dtype=torch.float32, device=dev)
        for scan, (chosen, vids, calls, row_of, _) in zip(scans, plans):
            for idx in calls:
                self._enqueue_ragged([(vids[i][:2], scan[1][chosen[i][0]], chosen[i][0], chosen[i][1]) for i in idx],
                                     [chosen[i][2] for i in idx], scan, V, cand=cand[row_of[idx[0]]:])
        # the segment table of the whole search, one upload: seg_cand (int64) | seg_n | seg_tag | every scan's seg_off (int32)
        n_seg = sum(len(p[0]) for p in plans)
        words = np.zeros(2 * n_seg + 2 * n_seg + sum(len(s[1]) + 1 for s in scans) + 1, dtype=np.int32)
        seg_cand, seg_n, seg_tag = words[:2 * n_seg].view(np.int64), words[2 * n_seg:3 * n_seg], words[3 * n_seg:4 * n_seg]
        off_at, seg_at, launches = 4 * n_seg, 0, []
        for scan, (chosen, _, _, row_of, pairs) in zip(scans, plans):
            nq = len(scan[1])
            seg_cand[seg_at:seg_at + len(chosen)] = row_of
            seg_n[seg_at:seg_at + len(chosen)] = [c[2] * Nq for c in chosen]
            seg_tag[seg_at:seg_at + len(chosen)] = [c[1] for c in chosen]
            words[off_at + 1:off_at + nq + 1] = np.cumsum([len(row) for row in pairs])
            launches.append((nq, off_at, seg_at, len(chosen)))
            off_at += nq + 1
            seg_at += len(chosen)
        tab = torch.from_numpy(words).to(dev)
        out = FuseOut([nq for nq, _, _, _ in launches], M, dev)
        p = lambda word: C.c_void_p(tab.data_ptr() + 4 * word)
        for i, (nq, off, seg0, ns) in enumerate(launches):
            out.launch(i, _lib.ptr(cand), p(off), p(2 * seg0), p(2 * n_seg + seg0), p(3 * n_seg + seg0), ns)
        res = []
        for (*_, pairs), (rows, seg, kept) in zip(plans, out.read()):                         # the moments' one read-back
            res += [pooled_moments(rows[q], seg[q], kept[q], [ids[slot] for slot, _ in pairs[q]]) for q in range(len(kept))]
        return res
