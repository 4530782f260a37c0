"""Video libraries: many resident videos in one arena, one call for queries on any mix of them
(``CONELocalizator.open_library``).

A ``VideoSession`` batches the queries of ONE video; a process that keeps many videos resident (a user's recordings, a
catalogue of episodes) receives queries for different videos and would pay the single-query price -- almost all of it launch
latency -- for each.  A ``VideoLibrary`` keeps the video half of ``predict_moment`` (run_on_video/cone_localizator.py:121-221)
of MANY videos in the rows of one arena and answers a list of ``(video, query)`` pairs in one C call per 64 pairs
(``cone_library_localize``, csrc/session.hip).  Nothing new is computed: the window ranking runs per video exactly as in a
session, everything after it is one launch over all windows of all pairs, and every answer equals the localizer's
``predict_moment(video_feats, query)`` with ``==``.

Rows are handed out first-fit from a free list and coalesce when a video is removed.  An open library neither grows nor
compacts: ``add`` raises when no hole fits, however many clips are free in total -- size it for the working set, or open a
second one.  Out of scope here: certified window ranking, growing a video in place, capturing the call in a graph.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, ops
from .session import MAX_QUERIES, NMS_THD, MAX_BEFORE, MAX_AFTER, VideoSession, _kept_bytes, check_queries


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


class VideoLibrary:
    """Many resident videos of a ``CONELocalizator`` (``open_library``).  ``add`` indexes a video into free rows and returns its
    id (never reused); ``predict_moments([(id, (tok, cls)), ...])`` returns, per pair and in the order given, what the
    localizer's ``predict_moment`` returns for that video and query, ``==``.  No compaction, no growth: see the module text."""

    def __init__(self, localizer, capacity_clips: int):
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
        n_arena = lib.cone_library_arena_bytes(h, self._rows.capacity, self._flags)
        if n_arena == 0:
            raise _lib.ConeHipError(f"libcone_hip error: {lib.cone_last_error().decode()}")
        self._arena = torch.empty(n_arena, dtype=torch.uint8, device=localizer.device)
        self._cl = _lib.Library()
        _lib.check(lib.cone_library_open(h, self._rows.capacity, self._flags, _lib.ptr(self._arena), n_arena, C.byref(self._cl)))
        self._params = _lib.SessionParams(int(a.max_v_l), int(a.max_q_l), float(a.clip_length), NMS_THD, MAX_BEFORE, MAX_AFTER)
        self._ws = Workspace()              # the per-call workspace (grow-only)
        self._open = True

    # ---- lifetime ------------------------------------------------------------------------------
    @property
    def nbytes(self) -> int:
        """Bytes that stay resident for the library (its arena, whatever it holds)."""
        return int(self._arena.numel()) if self._open else 0

    @property
    def free_clips(self) -> int:
        return self._rows.free if self._open else 0

    def close(self):
        self._open = False              # (the ids stay known: a call on a closed library says "closed", not "unknown id")
        self._arena = self._cl = self._ws = None

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
    def add(self, video_feats):
        """Index ``video_feats`` (clips, dim) into the first free row range that holds it; returns the video's id.  Raises
        ``ValueError`` when no hole fits (the message names the clips asked for and the largest free hole)."""
        self._check_live()
        a, m = self._loc.args, self._loc.localizator
        vid = video_feats.to(self._loc.device, torch.float32).contiguous()
        if vid.dim() != 2 or vid.shape[0] < 1:
            raise ValueError(f"add: video_feats must be (clips >= 1, dim), got {tuple(vid.shape)}")
        m._check_dim(vid, a.v_appear_feat_dim, "appearance clip features")
        m._check_dim(vid, a.v_motion_feat_dim, "motion clip features")
        n = int(vid.shape[0])
        row0 = self._rows.take(n)
        try:
            lib, h = _lib.load(), m._h()
            n_ws = lib.cone_library_add_workspace(h, n)
            ws = torch.empty(max(n_ws, 1), dtype=torch.uint8, device=vid.device)
            _lib.check(lib.cone_library_add(h, C.byref(self._cl), row0, _lib.ptr(vid), n, _lib.ptr(ws), n_ws, _lib.stream()))
        except Exception:
            self._rows.release(row0, n)
            raise
        vid_id, self._next_id = self._next_id, self._next_id + 1
        self._videos[vid_id] = (row0, n, min(int(a.topk_window), ops.num_windows(n, a.max_v_l)))
        return vid_id

    def remove(self, vid_id):
        """The video's rows become free (queries already enqueued on the stream have read them by the time a later ``add``
        overwrites them: one stream).  Its id is never handed out again."""
        row0, n, _ = self._video(vid_id)
        del self._videos[vid_id]
        self._rows.release(row0, n)

    def _video(self, vid_id):
        try:
            return self._videos[vid_id]
        except (KeyError, TypeError):
            raise ValueError(f"VideoLibrary: unknown or removed video id {vid_id!r}") from None

    # ---- queries -------------------------------------------------------------------------------
    def _enqueue(self, K, chunk):
        """One ``cone_library_localize`` call: ``chunk`` = [((row0, ctx_l), (tok, cls)), ...], at most MAX_QUERIES."""
        lib, m, dev = _lib.load(), self._loc.localizator, self._loc.device
        h, nq = m._h(), len(chunk)
        toks = [t.to(dev, torch.float32).contiguous() for _, (t, _) in chunk]
        tok_cat = toks[0] if nq == 1 else torch.cat(toks)
        cls = torch.stack([c.to(dev, torch.float32).reshape(-1) for _, (_, c) in chunk]).contiguous()
        i32 = C.c_int32 * nq
        row0, ctx, lens = i32(*(v[0] for v, _ in chunk)), i32(*(v[1] for v, _ in chunk)), i32(*(int(t.shape[0]) for t in toks))
        nbytes = lib.cone_library_localize_workspace(h, C.byref(self._cl), row0, ctx, lens, nq, K, C.byref(self._params))
        if nbytes == 0:
            raise _lib.ConeHipError(f"libcone_hip error: {lib.cone_last_error().decode()}")
        ws = self._ws.get(nbytes, dev)
        R, N = _kept_bytes(nq)
        buf = torch.empty(R + N, dtype=torch.uint8, device=dev)
        _lib.check(lib.cone_library_localize(h, C.byref(self._cl), row0, ctx, _lib.ptr(tok_cat, torch.float32), lens, nq,
                                             _lib.ptr(cls, torch.float32), K, C.byref(self._params), C.c_void_p(buf.data_ptr()),
                                             C.c_void_p(buf.data_ptr() + R), _lib.ptr(ws), ws.numel(), _lib.stream()))
        return buf

    @torch.no_grad()
    def predict_moments(self, pairs):
        """``[(video id, (text_token_feats, text_cls_feat)), ...]`` for any mix of the library's videos -> a list of moment
        lists in the order given, each ``==`` the localizer's ``predict_moment(video_feats, query)``.  Every pair is checked
        before any GPU work; the pairs are grouped by window count K (long videos all share ``topk_window``: usually one
        group), sorted by video inside a group, cut into calls of at most ``MAX_QUERIES``; every call is enqueued, then ONE
        read-back."""
        pairs = list(pairs)
        videos = [self._video(v) for v, _ in pairs]
        check_queries([int(q[0].shape[0]) for _, q in pairs], self.max_q_l)
        if not pairs:
            return []
        self._check_live()
        calls = plan_calls([v[0] for v in videos], [v[2] for v in videos])        # (a video is its first row: unique while it lives)
        where = inverse_order(calls, len(pairs))
        bufs = [self._enqueue(K, [(videos[i][:2], pairs[i][1]) for i in idx]) for K, idx in calls]
        host = (bufs[0] if len(bufs) == 1 else torch.cat(bufs)).cpu()             # the call's one read-back
        out, at = [], 0
        for _, idx in calls:
            n = sum(_kept_bytes(len(idx)))
            out += VideoSession.read_kept(host[at:at + n].clone() if at else host, len(idx))
            at += n
        return [out[w] for w in where]

    def predict_moment(self, vid_id, text_feats):
        """``localizer.predict_moment(video_feats, text_feats)`` for the resident video ``vid_id``."""
        return self.predict_moments([(vid_id, text_feats)])[0]
