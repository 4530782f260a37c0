"""Standing queries on a live video (``VideoLibrary.watch``): a fixed set of queries asked again after every few new clips.

``extend`` + ``trim`` keep the sliding window of a live recording resident; what such a recording is for is a set of queries that
is answered again whenever it has grown.  ``predict_moments`` runs the window model on all K ranked windows of every query every
time, although an ``extend`` by a handful of clips changes at most the last two or three windows of the video.  A window's
candidate rows depend on nothing outside the window -- ``cone_window_table`` gives window ``wi`` the clips
``[max((wi - 1) S, 0), min((wi - 1) S + W, ctx_l))``, every pair is padded to ``W``, a row ``[st, ed, prop, match]`` is made from
the window's start and its own outputs, and a row's bits do not depend on the call it is computed in
(tests/test_library_watch_gpu.py pins it) -- so a ``VideoWatcher`` keeps the ``num_queries`` rows of every (query, window) it has
computed, with the video's clip count at that time (the stamp), and a ``poll`` runs the window model only on listed windows it
has not seen or saw while they were still growing.  Stage C (``cone_corpus_fuse_nms``) then runs on the CACHE, over the windows
of the query's current list in list order: the pool of ``predict_moment``, so the answer is ``predict_moment``'s, ``==``.

One poll, per 64 queries: ``cone_library_scan`` on a one-video table (the per-video pre-filter's lists, bit for bit);
``cone_watch_plan`` (csrc/library_watch.hip) compacts the missing windows of every query and lays the segment table; ONE small
read-back of the miss counts; one ``cone_library_localize_candidates`` on the miss lists for the queries that miss anything;
``cone_watch_store`` scatters the new rows into the cache; ``cone_corpus_fuse_nms``; one read-back of the kept rows.  Two
read-backs a poll, whatever the query count.

The cache holds results, not row addresses: ``compact``, ``resize`` and a relocating ``extend`` change nothing.  A ``trim``
moves the first clip -- seconds and window indices shift -- so the library tells its watchers and the next poll runs every listed
window.  Memory: per query and per window of the video ``num_queries`` rows of 16 B and one int32 stamp
(``64 x 735 x (10 x 16 + 4)`` B = 7.7 MB for 64 queries on 33 000 clips at ``num_queries = 10``); when the video outgrows the
cache it is reallocated a quarter larger and the (query, window) planes and stamps are copied.
Not supported: ``prefilter_bf16`` and certified libraries, watchers over several videos, pools above 1 024 candidates, planning
on the device (the miss counts are read back), capturing a poll in a graph.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, ops
from .session import MAX_QUERIES, NMS_THD, MAX_BEFORE, MAX_AFTER


class VideoWatcher:
    """``lib.watch(vid_id, queries)``.  ``poll()`` returns one moment list per query, each ``==`` the localizer's
    ``predict_moment(<the video's current clips>, query)``; ``windows_run`` / ``windows_listed`` describe the last poll."""

    def __init__(self, library, vid_id, queries):
        self._lib, self._vid = library, vid_id
        loc = library._loc
        a, dev = loc.args, loc.device
        self._K, self._Nq, self._W = int(a.topk_window), int(a.num_queries), int(a.max_v_l)
        # the queries live on the device for the watcher's life, in chunks of one call each
        self._chunks = []
        for g in range(0, len(queries), MAX_QUERIES):
            self._chunks.append([(t.to(dev, torch.float32).contiguous(), c.to(dev, torch.float32).reshape(-1).contiguous())
                                 for t, c in queries[g:g + MAX_QUERIES]])
        self._nq = len(queries)
        K = self._K
        # the plan's outputs, per chunk (their sizes never change); the miss counts of ALL chunks are one tensor: one read-back
        self._n_miss = torch.zeros(self._nq, dtype=torch.int32, device=dev)
        self._plans = []
        for chunk in self._chunks:
            n = len(chunk)
            self._plans.append(dict(miss_widx=torch.empty(n * K, dtype=torch.int32, device=dev),
                                    miss_wval=torch.empty(n * K, dtype=torch.float32, device=dev),
                                    seg_cand=torch.empty(n * K, dtype=torch.int64, device=dev),
                                    seg=torch.empty(2 * n * K + n + 1, dtype=torch.int32, device=dev)))     # seg_n | seg_tag | seg_off
        _, ctx_l, _ = library._video(vid_id)
        self._n_win = ops.num_windows(ctx_l, self._W)
        self._cache = torch.empty(self._nq, self._n_win, self._Nq, 4, dtype=torch.float32, device=dev)
        self._stamp = torch.zeros(self._nq, self._n_win, dtype=torch.int32, device=dev)
        self._reset = False
        self._table = None                  # ((row0, ctx_l), the one-video scan table)
        self.windows_run = [0] * self._nq
        self.windows_listed = [0] * self._nq
        self._open = True

    # ---- lifetime ------------------------------------------------------------------------------
    @property
    def nbytes(self) -> int:
        """Bytes that stay resident for the watcher's cache: the candidate rows and the stamps."""
        return int(self._cache.numel() * 4 + self._stamp.numel() * 4) if self._open else 0

    def close(self):
        self._open = False
        self._cache = self._stamp = self._plans = self._chunks = self._n_miss = self._table = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _trimmed(self, vid_id):
        """The library's word that ``vid_id`` lost clips at its front: every entry of the cache is stale (nothing is launched
        here; the next poll zeroes the stamps)."""
        if vid_id == self._vid:
            self._reset = True

    def _grow(self, n_win):
        """The video has more windows than the cache has planes: a quarter more than it needs, the planes and stamps copied."""
        dev, old = self._cache.device, self._n_win
        new = max(n_win, old + old // 4 + 1)
        cache = torch.empty(self._nq, new, self._Nq, 4, dtype=torch.float32, device=dev)
        stamp = torch.zeros(self._nq, new, dtype=torch.int32, device=dev)
        cache[:, :old] = self._cache
        stamp[:, :old] = self._stamp
        self._cache, self._stamp, self._n_win = cache, stamp, new

    # ---- the poll ------------------------------------------------------------------------------
    @torch.no_grad()
    def poll(self):
        """One moment list per query, ``==`` ``predict_moment`` on the video as it is now.  The window model runs only on the
        listed windows the cache does not hold (``windows_run``); two read-backs."""
        if not self._open:
            raise RuntimeError("VideoWatcher: the watcher is closed")
        L = self._lib
        L._check_live()
        row0, ctx_l, _ = L._video(self._vid)
        lib, dev = _lib.load(), L._loc.device
        K, Nq, W = self._K, self._Nq, self._W
        n_win = ops.num_windows(ctx_l, W)
        if n_win > self._n_win:
            self._grow(n_win)
        if self._reset:
            self._stamp.zero_()
            self._reset = False
        if self._table is None or self._table[0] != (row0, ctx_l):
            self._table = ((row0, ctx_l), L._table([self._vid], [self._vid]))
        table = self._table[1]
        p32 = lambda t, word=0: C.c_void_p(t.data_ptr() + 4 * word)
        # 1-2. the lists and the plan of every chunk
        g = 0
        for chunk, P in zip(self._chunks, self._plans):
            n = len(chunk)
            widx, wval, _ = L._scan(table, chunk, 1)
            _lib.check(lib.cone_watch_plan(_lib.ptr(widx), _lib.ptr(wval), n, K, p32(self._stamp, g * self._n_win), self._n_win, ctx_l, W,
                                           Nq, _lib.ptr(P["miss_widx"]), _lib.ptr(P["miss_wval"]), p32(self._n_miss, g),
                                           p32(P["seg"], 2 * n * K), _lib.ptr(P["seg_cand"]), p32(P["seg"]), p32(P["seg"], n * K),
                                           _lib.stream()))
            g += n
        n_miss = self._n_miss.cpu().tolist()                                    # the one small read-back
        # 4-6. the query half on the missing windows, the scatter, stage C on the cache
        sizes = [(len(c) * MAX_AFTER * 5, (len(c) * MAX_AFTER + len(c) + 1) // 2) for c in self._chunks]
        out = torch.empty(sum(a + b for a, b in sizes), dtype=torch.float64, device=dev)
        g = o = 0
        for chunk, P, (n_r, n_i) in zip(self._chunks, self._plans, sizes):
            n = len(chunk)
            cache = p32(self._cache, g * self._n_win * Nq * 4)
            miss = [q for q in range(n) if n_miss[g + q] > 0]
            if miss:
                ks = [n_miss[g + q] for q in miss]
                cand = torch.empty(sum(ks) * Nq, 4, dtype=torch.float32, device=dev)
                L._enqueue_ragged([((row0, ctx_l), chunk[q], q, 0) for q in miss], ks, (g, chunk, P["miss_widx"], P["miss_wval"]), 1,
                                  cand=cand)
                _lib.check(lib.cone_watch_store(_lib.ptr(cand), _lib.ptr(P["miss_widx"]), p32(self._n_miss, g), n, K, self._n_win,
                                                ctx_l, Nq, cache, p32(self._stamp, g * self._n_win), _lib.stream()))
            _lib.check(lib.cone_corpus_fuse_nms(cache, p32(P["seg"], 2 * n * K), _lib.ptr(P["seg_cand"]), p32(P["seg"]),
                                                p32(P["seg"], n * K), n, n * K, NMS_THD, MAX_BEFORE, MAX_AFTER,
                                                C.c_void_p(out.data_ptr() + 8 * o), C.c_void_p(out.data_ptr() + 8 * (o + n_r)),
                                                C.c_void_p(out.data_ptr() + 8 * (o + n_r) + 4 * n * MAX_AFTER), _lib.stream()))
            g += n
            o += n_r + n_i
        host = out.cpu()                                                        # the moments' one read-back
        res, o = [], 0
        for chunk, (n_r, n_i) in zip(self._chunks, sizes):
            n = len(chunk)
            rows = host[o:o + n_r].view(n, MAX_AFTER, 5).tolist()
            kept = host[o + n_r:o + n_r + n_i].view(torch.int32)[n * MAX_AFTER:n * MAX_AFTER + n].tolist()
            o += n_r + n_i
            res += [[[r[0], r[1], r[4]] for r in rows[q][:kept[q]]] for q in range(n)]
        self.windows_run = n_miss
        self.windows_listed = [min(K, n_win)] * self._nq
        return res
