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

Standing queries over the LIBRARY (``VideoLibrary.watch_moments``): a ``LibraryWatcher`` asks the same of every resident video at
once and answers ``== lib.search_moments(queries, n_windows, n_moments, videos)``.  One cache ``(nq, n_win_total, Nq, 4)`` and one
stamp plane serve all videos: every watched video owns a slab ``[win0, win0 + cap)`` of the window axis, keyed on the host by its
id (``RowRanges``: first fit, a quarter of headroom, released on ``remove``; a video that outgrows its slab moves, planes and
stamps copied; when no range fits the axis grows by a quarter), and its stamps are ITS clip counts.  One poll, per 64 queries:
``cone_library_scan``; ``cone_library_budget``; ``cone_watch_pool_plan`` (csrc/library_watch_pool.hip) -- thread t owns the t-th
chosen window in ``search_moments``' pool order, a pair's missing windows are compacted into the scan's own ``(nq, V, K)`` layout,
the segment table has one segment per chosen window --; ONE small read-back (the budget's words and the miss counts); the
``cone_library_localize_candidates`` calls over the pairs that miss something; ``cone_watch_pool_store`` (a job per such pair);
``cone_corpus_fuse_nms`` on the cache; one read-back of the kept rows.  A ``trim`` zeroes that video's slab of stamps only.

Not supported: ``prefilter_bf16`` and certified libraries, pools above 1 024 candidates, planning on the device (the miss counts
are read back), shifting cached rows through a ``trim``, sharing cache between different queries, capturing a poll in a graph,
more than one GPU.
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


class LibraryWatcher:
    """``lib.watch_moments(queries, n_windows, n_moments, videos)``.  ``poll()`` returns one list per query, ``==``
    ``lib.search_moments(queries, n_windows, n_moments, videos)`` on the library as it is now; ``windows_listed`` /
    ``windows_run`` count, per query and for the last poll, the windows the budget chose and those the window model ran."""

    def __init__(self, library, queries, n_windows, n_moments, videos):
        from .library import RowRanges
        self._lib = library
        loc = library._loc
        a, dev = loc.args, loc.device
        self._K, self._Nq, self._W = int(a.topk_window), int(a.num_queries), int(a.max_v_l)
        self._Wb, self._M = int(n_windows), int(n_moments)
        self._ids = None if videos is None else list(videos)
        self._chunks = []
        for g in range(0, len(queries), MAX_QUERIES):
            self._chunks.append([(t.to(dev, torch.float32).contiguous(), c.to(dev, torch.float32).reshape(-1).contiguous())
                                 for t, c in queries[g:g + MAX_QUERIES]])
        self._nq = len(queries)
        Wb = self._Wb
        # the plan's outputs: the miss counts of ALL chunks are one tensor (they ride the poll's one small read-back); the segment
        # tables never change size, the miss lists follow the table's slot count
        self._pair_miss = torch.zeros(self._nq * Wb, dtype=torch.int32, device=dev)
        self._plans = [dict(seg_cand=torch.empty(len(c) * Wb, dtype=torch.int64, device=dev),
                            seg=torch.empty(2 * len(c) * Wb + len(c) + 1, dtype=torch.int32, device=dev),      # seg_n | seg_tag | seg_off
                            miss=None) for c in self._chunks]
        # the window axis: a slab per watched video, keyed by its id; free entries always carry a zero stamp
        watched = list(library._videos) if videos is None else self._ids
        n_tot = max(sum(self._cap(ops.num_windows(library._videos[v][1], self._W)) for v in watched), 1)
        self._axis = RowRanges(n_tot)
        self._slabs = {}                    # id -> (win0, cap)
        self._cache = torch.empty(self._nq, n_tot, self._Nq, 4, dtype=torch.float32, device=dev)
        self._stamp = torch.zeros(self._nq, n_tot, dtype=torch.int32, device=dev)
        self._stale = set()                 # ids trimmed since the last poll
        self._table = None                  # (key, scan table) of an explicit video list
        self._vtab = (None, None)           # (host v_win0 + v_cap by slot, their device copy)
        self.windows_run = [0] * self._nq
        self.windows_listed = [0] * self._nq
        self._open = True

    # ---- lifetime ------------------------------------------------------------------------------
    @property
    def nbytes(self) -> int:
        """Bytes that stay resident for the watcher's cache: the candidate rows and the stamps of the whole window axis."""
        return int(self._cache.numel() * 4 + self._stamp.numel() * 4) if self._open else 0

    def close(self):
        self._open = False
        self._cache = self._stamp = self._plans = self._chunks = self._pair_miss = self._table = self._vtab = None
        self._slabs = self._axis = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _trimmed(self, vid_id):
        """The library's word that ``vid_id`` lost clips at its front: its slab is stale for every query (nothing is launched
        here; the next poll zeroes that slab's stamps)."""
        self._stale.add(vid_id)

    # ---- the window axis -----------------------------------------------------------------------
    @staticmethod
    def _cap(n_win):
        """A video's slab: its windows and a quarter of headroom."""
        return n_win + (n_win + 3) // 4

    def _take(self, n):
        """First-fit on the axis; when no range fits the axis grows by a quarter (at least by ``n``) and is copied."""
        try:
            return self._axis.take(n)
        except ValueError:
            pass
        dev, old = self._cache.device, self._axis.capacity
        new = old + max(old // 4 + 1, n)
        cache = torch.empty(self._nq, new, self._Nq, 4, dtype=torch.float32, device=dev)
        stamp = torch.zeros(self._nq, new, dtype=torch.int32, device=dev)
        cache[:, :old] = self._cache
        stamp[:, :old] = self._stamp
        self._cache, self._stamp = cache, stamp
        self._axis.grow(new)
        return self._axis.take(n)

    def _sync(self, ids):
        """Makes the slabs those of the watched videos ``ids`` as they are now: slabs of videos that left are zeroed and
        released, a trimmed video's stamps are zeroed, a new video takes a slab, a video that outgrew its slab moves (planes and
        stamps copied, the old range zeroed and released).  Only ranges named here are touched."""
        L, watched = self._lib, set(ids)
        for v in [v for v in self._slabs if v not in watched]:
            win0, cap = self._slabs.pop(v)
            self._stamp[:, win0:win0 + cap].zero_()
            self._axis.release(win0, cap)
        for v in self._stale:
            if v in self._slabs:
                win0, cap = self._slabs[v]
                self._stamp[:, win0:win0 + cap].zero_()
        self._stale.clear()
        for v in ids:
            n_win = ops.num_windows(L._videos[v][1], self._W)
            if v not in self._slabs:
                cap = self._cap(n_win)
                self._slabs[v] = (self._take(cap), cap)
            elif n_win > self._slabs[v][1]:
                win0, cap = self._slabs[v]
                new_cap = self._cap(n_win)
                new0 = self._take(new_cap)                                  # (a free range: disjoint from the old slab)
                self._cache[:, new0:new0 + cap] = self._cache[:, win0:win0 + cap]
                self._stamp[:, new0:new0 + cap] = self._stamp[:, win0:win0 + cap]
                self._stamp[:, win0:win0 + cap].zero_()
                self._axis.release(win0, cap)
                self._slabs[v] = (new0, new_cap)

    # ---- the poll ------------------------------------------------------------------------------
    @torch.no_grad()
    def poll(self):
        """Per query ``[(video id, [st, ed, score]), ...]``, ``==`` ``search_moments`` on the library as it is now.  The window
        model runs only on the chosen windows the cache does not hold (``windows_run``, of ``windows_listed``); two read-backs."""
        from .library import plan_ragged_calls, pooled_moments
        if not self._open:
            raise RuntimeError("LibraryWatcher: the watcher is closed")
        L = self._lib
        L._check_live()
        subset, ids = L._search_ids(self._ids)
        if not ids:
            self._sync([])
            self.windows_run, self.windows_listed = [0] * self._nq, [0] * self._nq
            return [[] for _ in range(self._nq)]
        lib, dev = _lib.load(), L._loc.device
        K, Nq, W, Wb, M = self._K, self._Nq, self._W, self._Wb, self._M
        if subset is None:
            table = L._table(None, ids)
        else:
            key = tuple(L._videos[v][:2] for v in ids)
            if self._table is None or self._table[0] != key:
                self._table = (key, L._table(subset, ids))
            table = self._table[1]
        ids, V = table[0], len(table[0])                                        # (by table slot from here on)
        self._sync(ids)
        n_tot = self._axis.capacity
        vtab = [self._slabs[v][0] for v in ids] + [self._slabs[v][1] for v in ids]
        if self._vtab[0] != vtab:                                               # slabs or slots changed: one small upload
            self._vtab = (vtab, torch.tensor(vtab, dtype=torch.int32).to(dev))
        v_ctx_l, v_tab = table[2], self._vtab[1]
        p32 = lambda t, word=0: C.c_void_p(t.data_ptr() + 4 * word)
        # 1-3. the lists, the budget and the plan of every chunk
        budgets, g = [], 0
        for chunk, P in zip(self._chunks, self._plans):
            n = len(chunk)
            widx, wval, _ = L._scan(table, chunk, 1)
            b = L._budget((g, chunk, widx, wval), V, Wb)                        # n_pairs | pair_slot | pair_k | pair_best
            if P["miss"] is None or P["miss"].numel() < 2 * n * V * K:
                P["miss"] = torch.empty(2 * n * V * K, dtype=torch.int32, device=dev)          # miss_widx | miss_wval
            _lib.check(lib.cone_watch_pool_plan(_lib.ptr(widx), _lib.ptr(wval), p32(b), p32(b, n), p32(b, n + n * Wb), _lib.ptr(v_ctx_l),
                                                p32(v_tab), p32(v_tab, V), p32(self._stamp, g * n_tot), n, V, K, Wb, n_tot, W, Nq,
                                                p32(P["miss"]), p32(P["miss"], n * V * K), p32(self._pair_miss, g * Wb),
                                                p32(P["seg"], 2 * n * Wb), _lib.ptr(P["seg_cand"]), p32(P["seg"]),
                                                p32(P["seg"], n * Wb), _lib.stream()))
            budgets.append(b)
            g += n
        host = torch.cat(budgets + [self._pair_miss]).cpu().tolist()            # the one small read-back
        # the host's plan: every query's pairs in the budget's order, the calls over the pairs that miss something, their jobs
        miss_at = sum(b.numel() for b in budgets)
        plans, jobs, n_rows, at, g = [], [], 0, 0, 0
        run, listed = [], []
        for chunk in self._chunks:
            n = len(chunk)
            pairs = []                                                          # per query [(slot, k, miss), ...]
            for q in range(n):
                np_q = host[at + q]
                row = at + n + q * Wb
                pairs.append([(host[row + i], host[row + n * Wb + i], host[miss_at + (g + q) * Wb + i]) for i in range(np_q)])
                listed.append(sum(p[1] for p in pairs[-1]))
                run.append(sum(p[2] for p in pairs[-1]))
            at += n + 3 * n * Wb
            missing = [(q, slot, m) for q in range(n) for slot, _, m in pairs[q] if m > 0]
            vids = [L._videos[ids[slot]] for _, slot, _ in missing]
            calls = plan_ragged_calls([v[0] for v in vids], [m[2] for m in missing]) if missing else []
            first_job, rows_of = len(jobs), []
            for idx in calls:
                rows_of.append(n_rows)
                for i in idx:
                    jobs.append((missing[i][0], missing[i][1], missing[i][2], n_rows))
                    n_rows += missing[i][2] * Nq
            plans.append((pairs, missing, vids, calls, rows_of, first_job, len(jobs) - first_job))
            g += n
        if jobs:
            cand = torch.empty(n_rows, 4, dtype=torch.float32, device=dev)
            job_tab = torch.tensor(jobs, dtype=torch.int32).to(dev)             # the poll's one small upload
        # 5-7. the query half on the missing windows, the scatter, stage C on the cache
        sizes = [(len(c) * M * 5, (len(c) * M + len(c) + 1) // 2) for c in self._chunks]
        out = torch.empty(sum(a + b for a, b in sizes), dtype=torch.float64, device=dev)
        g = o = 0
        for chunk, P, (pairs, missing, vids, calls, rows_of, job0, n_jobs), (n_r, n_i) in zip(self._chunks, self._plans, plans, sizes):
            n = len(chunk)
            cache = p32(self._cache, g * n_tot * Nq * 4)
            miss_widx, miss_wval = P["miss"][:n * V * K], P["miss"][n * V * K:2 * n * V * K].view(torch.float32)
            for idx, row in zip(calls, rows_of):
                L._enqueue_ragged([(vids[i][:2], chunk[missing[i][0]], missing[i][0], missing[i][1]) for i in idx],
                                  [missing[i][2] for i in idx], (g, chunk, miss_widx, miss_wval), V, cand=cand[row:])
            if n_jobs:
                _lib.check(lib.cone_watch_pool_store(_lib.ptr(cand), p32(job_tab, 4 * job0), n_jobs, p32(miss_widx), _lib.ptr(v_ctx_l),
                                                     p32(v_tab), p32(v_tab, V), n, V, K, n_tot, Nq, cache, p32(self._stamp, g * n_tot),
                                                     _lib.stream()))
            _lib.check(lib.cone_corpus_fuse_nms(cache, p32(P["seg"], 2 * n * Wb), _lib.ptr(P["seg_cand"]), p32(P["seg"]),
                                                p32(P["seg"], n * Wb), n, n * Wb, NMS_THD, MAX_BEFORE, M,
                                                C.c_void_p(out.data_ptr() + 8 * o), C.c_void_p(out.data_ptr() + 8 * (o + n_r)),
                                                C.c_void_p(out.data_ptr() + 8 * (o + n_r) + 4 * n * M), _lib.stream()))
            g += n
            o += n_r + n_i
        host = out.cpu()                                                        # the moments' one read-back
        res, o = [], 0
        for chunk, (pairs, *_), (n_r, n_i) in zip(self._chunks, plans, sizes):
            n = len(chunk)
            rows = host[o:o + n_r].view(n, M, 5).tolist()
            ints = host[o + n_r:o + n_r + n_i].view(torch.int32)
            seg, kept = ints[:n * M].view(n, M).tolist(), ints[n * M:n * M + n].tolist()
            o += n_r + n_i
            for q in range(n):      # a segment is a chosen window here: window t of the pool belongs to the pair that owns ordinal t
                seg_video = [ids[slot] for slot, k, _ in pairs[q] for _ in range(k)]
                res.append(pooled_moments(rows[q], seg[q], kept[q], seg_video))
        self.windows_run, self.windows_listed = run, listed
        return res
