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

Shared.  Both watchers are a ``_Watcher``: the standing queries uploaded once in chunks of one call, the cache and stamp planes
and their widening along the window axis, the lifetime; both polls write stage C's output through a ``FuseOut``
(cone_amd/library.py), the one owner of that layout, which the watcher keeps for its life.  The polls plan differently -- K
listed windows of one video; a budget over the slab axis -- and stay apart; ``LibraryWatcher.poll`` takes its budget through the
pieces ``search_moments`` uses: ``_scan_budget``, ``decode_budget`` and ``place_calls``.  On the device csrc/watch_common.h holds
the validity rule and the store loop of both store kernels.

On a certified library (``open_library(..., certified=True)``) both watchers run this fp32 path unchanged -- ``_scan_budget``, not
the certified scan: a poll plans chunk by chunk before a read-back, where a certificate's flags would have to be known.

Not supported: ``prefilter_bf16`` libraries, certified polls, pools above 1 024 candidates, planning on the device (the miss counts
are read back), shifting cached rows through a ``trim``, sharing cache between different queries, capturing a poll in a graph,
more than one GPU.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, ops
from .session import MAX_QUERIES, MAX_AFTER


class _Watcher:
    """What the two watchers share: the standing queries on the device, the cache ``(nq, windows, Nq, 4)`` with its stamp plane
    ``(nq, windows)``, and the lifetime.  A subclass names in ``_held`` what else ``close`` lets go of."""

    _held = ()

    def _upload(self, library, queries):
        """The queries live on the device for the watcher's life, in chunks of one call each."""
        self._lib = library
        a, dev = library._loc.args, library._loc.device
        self._K, self._Nq, self._W = int(a.topk_window), int(a.num_queries), int(a.max_v_l)
        self._chunks = [[(t.to(dev, torch.float32).contiguous(), c.to(dev, torch.float32).reshape(-1).contiguous())
                         for t, c in queries[g:g + MAX_QUERIES]] for g in range(0, len(queries), MAX_QUERIES)]
        self._nq = len(queries)
        self.windows_run = [0] * self._nq
        self.windows_listed = [0] * self._nq
        return dev

    def _planes(self, n_win, dev):
        """The cache rows and the stamps (0: never computed) of ``n_win`` windows per query."""
        self._cache = torch.empty(self._nq, n_win, self._Nq, 4, dtype=torch.float32, device=dev)
        self._stamp = torch.zeros(self._nq, n_win, dtype=torch.int32, device=dev)

    def _widen(self, n_win):
        """The window axis becomes ``n_win`` long: new planes and stamps, the old ones copied to their front."""
        old_cache, old_stamp = self._cache, self._stamp
        self._planes(n_win, old_cache.device)
        self._cache[:, :old_cache.shape[1]] = old_cache
        self._stamp[:, :old_stamp.shape[1]] = old_stamp

    @property
    def nbytes(self) -> int:
        """Bytes that stay resident for the watcher's cache: the candidate rows and the stamps of the whole window axis (not
        counted: the queries, the plan's tables and stage C's output buffer, a few hundred bytes per query)."""
        return int(self._cache.numel() * 4 + self._stamp.numel() * 4) if self._open else 0

    def close(self):
        self._open = False
        for name in ("_cache", "_stamp", "_plans", "_chunks", "_table", "_out") + self._held:
            setattr(self, name, None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _check_open(self):
        if not self._open:
            raise RuntimeError(f"{type(self).__name__}: the watcher is closed")


class VideoWatcher(_Watcher):
    """``lib.watch(vid_id, queries)``.  ``poll()`` returns one moment list per query, each ``==`` the localizer's
    ``predict_moment(<the video's current clips>, query)``; ``windows_run`` / ``windows_listed`` describe the last poll."""

    _held = ("_n_miss",)

    def __init__(self, library, vid_id, queries):
        from .library import FuseOut
        dev = self._upload(library, queries)
        self._vid, K = vid_id, self._K
        # the plan's outputs, per chunk (their sizes never change); the miss counts of ALL chunks are one tensor: one read-back
        self._n_miss = torch.zeros(self._nq, dtype=torch.int32, device=dev)
        self._plans = [dict(miss_widx=torch.empty(n * K, dtype=torch.int32, device=dev),
                            miss_wval=torch.empty(n * K, dtype=torch.float32, device=dev),
                            seg_cand=torch.empty(n * K, dtype=torch.int64, device=dev),
                            seg=torch.empty(2 * n * K + n + 1, dtype=torch.int32, device=dev))              # seg_n | seg_tag | seg_off
                       for n in map(len, self._chunks)]
        _, ctx_l, _ = library._video(vid_id)
        self._n_win = ops.num_windows(ctx_l, self._W)
        self._reset = False
        self._table = None                  # ((row0, ctx_l), the one-video scan table)
        self._planes(self._n_win, dev)
        self._out = FuseOut([len(c) for c in self._chunks], MAX_AFTER, dev)      # stage C's outputs, every poll's
        self._open = True

    def _trimmed(self, vid_id):
        """The library's word that ``vid_id`` lost clips at its front: every entry of the cache is stale (nothing is launched
        here; the next poll zeroes the stamps)."""
        if vid_id == self._vid:
            self._reset = True

    def _grow(self, n_win):
        """The video has more windows than the cache has planes: a quarter more than it needs."""
        self._n_win = max(n_win, self._n_win + self._n_win // 4 + 1)
        self._widen(self._n_win)

    # ---- the poll ------------------------------------------------------------------------------
    @torch.no_grad()
    def poll(self):
        """One moment list per query, ``==`` ``predict_moment`` on the video as it is now.  The window model runs only on the
        listed windows the cache does not hold (``windows_run``); two read-backs."""
        self._check_open()
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
        out, g = self._out, 0
        for i, (chunk, P) in enumerate(zip(self._chunks, self._plans)):
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
            out.launch(i, cache, p32(P["seg"], 2 * n * K), _lib.ptr(P["seg_cand"]), p32(P["seg"]), p32(P["seg"], n * K), n * K)
            g += n
        res = []
        for rows, _, kept in out.read(seg=False):                               # the moments' one read-back
            res += [[[r[0], r[1], r[4]] for r in rows[q][:kept[q]]] for q in range(len(kept))]
        self.windows_run = n_miss
        self.windows_listed = [min(K, n_win)] * self._nq
        return res


class LibraryWatcher(_Watcher):
    """``lib.watch_moments(queries, n_windows, n_moments, videos)``.  ``poll()`` returns one list per query, ``==``
    ``lib.search_moments(queries, n_windows, n_moments, videos)`` on the library as it is now; ``windows_listed`` /
    ``windows_run`` count, per query and for the last poll, the windows the budget chose and those the window model ran."""

    _held = ("_pair_miss", "_vtab", "_slabs", "_axis")

    def __init__(self, library, queries, n_windows, n_moments, videos):
        from .library import FuseOut, RowRanges
        dev = self._upload(library, queries)
        self._Wb, self._M = int(n_windows), int(n_moments)
        self._ids = None if videos is None else list(videos)
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
        self._stale = set()                 # ids trimmed since the last poll
        self._table = None                  # (key, scan table) of an explicit video list
        self._vtab = (None, None)           # (host v_win0 + v_cap by slot, their device copy)
        self._planes(n_tot, dev)
        self._out = FuseOut([len(c) for c in self._chunks], self._M, dev)       # stage C's outputs, every poll's
        self._open = True

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
        """First-fit on the axis; when no range fits the axis grows by a quarter (at least by ``n``)."""
        try:
            return self._axis.take(n)
        except ValueError:
            pass
        new = self._axis.capacity + max(self._axis.capacity // 4 + 1, n)
        self._widen(new)
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
        self._check_open()
        from .library import decode_budget, place_calls, plan_ragged_calls, pooled_moments
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
        scans, budgets = [], []
        for ((g, chunk, widx, wval), b), P in zip(L._scan_budget(table, self._chunks, Wb), self._plans):
            n = len(chunk)                                                      # b = n_pairs | pair_slot | pair_k | pair_best
            scans.append((g, chunk))
            budgets.append(b)
            if P["miss"] is None or P["miss"].numel() < 2 * n * V * K:
                P["miss"] = torch.empty(2 * n * V * K, dtype=torch.int32, device=dev)          # miss_widx | miss_wval
            _lib.check(lib.cone_watch_pool_plan(_lib.ptr(widx), _lib.ptr(wval), p32(b), p32(b, n), p32(b, n + n * Wb), _lib.ptr(v_ctx_l),
                                                p32(v_tab), p32(v_tab, V), p32(self._stamp, g * n_tot), n, V, K, Wb, n_tot, W, Nq,
                                                p32(P["miss"]), p32(P["miss"], n * V * K), p32(self._pair_miss, g * Wb),
                                                p32(P["seg"], 2 * n * Wb), _lib.ptr(P["seg_cand"]), p32(P["seg"]),
                                                p32(P["seg"], n * Wb), _lib.stream()))
        host = torch.cat(budgets + [self._pair_miss]).cpu().tolist()            # the one small read-back
        # the host's plan: every query's pairs in the budget's order, the calls over the pairs that miss something, their jobs
        miss_at = sum(b.numel() for b in budgets)
        plans, jobs, n_rows, at = [], [], 0, 0
        run, listed = [], []
        for g, chunk in scans:
            n = len(chunk)
            pairs, at = decode_budget(host, at, n, Wb, miss_at=miss_at + g * Wb)            # per query [(slot, k, miss), ...]
            listed += [sum(p[1] for p in row) for row in pairs]
            run += [sum(p[2] for p in row) for row in pairs]
            missing = [(q, slot, m) for q in range(n) for slot, _, m in pairs[q] if m > 0]
            vids = [L._videos[ids[slot]] for _, slot, _ in missing]
            calls = plan_ragged_calls([v[0] for v in vids], [m[2] for m in missing]) if missing else []
            row_of, n_rows = place_calls(calls, [m[2] for m in missing], Nq, n_rows)
            first_job = len(jobs)
            jobs += [missing[i] + (row_of[i],) for idx in calls for i in idx]
            plans.append((pairs, missing, vids, calls, row_of, first_job, len(jobs) - first_job))
        if jobs:
            cand = torch.empty(n_rows, 4, dtype=torch.float32, device=dev)
            job_tab = torch.tensor(jobs, dtype=torch.int32).to(dev)             # the poll's one small upload
        # 5-7. the query half on the missing windows, the scatter, stage C on the cache
        out = self._out
        for i, ((g, chunk), P, (pairs, missing, vids, calls, row_of, job0, n_jobs)) in enumerate(zip(scans, self._plans, plans)):
            n = len(chunk)
            cache = p32(self._cache, g * n_tot * Nq * 4)
            miss_widx, miss_wval = P["miss"][:n * V * K], P["miss"][n * V * K:2 * n * V * K].view(torch.float32)
            for idx in calls:
                L._enqueue_ragged([(vids[i][:2], chunk[missing[i][0]], missing[i][0], missing[i][1]) for i in idx],
                                  [missing[i][2] for i in idx], (g, chunk, miss_widx, miss_wval), V, cand=cand[row_of[idx[0]]:])
            if n_jobs:
                _lib.check(lib.cone_watch_pool_store(_lib.ptr(cand), p32(job_tab, 4 * job0), n_jobs, p32(miss_widx), _lib.ptr(v_ctx_l),
                                                     p32(v_tab), p32(v_tab, V), n, V, K, n_tot, Nq, cache, p32(self._stamp, g * n_tot),
                                                     _lib.stream()))
            out.launch(i, cache, p32(P["seg"], 2 * n * Wb), _lib.ptr(P["seg_cand"]), p32(P["seg"]), p32(P["seg"], n * Wb), n * Wb)
        res = []
        for (pairs, *_), (rows, seg, kept) in zip(plans, out.read()):           # the moments' one read-back
            for q in range(len(kept)):      # a segment is a chosen window here: window t of the pool belongs to the pair that owns ordinal t
                seg_video = [ids[slot] for slot, k, _ in pairs[q] for _ in range(k)]
                res.append(pooled_moments(rows[q], seg[q], kept[q], seg_video))
        self.windows_run, self.windows_listed = run, listed
        return res
