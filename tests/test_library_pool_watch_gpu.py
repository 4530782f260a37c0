"""Standing queries over a library on the GPU.

Kernel level: ``cone_watch_pool_plan`` / ``cone_watch_pool_store`` on dictated inputs (tests/pool_watch_refs.py), every buffer
inside a poisoned, guarded buffer, against the numpy models word for word.

End to end: ``lib.watch_moments(...).poll() == lib.search_moments(...)`` with the same arguments after every kind of change to the
library, ``windows_run ==`` a host mirror's count on the scan's own lists and the budget's own pairs, two read-backs a poll."""
import ctypes as C

import numpy as np
import pytest
import torch

import pool_watch_refs as R
import test_library_budget_gpu as T
from watch_refs import valid_rule

pytestmark = pytest.mark.gpu

POISON = R.POISON
GUARD = 64


def _guarded(n, dtype, fill=None):
    """``n`` elements of ``dtype`` between two guards of 64 words; the inside poisoned too unless ``fill`` (numpy) is given."""
    words = n * (2 if dtype == torch.int64 else 1)
    whole = torch.full((words + 2 * GUARD,), POISON, dtype=torch.int32, device="cuda")
    inner = whole[GUARD:GUARD + words].view(dtype)
    if fill is not None:
        inner.copy_(torch.from_numpy(np.ascontiguousarray(fill).reshape(-1)).cuda().view(dtype))
    return whole, inner


def _guards_hold(whole, inner):
    n = inner.view(torch.int32).numel()
    return bool((whole[:GUARD] == POISON).all()) and bool((whole[GUARD + n:] == POISON).all())


def _words(a):
    return np.ascontiguousarray(a).view(np.int32) if a.dtype != np.int64 else a


# ------------------------------------------------------------------------------------------------ the two kernels
def _plan(d, Nq, stamp=None):
    from cone_amd import _lib
    lib = _lib.load()
    nq, V, K, Wb, n_tot = d["nq"], d["V"], d["K"], d["Wb"], d["n_tot"]
    stamp = d["stamp"] if stamp is None else stamp
    i32, f32 = torch.int32, torch.float32
    ins = [_guarded(nq * V * K, i32, d["widx"]), _guarded(nq * V * K, f32, d["wval"]), _guarded(nq, i32, d["n_pairs"]),
           _guarded(nq * Wb, i32, d["pair_slot"]), _guarded(nq * Wb, i32, d["pair_k"]), _guarded(V, i32, d["v_ctx_l"]),
           _guarded(V, i32, d["v_win0"]), _guarded(V, i32, d["v_cap"]), _guarded(nq * n_tot, i32, stamp)]
    outs = [_guarded(nq * V * K, i32), _guarded(nq * V * K, f32), _guarded(nq * Wb, i32), _guarded(nq + 1, i32),
            _guarded(nq * Wb, torch.int64), _guarded(nq * Wb, i32), _guarded(nq * Wb, i32)]
    p = lambda b: C.c_void_p(b[1].data_ptr())
    rc = lib.cone_watch_pool_plan(*(p(b) for b in ins), nq, V, K, Wb, n_tot, d["W"], Nq, *(p(o) for o in outs), _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.cone_last_error()
    for b in ins + outs:
        assert _guards_hold(*b)
    assert np.array_equal(ins[8][1].cpu().numpy().reshape(stamp.shape), stamp)              # the plan writes no stamp (it is handed
    mw, mv, pm, off, cand, sn, tag = (o[1].cpu().numpy() for o in outs)                     #  no cache at all)
    return mw.reshape(nq, V, K), mv.reshape(nq, V, K), pm.reshape(nq, Wb), off, cand, sn, tag


def _store(d, Nq, cand, jobs, miss_widx, cache, stamp):
    from cone_amd import _lib
    lib = _lib.load()
    nq, V, K, n_tot = d["nq"], d["V"], d["K"], d["n_tot"]
    i32 = torch.int32
    bufs = [_guarded(cand.size, torch.float32, cand), _guarded(jobs.size, i32, jobs), _guarded(miss_widx.size, i32, miss_widx),
            _guarded(V, i32, d["v_ctx_l"]), _guarded(V, i32, d["v_win0"]), _guarded(V, i32, d["v_cap"]),
            _guarded(cache.size, torch.float32, cache), _guarded(stamp.size, i32, stamp)]
    p = lambda b: C.c_void_p(b[1].data_ptr())
    rc = lib.cone_watch_pool_store(p(bufs[0]), p(bufs[1]), len(jobs), *(p(b) for b in bufs[2:6]), nq, V, K, n_tot, Nq, p(bufs[6]),
                                   p(bufs[7]), _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.cone_last_error()
    for b in bufs:
        assert _guards_hold(*b)
    return bufs[6][1].cpu().numpy().reshape(cache.shape), bufs[7][1].cpu().numpy().reshape(stamp.shape)


def _poisoned_cache(nq, n_tot, Nq):
    return np.full((nq, n_tot, Nq, 4), POISON, np.int32).view(np.float32)


NAMES = ("miss_widx", "miss_wval", "pair_miss", "seg_off", "seg_cand", "seg_n", "seg_tag")


@pytest.mark.parametrize("Wb", R.BUDGETS)
def test_plan_and_store_equal_the_models_word_for_word(Wb):
    """Every pattern at this budget (the pair prefix sum's and the compaction's wave edges); K, V, the query count and the slot
    count rotate so that every value meets every budget.  The miss buffers start as poison: the model keeps poison wherever the
    contract names no element, so rows of unchosen slots are compared too.  The store runs on the plan's own lists and a cache of
    poison: rows and stamps it does not name keep their words; a second plan on the stored stamps misses nothing."""
    a, stored = R.BUDGETS.index(Wb), 0
    for b, pattern in enumerate(R.PATTERNS):
        K, V, nq = R.shape_for(a, b)
        Nq = R.SLOTS[(a + b) % 3]
        d = R.dictated(nq, V, K, Wb, pattern)
        V, K = d["V"], d["K"]
        want = R.plan_ref(*R.plan_args(d), Nq)
        got = _plan(d, Nq)
        for name, g, w in zip(NAMES, got, want):
            assert np.array_equal(_words(g).reshape(-1), _words(w).reshape(-1)), (name, pattern, K, V, nq, Nq)
        jobs, n_rows = R.jobs_for(want[2], d["n_pairs"], d["pair_slot"], d["pair_k"], V, K, Nq)
        if not len(jobs):                                                       # (nothing misses: the store refuses n_jobs = 0)
            assert not got[2].any()
            continue
        stored += 1
        cand, cache = R.cand_rows(n_rows), _poisoned_cache(nq, d["n_tot"], Nq)
        want_cache, want_stamp = R.store_ref(cand, jobs, want[0], d["v_ctx_l"], d["v_win0"], d["v_cap"], Nq, cache, d["stamp"])
        got_cache, got_stamp = _store(d, Nq, cand, jobs, got[0], cache, d["stamp"])
        assert np.array_equal(_words(got_cache), _words(want_cache)), (pattern, K, V, nq, Nq)
        assert np.array_equal(got_stamp, want_stamp), (pattern, K, V, nq, Nq)
        again = _plan(d, Nq, stamp=got_stamp)
        assert not again[2].any(), pattern
        for name, g, w in zip(NAMES[3:], again[3:], want[3:]):                  # the segment table does not depend on hit or miss
            assert np.array_equal(g, w), (name, pattern)
    assert stored >= 1


@pytest.mark.parametrize("K,V,nq", [(256, 300, 5), (1, 300, 64), (256, 1, 64), (20, 3, 64)])
def test_the_plan_at_the_largest_shapes(K, V, nq):
    for Wb, pattern, Nq in ((256, "alternating", 10), (255, "hostile", 3), (65, "threshold", 5)):
        d = R.dictated(nq, V, K, Wb, pattern)
        want = R.plan_ref(*R.plan_args(d), Nq)
        got = _plan(d, Nq)
        for name, g, w in zip(NAMES, got, want):
            assert np.array_equal(_words(g).reshape(-1), _words(w).reshape(-1)), (name, pattern)


def test_the_store_clamps_hostile_jobs_and_skips_indices_outside_the_slab():
    Nq = 3
    d = R.dictated(5, 3, 5, 20, "all_missing")
    K, V = d["K"], d["V"]
    miss = np.full((5, V, K), -1, np.int32)
    miss[0, 0], miss[1, 2], miss[2, 1], miss[3, 0], miss[4, 1] = [1, 2, 3, 4, 5], [0, 99, -1, 7, 6], [6, 5, 4, 3, 2], \
        [7, -3, 1 << 30, 0, 1], [2, 3, 4, 5, 6]
    # n_miss below 0, inside (one index past the slab, one negative), above K, a query and a slot outside, a negative first row
    jobs = np.asarray([[0, 0, -3, 0], [1, 2, 4, 0], [3, 0, 9, 4 * Nq], [5, 1, 2, 0], [-1, 1, 2, 0], [2, 3, 2, 0], [2, -1, 2, 0],
                       [2, 1, 2, -Nq], [4, 1, 2, 9 * Nq]], np.int32)
    cand = R.cand_rows(11 * Nq)
    cache, stamp = _poisoned_cache(5, d["n_tot"], Nq), np.full((5, d["n_tot"]), 7, np.int32)
    want = R.store_ref(cand, jobs, miss, d["v_ctx_l"], d["v_win0"], d["v_cap"], Nq, cache, stamp)
    got = _store(d, Nq, cand, jobs, miss, cache, stamp)
    assert np.array_equal(_words(got[0]), _words(want[0])) and np.array_equal(got[1], want[1])
    assert (got[1][0] == 7).all() and (got[1][2] == 7).all() and int((got[1] != 7).sum()) == 2 + 3 + 2
    assert np.array_equal(got[0][4, d["v_win0"][1] + 3], cand[10 * Nq:11 * Nq])
    assert (got[1][4, d["v_win0"][1] + np.asarray([2, 3])] == d["v_ctx_l"][1]).all()


def test_the_store_stops_at_the_end_of_the_axis_when_a_slab_overhangs_it():
    """Slot 1 owns windows [4, 8) of an axis of 6: windows 1, 2, 3 of the slab are inside ``v_cap`` and only window 1 (axis
    entry 5) is inside the axis.  The axis bound is the one predicate the one-video store does not have."""
    Nq, K = 3, 3
    d = dict(nq=1, V=2, K=K, n_tot=6, v_ctx_l=np.asarray([100, 200], np.int32), v_win0=np.asarray([0, 4], np.int32),
             v_cap=np.asarray([4, 4], np.int32))
    miss = np.full((1, 2, K), -1, np.int32)
    miss[0, 1] = [1, 2, 3]
    jobs = np.asarray([[0, 1, 3, 0]], np.int32)
    cand = R.cand_rows(3 * Nq)
    cache, stamp = _poisoned_cache(1, 6, Nq), np.full((1, 6), 7, np.int32)
    want = R.store_ref(cand, jobs, miss, d["v_ctx_l"], d["v_win0"], d["v_cap"], Nq, cache, stamp)
    got = _store(d, Nq, cand, jobs, miss, cache, stamp)                          # (checks the guards around every buffer)
    assert np.array_equal(_words(got[0]), _words(want[0])) and np.array_equal(got[1], want[1])
    assert got[1].tolist() == [[7, 7, 7, 7, 7, 200]]
    assert np.array_equal(got[0][0, 5], cand[:Nq]) and (_words(got[0][0, :5]) == POISON).all()


# ------------------------------------------------------------------------------------------------ end to end
class _Mirror:
    """The host's mirror of a library watcher's stamps: per (query, video id) the clip count each window was run at.  ``poll``
    reads the scan's own lists and the budget's own pairs and says, per query, how many windows are chosen and how many of them
    must run -- and, per video, how many of those had been run before.  (A change to one video moves the budget: windows of
    OTHER videos that were never chosen before may enter it and run for the first time; what a change to video X must not cause
    is a second run of a cached window of another video.)"""

    def __init__(self, lib, queries, n_windows, videos=None):
        self.lib, self.queries, self.W, self.videos = lib, queries, n_windows, videos
        self.stamp = {}

    def reset(self, vid):
        self.stamp = {k: v for k, v in self.stamp.items() if k[1] != vid}

    def poll(self):
        lib, Wv, Wb = self.lib, int(self.lib._loc.args.max_v_l), self.W
        subset, ids = lib._search_ids(self.videos)
        table = lib._table(subset, ids)
        ids, V = table[0], len(table[0])
        run, listed, by_video = [], [], {}
        for g in range(0, len(self.queries), 64):
            chunk = self.queries[g:g + 64]
            n = len(chunk)
            widx, wval, _ = lib._scan(table, chunk, 1)
            words = lib._budget((g, chunk, widx, wval), V, Wb).cpu()
            widx = widx.cpu().view(n, V, -1)
            n_pairs, slots, counts = words[:n].tolist(), words[n:n + n * Wb].view(n, Wb).tolist(), \
                words[n + n * Wb:n + 2 * n * Wb].view(n, Wb).tolist()
            for q in range(n):
                n_run = n_listed = 0
                for i in range(n_pairs[q]):
                    vid, k = ids[slots[q][i]], counts[q][i]
                    ctx_l = lib._videos[vid][1]
                    for wi in widx[q, slots[q][i], :k].tolist():
                        n_listed += 1
                        seen = self.stamp.get((g + q, vid, wi), 0)
                        if not valid_rule(wi, seen, ctx_l, Wv):
                            self.stamp[(g + q, vid, wi)] = ctx_l
                            n_run += 1
                            if seen:                                            # run before, and run AGAIN now
                                by_video[vid] = by_video.get(vid, 0) + 1
                run.append(n_run)
                listed.append(n_listed)
        return run, listed, by_video


def _check(w, mirror, lib, queries, n_windows, monkeypatch, tag, n_moments=5, videos=None):
    want_run, want_listed, by_video = mirror.poll()
    calls = T._count_readbacks(monkeypatch)
    got = w.poll()
    n_calls = len(calls)
    monkeypatch.undo()
    assert n_calls == 2, tag
    assert w.windows_run == want_run and w.windows_listed == want_listed, (tag, w.windows_run, want_run)
    want = lib.search_moments(queries, n_windows, n_moments, videos)
    assert all(len(m) >= 1 for m in want), tag
    assert got == want, tag
    return want_run, by_video


CLIPS = (1, 40, 200, 900)


@pytest.mark.parametrize("n_windows", (1, 20))
@pytest.mark.parametrize("n_queries", (1, 5, 65))
def test_poll_is_search_moments_after_every_kind_of_change(n_queries, n_windows, monkeypatch):
    loc = T._localizer()
    S = int(loc.args.max_v_l) // 2
    Nq = int(loc.args.num_queries)
    queries = T._queries(T._mixed_lens(n_queries), seed=31)
    more = T._video(600, seed=41)
    with loc.open_library(2400) as lib:
        ids = lib.add_many([T._video(n, seed=30 + i) for i, n in enumerate(CLIPS)])
        with lib.watch_moments(queries, n_windows=n_windows, n_moments=5) as w:
            check = lambda tag: _check(w, mirror, lib, queries, n_windows, monkeypatch, tag)
            mirror = _Mirror(lib, queries, n_windows)
            assert w.windows_run == [0] * n_queries and w.nbytes == n_queries * w._axis.capacity * (Nq * 16 + 4)
            assert w._axis.capacity == sum(w._cap(n) for n in (2, 2, 6, 21))
            cold, _ = check("cold")
            assert cold == w.windows_listed and all(1 <= c <= n_windows for c in cold)      # every chosen window runs once
            # nothing changed: no window runs and the query half is not called at all
            half = []
            real = lib._enqueue_ragged
            monkeypatch.setattr(lib, "_enqueue_ragged", lambda *a, **k: (half.append(1), real(*a, **k))[1])
            again = w.poll()
            monkeypatch.undo()
            assert not half and w.windows_run == [0] * n_queries and again == lib.search_moments(queries, n_windows, 5)
            assert mirror.poll()[0] == [0] * n_queries
            # extend of the last video by 8 clips, in place: only its windows can run
            row0, at = lib._videos[ids[3]][0], 0
            lib.extend(ids[3], more[at:at + 8])
            at += 8
            assert lib._videos[ids[3]][0] == row0
            # (a video that never grew keeps every cached window valid: only videos extended so far can have a window run twice)
            ran, by_video = check("extend in place")
            assert set(by_video) <= {ids[3]} and sum(by_video.values()) <= 3 * n_queries
            # an extend that relocates (the rows behind video 1 belong to video 2)
            row0 = lib._videos[ids[1]][0]
            lib.extend(ids[1], more[at:at + 8])
            at += 8
            assert lib._videos[ids[1]][0] != row0
            ran, by_video = check("relocating extend")
            assert set(by_video) <= {ids[1], ids[3]}
            # an extend that makes a video outgrow its slab: 200 -> 380 clips, 6 -> 10 windows in a slab of 8
            slab, planes = w._slabs[ids[2]], w.nbytes
            lib.extend(ids[2], more[at:at + 180])
            at += 180
            ran, by_video = check("outgrown slab")
            assert w._slabs[ids[2]] != slab and w._slabs[ids[2]][1] == w._cap(10) and w.nbytes > planes and set(by_video) <= set(ids[1:])
            assert check("after the move")[0] == [0] * n_queries
            # a trim: that video's windows run again, no other's
            lib.trim(ids[3], S + 7)
            mirror.reset(ids[3])
            before = w._stamp.clone()
            ran, by_video = check("trim")
            assert set(by_video) <= set(ids[1:3])                               # (the mirror has forgotten the trimmed video)
            lost = (before != 0) & (w._stamp == 0)                              # only the trimmed video's slab was zeroed
            win0, cap = w._slabs[ids[3]]
            lost[:, win0:win0 + cap] = False
            assert not lost.any()
            if n_windows == 20:
                assert sum(ran) > 0                                             # (the long video holds some of the 20 best windows)
            # add / remove / compact / resize
            fifth = lib.add(T._video(120, seed=45))
            ran, by_video = check("add")
            assert not by_video and fifth in w._slabs
            lib.remove(ids[0])
            freed = w._slabs[ids[0]]
            assert not check("remove")[1]                                       # (windows never chosen before may take its place)
            assert ids[0] not in w._slabs and not w._stamp[:, freed[0]:freed[0] + freed[1]].any()
            assert lib.compact() > 0
            assert check("compact")[0] == [0] * n_queries
            lib.resize(3000)
            assert check("resize")[0] == [0] * n_queries
            lib.extend(ids[3], more[at:at + 8])
            ran, by_video = check("extend after it all")
            assert set(by_video) <= set(ids[1:])
            assert w.nbytes == n_queries * w._axis.capacity * (Nq * 16 + 4)


def test_an_explicit_video_list_a_one_video_watcher_and_lifetime(monkeypatch):
    loc = T._localizer()
    queries = T._queries(T._mixed_lens(3), seed=32)
    feats = [T._video(n, seed=50 + i) for i, n in enumerate((300, 150, 500))]
    with loc.open_library(1500) as lib:
        ids = lib.add_many(feats)
        # one video: the answer is predict_moment at topk_window = the video's share, as search_moments' is
        for i, W in ((0, 5), (1, 20)):
            k = min(W, lib._videos[ids[i]][2])
            with lib.watch_moments(queries[:1], n_windows=W, videos=[ids[i]]) as w1:
                got = w1.poll()[0]
                want = T._localizer(topk_window=k).predict_moment(feats[i], queries[0])
                assert [v for v, _ in got] == [ids[i]] * len(got) and [m for _, m in got] == want and len(want) >= 1
                assert w1.windows_run == [k] and w1.windows_listed == [k]
        sub = [ids[2], ids[0]]
        w = lib.watch_moments(queries, n_windows=7, n_moments=3, videos=sub)
        mirror = _Mirror(lib, queries, 7, videos=sub)
        _check(w, mirror, lib, queries, 7, monkeypatch, "subset cold", n_moments=3, videos=sub)
        assert set(w._slabs) == set(sub)
        lib.extend(ids[1], T._video(20, seed=60))                               # not watched: nothing runs
        ran, _ = _check(w, mirror, lib, queries, 7, monkeypatch, "unwatched extend", n_moments=3, videos=sub)
        assert ran == [0] * 3
        lib.extend(ids[0], T._video(20, seed=61))
        _, by_video = _check(w, mirror, lib, queries, 7, monkeypatch, "watched extend", n_moments=3, videos=sub)
        assert set(by_video) <= {ids[0]}
        w2 = lib.watch_moments(queries[:1])
        w2.close()
        with pytest.raises(RuntimeError, match="the watcher is closed"):
            w2.poll()
        lib.remove(ids[0])
        with pytest.raises(ValueError, match="unknown or removed video id"):
            w.poll()
        with pytest.raises(ValueError, match="unknown or removed video id"):
            lib.search_moments(queries, 7, 3, sub)
        w3 = lib.watch_moments(queries)
        lib.remove(ids[1])
        lib.remove(ids[2])
        assert w3.poll() == [[], [], []] == lib.search_moments(queries) and w3.windows_run == [0, 0, 0]
    with pytest.raises(RuntimeError, match="the library is closed"):
        w3.poll()
