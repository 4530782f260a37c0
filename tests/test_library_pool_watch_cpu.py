"""Standing queries over a library, the part that needs no GPU: the numpy models against plain loops, the segment table against
the pool a search lays out, the slab allocator of a ``LibraryWatcher``, the refusals the two new entries make on the host before
any pointer is read, and ``watch_moments``' refusals before any GPU work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pool_watch_refs as R
from watch_refs import valid_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ header and binding
def test_header_binding_and_library_agree_on_the_pool_entries():
    from cone_amd import _lib, build
    with open(os.path.join(ROOT, "include", "cone_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"#define\s+CONE_HIP_ABI_VERSION\s+8\b", hdr)
    declared = set(re.findall(r"\b(cone_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in R.NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert declared == set(_lib.EXPORTS)
    at = hdr.index("standing queries over a library")
    assert hdr.index("standing queries (additive in ABI 8)") < at < hdr.index("metrics on the device")
    section = hdr[at:hdr.index("metrics on the device")]
    for name in R.NEW_SYMBOLS:
        assert name + "(" in section
    for word in ("POOL ORDER", "PRECONDITION", "distinct", "every element named here written", "DENSE", "clamped, never trusted",
                 "16-B aligned", "one writer"):
        assert word in section, word
    for name, n in R.N_ARGS.items():
        assert len(_lib._SIGNATURES[name][1]) == n, name
        decl = re.search(r"\b%s\(([^;]*)\);" % name, hdr).group(1)
        assert decl.count(",") + 1 == n, name
    assert "library_watch_pool.hip" in build.SOURCES
    with open(os.path.join(ROOT, "cone_amd", "csrc", "library_watch_pool.hip")) as f:
        src = f.read()
    assert "asm" not in src and "atomic" not in src.replace("no atomics", "")


# ------------------------------------------------------------------------------------------------ the models against plain loops
def _plain_plan(d, Nq):
    """The contract once more, as one flat walk over (query, pair, list position) with nothing shared with ``plan_ref``."""
    nq, V, K, Wb, n_tot, W = d["nq"], d["V"], d["K"], d["Wb"], d["n_tot"], d["W"]
    misses, segs, counts = {}, {}, np.zeros((nq, Wb), np.int32)
    for q in range(nq):
        t = 0
        n = d["n_pairs"][q]
        n = 0 if n < 0 else Wb if n > Wb else n
        for i in range(n):
            s, k = int(d["pair_slot"][q, i]), int(d["pair_k"][q, i])
            k = 0 if k < 0 else K if k > K else k
            if s < 0 or s >= V:
                continue
            for j in range(k):
                if t >= Wb:
                    break
                wi = int(d["widx"][q, s, j])
                seg = (0, 0, s)
                if 0 <= wi < d["v_cap"][s] and d["v_win0"][s] >= 0 and d["v_win0"][s] + wi < n_tot:
                    at = int(d["v_win0"][s]) + wi
                    seg = ((q * n_tot + at) * Nq, Nq, s)
                    e = (wi - 1) * (W // 2) + W
                    st = int(d["stamp"][q, at])
                    if not (st == d["v_ctx_l"][s] or (st > 0 and e <= st)):
                        misses.setdefault((q, s), []).append((wi, d["wval"][q, s, j]))
                        counts[q, i] += 1
                misses.setdefault((q, s), [])
                segs[q * Wb + t] = seg
                t += 1
    return misses, segs, counts


@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_the_models_equal_a_plain_loop_and_a_store_then_plan_misses_nothing(pattern):
    for a, Wb in enumerate(R.BUDGETS):
        K, V, nq = R.shape_for(a, R.PATTERNS.index(pattern))
        nq, V, K = min(nq, 5), min(V, 12), min(K, 70)                # (the GPU tests run the large shapes; the loops here are Python)
        Nq = R.SLOTS[a % 3]
        d = R.dictated(nq, V, K, Wb, pattern)
        nq, V, K = d["nq"], d["V"], d["K"]
        mw, mv, pm, off, sc, sn, tag = R.plan_ref(*R.plan_args(d), Nq)
        misses, segs, counts = _plain_plan(d, Nq)
        assert np.array_equal(pm, counts) and off.tolist() == [q * Wb for q in range(nq + 1)]
        for s in range(nq * Wb):
            assert (int(sc[s]), int(sn[s]), int(tag[s])) == segs.get(s, (0, 0, 0)), (Wb, s)
        for q in range(nq):
            for s in range(V):
                if (q, s) not in misses:
                    assert (mw[q, s] == R.POISON).all() and (mv[q, s].view(np.int32) == R.POISON).all()     # an unchosen slot's row
                    continue
                got = mw[q, s][mw[q, s] != R.POISON]
                n = len(misses[(q, s)])
                assert got[:n].tolist() == [m[0] for m in misses[(q, s)]] and (got[n:] == -1).all()
                assert mv[q, s, :n].tolist() == [m[1] for m in misses[(q, s)]] and np.isneginf(mv[q, s, n:len(got)]).all()
        # the store on the plan's lists, then the plan again: nothing is missing, the segment table is the same
        jobs, n_rows = R.jobs_for(pm, d["n_pairs"], d["pair_slot"], d["pair_k"], V, K, Nq)
        assert n_rows == int(pm.sum()) * Nq
        cache = np.zeros((nq, d["n_tot"], Nq, 4), np.float32)
        cache2, stamp2 = R.store_ref(R.cand_rows(n_rows), jobs, mw, d["v_ctx_l"], d["v_win0"], d["v_cap"], Nq, cache, d["stamp"])
        assert int((stamp2 != d["stamp"]).sum()) == int(pm.sum())
        again = R.plan_ref(*R.plan_args(dict(d, stamp=stamp2)), Nq)
        assert not again[2].any() and all(np.array_equal(x, y) for x, y in zip(again[3:], (off, sc, sn, tag)))
        # every stored window holds the rows of its own job, in list order
        rows = R.cand_rows(n_rows)
        for q, s, n, first in jobs.tolist():
            for m in range(n):
                at = int(d["v_win0"][s]) + int(mw[q, s, m])
                assert np.array_equal(cache2[q, at], rows[first + m * Nq:first + (m + 1) * Nq])


def test_the_patterns_hold_what_they_name():
    Nq = 5
    for Wb in R.BUDGETS:
        plan = lambda d: R.plan_ref(*R.plan_args(d), Nq)
        d = R.dictated(5, 3, 20, Wb, "all_valid")
        assert not plan(d)[2].any()
        d = R.dictated(5, 3, 20, Wb, "all_missing")
        assert plan(d)[2].sum(axis=1).tolist() == d["pair_k"].sum(axis=1).tolist() == [min(Wb, 60)] * 5
        d = R.dictated(5, 3, 20, Wb, "alternating")
        assert plan(d)[2].sum(axis=1).tolist() == [min(Wb, 60) // 2] * 5
        d = R.dictated(5, 3, 20, Wb, "one_pair_all")
        assert d["n_pairs"].tolist() == [1] * 5 and (d["pair_k"][:, 0] == Wb).all()
        d = R.dictated(5, 3, 20, Wb, "pairs_of_one")
        assert d["n_pairs"].tolist() == [Wb] * 5 and (d["pair_k"] == 1).all()
        d = R.dictated(5, 3, 20, Wb, "pair_seam")
        ends = np.cumsum(d["pair_k"][0, :d["n_pairs"][0]]).tolist()
        assert [e for e in (63, 64, 65, 127, 128) if e <= Wb] == [e for e in ends if e in (63, 64, 65, 127, 128)]
        d = R.dictated(5, 3, 20, Wb, "threshold")
        pm = plan(d)[2]
        assert pm.sum() == sum(t % 2 for q in range(5) for t in range(int(d["pair_k"][q].sum())))      # the odd ordinals, all of them
        d = R.dictated(5, 3, 20, Wb, "short_budget")
        assert d["n_pairs"][0] == 0 and d["n_pairs"][3] == 0 and (d["pair_k"].sum(axis=1) < Wb).all()
        assert Wb < 2 or d["n_pairs"].any()
        d = R.dictated(5, 3, 20, Wb, "hostile")
        assert d["n_pairs"][0] > Wb and d["n_pairs"][1] < 0 and (d["pair_k"] > 20).any() and (d["pair_k"] < 0).any()
        assert (d["pair_slot"] >= 3).any() or Wb < 2
        d = R.dictated(5, 3, 20, Wb, "out_of_slab")
        chosen_bad = [int(d["widx"][q, s, j]) for q in range(5) for _, s, _, n in R.chosen(d["n_pairs"], d["pair_slot"], d["pair_k"], q, 3, 20)
                      for j in range(n) if not 0 <= d["widx"][q, s, j] < d["v_cap"][s]]
        assert any(w < 0 for w in chosen_bad) and (Wb < 3 or any(w > 0 for w in chosen_bad))
        assert (plan(d)[5].reshape(5, Wb).sum(axis=1) < d["pair_k"].sum(axis=1) * Nq).all()
    # the same window and the same stamp, valid in one slot and missing in the other: only the videos' clip counts differ
    d = R.dictated(1, 2, 20, 64, "per_video_ctx")
    wi = int(d["n_win"][0]) - 1
    assert d["n_win"][0] == d["n_win"][1] and d["v_ctx_l"][0] != d["v_ctx_l"][1]
    st = [int(d["stamp"][0, d["v_win0"][s] + wi]) for s in (0, 1)]
    assert st[0] == st[1]
    assert not valid_rule(wi, st[0], int(d["v_ctx_l"][0]), d["W"]) and valid_rule(wi, st[1], int(d["v_ctx_l"][1]), d["W"])
    pm = R.plan_ref(*R.plan_args(d), Nq)[2]
    assert pm[0, list(d["pair_slot"][0]).index(0)] > 0 and pm[0, list(d["pair_slot"][0]).index(1)] == 0


@pytest.mark.parametrize("pattern", ("alternating", "pair_seam", "out_of_slab", "short_budget"))
def test_the_segment_table_over_a_cache_is_the_pool_a_search_lays_out(pattern):
    """``search_moments`` lays a query's pool pair by pair in the budget's order, each pair's windows in list order, ``Nq`` rows a
    window.  The watcher's table over a cache whose every row names its own (query, slot, window, row) gathers the same rows in
    the same order (windows outside their slab contribute nothing on either side)."""
    Nq, Wb = 3, 65
    d = R.dictated(4, 9, 20, Wb, pattern)
    nq, V, K, n_tot = d["nq"], d["V"], d["K"], d["n_tot"]
    cache = np.full((nq, n_tot, Nq, 4), -1.0, np.float32)
    for q in range(nq):
        for s in range(V):
            for wi in range(int(d["v_cap"][s])):
                for r in range(Nq):
                    cache[q, d["v_win0"][s] + wi, r] = (q, s, wi, r)
    _, _, _, off, sc, sn, tag = R.plan_ref(*R.plan_args(d), Nq)
    flat = cache.reshape(-1, 4)
    for q in range(nq):
        direct, tags = [], []
        for i in range(int(d["n_pairs"][q])):
            s = int(d["pair_slot"][q, i])
            for j in range(int(d["pair_k"][q, i])):
                wi = int(d["widx"][q, s, j])
                if 0 <= wi < d["v_cap"][s]:
                    direct += [(q, s, wi, r) for r in range(Nq)]
                    tags += [s] * Nq
        got = [tuple(int(x) for x in row) for s in range(off[q], off[q + 1]) for row in flat[sc[s]:sc[s] + sn[s]]]
        got_tags = [int(tag[s]) for s in range(off[q], off[q + 1]) for _ in range(sn[s])]
        assert got == direct and got_tags == tags, q
        assert direct or d["n_pairs"][q] == 0


# ------------------------------------------------------------------------------------------------ host refusals
# (nq, V, K, Wb, n_win_total, W, Nq) -> the message; the first that applies, in the header's order
PLAN_REFUSALS = [
    ((0, 3, 20, 20, 100, 90, 5), "nq=0 not in [1, 64]"),
    ((65, 0, 0, 0, 0, 0, 0), "nq=65 not in [1, 64]"),
    ((1, 0, 0, 0, 0, 0, 0), "V=0 < 1"),
    ((1, 3, 0, 0, 0, 0, 0), "K=0 not in [1, 256]"),
    ((1, 3, 257, 0, 0, 0, 0), "K=257 not in [1, 256]"),
    ((1, 3, 20, 0, 0, 0, 0), "Wb=0 not in [1, 256]"),
    ((1, 3, 20, 257, 0, 0, 0), "Wb=257 not in [1, 256]"),
    ((1, 3, 20, 20, 0, 0, 0), "Nq=0 not in [1, 16]"),
    ((1, 3, 20, 20, 0, 0, 17), "Nq=17 not in [1, 16]"),
    ((1, 3, 20, 20, 0, 0, 5), "n_win_total=0 < 1"),
    ((1, 3, 20, 20, 100, 1, 5), "W=1 < 2"),
    ((64, 300, 256, 256, 1, 2, 16), "null argument"),
]


@pytest.mark.parametrize("case", range(len(PLAN_REFUSALS)))
def test_the_plan_refuses_by_name_with_every_device_pointer_null(case):
    from cone_amd import _lib
    lib = _lib.load()
    (nq, V, K, Wb, n_tot, W, Nq), want = PLAN_REFUSALS[case]
    rc = lib.cone_watch_pool_plan(*[None] * 9, nq, V, K, Wb, n_tot, W, Nq, *[None] * 8)
    msg = lib.cone_last_error().decode()
    assert rc == -1 and msg == "watch_pool_plan: " + want, msg


# (nq, V, K, n_win_total, Nq, n_jobs)
STORE_REFUSALS = [
    ((0, 3, 20, 100, 5, 1), "nq=0 not in [1, 64]"),
    ((65, 0, 0, 0, 0, 0), "nq=65 not in [1, 64]"),
    ((1, 0, 0, 0, 0, 0), "V=0 < 1"),
    ((1, 3, 0, 0, 0, 0), "K=0 not in [1, 256]"),
    ((1, 3, 257, 0, 0, 0), "K=257 not in [1, 256]"),
    ((1, 3, 20, 0, 0, 0), "Nq=0 not in [1, 16]"),
    ((1, 3, 20, 0, 17, 0), "Nq=17 not in [1, 16]"),
    ((1, 3, 20, 0, 5, 0), "n_win_total=0 < 1"),
    ((1, 3, 20, 100, 5, 0), "n_jobs=0 < 1"),
    ((64, 300, 256, 1, 16, 1), "null argument"),
]


@pytest.mark.parametrize("case", range(len(STORE_REFUSALS)))
def test_the_store_refuses_by_name_with_every_device_pointer_null(case):
    from cone_amd import _lib
    lib = _lib.load()
    (nq, V, K, n_tot, Nq, n_jobs), want = STORE_REFUSALS[case]
    rc = lib.cone_watch_pool_store(None, None, n_jobs, None, None, None, None, nq, V, K, n_tot, Nq, None, None, None)
    msg = lib.cone_last_error().decode()
    assert rc == -1 and msg == "watch_pool_store: " + want, msg


def test_both_entries_miss_each_pointer_by_name_and_the_store_wants_aligned_rows():
    from cone_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x10000)
    for missing in range(16):
        p = [None if i == missing else fake for i in range(16)]
        rc = lib.cone_watch_pool_plan(*p[:9], 4, 3, 20, 20, 100, 90, 5, *p[9:], None)
        assert rc == -1 and lib.cone_last_error().decode() == "watch_pool_plan: null argument", missing
    for missing in range(8):
        p = [None if i == missing else fake for i in range(8)]
        rc = lib.cone_watch_pool_store(p[0], p[1], 2, *p[2:6], 4, 3, 20, 100, 5, p[6], p[7], None)
        assert rc == -1 and lib.cone_last_error().decode() == "watch_pool_store: null argument", missing
    for cand, cache in ((0x10008, 0x10000), (0x10000, 0x10004)):
        rc = lib.cone_watch_pool_store(ctypes.c_void_p(cand), fake, 2, fake, fake, fake, fake, 4, 3, 20, 100, 5, ctypes.c_void_p(cache),
                                       fake, None)
        assert rc == -1 and lib.cone_last_error().decode() == "watch_pool_store: cand and cache must be 16-B aligned"


# ------------------------------------------------------------------------------------------------ the slab allocator
def test_row_ranges_grow_adds_one_hole_behind_and_coalesces():
    from cone_amd.library import RowRanges
    r = RowRanges(10)
    assert r.take(10) == 0
    r.grow(15)
    assert r.capacity == 15 and r.holes == [(10, 5)]
    r.release(7, 3)
    r.grow(20)
    assert r.holes == [(7, 13)] and r.free == 13
    with pytest.raises(ValueError, match="grow: capacity=20 is not above"):
        r.grow(20)


class _Lib:
    """What ``LibraryWatcher._sync`` reads of a library: ``_videos`` = id -> (row0, ctx_l, K)."""

    def __init__(self, videos):
        self._videos = dict(videos)


def _bare_watcher(videos, nq=2, Nq=3, W=90):
    from cone_amd import library, watch
    w = object.__new__(watch.LibraryWatcher)
    w._lib, w._nq, w._Nq, w._W = _Lib(videos), nq, Nq, W
    n_tot = max(sum(w._cap(R.num_windows(v[1], W)) for v in videos.values()), 1)
    w._axis, w._slabs, w._stale = library.RowRanges(n_tot), {}, set()
    w._cache = torch.zeros(nq, n_tot, Nq, 4)
    w._stamp = torch.zeros(nq, n_tot, dtype=torch.int32)
    return w


def _fill(w, vid, value):
    win0, cap = w._slabs[vid]
    w._cache[:, win0:win0 + cap] = float(value)
    w._stamp[:, win0:win0 + cap] = int(value)


def test_slabs_join_outgrow_move_release_and_reuse_with_zeroed_stamps():
    S = 45
    videos = {1: (0, 40, 2), 2: (40, 900, 20), 3: (940, 200, 6)}               # 2, 21 and 6 windows
    w = _bare_watcher(videos)
    assert [w._cap(n) for n in (1, 2, 6, 21)] == [2, 3, 8, 27]
    w._sync([1, 2, 3])
    assert w._slabs == {1: (0, 3), 2: (3, 27), 3: (30, 8)} and w._axis.free == 0 and w._axis.capacity == 38
    for v in (1, 2, 3):
        _fill(w, v, v)
    # growing inside the headroom changes nothing; a trim zeroes that video's stamps only
    w._lib._videos[3] = (940, 200 + 2 * S, 8)                                   # 8 windows: the slab's last
    w._trimmed(2)
    w._sync([1, 2, 3])
    assert w._slabs[3] == (30, 8) and not w._stamp[:, 3:30].any() and not w._stale
    assert (w._stamp[:, :3] == 1).all() and (w._stamp[:, 30:38] == 3).all() and (w._cache[:, 3:30] == 2).all()
    # outgrowing: no range fits, the axis grows by a quarter (at least by the slab) and the planes and stamps move
    w._lib._videos[3] = (940, 200 + 3 * S, 8)                                   # 9 windows
    w._sync([1, 2, 3])
    assert w._axis.capacity == 38 + 12 and w._slabs[3] == (38, 12) and w._cache.shape[1] == 50
    assert (w._stamp[:, 38:46] == 3).all() and (w._cache[:, 38:46] == 3).all() and not w._stamp[:, 46:].any()
    assert not w._stamp[:, 30:38].any() and w._axis.holes == [(30, 8)]          # the old slab: zeroed, free
    assert (w._stamp[:, :3] == 1).all() and (w._cache[:, 3:30] == 2).all()
    # a video that joins takes the first hole that fits; one that left frees its slab, stamps zeroed
    w._lib._videos[4] = (1200, 3 * S, 4)                                        # 4 windows + 1
    w._sync([1, 2, 3, 4])
    assert w._slabs[4] == (30, 5) and w._axis.holes == [(35, 3)]
    del w._lib._videos[1]
    w._sync([2, 3, 4])
    assert 1 not in w._slabs and not w._stamp[:, :3].any() and w._axis.holes == [(0, 3), (35, 3)]
    w._lib._videos[5] = (0, 40, 2)
    w._sync([2, 3, 4, 5])
    assert w._slabs[5] == (0, 3) and not w._stamp[:, :3].any()                  # reused, and clean
    assert w._cache.numel() * 4 + w._stamp.numel() * 4 == 2 * 50 * (3 * 16 + 4)


# ------------------------------------------------------------------------------------------------ the wrapper
def _bare_library(videos, flags=0, num_queries=5, topk_window=20):
    from cone_amd.library import VideoLibrary
    lib = object.__new__(VideoLibrary)         # no handle, no arena, no GPU: the refusals come first
    lib.max_q_l = 20
    lib._videos = dict(videos)
    lib._flags = flags
    lib._open = False
    lib._loc = type("Loc", (), {"args": type("Args", (), {"topk_window": topk_window, "num_queries": num_queries, "max_v_l": 90})()})()
    return lib


def _q(n):
    return (torch.zeros(n, 768), torch.zeros(256))


def test_watch_moments_refuses_before_any_gpu_work(monkeypatch):
    from cone_amd import _lib, library, watch
    assert hasattr(library.VideoLibrary, "watch_moments")
    monkeypatch.setattr(watch.LibraryWatcher, "__init__", lambda *a: pytest.fail("a watcher was built"))
    lib = _bare_library({1: (0, 900, 20), 2: (900, 90, 3)})
    with pytest.raises(ValueError, match="watch_moments: an empty query list"):
        lib.watch_moments([], n_windows=0)
    with pytest.raises(ValueError, match="query has 21 tokens > max_q_l=20"):
        lib.watch_moments([_q(5), _q(21)], n_windows=0)
    for bad in (0, 257, -1):
        with pytest.raises(ValueError, match=r"n_windows=%d not in \[1, 256\]" % bad):
            lib.watch_moments([_q(5)], n_windows=bad, n_moments=0)
    with pytest.raises(ValueError, match="n_windows must be an integer"):
        lib.watch_moments([_q(5)], n_windows=2.5)
    with pytest.raises(ValueError, match="n_moments must be an integer, got None"):
        lib.watch_moments([_q(5)], n_moments=None, videos=[7])
    for bad in (0, 101):
        with pytest.raises(ValueError, match=r"n_moments=%d not in \[1, 100\]" % bad):
            lib.watch_moments([_q(5)], n_windows=205, n_moments=bad)
    with pytest.raises(ValueError, match=r"n_windows=205 x num_queries=5 = 1025 candidates > 1024 in one pool"):
        lib.watch_moments([_q(5)], n_windows=205, videos=[7])
    with pytest.raises(ValueError, match=r"n_windows=103 x num_queries=10 = 1030 candidates > 1024 in one pool"):
        _bare_library({1: (0, 900, 20)}, num_queries=10).watch_moments([_q(5)], n_windows=103)
    with pytest.raises(ValueError, match="unknown or removed video id 7"):
        lib.watch_moments([_q(5)], videos=[1, 7])
    with pytest.raises(ValueError, match="video id 2 is listed more than once"):
        lib.watch_moments([_q(5)], videos=[2, 1, 2])
    with pytest.raises(RuntimeError, match="the library is closed"):
        lib.watch_moments([_q(5)])
    monkeypatch.setattr(library.VideoLibrary, "_check_live", lambda self: None)
    with pytest.raises(_lib.ConeHipError, match="^watch_moments: CONE_SESSION_BF16 libraries are not supported"):
        _bare_library({1: (0, 900, 20)}, flags=_lib.SESSION_BF16).watch_moments([_q(5)])


def test_a_trim_reaches_a_library_watcher_and_launches_nothing():
    import weakref
    from cone_amd import library, watch
    lib = _bare_library({1: (0, 900, 20), 2: (900, 300, 8)})
    lib._rows = library.RowRanges(1200)
    lib._rows.take(1200)
    lib._scan_cache = None
    w = object.__new__(watch.LibraryWatcher)
    w._stale = set()
    lib._watchers = weakref.WeakSet([w])
    assert lib.trim(1, 0) == 900 and not w._stale                               # n_front == 0 changes nothing
    assert lib.trim(2, 45) == 255 and w._stale == {2}


def test_a_closed_library_watcher_raises_and_holds_nothing():
    from cone_amd import watch
    w = object.__new__(watch.LibraryWatcher)
    w._open = True
    w.close()
    assert w.nbytes == 0
    with pytest.raises(RuntimeError, match="the watcher is closed"):
        w.poll()


def test_search_moments_and_the_watcher_share_the_helper_that_names_a_segments_video():
    from cone_amd import library
    rows = [[1.0, 2.0, .5, .25, .75], [3.0, 4.0, .1, .2, .3], [0.0] * 5]
    assert library.pooled_moments(rows, [2, 0, -1], 2, [11, 12, 13]) == [(13, [1.0, 2.0, .75]), (11, [3.0, 4.0, .3])]
    import inspect
    assert "pooled_moments(" in inspect.getsource(library.VideoLibrary.search_moments)
    from cone_amd import watch
    assert "pooled_moments(" in inspect.getsource(watch.LibraryWatcher.poll)


# ------------------------------------------------------------------------------------------------ the shared host helpers
def _bits(x):
    return int(np.asarray(x, np.float32).view(np.int32))


@pytest.mark.parametrize("W", (1, 3))
@pytest.mark.parametrize("tail", (False, True))
def test_the_budget_decoder_against_a_plain_loop_over_hand_written_words(W, tail):
    """Two chunks of 2 and 3 queries; per query ``n_pairs`` runs 0, W, 1, 0, W (clamped to W); the slots, counts, score bits and
    miss counts of every (query, column) are distinct, so a word taken from the wrong place shows."""
    from cone_amd.library import decode_budget
    nqs, n_pairs = (2, 3), [[0, W], [1, 0, W]]
    scores = [[[0.5 - 0.01 * (10 * q + i) - c for i in range(W)] for q in range(nq)] for c, nq in enumerate(nqs)]
    words = []
    for c, nq in enumerate(nqs):
        words += n_pairs[c]
        words += [100 * c + 10 * q + i for q in range(nq) for i in range(W)]                   # pair_slot
        words += [1000 + 100 * c + 10 * q + i for q in range(nq) for i in range(W)]            # pair_k
        words += [_bits(scores[c][q][i]) for q in range(nq) for i in range(W)]                 # pair_best
    miss_at = len(words)
    if tail:
        words += [5000 + 10 * g + i for g in range(sum(nqs)) for i in range(W)]                # pair_miss of ALL queries
    at = g = 0
    for c, nq in enumerate(nqs):
        want_plain, want_best, want_miss = [], [], []
        for q in range(nq):                                                                    # the layout, word by word
            row_p, row_b, row_m = [], [], []
            for i in range(n_pairs[c][q]):
                slot, k = words[at + nq + q * W + i], words[at + nq + nq * W + q * W + i]
                row_p.append((slot, k))
                row_b.append((slot, k, float(np.float32(scores[c][q][i]))))
                if tail:
                    row_m.append((slot, k, words[miss_at + (g + q) * W + i]))
            want_plain.append(row_p), want_best.append(row_b), want_miss.append(row_m)
        assert decode_budget(words, at, nq, W) == (want_plain, at + nq + 3 * nq * W)
        assert decode_budget(words, at, nq, W, best=True)[0] == want_best
        if tail:
            assert decode_budget(words, at, nq, W, miss_at=miss_at + g * W)[0] == want_miss
            assert want_miss[-1] == [] or want_miss[-1][-1][2] == 5000 + 10 * (g + nq - 1) + W - 1
        assert want_plain[0 if c == 0 else 1] == [] and len(want_plain[-1]) == W
        at, g = at + nq + 3 * nq * W, g + nq
    assert at == miss_at
    for bad in (W + 1, -1):                                                                    # a count the budget cannot have written
        with pytest.raises(IndexError, match="n_pairs=%d" % bad):
            decode_budget([bad] + [0] * (3 * W), 0, 1, W)


def test_ragged_calls_are_placed_in_call_order_whatever_the_pair_order():
    from cone_amd.library import place_calls, plan_ragged_calls
    Nq = 3
    assert place_calls([], [], Nq) == ([], 0) and place_calls([], [], Nq, 7) == ([], 7)
    # pairs 0 .. 3 with 2, 1, 4, 3 windows; the first call holds pairs 3 and 2, the second pairs 1 and 0
    row_of, end = place_calls([[3, 2], [1, 0]], [2, 1, 4, 3], Nq)
    assert row_of == [(3 + 4 + 1) * Nq, (3 + 4) * Nq, 3 * Nq, 0] and end == 10 * Nq
    assert place_calls([[3, 2], [1, 0]], [2, 1, 4, 3], Nq, 5) == ([r + 5 for r in row_of], 10 * Nq + 5)
    # as plan_ragged_calls cuts them: sorted by video, so the pairs of the video that lies first come first
    counts, video_of = [2, 1, 4, 3], [30, 20, 10, 0]
    calls = plan_ragged_calls(video_of, counts, limit=2)
    assert calls == [[3, 2], [1, 0]] and place_calls(calls, counts, Nq) == (row_of, end)


@pytest.mark.parametrize("M", (1, 5))
def test_the_stage_c_output_buffer_is_three_disjoint_regions_a_chunk_in_order(M):
    """Chunks of 1, 64 and 3 queries: ``nq * M + nq`` is even for every ``nq`` at M = 1 and at M = 5, so chunks of 2 queries at
    M = 2 (6 words) and of 1 and 3 at M = 2 (3 and 9 words) add the odd parity."""
    from cone_amd.library import FuseOut
    for nqs, m in (((1, 64, 3), M), ((1, 2, 3), 2 * M)):
        out = FuseOut(nqs, m, "cpu")
        assert out.buf.dtype == torch.float64 and out.buf.device.type == "cpu"
        raw, at, parities = out.buf.view(torch.uint8), 0, set()
        raw.fill_(0xEE)
        written = []
        for i, nq in enumerate(nqs):
            (r, n_r), (s, n_s), (k, n_k) = out.regions[i]
            assert r == at and r % 8 == 0 and s == r + n_r and k == s + n_s                     # in order, back to back, disjoint
            assert (n_r, n_s, n_k) == (8 * nq * m * 5, 4 * nq * m, 4 * nq)
            pad = 4 * ((nq * m + nq) % 2)                                                       # the int32 words fill 8-byte words
            parities.add(pad)
            at = k + n_k + pad
            rows = torch.arange(nq * m * 5, dtype=torch.float64) + 1000.0 * i
            seg = torch.arange(nq * m, dtype=torch.int32) + 100 * i
            kept = torch.arange(nq, dtype=torch.int32) + 7 * i
            raw[r:r + n_r] = rows.view(torch.uint8)
            raw[s:s + n_s] = seg.view(torch.uint8)
            raw[k:k + n_k] = kept.view(torch.uint8)
            written.append((rows.view(nq, m, 5).tolist(), seg.view(nq, m).tolist(), kept.tolist()))
        assert at == raw.numel()                                                                # nothing else in the buffer
        assert out.read() == written
        assert out.read(seg=False) == [(rows, None, kept) for rows, _, kept in written]
        assert parities == ({0} if nqs == (1, 64, 3) and m in (1, 5) else {0, 4})
