"""Standing queries, the part that needs no GPU: the C ABI's declarations and binding, the validity rule against brute-force clip
ranges, the planted errors, the refusals the two new entries make on the host before any pointer is read, and the wrapper's
refusals before any GPU work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import watch_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "cone_hip.h")) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ header and binding
def test_header_binding_and_library_agree_on_the_watch_entries():
    from cone_amd import _lib
    hdr = _header()
    assert re.search(r"#define\s+CONE_HIP_ABI_VERSION\s+8\b", hdr)
    declared = set(re.findall(r"\b(cone_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in R.NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert declared == set(_lib.EXPORTS)
    at = hdr.index("standing queries (additive in ABI 8)")
    assert hdr.index("library moment search (additive in ABI 8)") < at < hdr.index("metrics on the device")
    section = hdr[at:hdr.index("metrics on the device")]
    assert section.count("(additive in ABI 8)") == 1
    for name in R.NEW_SYMBOLS:
        assert name + "(" in section
    for word in ("(wi - 1) S + W <= stamp", "stamp == ctx_l", "PRECONDITION", "distinct", "every element written", "DENSE",
                 "run_on_video/cone_localizator.py:150-198", "16-B aligned"):
        assert word in section, word
    for name, n in R.N_ARGS.items():
        assert len(_lib._SIGNATURES[name][1]) == n, name
        decl = re.search(r"\b%s\(([^;]*)\);" % name, hdr).group(1)
        assert decl.count(",") + 1 == n, name
    with open(os.path.join(ROOT, "cone_amd", "build.py")) as f:
        assert '"library_watch.hip"' in f.read()


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("W", (2, 3, 90, 91))
def test_the_rule_is_the_clip_ranges_of_then_and_now(W):
    """Every (window, stamp, ctx_l) with 0 <= stamp <= ctx_l on short videos: the formula says valid exactly where the window's
    clips at stamp time are its clips now."""
    S = W // 2
    for ctx_l in sorted({1, 2, S, S + 1, W - 1, W, W + 1, 2 * W, 2 * W + 1, 3 * W + S - 1, 5 * S + 1}):
        for wi in range(R.num_windows(ctx_l, W)):
            for stamp in range(0, ctx_l + 1):
                assert R.valid_rule(wi, stamp, ctx_l, W) == R.valid_by_ranges(wi, stamp, ctx_l, W), (W, ctx_l, wi, stamp)


@pytest.mark.parametrize("W", (2, 3, 90, 91))
def test_the_rules_edges(W):
    S = W // 2
    ctx_l = 7 * S + 1
    # window 0 is the half window ahead of the video: clips [0, W - S), full as soon as the video has them
    assert R.clip_range(0, ctx_l, W) == (0, W - S)
    assert R.valid_rule(0, W - S, ctx_l, W) and not R.valid_rule(0, W - S - 1, ctx_l, W)
    assert not R.valid_rule(0, 0, ctx_l, W)                                    # never computed
    # the window that ends exactly at the video's end when it was stamped, and one clip short of it
    for wi in range(1, 6):
        end = (wi - 1) * S + W
        assert R.valid_rule(wi, end, ctx_l + W, W) and R.valid_by_ranges(wi, end, ctx_l + W, W)
        assert not R.valid_rule(wi, end - 1, ctx_l + W, W) and not R.valid_by_ranges(wi, end - 1, ctx_l + W, W)
        assert not R.valid_rule(wi, end, ctx_l + W, W, mut=("lt_for_le",))
    # a short window stays valid only while the video has not grown
    last = R.num_windows(ctx_l, W) - 1
    assert R.clip_range(last, ctx_l, W)[1] == ctx_l < (last - 1) * S + W
    assert R.valid_rule(last, ctx_l, ctx_l, W) and not R.valid_rule(last, ctx_l, ctx_l + 1, W)


def test_the_plan_on_a_hand_written_list():
    W, Nq = 90, 5
    ctx_l = 400                                                                 # windows 0 .. 9; window 9 is clips [360, 400)
    widx = np.asarray([[9, 3, -1, 0, 12, 8, -4]], np.int32)
    wval = np.asarray([[.9, .8, -np.inf, .6, .5, .4, .3]], np.float32)
    stamp = np.zeros((1, 10), np.int32)
    stamp[0, [9, 3, 0, 8]] = [400, 179, 45, 392]                                # equal; one short of 180; exactly 45; 8 ends at 405
    mw, mv, n, off, cand, sn, tag = R.plan_ref(widx, wval, stamp, ctx_l, W, Nq)
    assert n.tolist() == [2] and mw[0].tolist() == [3, 8, -1, -1, -1, -1, -1]
    assert mv[0, :2].tolist() == [np.float32(.8), np.float32(.4)] and np.isneginf(mv[0, 2:]).all()
    assert off.tolist() == [0, 7] and sn.tolist() == [5, 5, 0, 5, 0, 5, 0] and not tag.any()
    assert cand.tolist() == [45, 15, 0, 0, 0, 40, 0]
    cache, st = R.store_ref(R.cand_rows(n, 7, Nq), mw, n, ctx_l, Nq, np.zeros((1, 10, Nq, 4), np.float32), stamp)
    assert st[0].tolist() == [45, 0, 0, 400, 0, 0, 0, 0, 400, 400]
    assert cache[0, 3, 0].tolist() == [1, 2, 3, 4] and cache[0, 8, 0].tolist() == [21, 22, 23, 24] and not cache[0, 9].any()
    assert R.plan_ref(widx, wval, st, ctx_l, W, Nq)[2].tolist() == [0]          # the next poll runs nothing


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_planted_error_is_caught_by_its_named_case(mut):
    pattern, K, nq = R.CAUGHT_BY[mut]
    widx, wval, stamp, ctx_l = R.dictated(nq, K, pattern)
    Nq = 5
    good = R.plan_ref(widx, wval, stamp, ctx_l, R.W_DICTATED, Nq)
    bad = R.plan_ref(widx, wval, stamp, ctx_l, R.W_DICTATED, Nq, mut=(mut,))
    cand = R.cand_rows(np.maximum(good[2], bad[2]), K, Nq)
    cache = np.zeros(stamp.shape + (Nq, 4), np.float32)
    good += R.store_ref(cand, good[0], good[2], ctx_l, Nq, cache, stamp)
    bad += R.store_ref(cand, bad[0], bad[2], ctx_l, Nq, cache, stamp, mut=(mut,))
    assert not all(np.array_equal(a, b) for a, b in zip(good, bad)), mut


@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_the_dictated_cases_hold_what_their_pattern_names(pattern):
    for K in R.KS:
        widx, wval, stamp, ctx_l = R.dictated(5, K, pattern)
        n_win = stamp.shape[1]
        n = R.plan_ref(widx, wval, stamp, ctx_l, R.W_DICTATED, 5)[2]
        listed = ((widx >= 0) & (widx < n_win)).sum(axis=1)
        for q in range(5):
            live = widx[q][(widx[q] >= 0) & (widx[q] < n_win)]
            assert len(set(live.tolist())) == len(live)                        # the store's precondition
        if pattern == "all_valid":
            assert not n.any()
        if pattern == "all_missing":
            assert (n == K).all()
        if pattern == "alternating":
            assert (n == K // 2).all()
        if pattern == "pad_middle" and K >= 3:
            assert (listed < K).all() and (widx[:, 0] != -1).all() and (widx[:, -1] != -1).all()
        if pattern == "out_of_range":
            assert (listed < K).all() and (widx >= n_win).any() and ((widx < -1).any() or K < 2)
        if pattern == "zero_between" and K >= 2:
            assert n[1] == 0 and n[4] == 0 and n[0] > 0 and n[2] > 0 and n[3] > 0
        if pattern == "short_equal":
            assert n[0] == 0 and n[2] == 0 and (n[[1, 3]] >= 1).all()           # the short last window, and any that ctx_l - 1 cuts


# ------------------------------------------------------------------------------------------------ host refusals
# (nq, K, n_win, ctx_l, W, Nq) -> the message; the first that applies, in the header's order
PLAN_REFUSALS = [
    ((0, 20, 21, 900, 90, 5), "nq=0 not in [1, 64]"),
    ((65, 20, 21, 900, 90, 5), "nq=65 not in [1, 64]"),
    ((0, 0, 0, 0, 0, 0), "nq=0 not in [1, 64]"),
    ((1, 0, 21, 900, 90, 5), "K=0 not in [1, 256]"),
    ((1, 257, 0, 0, 0, 0), "K=257 not in [1, 256]"),
    ((1, 20, 21, 900, 90, 0), "Nq=0 not in [1, 16]"),
    ((1, 20, 0, 0, 0, 17), "Nq=17 not in [1, 16]"),
    ((1, 20, 0, 0, 0, 5), "n_win=0 < 1"),
    ((1, 20, 21, 0, 1, 5), "ctx_l=0 < 1"),
    ((1, 20, 21, 900, 1, 5), "W=1 < 2"),
    ((64, 256, 21, 900, 2, 16), "null argument"),
]


@pytest.mark.parametrize("case", range(len(PLAN_REFUSALS)))
def test_the_plan_refuses_by_name_with_every_device_pointer_null(case):
    from cone_amd import _lib
    lib = _lib.load()
    (nq, K, n_win, ctx_l, W, Nq), want = PLAN_REFUSALS[case]
    rc = lib.cone_watch_plan(None, None, nq, K, None, n_win, ctx_l, W, Nq, None, None, None, None, None, None, None, None)
    msg = lib.cone_last_error().decode()
    assert rc == -1 and msg == "watch_plan: " + want, msg


# (nq, K, n_win, ctx_l, Nq)
STORE_REFUSALS = [
    ((0, 20, 21, 900, 5), "nq=0 not in [1, 64]"),
    ((65, 0, 0, 0, 0), "nq=65 not in [1, 64]"),
    ((1, 0, 0, 0, 0), "K=0 not in [1, 256]"),
    ((1, 257, 21, 900, 5), "K=257 not in [1, 256]"),
    ((1, 20, 0, 0, 0), "n_win=0 < 1"),
    ((1, 20, 21, 0, 0), "ctx_l=0 < 1"),
    ((1, 20, 21, 900, 0), "Nq=0 not in [1, 16]"),
    ((1, 20, 21, 900, 17), "Nq=17 not in [1, 16]"),
    ((64, 256, 1, 1, 16), "null argument"),
]


@pytest.mark.parametrize("case", range(len(STORE_REFUSALS)))
def test_the_store_refuses_by_name_with_every_device_pointer_null(case):
    from cone_amd import _lib
    lib = _lib.load()
    (nq, K, n_win, ctx_l, Nq), want = STORE_REFUSALS[case]
    rc = lib.cone_watch_store(None, None, None, nq, K, n_win, ctx_l, Nq, None, None, None)
    msg = lib.cone_last_error().decode()
    assert rc == -1 and msg == "watch_store: " + want, msg


def test_both_entries_miss_each_pointer_by_name_and_the_store_wants_aligned_rows():
    from cone_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x10000)
    for missing in range(10):
        p = [None if i == missing else fake for i in range(10)]
        rc = lib.cone_watch_plan(p[0], p[1], 4, 20, p[2], 21, 900, 90, 5, *p[3:], None)
        assert rc == -1 and lib.cone_last_error().decode() == "watch_plan: null argument", missing
    for missing in range(5):
        p = [None if i == missing else fake for i in range(5)]
        rc = lib.cone_watch_store(*p[:3], 4, 20, 21, 900, 5, *p[3:], None)
        assert rc == -1 and lib.cone_last_error().decode() == "watch_store: null argument", missing
    for cand, cache in ((0x10008, 0x10000), (0x10000, 0x10004)):
        rc = lib.cone_watch_store(ctypes.c_void_p(cand), fake, fake, 4, 20, 21, 900, 5, ctypes.c_void_p(cache), fake, None)
        assert rc == -1 and lib.cone_last_error().decode() == "watch_store: cand and cache must be 16-B aligned"


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


def test_watch_refuses_before_any_gpu_work(monkeypatch):
    from cone_amd import _lib, library, watch
    monkeypatch.setattr(watch.VideoWatcher, "__init__", lambda *a: pytest.fail("a watcher was built"))
    lib = _bare_library({1: (0, 900, 20)})
    with pytest.raises(ValueError, match="unknown or removed video id 2"):
        lib.watch(2, [_q(5)])
    with pytest.raises(ValueError, match="watch: an empty query list"):
        lib.watch(1, [])
    with pytest.raises(ValueError, match="query has 21 tokens > max_q_l=20"):
        lib.watch(1, [_q(5), _q(21)])
    with pytest.raises(ValueError, match=r"topk_window=205 x num_queries=5 = 1025 candidates > 1024 in one pool"):
        _bare_library({1: (0, 900, 20)}, topk_window=205).watch(1, [_q(5)])
    with pytest.raises(ValueError, match=r"topk_window=103 x num_queries=10 = 1030 candidates > 1024 in one pool"):
        _bare_library({1: (0, 900, 20)}, topk_window=103, num_queries=10).watch(1, [_q(5)])
    with pytest.raises(RuntimeError, match="the library is closed"):
        lib.watch(1, [_q(5)])
    # a live prefilter_bf16 library: a message of its own, before anything is uploaded or launched
    monkeypatch.setattr(library.VideoLibrary, "_check_live", lambda self: None)
    with pytest.raises(_lib.ConeHipError, match="^watch: CONE_SESSION_BF16 libraries are not supported"):
        _bare_library({1: (0, 900, 20)}, flags=_lib.SESSION_BF16).watch(1, [_q(5)])


def test_a_trim_reaches_the_watchers_of_that_video_only_and_launches_nothing():
    from cone_amd import library, watch
    lib = _bare_library({1: (0, 900, 20), 2: (900, 300, 8)})
    lib._rows = library.RowRanges(1200)
    lib._rows.take(1200)
    lib._scan_cache = None
    ws = []
    for vid in (1, 2):
        w = object.__new__(watch.VideoWatcher)
        w._vid, w._reset = vid, False
        ws.append(w)
    import weakref
    lib._watchers = weakref.WeakSet(ws)
    assert lib.trim(1, 0) == 900 and not ws[0]._reset and not ws[1]._reset      # n_front == 0 changes nothing
    assert lib.trim(1, 45) == 855 and ws[0]._reset and not ws[1]._reset


def test_a_closed_watcher_raises_and_holds_nothing():
    from cone_amd import watch
    w = object.__new__(watch.VideoWatcher)
    w._open = True
    w.close()
    assert w.nbytes == 0
    with pytest.raises(RuntimeError, match="the watcher is closed"):
        w.poll()
