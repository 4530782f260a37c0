"""Library window budgets, the part that needs no GPU: the C ABI's declarations and binding, the contract's model on hand-written
lists, the ragged planner, every refusal the three new entries make on the host before any pointer is read, and the wrapper's
refusals before any GPU work."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

import budget_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = float("-inf")


def _header():
    with open(os.path.join(ROOT, "include", "cone_hip.h")) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ header and binding
def test_header_binding_and_library_agree_on_the_budget_entries():
    from cone_amd import _lib
    hdr = _header()
    assert re.search(r"#define\s+CONE_HIP_ABI_VERSION\s+8\b", hdr)
    declared = set(re.findall(r"\b(cone_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in R.NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert declared == set(_lib.EXPORTS)
    assert lib.cone_abi_version() == 8
    # behind the maintenance section, before the device metrics, nothing in between; every entry cites the reference sites
    at = hdr.index("library window budgets (additive in ABI 8)")
    assert hdr.index("library maintenance (additive in ABI 8)") < at < hdr.index("metrics on the device")
    between = hdr[hdr.index("library maintenance (additive in ABI 8)"):at]
    assert "cone_library_move_rows(" in between and between.count("(additive in ABI 8)") == 1
    section = hdr[at:hdr.index("metrics on the device")]
    for name in R.NEW_SYMBOLS:
        assert name + "(" in section
    assert section.count("run_on_video/cone_localizator.py:121-221") >= 3
    assert section.count("cone/inference.py:276-299") >= 3
    for word in ("SPENDS ITS BUDGET SHORT", "NEVER chosen", "a prefix", "topk_window = k", "CONE_SESSION_BF16", "first appearance"):
        assert word in section, word


def test_the_structs_stay_and_the_signatures_mirror_the_header():
    from cone_amd import _lib
    hdr = _header()
    assert ctypes.sizeof(_lib.Library) == 72 and len(_lib.Library._fields_) == 10
    assert ctypes.sizeof(_lib.Session) == 80 and ctypes.sizeof(_lib.SessionParams) == 32
    for name, n in R.N_ARGS.items():
        assert len(_lib._SIGNATURES[name][1]) == n, name
        decl = re.search(r"\b%s\(([^;]*)\);" % name, hdr).group(1)
        assert decl.count(",") + 1 == n, name
    for name in ("cone_library_budget_workspace", "cone_library_localize_ragged_workspace"):
        assert _lib._SIGNATURES[name][0] is ctypes.c_size_t
    with open(os.path.join(ROOT, "cone_amd", "build.py")) as f:
        assert '"library_budget.hip"' in f.read()


# ------------------------------------------------------------------------------------------------ the contract's model
def _ref(lists, W):
    """``lists`` = per query, per slot, the values (padded to the longest with -inf)."""
    K = max(len(l) for q in lists for l in q)
    wval = np.full((len(lists), len(lists[0]), K), NINF, dtype=np.float32)
    for q, slots in enumerate(lists):
        for s, l in enumerate(slots):
            wval[q, s, :len(l)] = l
    n, slot, k, best = R.budget_ref(wval, W)
    return [(int(n[q]), slot[q].tolist(), k[q].tolist(), best[q].tolist()) for q in range(len(lists))]


def test_budget_ref_on_hand_written_lists():
    # distinct values: 9 8 | 7 from slot 1, then 6 from slot 0: the first appearance orders the pairs
    assert _ref([[[6, 5, 1], [9, 8, 7], [4, 3, 2]]], 4) == [(2, [1, 0, -1, -1], [3, 1, 0, 0], [9.0, 6.0, NINF, NINF])]
    assert _ref([[[6, 5, 1], [9, 8, 7], [4, 3, 2]]], 6) == [(3, [1, 0, 2, -1, -1, -1], [3, 2, 1, 0, 0, 0], [9.0, 6.0, 4.0, NINF, NINF, NINF])]
    # W = 1
    assert _ref([[[6, 5], [9, 8]]], 1) == [(1, [1], [1], [9.0])]
    # ties across slots go to the lower slot, ties inside a list to the lower position: the budget of 3 ends inside the tie
    assert _ref([[[5, 5, 5], [5, 5, 5]]], 3) == [(1, [0, -1, -1], [3, 0, 0], [5.0, NINF, NINF])]
    assert _ref([[[5, 5, 5], [5, 5, 5]]], 4) == [(2, [0, 1, -1, -1], [3, 1, 0, 0], [5.0, 5.0, NINF, NINF])]
    assert _ref([[[7, 5], [7, 5], [7, 4]]], 4) == [(3, [0, 1, 2, -1], [2, 1, 1, 0], [7.0, 7.0, 7.0, NINF])]
    # -0.0 ties with +0.0 (the lower flat index wins, whatever the sign) and the score keeps its bits
    got = _ref([[[1, -0.0], [0.0, -1]], [[1, 0.0], [-0.0, -1]]], 2)
    assert [g[:3] for g in got] == [(1, [0, -1], [2, 0])] * 2
    got = _ref([[[-0.0, -1], [0.0, -2]]], 1)
    assert got[0][:3] == (1, [0], [1]) and np.signbit(np.float32(got[0][3][0]))
    # W above the number of finite entries: the budget is spent short; -inf is never chosen, padding and dead windows alike
    assert _ref([[[3, NINF, NINF], [2, 1, NINF]]], 5) == [(2, [0, 1, -1, -1, -1], [1, 2, 0, 0, 0], [3.0, 2.0, NINF, NINF, NINF])]
    assert _ref([[[NINF, NINF], [NINF, NINF]]], 3) == [(0, [-1, -1, -1], [0, 0, 0], [NINF, NINF, NINF])]
    assert _ref([[[NINF], [2]]], 1) == [(1, [1], [1], [2.0])]
    # +inf is a number; every query on its own
    assert _ref([[[np.inf, 1], [np.inf, np.inf]], [[1, 0], [3, 2]]], 3) == [(2, [0, 1, -1], [1, 2, 0], [np.inf, np.inf, NINF]),
                                                                            (2, [1, 0, -1], [2, 1, 0], [3.0, 1.0, NINF])]


@pytest.mark.parametrize("family", R.FAMILIES)
def test_the_dictated_lists_are_descending_and_the_model_spends_what_it_can(family):
    for V, K in R.SHAPES[:3]:
        for W in (1, 2, 63, 256):
            wval, widx = R.dictated(V, K, 5, family, W)
            n, slot, k, best = R.budget_ref(wval, W)
            finite = (wval > NINF).reshape(5, -1).sum(axis=1)
            assert (k.sum(axis=1) == np.minimum(W, finite)).all()
            assert ((widx >= 0) == (wval > NINF)).all()
            for q in range(5):
                assert len(set(slot[q, :n[q]].tolist())) == n[q] and (slot[q, n[q]:] == -1).all() and (k[q, :n[q]] >= 1).all()
                assert best[q, :n[q]].tolist() == [wval[q, s, 0] for s in slot[q, :n[q]]]       # a prefix: the slot's first entry
                assert best[q, :n[q]].tolist() == sorted(best[q, :n[q]].tolist(), reverse=True)


# ------------------------------------------------------------------------------------------------ the planner
def test_plan_ragged_calls_on_named_cases():
    from cone_amd.library import inverse_order, plan_ragged_calls
    assert plan_ragged_calls([], []) == []
    # sorted by video, stable; different k of one video stay adjacent in one call
    assert plan_ragged_calls([900, 0, 900, 0, 333], [20, 2, 1, 1, 9]) == [[1, 3, 4, 0, 2]]
    assert plan_ragged_calls([5] * 5, [1] * 5, limit=2) == [[0, 1], [2, 3], [4]]
    assert plan_ragged_calls([0, 1, 2, 3], [20, 20, 20, 5], max_windows=40) == [[0, 1], [2, 3]]
    assert plan_ragged_calls([0, 1, 2], [40, 1, 40], max_windows=40) == [[0], [1], [2]]
    assert [len(c) for c in plan_ragged_calls(list(range(130)), [20] * 130)] == [64, 64, 2]
    assert [len(c) for c in plan_ragged_calls(list(range(130)), [256] * 130)] == [64, 64, 2]         # 64 x 256 windows: the default
    calls = plan_ragged_calls([3, 1, 2, 1], [1, 2, 3, 4], limit=3)
    assert calls == [[1, 3, 2], [0]] and inverse_order([(None, idx) for idx in calls], 4) == [3, 0, 2, 1]
    for bad in (dict(limit=0), dict(max_windows=0)):
        with pytest.raises(ValueError, match="< 1"):
            plan_ragged_calls([0], [1], **bad)
    with pytest.raises(ValueError, match="pair 1 asks for 0 windows"):
        plan_ragged_calls([0, 0], [1, 0])
    with pytest.raises(ValueError, match="pair 0 asks for 41 windows, not in \\[1, max_windows=40\\]"):
        plan_ragged_calls([0], [41], max_windows=40)
    with pytest.raises(ValueError, match="2 videos for 1 window counts"):
        plan_ragged_calls([0, 1], [1])


@pytest.mark.parametrize("seed", range(40))
def test_plan_ragged_calls_on_random_inputs(seed):
    from cone_amd.library import inverse_order, plan_ragged_calls
    rng = random.Random(seed)
    n = rng.randrange(0, 200)
    limit, max_windows = rng.choice((1, 2, 7, 64)), rng.choice((20, 21, 100, 64 * 256))
    video_of = [rng.randrange(0, 12) * 100 for _ in range(n)]
    k_of = [rng.randint(1, 20) for _ in range(n)]
    calls = plan_ragged_calls(video_of, k_of, limit=limit, max_windows=max_windows)
    R.check_ragged_plan(video_of, k_of, calls, limit, max_windows)
    where = inverse_order([(None, idx) for idx in calls], n)
    flat = [i for idx in calls for i in idx]
    assert all(flat[where[i]] == i for i in range(n))


def test_plan_calls_and_inverse_order_stay():
    from cone_amd.library import inverse_order, plan_calls
    calls = plan_calls([900, 0, 900, 0, 333], [20, 2, 20, 2, 9])
    assert calls == [(2, [1, 3]), (9, [4]), (20, [0, 2])] and inverse_order(calls, 5) == [3, 0, 4, 1, 2]


# ------------------------------------------------------------------------------------------------ host refusals
def _i32(v):
    return (ctypes.c_int32 * max(len(v), 1))(*v)


def _handle(flags=0, capacity=10000):
    from cone_amd import _lib
    return _lib.Library(None, capacity, flags, 256, 256, None, None, None, None, None)


# (nq, n_videos, scan_K, W) -> what the message must hold
BUDGET_REFUSALS = [
    ((0, 3, 20, 20), "nq=0 not in [1, 64]"),
    ((65, 3, 20, 20), "nq=65 not in [1, 64]"),
    ((1, 0, 20, 20), "n_videos=0 < 1"),
    ((1, -2, 20, 20), "n_videos=-2 < 1"),
    ((1, 3, 0, 20), "scan_K=0 not in [1, 256]"),
    ((1, 3, 257, 20), "scan_K=257 not in [1, 256]"),
    ((1, 3, 20, 0), "W=0 not in [1, 256]"),
    ((1, 3, 20, 257), "W=257 not in [1, 256]"),
    ((1, 1 << 27, 20, 20), "entries per query do not fit an int32 index"),
]


@pytest.mark.parametrize("case", range(len(BUDGET_REFUSALS)))
def test_the_budget_refuses_by_name_with_every_device_pointer_null(case):
    from cone_amd import _lib
    lib = _lib.load()
    (nq, V, K, W), want = BUDGET_REFUSALS[case]
    rc = lib.cone_library_budget(None, nq, V, K, W, None, None, None, None, None, 0, None)
    msg = lib.cone_last_error().decode()
    assert rc == -1 and want in msg and msg.startswith("library_budget: "), msg
    assert lib.cone_library_budget_workspace(nq, V, K, W) == 0 and want in lib.cone_last_error().decode()


def test_a_budget_that_passes_the_host_values_then_misses_its_pointers_and_its_workspace():
    from cone_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x10000)
    assert lib.cone_library_budget(None, 4, 3, 20, 20, None, None, None, None, None, 0, None) == -1
    assert lib.cone_last_error().decode() == "library_budget: null argument"
    for missing in range(6):
        ptrs = [None if i == missing else fake for i in range(6)]
        rc = lib.cone_library_budget(ptrs[0], 4, 3, 20, 20, *ptrs[1:5], ptrs[5], 1 << 20, None)
        assert rc == -1 and lib.cone_last_error().decode() == "library_budget: null argument", missing
    n = lib.cone_library_budget_workspace(4, 3, 20, 20)
    assert n >= 2 * 4 * 20 * 4 and n % 256 == 0
    assert lib.cone_library_budget_workspace(4, 1, 5, 256) == 2 * 256          # min(W, entries) = 5 selected per query, no scratch
    assert lib.cone_library_budget_workspace(64, 410, 20, 256) > 2 * 64 * 256 * 4   # a row above 8 192: the selection's scratch
    rc = lib.cone_library_budget(fake, 4, 3, 20, 20, fake, fake, fake, fake, ctypes.c_void_p(0x10010), n, None)
    assert rc == -1 and "library_budget: the workspace must be 256-B aligned" in lib.cone_last_error().decode()
    rc = lib.cone_library_budget(fake, 4, 3, 20, 20, fake, fake, fake, fake, fake, n - 1, None)
    assert rc == -3 and f"library_budget: workspace too small ({n - 1} < {n})" in lib.cone_last_error().decode()


# the pairs' refusals of cone_library_localize, then the ragged entry's own: (lens, ctx, row0, pair_k, pair_query, pair_slot, flags)
RAGGED_REFUSALS = [
    (([], [], [], [], [], [], 0), "nq=0 not in [1, 64]"),
    (([5] * 65, [900] * 65, [0] * 65, [1] * 65, [0] * 65, [0] * 65, 0), "nq=65 not in [1, 64]"),
    (([5, 21], [900, 900], [0, 0], [1, 1], [0, 0], [0, 0], 0), "tok_len[1]=21 not in [1, max_q_l=20]"),
    (([5, 5], [900, 0], [0, 900], [1, 1], [0, 0], [0, 1], 0), "q_ctx_l[1]=0 < 1"),
    (([5, 5], [900, 900], [0, -1], [1, 1], [0, 0], [0, 1], 0), "q_row0[1]=-1 < 0"),
    (([5, 5], [900, 900], [0, 9101], [1, 1], [0, 0], [0, 1], 0), "q_row0[1] + q_ctx_l[1] = 10001 > capacity=10000"),
    (([5], [900], [0], [20], [0], [0], 2), "CONE_SESSION_CERTIFIED libraries are not supported"),
    (([5, 5, 5], [900, 900, 91], [0, 0, 900], [20, 1, 5], [0, 1, 2], [0, 0, 1], 0), "pair_k[2]=5 not in [1, min(num_window=4, 256)]"),
    (([5, 5], [900, 900], [0, 0], [20, 0], [0, 1], [0, 0], 0), "pair_k[1]=0 not in [1, min(num_window=21, 256)]"),
    (([5], [90000], [0], [257], [0], [0], 0), "pair_k[0]=257 not in [1, min(num_window=2001, 256)]"),
    (([5], [900], [0], [20], [0], [0], 1), "library_localize_ragged: CONE_SESSION_BF16 libraries are not supported with a scan's lists"),
    (([5, 5], [900, 900], [0, 0], [3, 21], [0, 0], [0, 0], 0), "max pair_k=21 not in [1, scan_K=20]"),
    (([5, 5], [900, 900], [0, 0], [20, 1], [0, 3], [0, 0], 0), "pair_query[1]=3 not in [0, scan_nq=3)"),
    (([5, 5], [900, 900], [0, 0], [20, 1], [0, -1], [0, 0], 0), "pair_query[1]=-1 not in [0, scan_nq=3)"),
    (([5, 5], [900, 900], [0, 0], [20, 1], [0, 2], [7, 0], 0), "pair_slot[0]=7 not in [0, scan_n_videos=7)"),
]


@pytest.mark.parametrize("case", range(len(RAGGED_REFUSALS)))
def test_the_ragged_query_half_refuses_by_name_with_every_device_pointer_null(case):
    """The lists' form: the two host arrays of the block are there, every device pointer is NULL."""
    from cone_amd import _lib
    lib = _lib.load()
    (lens, ctx, row0, ks, pq, ps, flags), want = RAGGED_REFUSALS[case]
    cap = 100000 if max(ctx, default=0) > 10000 else 10000
    handle, p = _handle(flags, cap), _lib.SessionParams(90, 20, 0.5333, 0.5, 100, 5)
    rc = lib.cone_library_localize_ragged(None, ctypes.byref(handle), _i32(row0), _i32(ctx), None, _i32(lens), len(lens), None, _i32(ks),
                                          ctypes.byref(p), _i32(pq), _i32(ps), None, None, 3, 7, 20, None, None, None, 0, None)
    msg = lib.cone_last_error().decode()
    assert rc == -1 and want in msg and msg.startswith("library_localize_ragged: "), msg
    if "scan_" not in want:     # (the size entry knows the pairs, the counts, the library and the form, not the scan)
        n = lib.cone_library_localize_ragged_workspace(None, ctypes.byref(handle), _i32(row0), _i32(ctx), _i32(lens), len(lens),
                                                       _i32(ks), ctypes.byref(p), 1)
        assert n == 0 and want in lib.cone_last_error().decode()


def test_the_ragged_query_half_without_lists_and_with_half_a_block():
    from cone_amd import _lib
    lib = _lib.load()
    p = _lib.SessionParams(90, 20, 0.5333, 0.5, 100, 5)
    fake = ctypes.c_void_p(0x10000)

    def call(handle, ks, pq=None, ps=None, widx=None, wval=None, m=None, pairs=True):
        rc = lib.cone_library_localize_ragged(m, ctypes.byref(handle), _i32([0]) if pairs else None, _i32([900]), None, _i32([5]), 1, None,
                                              _i32(ks) if ks is not None else None, ctypes.byref(p), pq, ps, widx, wval, 3, 7, 20, None,
                                              None, None, 0, None)
        return rc, lib.cone_last_error().decode()

    assert call(_handle(), [20], pairs=False) == (-1, "library_localize_ragged: null argument")
    assert call(_handle(), None) == (-1, "library_localize_ragged: null argument")
    # no lists: the counts are checked all the same, a bf16 library passes the host values and then misses its pointers
    rc, msg = call(_handle(), [22])
    assert rc == -1 and "pair_k[0]=22 not in [1, min(num_window=21, 256)]" in msg
    assert call(_handle(1), [20]) == (-1, "library_localize_ragged: null argument")
    assert call(_handle(), [20]) == (-1, "library_localize_ragged: null argument")
    # a block that is only partly there is refused, whichever part it is
    for part in (dict(pq=_i32([0])), dict(ps=_i32([0])), dict(widx=fake), dict(wval=fake), dict(pq=_i32([0]), ps=_i32([0]), widx=fake)):
        assert call(_handle(), [20], **part) == (-1, "library_localize_ragged: null argument"), part
    rc, msg = call(_handle(1), [20], widx=fake)                # ... and is the lists' form: no bf16 library
    assert rc == -1 and "CONE_SESSION_BF16 libraries are not supported with a scan's lists" in msg
    # the size entry: no handle, no size
    for ranked in (0, 1):
        assert lib.cone_library_localize_ragged_workspace(None, ctypes.byref(_handle()), _i32([0]), _i32([900]), _i32([5]), 1, _i32([20]),
                                                          ctypes.byref(p), ranked) == 0
        assert lib.cone_last_error().decode() == "library_localize_ragged: null argument"


# ------------------------------------------------------------------------------------------------ the wrapper
def _bare_library(videos, flags=0):
    from cone_amd.library import VideoLibrary
    lib = object.__new__(VideoLibrary)         # no handle, no arena, no GPU: the refusals and the empty answers come first
    lib.max_q_l = 20
    lib._videos = dict(videos)
    lib._flags = flags
    lib._open = False
    lib._loc = type("Loc", (), {"args": type("Args", (), {"topk_window": 20})()})()
    return lib


def _q(n):
    return (torch.zeros(n, 768), torch.zeros(256))


def test_predict_moments_refuses_bad_window_counts_before_any_gpu_work():
    lib = _bare_library({1: (0, 900, 20), 3: (900, 91, 4)})
    pairs = [(1, _q(5)), (3, _q(7))]
    with pytest.raises(ValueError, match="1 window counts for 2 pairs"):
        lib.predict_moments(pairs, windows=[3])
    with pytest.raises(ValueError, match=r"windows\[1\]=5 not in \[1, 4\] for video 3"):
        lib.predict_moments(pairs, windows=[20, 5])
    with pytest.raises(ValueError, match=r"windows\[0\]=0 not in \[1, 20\] for video 1"):
        lib.predict_moments(pairs, windows=[0, 4])
    with pytest.raises(ValueError, match=r"windows\[0\]=21 not in \[1, 20\]"):
        lib.predict_moments(pairs, windows=[21, 4], ragged=True)
    with pytest.raises(ValueError, match=r"windows\[1\] must be an integer, got 2.5"):
        lib.predict_moments(pairs, windows=[1, 2.5])
    with pytest.raises(ValueError, match="unknown or removed video id 2"):
        lib.predict_moments([(2, _q(5))], windows=[1])
    with pytest.raises(ValueError, match="query has 21 tokens > max_q_l=20"):
        lib.predict_moments([(1, _q(21))], ragged=True)
    assert lib.predict_moments([], ragged=True) == [] and lib.predict_moments([], windows=[]) == []
    for kw in (dict(ragged=True), dict(windows=[20, 4])):      # everything passes: the closed library is what is left to refuse
        with pytest.raises(RuntimeError, match="the library is closed"):
            lib.predict_moments(pairs, **kw)


def test_search_windows_refuses_and_answers_empty_before_any_gpu_work(monkeypatch):
    from cone_amd import _lib, library
    lib = _bare_library({1: (0, 900, 20), 3: (900, 91, 4)})
    for bad in (0, 257, -1):
        with pytest.raises(ValueError, match=f"n_windows={bad} not in \\[1, 256\\]"):
            lib.search_windows([_q(5)], n_windows=bad)
    with pytest.raises(ValueError, match="n_windows must be an integer, got 2.5"):
        lib.search_windows([_q(5)], n_windows=2.5)
    with pytest.raises(ValueError, match="unknown or removed video id 2"):
        lib.search_windows([_q(5)], videos=[1, 2])
    with pytest.raises(ValueError, match="video id 3 is listed more than once"):
        lib.search_windows([_q(5)], videos=[3, 1, 3])
    with pytest.raises(ValueError, match="query has 21 tokens > max_q_l=20"):
        lib.search_windows([_q(5), _q(21)])
    assert lib.search_windows([_q(5), _q(7)], videos=[]) == [[], []]
    assert lib.search_windows([]) == [] and lib.search_windows([], n_windows=256) == []
    assert _bare_library({}).search_windows([_q(5), _q(1)], n_windows=5) == [[], []]
    with pytest.raises(RuntimeError, match="the library is closed"):
        lib.search_windows([_q(5)])
    # a live prefilter_bf16 library is refused by name before a table is built or anything is launched
    monkeypatch.setattr(library.VideoLibrary, "_check_live", lambda self: None)
    monkeypatch.setattr(library.VideoLibrary, "_table", lambda *a: pytest.fail("a table was built"))
    bf16 = _bare_library({1: (0, 900, 20)}, flags=_lib.SESSION_BF16)
    with pytest.raises(_lib.ConeHipError, match="search_windows: CONE_SESSION_BF16 libraries are not supported"):
        bf16.search_windows([_q(5)])
