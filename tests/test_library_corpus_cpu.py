"""Library moment search, the part that needs no GPU: the C ABI's declarations and binding, the pooled stage C's model against the
existing stage-C model and on hand-made tables, every planted error caught by a named table, the refusals the two new entries
make on the host before any pointer is read, and the wrapper's refusals and empty answers before any GPU work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import backend_refs as B
import corpus_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "cone_hip.h")) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ header and binding
def test_header_binding_and_library_agree_on_the_corpus_entries():
    from cone_amd import _lib
    hdr = _header()
    assert re.search(r"#define\s+CONE_HIP_ABI_VERSION\s+8\b", hdr)
    declared = set(re.findall(r"\b(cone_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in R.NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert declared == set(_lib.EXPORTS)
    assert lib.cone_abi_version() == 8
    at = hdr.index("library moment search (additive in ABI 8)")
    assert hdr.index("library window budgets (additive in ABI 8)") < at < hdr.index("metrics on the device")
    section = hdr[at:hdr.index("metrics on the device")]
    for name in R.NEW_SYMBOLS:
        assert name + "(" in section
    for word in ("run_on_video/cone_localizator.py:187-221", "WHOLE pool", "TAGS ARE EQUAL", "FIRST 1 024 CANDIDATES", "(tag, st, ed)"):
        assert word in section, word
    for name, n in R.N_ARGS.items():
        assert len(_lib._SIGNATURES[name][1]) == n, name
        decl = re.search(r"\b%s\(([^;]*)\);" % name, hdr).group(1)
        assert decl.count(",") + 1 == n, name
    assert _lib._SIGNATURES["cone_library_localize_candidates_workspace"][0] is ctypes.c_size_t
    with open(os.path.join(ROOT, "cone_amd", "build.py")) as f:
        assert '"library_corpus.hip"' in f.read()


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("family", sorted(B.STAGE_C_FAMILIES))
def test_one_segment_is_the_existing_stage_c_model(family):
    """A pool of ONE segment is one (video, query) pair: the fused type of tests/backend_refs.py's model of fuse_nms_kernel, on
    that file's own candidate families."""
    for n in (1, 2, 65, 257):
        cand, _ = B.stage_c_case(family, n)
        for thd, mb, ma in ((0.5, 100, 5), (0.5, 100, 100), (-1, 200, 5), (0.3, 200, 1024)):
            rows, idx, kept = B.stage_c_model(cand, float(thd), mb, ma)[0]
            got_rows, got_seg, got_n = R.pool_ref(cand, [(0, n, 3)], thd, mb, ma)
            assert got_n == kept and np.array_equal(R.bits(got_rows), R.bits(rows)), (n, thd, mb, ma)
            assert got_seg.tolist() == [0] * kept + [-1] * (ma - kept)
            # a segment per candidate of one tag: the same pool, and the segment ordinal is the existing kernel's idx
            got_rows, got_seg, got_n = R.pool_ref(cand, [(i, 1, 3) for i in range(n)], thd, mb, ma)
            assert got_n == kept and np.array_equal(R.bits(got_rows), R.bits(rows)) and got_seg.tolist() == idx.tolist()


def test_the_pool_separates_what_per_pair_normalisation_ties():
    cand, segs = R.two_videos()
    per_pair = [R.pool_ref(cand, [s], 0.5, 100, 5) for s in segs]
    assert [float(r[0][0, 4]) for r in per_pair] == [1.5, 1.5]                 # sorting the concatenated lists sorts noise
    rows, seg, n = R.pool_ref(cand, segs, 0.5, 100, 5)
    assert n == 4 and rows[:4, 4].tolist() == [1.5, 0.75, 0.625, 0.5] and seg.tolist() == [0, 1, 1, 0, -1]
    assert R.moments_of(rows, seg, n, [t for _, _, t in segs]) == [(7, [0.0, 10.0, 1.5]), (9, [0.0, 10.0, 0.75]),
                                                                   (9, [20.0, 30.0, 0.625]), (7, [20.0, 30.0, 0.5])]


def test_the_hand_made_tables_answer_as_written():
    def ans(name, thd=0.5, mb=100, ma=5):
        cand, segs = R.HAND_MADE[name]()
        rows, seg, n = R.pool_ref(cand, segs, thd, mb, ma)
        return [(int(seg[j]), rows[j, 0], rows[j, 1]) for j in range(n)]
    assert ans("same_span_two_tags") == [(1, 5, 15), (0, 5, 15), (1, 70, 80), (0, 40, 50)]      # the span twice: once per video
    assert ans("identical_spans_two_videos") == [(0, 0, 10), (1, 0, 10), (1, 100, 110)]         # (1, 10) of video 0 is suppressed
    assert ans("identical_spans_two_videos", thd=-1) == [(0, 0, 10), (1, 0, 10), (0, 1, 10), (1, 100, 110)]
    cand, segs = R.dup_in_segment()
    rows, seg, n = R.pool_ref(cand, segs, 0.5, 100, 5)
    assert n == 3 and [r[1:] for r in ans("dup_in_segment")] == [(40, 50), (70, 80), (5, 15)]
    assert rows[2, 2:4].tolist() == [0.7, 0.3]                                 # the values of the last (5, 15)
    assert ans("ties_across_segments") == [(0, 0, 10), (0, 20, 30), (1, 40, 50), (1, 60, 70), (2, 80, 90)]   # pool order
    assert ans("cut_then_nms", mb=3) == [(0, 0, 10)] and ans("cut_then_nms", mb=4) == [(0, 0, 10), (0, 50, 60)]
    assert ans("iou_edges") == [(0, 0, 10), (0, 0, 20), (1, 0, np.float64(19.9)), (1, 300, 310)]
    assert ans("two_segments_one_tag") == [(0, 40, 50), (0, 5, 15), (1, 5, 15)]                 # (41, 50) of segment 2: suppressed
    assert ans("two_segments_one_tag", ma=1) == [(0, 40, 50)]
    # a list of one is returned untouched; no segments, and segments without rows, answer nothing
    assert R.pool_ref(cand, [(1, 1, 0)], 0.5, 100, 5)[2] == 1
    assert R.pool_ref(cand, [], 0.5, 100, 5)[2] == 0 and R.pool_ref(cand, [(0, 0, 1)], 0.5, 100, 5)[2] == 0


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_planted_error_is_caught_by_its_named_table(mut):
    name, (thd, mb, ma) = R.CAUGHT_BY[mut]
    cand, segs = R.HAND_MADE[name]()
    good, bad = R.pool_ref(cand, segs, thd, mb, ma), R.pool_ref(cand, segs, thd, mb, ma, mut=(mut,))
    same = good[2] == bad[2] and np.array_equal(R.bits(good[0]), R.bits(bad[0])) and np.array_equal(good[1], bad[1])
    assert not same, mut


@pytest.mark.parametrize("family", R.FAMILIES)
def test_the_dictated_pools_hold_what_their_family_names(family):
    cand, segs = R.pool_case(family, R.split(200, 64, 1))
    assert cand.shape == (200, 4) and sorted(r0 for r0, _, _ in segs) != [r0 for r0, _, _ in segs]    # the buffer's own order
    assert sorted((r0, n) for r0, n, _ in segs)[-1][0] + sorted((r0, n) for r0, n, _ in segs)[-1][1] == 200
    rows, seg, n = R.pool_ref(cand, segs, 0.5, 100, 100)
    assert 1 <= n <= 100 and (seg[:n] >= 0).all() and (seg[n:] == -1).all()
    if family == "all_equal":
        assert set(rows[:n, 4].tolist()) == {0.0 + 0.3125 + -0.125}            # mn == mx: the raw values
    if family == "cut_in_ties":
        assert n == 100 and len(set(rows[90:100, 4].tolist())) == 1            # the cut falls inside the run of ties
        assert R.pool_ref(cand, segs, 0.5, 100, 100, mut=("unstable_sort",))[1].tolist() != seg.tolist()
    if family == "past_fourth":
        assert n <= 9                                                           # three spans under three tags after rounding


def test_the_cap_truncates_the_segment_that_crosses_it():
    cand = np.tile(np.asarray([[0, 1, .5, .5]], np.float32), (1100, 1))
    cand[:, 0] = np.arange(1100) * 2
    cand[:, 1] = cand[:, 0] + 1
    cand[:, 2] = np.linspace(0, 1, 1100)
    rows, seg, n = R.pool_ref(cand, [(0, 1000, 1), (1000, 100, 2)], -1, 100, 5)
    assert n == 5 and rows[0, 0] == 2 * 1023 and seg[:5].tolist() == [1] * 5   # row 1023 is the pool's last


# ------------------------------------------------------------------------------------------------ host refusals
# (nq, n_seg, max_before, max_after) -> what the message must hold; the first that applies, in this order
CORPUS_REFUSALS = [
    ((0, 3, 100, 5), "nq=0 not in [1, 1024]"),
    ((1025, 3, 100, 5), "nq=1025 not in [1, 1024]"),
    ((0, -1, 0, 0), "nq=0 not in [1, 1024]"),
    ((1, -1, 100, 5), "n_seg=-1 < 0"),
    ((1, -1, 0, 0), "n_seg=-1 < 0"),
    ((1, 3, 100, 0), "max_after=0 not in [1, 1024]"),
    ((1, 3, 100, 1025), "max_after=1025 not in [1, 1024]"),
    ((1, 3, 0, 0), "max_after=0 not in [1, 1024]"),
    ((1, 3, 0, 5), "max_before=0 < 1"),
    ((1024, 3, 1, 1024), "null argument"),
    ((1, 0, 100, 5), "null argument"),
]


@pytest.mark.parametrize("case", range(len(CORPUS_REFUSALS)))
def test_the_pooled_stage_c_refuses_by_name_with_every_device_pointer_null(case):
    from cone_amd import _lib
    lib = _lib.load()
    (nq, n_seg, mb, ma), want = CORPUS_REFUSALS[case]
    rc = lib.cone_corpus_fuse_nms(None, None, None, None, None, nq, n_seg, 0.5, mb, ma, None, None, None, None)
    msg = lib.cone_last_error().decode()
    assert rc == -1 and want in msg and msg.startswith("corpus_fuse_nms: "), msg


def test_the_pooled_stage_c_misses_each_pointer_by_name():
    from cone_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x10000)
    for missing in range(8):
        p = [None if i == missing else fake for i in range(8)]
        rc = lib.cone_corpus_fuse_nms(*p[:5], 4, 3, 0.5, 100, 5, *p[5:], None)
        assert rc == -1 and lib.cone_last_error().decode() == "corpus_fuse_nms: null argument", missing
    for missing in (1, 5, 6, 7):        # a table of no segments still needs its offsets and its outputs
        p = [None if i in (0, 2, 3, 4, missing) else fake for i in range(8)]
        rc = lib.cone_corpus_fuse_nms(*p[:5], 4, 0, 0.5, 100, 5, *p[5:], None)
        assert rc == -1 and lib.cone_last_error().decode() == "corpus_fuse_nms: null argument", missing


def _i32(v):
    return (ctypes.c_int32 * max(len(v), 1))(*v)


def _handle(flags=0, capacity=10000):
    from cone_amd import _lib
    return _lib.Library(None, capacity, flags, 256, 256, None, None, None, None, None)


# cone_library_localize_ragged's refusals, in its order: (lens, ctx, row0, pair_k, pair_query, pair_slot, flags)
CANDIDATES_REFUSALS = [
    (([], [], [], [], [], [], 0), "nq=0 not in [1, 64]"),
    (([5] * 65, [900] * 65, [0] * 65, [1] * 65, [0] * 65, [0] * 65, 0), "nq=65 not in [1, 64]"),
    (([5, 21], [900, 900], [0, 0], [1, 1], [0, 0], [0, 0], 0), "tok_len[1]=21 not in [1, max_q_l=20]"),
    (([5, 5], [900, 0], [0, 900], [1, 1], [0, 0], [0, 1], 0), "q_ctx_l[1]=0 < 1"),
    (([5, 5], [900, 900], [0, -1], [1, 1], [0, 0], [0, 1], 0), "q_row0[1]=-1 < 0"),
    (([5, 5], [900, 900], [0, 9101], [1, 1], [0, 0], [0, 1], 0), "q_row0[1] + q_ctx_l[1] = 10001 > capacity=10000"),
    (([5], [900], [0], [20], [0], [0], 2), "CONE_SESSION_CERTIFIED libraries are not supported"),
    (([5, 5, 5], [900, 900, 91], [0, 0, 900], [20, 1, 5], [0, 1, 2], [0, 0, 1], 0), "pair_k[2]=5 not in [1, min(num_window=4, 256)]"),
    (([5, 5], [900, 900], [0, 0], [20, 0], [0, 1], [0, 0], 0), "pair_k[1]=0 not in [1, min(num_window=21, 256)]"),
    (([5], [900], [0], [20], [0], [0], 1), "library_localize_candidates: CONE_SESSION_BF16 libraries are not supported with a scan's lists"),
    (([5, 5], [900, 900], [0, 0], [3, 21], [0, 0], [0, 0], 0), "max pair_k=21 not in [1, scan_K=20]"),
    (([5, 5], [900, 900], [0, 0], [20, 1], [0, 3], [0, 0], 0), "pair_query[1]=3 not in [0, scan_nq=3)"),
    (([5, 5], [900, 900], [0, 0], [20, 1], [0, 2], [7, 0], 0), "pair_slot[0]=7 not in [0, scan_n_videos=7)"),
    (([5, 5], [900, 900], [0, 0], [20, 1], [0, 2], [6, 0], 0), "null argument"),
    # two things wrong: the earlier one in the ragged call's order is named
    (([5, 21], [900, 900], [0, 0], [0, 1], [9, 0], [0, 0], 0), "tok_len[1]=21 not in [1, max_q_l=20]"),
    (([5, 5], [900, 900], [0, 0], [0, 1], [9, 0], [0, 0], 0), "pair_k[0]=0 not in [1, min(num_window=21, 256)]"),
]


@pytest.mark.parametrize("case", range(len(CANDIDATES_REFUSALS)))
def test_the_candidates_entry_refuses_as_the_ragged_call_with_every_device_pointer_null(case):
    from cone_amd import _lib
    lib = _lib.load()
    (lens, ctx, row0, ks, pq, ps, flags), want = CANDIDATES_REFUSALS[case]
    handle, p = _handle(flags), _lib.SessionParams(90, 20, 0.5333, 0.5, 100, 5)
    args = (None, ctypes.byref(handle), _i32(row0), _i32(ctx), None, _i32(lens), len(lens), None, _i32(ks), ctypes.byref(p), _i32(pq),
            _i32(ps), None, None, 3, 7, 20)
    rc = lib.cone_library_localize_candidates(*args, None, None, 0, None)
    msg = lib.cone_last_error().decode()
    assert rc == -1 and want in msg and msg.startswith("library_localize_candidates: "), msg
    # the ragged call names the same thing under its own prefix
    rc = lib.cone_library_localize_ragged(*args, None, None, None, 0, None)
    ragged = lib.cone_last_error().decode()
    assert rc == -1 and ragged == msg.replace("library_localize_candidates: ", "library_localize_ragged: ")
    if "scan_" not in want and want != "null argument":
        n = lib.cone_library_localize_candidates_workspace(None, ctypes.byref(handle), _i32(row0), _i32(ctx), _i32(lens), len(lens),
                                                           _i32(ks), ctypes.byref(p), 1)
        assert n == 0 and want in lib.cone_last_error().decode()


def test_the_candidates_entry_without_lists_and_with_half_a_block():
    from cone_amd import _lib
    lib = _lib.load()
    p = _lib.SessionParams(90, 20, 0.5333, 0.5, 100, 5)
    fake = ctypes.c_void_p(0x10000)

    def call(handle, ks, pq=None, ps=None, widx=None, wval=None):
        rc = lib.cone_library_localize_candidates(None, ctypes.byref(handle), _i32([0]), _i32([900]), None, _i32([5]), 1, None, _i32(ks),
                                                  ctypes.byref(p), pq, ps, widx, wval, 3, 7, 20, None, None, 0, None)
        return rc, lib.cone_last_error().decode()

    rc, msg = call(_handle(), [22])
    assert rc == -1 and "pair_k[0]=22 not in [1, min(num_window=21, 256)]" in msg
    assert call(_handle(1), [20]) == (-1, "library_localize_candidates: null argument")       # its own stage A serves bf16 rows
    for part in (dict(pq=_i32([0])), dict(ps=_i32([0])), dict(widx=fake), dict(wval=fake)):
        assert call(_handle(), [20], **part) == (-1, "library_localize_candidates: null argument"), part
    assert lib.cone_library_localize_candidates_workspace(None, ctypes.byref(_handle()), _i32([0]), _i32([900]), _i32([5]), 1, _i32([20]),
                                                          ctypes.byref(p), 0) == 0
    assert lib.cone_last_error().decode() == "library_localize_candidates: null argument"


# ------------------------------------------------------------------------------------------------ the wrapper
def _bare_library(videos, flags=0, num_queries=5):
    from cone_amd.library import VideoLibrary
    lib = object.__new__(VideoLibrary)         # no handle, no arena, no GPU: the refusals and the empty answers come first
    lib.max_q_l = 20
    lib._videos = dict(videos)
    lib._flags = flags
    lib._open = False
    lib._loc = type("Loc", (), {"args": type("Args", (), {"topk_window": 20, "num_queries": num_queries})()})()
    return lib


def _q(n):
    return (torch.zeros(n, 768), torch.zeros(256))


def test_search_moments_refuses_and_answers_empty_before_any_gpu_work(monkeypatch):
    from cone_amd import _lib, library
    lib = _bare_library({1: (0, 900, 20), 3: (900, 91, 4)})
    for bad in (0, 257, -1):
        with pytest.raises(ValueError, match=f"n_windows={bad} not in \\[1, 256\\]"):
            lib.search_moments([_q(5)], n_windows=bad)
    with pytest.raises(ValueError, match="n_windows must be an integer, got 2.5"):
        lib.search_moments([_q(5)], n_windows=2.5)
    for bad in (0, 101, -3):
        with pytest.raises(ValueError, match=f"n_moments={bad} not in \\[1, 100\\]"):
            lib.search_moments([_q(5)], n_moments=bad)
    with pytest.raises(ValueError, match="n_moments must be an integer, got 1.5"):
        lib.search_moments([_q(5)], n_moments=1.5)
    with pytest.raises(ValueError, match="n_moments must be an integer, got None"):     # (None is n_windows' default, not this one's)
        lib.search_moments([_q(5)], n_moments=None)
    with pytest.raises(ValueError, match="n_moments must be an integer, got None"):     # ... before the empty answers too
        lib.search_moments([], n_moments=None)
    with pytest.raises(ValueError, match=r"n_windows=205 x num_queries=5 = 1025 candidates > 1024"):
        lib.search_moments([_q(5)], n_windows=205)
    with pytest.raises(ValueError, match=r"n_windows=103 x num_queries=10 = 1030 candidates > 1024"):
        _bare_library({1: (0, 900, 20)}, num_queries=10).search_moments([_q(5)], n_windows=103)
    with pytest.raises(ValueError, match="unknown or removed video id 2"):
        lib.search_moments([_q(5)], videos=[1, 2])
    with pytest.raises(ValueError, match="video id 3 is listed more than once"):
        lib.search_moments([_q(5)], videos=[3, 1, 3])
    with pytest.raises(ValueError, match="query has 21 tokens > max_q_l=20"):
        lib.search_moments([_q(5), _q(21)])
    assert lib.search_moments([_q(5), _q(7)], videos=[]) == [[], []]
    assert lib.search_moments([]) == [] and lib.search_moments([], n_windows=204, n_moments=100) == []
    assert _bare_library({}).search_moments([_q(5), _q(1)], n_windows=5) == [[], []]
    with pytest.raises(RuntimeError, match="the library is closed"):
        lib.search_moments([_q(5)], n_windows=204, n_moments=100)
    # a live prefilter_bf16 library is refused by name before a table is built or anything is launched
    monkeypatch.setattr(library.VideoLibrary, "_check_live", lambda self: None)
    monkeypatch.setattr(library.VideoLibrary, "_table", lambda *a: pytest.fail("a table was built"))
    bf16 = _bare_library({1: (0, 900, 20)}, flags=_lib.SESSION_BF16)
    with pytest.raises(_lib.ConeHipError, match="search_moments: CONE_SESSION_BF16 libraries are not supported"):
        bf16.search_moments([_q(5)])
    with pytest.raises(_lib.ConeHipError, match="search_windows: CONE_SESSION_BF16 libraries are not supported"):
        bf16.search_windows([_q(5)])                                            # the pinned refusal stays
    assert "not comparable across videos" in library.VideoLibrary.search_windows.__doc__
