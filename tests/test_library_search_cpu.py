"""Library search, the part that needs no GPU: the C ABI's declarations and binding, the refusals that fire on the host before
any pointer is read, the scan's table against a first-principles model, the numpy models the GPU tests rely on -- with a table
of which case family catches which planted error --, and the wrapper's behaviour before any GPU work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import search_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "cone_hip.h")) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ header and binding
def test_header_binding_and_library_agree_on_the_search_entries():
    from cone_amd import _lib
    hdr = _header()
    assert re.search(r"#define\s+CONE_HIP_ABI_VERSION\s+8\b", hdr)
    declared = set(re.findall(r"\b(cone_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in R.NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert declared == set(_lib.EXPORTS)
    assert lib.cone_abi_version() == 8
    # directly behind the libraries' section, before the device metrics; every entry cites the reference sites
    at = hdr.index("library search (additive in ABI 8)")
    assert hdr.index("video libraries (additive in ABI 8)") < at < hdr.index("metrics on the device")
    between = hdr[hdr.index("video libraries (additive in ABI 8)"):at]
    assert "cone_library_localize(" in between and between.count("(additive in ABI 8)") == 1      # no section in between
    section = hdr[at:hdr.index("metrics on the device")]
    assert section.count("run_on_video/cone_localizator.py:121-221") >= 2
    assert section.count("cone/inference.py:276-299") >= 3
    for word in ("the bits", "CONE_SESSION_BF16", "CONE_SESSION_CERTIFIED", "never read", "TABLE SLOTS"):
        assert word in section, word


def test_the_library_struct_stays_and_the_signatures_mirror_the_header():
    from cone_amd import _lib
    hdr = _header()
    assert ctypes.sizeof(_lib.Library) == 72 and len(_lib.Library._fields_) == 10
    n_args = dict(cone_library_scan_workspace=6, cone_library_scan=19, cone_library_localize_ranked_workspace=8,
                  cone_library_localize_ranked=22)
    for name, n in n_args.items():
        assert len(_lib._SIGNATURES[name][1]) == n, name
        decl = re.search(r"\b%s\(([^;]*)\);" % name, hdr).group(1)
        assert decl.count(",") + 1 == n, name
    for name in ("cone_library_scan_workspace", "cone_library_localize_ranked_workspace"):
        assert _lib._SIGNATURES[name][0] is ctypes.c_size_t


# ------------------------------------------------------------------------------------------------ host refusals
def _i32(v):
    return (ctypes.c_int32 * max(len(v), 1))(*v)


def _handle(flags=0, capacity=10000):
    from cone_amd import _lib
    return _lib.Library(None, capacity, flags, 256, 256, None, None, None, None, None)


# (n_videos, total_hb, nq, K, n_rank, flags, max_v_l) -> what the message must hold; capacity 10000
SCAN_REFUSALS = [
    ((3, 60, 0, 20, 1, 0, 90), "nq=0 not in [1, 64]"),
    ((3, 60, 65, 20, 1, 0, 90), "nq=65 not in [1, 64]"),
    ((0, 60, 1, 20, 1, 0, 90), "n_videos=0 < 1"),
    ((3, 2, 1, 20, 1, 0, 90), "total_hb=2 not in [n_videos=3, capacity=10000]"),
    ((3, 10001, 1, 20, 1, 0, 90), "total_hb=10001 not in [n_videos=3, capacity=10000]"),
    ((3, 60, 1, 0, 1, 0, 90), "K=0 not in [1, 256]"),
    ((3, 60, 1, 257, 1, 0, 90), "K=257 not in [1, 256]"),
    ((3, 60, 1, 20, 0, 0, 90), "n_rank=0 not in [1, n_videos=3]"),
    ((3, 60, 1, 20, 4, 0, 90), "n_rank=4 not in [1, n_videos=3]"),
    ((3, 60, 1, 20, 1, 0, 1), "max_v_l=1"),
    ((3, 60, 1, 20, 1, 2, 90), "CONE_SESSION_CERTIFIED libraries are not supported"),
    ((3, 60, 1, 20, 1, 1, 90), "library_scan: CONE_SESSION_BF16 libraries are not supported"),
]


@pytest.mark.parametrize("case", range(len(SCAN_REFUSALS)))
def test_the_scan_refuses_by_name_with_every_device_pointer_null(case):
    """Before a table, an output, the workspace or the handle is looked at: all of them are NULL here."""
    from cone_amd import _lib
    lib = _lib.load()
    (V, total_hb, nq, K, n_rank, flags, W), want = SCAN_REFUSALS[case]
    handle, p = _handle(flags), _lib.SessionParams(W, 20, 0.5333, 0.5, 100, 5)
    rc = lib.cone_library_scan(None, ctypes.byref(handle), None, None, None, V, total_hb, None, nq, K, n_rank, ctypes.byref(p),
                               None, None, None, None, None, 0, None)
    msg = lib.cone_last_error().decode()
    assert rc == -1 and want in msg and msg.startswith("library_scan: "), msg
    if W >= 2:      # (the size entry knows no window length)
        assert lib.cone_library_scan_workspace(ctypes.byref(handle), V, total_hb, nq, K, n_rank) == 0
        assert want in lib.cone_last_error().decode()


def test_a_scan_that_passes_the_host_checks_then_misses_its_pointers():
    from cone_amd import _lib
    lib = _lib.load()
    handle, p = _handle(), _lib.SessionParams(90, 20, 0.5333, 0.5, 100, 5)
    rc = lib.cone_library_scan(None, ctypes.byref(handle), None, None, None, 3, 60, None, 4, 20, 2, ctypes.byref(p),
                               None, None, None, None, None, 0, None)
    assert rc == -1 and lib.cone_last_error().decode() == "library_scan: null argument"
    n = lib.cone_library_scan_workspace(ctypes.byref(handle), 3, 60, 4, 20, 2)
    assert n >= 2 * 4 * 60 * 4 + 4 * 3 * 4 and n % 256 == 0             # two planes and best, nothing per frame


# the pairs' refusals of cone_library_localize, then the ranked entry's own: (lens, ctx, row0, K, pair_query, pair_slot, flags)
RANKED_REFUSALS = [
    (([], [], [], 20, [], [], 0), "nq=0 not in [1, 64]"),
    (([5, 21], [900, 900], [0, 0], 20, [0, 0], [0, 0], 0), "tok_len[1]=21 not in [1, max_q_l=20]"),
    (([5, 5], [900, 0], [0, 900], 20, [0, 0], [0, 1], 0), "q_ctx_l[1]=0 < 1"),
    (([5, 5], [900, 900], [0, 9101], 20, [0, 0], [0, 1], 0), "q_row0[1] + q_ctx_l[1] = 10001 > capacity=10000"),
    (([5, 5, 5], [900, 900, 91], [0, 0, 900], 20, [0, 1, 2], [0, 0, 1], 0), "K=20 not in [1, min(num_window=4, 256)] for query 2"),
    (([5], [900], [0], 20, [0], [0], 2), "CONE_SESSION_CERTIFIED libraries are not supported"),
    (([5], [900], [0], 20, [0], [0], 1), "library_localize_ranked: CONE_SESSION_BF16 libraries are not supported"),
    (([5], [900], [0], 21, [0], [0], 0), "K=21 not in [1, scan_K=20]"),
    (([5, 5], [900, 900], [0, 0], 20, [0, 3], [0, 0], 0), "pair_query[1]=3 not in [0, scan_nq=3)"),
    (([5, 5], [900, 900], [0, 0], 20, [0, -1], [0, 0], 0), "pair_query[1]=-1 not in [0, scan_nq=3)"),
    (([5, 5], [900, 900], [0, 0], 20, [0, 2], [7, 0], 0), "pair_slot[0]=7 not in [0, scan_n_videos=7)"),
]


@pytest.mark.parametrize("case", range(len(RANKED_REFUSALS)))
def test_the_ranked_query_half_refuses_by_name_with_every_device_pointer_null(case):
    from cone_amd import _lib
    lib = _lib.load()
    (lens, ctx, row0, K, pq, ps, flags), want = RANKED_REFUSALS[case]
    handle, p = _handle(flags), _lib.SessionParams(90, 20, 0.5333, 0.5, 100, 5)
    rc = lib.cone_library_localize_ranked(None, ctypes.byref(handle), _i32(row0), _i32(ctx), None, _i32(lens), len(lens), None, K,
                                          ctypes.byref(p), _i32(pq), _i32(ps), None, None, 3, 7, 20, None, None, None, 0, None)
    msg = lib.cone_last_error().decode()
    assert rc == -1 and want in msg and msg.startswith("library_localize_ranked: "), msg
    if "scan_" not in want:     # (the size entry knows the pairs and the library, not the scan)
        n = lib.cone_library_localize_ranked_workspace(None, ctypes.byref(handle), _i32(row0), _i32(ctx), _i32(lens), len(lens), K,
                                                       ctypes.byref(p))
        assert n == 0 and want in lib.cone_last_error().decode()


# ------------------------------------------------------------------------------------------------ the table
def _check_table(videos, S):
    from cone_amd.library import scan_table
    order, row0, ctx, hb_off = scan_table(videos, S)
    want_order, units = R.table_model(videos, S)
    assert list(order) == want_order
    assert row0.dtype == np.int64 and ctx.dtype == np.int32 and hb_off.dtype == np.int64 and len(hb_off) == len(videos) + 1
    assert [(int(row0[s]), int(ctx[s])) for s in range(len(videos))] == [videos[i] for i in want_order]
    assert hb_off[0] == 0 and int(hb_off[-1]) == len(units) == sum(-(-n // S) for _, n in videos)
    # every unit g of the flat list: slot = the last one with hb_off <= g (the kernel's search), h = g - hb_off[slot]
    for g, (slot, h, first, rows) in enumerate(units):
        s = int(np.searchsorted(hb_off, g, side="right")) - 1
        assert (s, g - int(hb_off[s])) == (slot, h)
        assert first == int(row0[s]) + h * S and rows == min(S, int(ctx[s]) - h * S) and rows >= 1
    # no unit holds a row of another video, and no row of a hole
    owned = set()
    for slot, h, first, rows in units:
        lo, n = int(row0[slot]), int(ctx[slot])
        assert lo <= first and first + rows <= lo + n
        owned.update(range(first, first + rows))
    assert owned == {r for lo, n in videos for r in range(lo, lo + n)}


@pytest.mark.parametrize("S", [45, 62])
def test_scan_table_follows_the_first_principles_model(S):
    """The issue's lengths at S = 45 (and at the odd window's S = 62): adjacent without a gap, with gaps, shuffled input order."""
    _check_table(R.stacked(R.TABLE_LENGTHS), S)
    _check_table(R.stacked(R.TABLE_LENGTHS, gaps=[0, 1, 0, 44, 45, 0, 7, 3]), S)
    _check_table(R.stacked(R.TABLE_LENGTHS[::-1], gaps=[5] * 8)[::-1], S)
    rng = np.random.default_rng(S)
    shuffled = R.stacked([int(n) for n in rng.integers(1, 200, 40)], gaps=[int(n) for n in rng.integers(0, 3, 40)])
    _check_table([shuffled[i] for i in rng.permutation(40)], S)
    _check_table([(123, 1)], S)


def test_scan_table_after_remove_and_add_into_the_hole_and_for_a_subset():
    from cone_amd.library import RowRanges, scan_table
    rows, videos = RowRanges(2000), {}
    for name, n in zip("abcdefgh", R.TABLE_LENGTHS):
        videos[name] = (rows.take(n), n)
    for name in ("c", "f"):                                     # 45 and 90 rows free
        rows.release(*videos.pop(name))
    videos["i"] = (rows.take(46), 46)                           # first fit: into f's hole, 44 rows stay free behind it
    videos["j"] = (rows.take(45), 45)                           # exactly c's hole: adjacent to both neighbours
    assert videos["i"][0] == 1 + 44 + 45 + 46 + 89 and videos["j"][0] == 1 + 44
    _check_table(list(videos.values()), 45)
    _check_table([videos[k] for k in ("h", "a", "j")], 45)      # a subset, given out of order
    order, row0, _, hb_off = scan_table([videos[k] for k in ("h", "a", "j")], 45)
    assert list(order) == [1, 2, 0] and int(hb_off[-1]) == 1 + 1 + 20
    with pytest.raises(ValueError, match="share arena rows"):
        scan_table([(0, 10), (9, 5)], 45)
    with pytest.raises(ValueError):
        scan_table([(0, 0)], 45)


# ------------------------------------------------------------------------------------------------ the models
@pytest.mark.parametrize("name", R.FAMILIES)
def test_the_algorithm_model_equals_the_definition_on_every_family(name):
    """Flat half-block planes + windows from two planes == the reference's window definition on each video alone."""
    arena, videos, cls, W = R.family(name)
    for K in (1, 30):
        want = R.scan_truth(arena, videos, cls, W, K, len(videos))
        assert R.same_scan(R.scan_algorithm(arena, videos, cls, W, K, len(videos)), want), (name, K)
        assert (want["widx"][..., 0] >= 0).all()


def test_the_families_hold_what_their_names_say():
    arena, videos, cls, W = R.family("seam")
    t = R.scan_truth(arena, videos, cls, W, 20, 3)
    assert videos[1][0] == videos[0][0] + videos[0][1]                                  # adjacent, no gap
    assert t["wval"][0, 0, 0] == pytest.approx(3.0) and t["wval"][0, 1, 0] == pytest.approx(6.0)
    assert t["widx"][0, 0, 0] == 1 and t["widx"][0, 1, :2].tolist() == [0, 1]           # the last row: windows 1 and 2; the first: 0 and 1
    arena, videos, cls, W = R.family("half_first")
    t = R.scan_truth(arena, videos, cls, W, 20, 3)
    assert W == 125 and t["wval"][0, 1, :3].tolist() == pytest.approx([3.0] * 3) and t["widx"][0, 1, :3].tolist() == [1, 2, 3]
    arena, videos, cls, W = R.family("twins")
    t = R.scan_truth(arena, videos, cls, W, 20, 4)
    assert np.array_equal(t["wval"][:, 1], t["wval"][:, 3]) and t["rank_slot"][0, :2].tolist() == [1, 3]
    arena, videos, cls, W = R.family("flat")
    t = R.scan_truth(arena, videos, cls, W, 20, 3)
    assert t["widx"][0, 1, :9].tolist() == list(range(9)) and len(set(t["wval"][0, 1, :9].tolist())) == 1
    arena, videos, cls, W = R.family("all_nan")
    t = R.scan_truth(arena, videos, cls, W, 4, 3)
    assert t["widx"][0, 1].tolist() == [0, 1, 2, 3] and (t["wval"][:, 1] == -np.inf).all() and t["rank_slot"][0, 2] == 1
    arena, videos, cls, W = R.family("nan_row")
    assert np.isnan(arena[videos[1][0] + 45]).all() and np.isfinite(R.scan_truth(arena, videos, cls, W, 6, 3)["wval"][:, 1]).all()


def test_which_family_catches_which_planted_error():
    """The power of the case list: every planted error is told from the definition by the families named for it."""
    table = {}
    for planted in R.PLANTED:
        table[planted] = []
        for name in R.FAMILIES:
            arena, videos, cls, W = R.family(name)
            V = len(videos)
            if not R.same_scan(R.scan_algorithm(arena, videos, cls, W, 20, V, planted), R.scan_truth(arena, videos, cls, W, 20, V)):
                table[planted].append(name)
    print("[library_search] planted error -> families that catch it:")
    for planted, names in table.items():
        print(f"    {planted:26s} {', '.join(names) or '-'}")
    for planted, names in R.CATCHES.items():
        assert set(names) <= set(table[planted]), (planted, table[planted])
    assert "seam" not in table["odd_term_from_next_video"]             # an even window has no odd term: W = 125 is needed
    assert table["ties_by_value"] == ["twins"]                         # only byte-identical videos tie across videos


def test_case_lists_cover_what_the_issue_names():
    assert R.TABLE_LENGTHS == (1, 44, 45, 46, 89, 90, 91, 900)
    assert set(R.KERNEL_LENGTHS) >= {1, 3, 4, 5, 15, 16, 17, 44, 45, 46, 89, 90, 91, 135, 333, 900}
    assert R.num_windows(R.LONG_VIDEO, 90) == 1101 > 1024
    assert R.WINDOWS == (90, 125) and R.N_VIDEOS == (1, 2, 7, 65, 300) and R.N_QUERIES == (1, 4, 5, 64) and R.TOPK == (1, 20, 30)


# ------------------------------------------------------------------------------------------------ the wrapper
def _bare_library(videos):
    from cone_amd.library import VideoLibrary
    lib = object.__new__(VideoLibrary)         # no handle, no arena, no GPU: the refusals and the empty answers come first
    lib.max_q_l = 20
    lib._videos = dict(videos)
    return lib


def test_search_refuses_and_answers_empty_before_any_gpu_work():
    lib = _bare_library({1: (0, 900, 20), 3: (900, 91, 4)})
    q = lambda n: (torch.zeros(n, 768), torch.zeros(256))
    for call in (lib.rank_videos, lib.search):
        with pytest.raises(ValueError, match="unknown or removed video id 2"):
            call([q(5)], videos=[1, 2])
        with pytest.raises(ValueError, match="video id 3 is listed more than once"):
            call([q(5)], videos=[3, 1, 3])
        with pytest.raises(ValueError, match="query has 21 tokens > max_q_l=20"):
            call([q(5), q(21)])
        with pytest.raises(ValueError, match="query has 0 tokens"):
            call([q(0)], videos=[])
        with pytest.raises(ValueError, match="n_videos=0 < 1"):
            call([q(5)], n_videos=0)
        assert call([q(5), q(7)], videos=[]) == [[], []]            # nothing to search: an empty list per query
        assert call([q(5)], videos=iter(())) == [[]]
        assert call([]) == []
    empty = _bare_library({})
    assert empty.rank_videos([q(5)]) == [[]] and empty.search([q(5), q(1)], n_videos=3) == [[], []]


def test_n_videos_is_clamped_to_the_videos_searched(monkeypatch):
    """The scans are stubbed: what reaches them is the clamped n_rank, the table of the subset and chunks of at most 64."""
    from cone_amd import library
    lib = _bare_library({i: (100 * i, 100, 4) for i in range(1, 8)})
    seen = []
    monkeypatch.setattr(library.VideoLibrary, "_check_live", lambda self: None)
    monkeypatch.setattr(library.VideoLibrary, "_table", lambda self, subset, ids: (list(ids), None, None, None, 0))

    def scan(self, table, queries, n_rank):
        seen.append((len(table[0]), len(queries), n_rank))
        rank = torch.zeros(2, len(queries), n_rank, dtype=torch.int32)
        rank[0] = torch.arange(n_rank, dtype=torch.int32)
        rank[1] = torch.full((n_rank,), 0.5).view(torch.int32)
        return None, None, rank
    monkeypatch.setattr(library.VideoLibrary, "_scan", scan)
    q = (torch.zeros(5, 768), torch.zeros(256))
    assert lib.rank_videos([q], n_videos=3) == [[(1, 0.5), (2, 0.5), (3, 0.5)]]
    assert len(lib.rank_videos([q], n_videos=50)[0]) == 7 and len(lib.rank_videos([q])[0]) == 7
    assert lib.rank_videos([q], n_videos=50, videos=[5, 2]) == [[(5, 0.5), (2, 0.5)]]
    assert len(lib.rank_videos([q] * 130, n_videos=2)) == 130
    assert seen == [(7, 1, 3), (7, 1, 7), (7, 1, 7), (2, 1, 2), (7, 64, 2), (7, 64, 2), (7, 2, 2)]
