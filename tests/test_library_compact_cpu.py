"""Library maintenance, the part that needs no GPU: the C ABI's declarations and binding, the refusals that fire on the host
before any pointer is read, the planner (compaction_moves / plan_steps) against the arena model of tests/move_refs.py -- with
a table of which named case catches which planted error --, and the wrapper's behaviour before any GPU work."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import move_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "cone_hip.h")) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ header and binding
def test_header_binding_and_library_agree_on_the_move_entries():
    from cone_amd import _lib
    hdr = _header()
    assert re.search(r"#define\s+CONE_HIP_ABI_VERSION\s+8\b", hdr)
    declared = set(re.findall(r"\b(cone_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in R.NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert declared == set(_lib.EXPORTS)
    assert lib.cone_abi_version() == 8
    at = hdr.index("library maintenance (additive in ABI 8)")
    assert hdr.index("library search (additive in ABI 8)") < at < hdr.index("metrics on the device")
    between = hdr[hdr.index("video libraries (additive in ABI 8)"):hdr.index("library search (additive in ABI 8)")]
    assert between.count("(additive in ABI 8)") == 1                    # nothing between the libraries and the search
    section = hdr[at:hdr.index("metrics on the device")]
    for name in R.NEW_SYMBOLS:
        assert name + "(" in section
    assert section.count("run_on_video/cone_localizator.py:121-221") >= 2
    for word in ("the bits they had", "predict_moment", "CONE_SESSION_BF16", "CONE_SESSION_CERTIFIED", "skipped whole", "DEVICE table"):
        assert word in section, word


def test_the_structs_stay_and_the_signatures_mirror_the_header():
    from cone_amd import _lib
    hdr = _header()
    assert ctypes.sizeof(_lib.Library) == 72 and len(_lib.Library._fields_) == 10
    assert ctypes.sizeof(_lib.Session) == 80 and ctypes.sizeof(_lib.SessionParams) == 32
    for name, n in dict(cone_library_move_stage_bytes=2, cone_library_move_rows=13).items():
        assert len(_lib._SIGNATURES[name][1]) == n, name
        decl = re.search(r"\b%s\(([^;]*)\);" % name, hdr).group(1)
        assert decl.count(",") + 1 == n, name
    assert _lib._SIGNATURES["cone_library_move_stage_bytes"][0] is ctypes.c_size_t
    with open(os.path.join(ROOT, "cone_amd", "csrc", "library_move.hip")) as f:
        src = f.read()
    assert int(re.search(r"constexpr int MOVE_TILE = (\d+);", src).group(1)) == R.TILE        # the constant the case list is cut to


# ------------------------------------------------------------------------------------------------ host refusals
def _handle(flags=0, capacity=10000, fake=0, **kw):
    """A host struct whose device pointers are NULL (or ``fake``: never dereferenced on the host)."""
    from cone_amd import _lib
    p = fake or None
    f = dict(model=None, capacity=capacity, flags=flags, v_dim=256, hidden_dim=256, vid_norm=p, adapted=None if flags & 1 else p,
             adapted_bf16=p if flags & 1 else None, vproj=p, qkv_vid=p)
    f.update(kw)
    return _lib.Library(*(f[k] for k, _ in _lib.Library._fields_))


# (n_moves, total_rows, row_begin, row_end, src flags, dst flags) -> what the message must hold
MOVE_REFUSALS = [
    ((0, 10, 0, 10, 0, 0), "n_moves=0 < 1"),
    ((-3, 10, 0, 10, 0, 0), "n_moves=-3 < 1"),
    ((4, 3, 0, 3, 0, 0), "total_rows=3 < n_moves=4"),
    ((2, 10, -1, 10, 0, 0), "rows [-1, 10) not in 0 <= begin < end <= total_rows=10"),
    ((2, 10, 5, 5, 0, 0), "rows [5, 5) not in 0 <= begin < end <= total_rows=10"),
    ((2, 10, 0, 11, 0, 0), "rows [0, 11) not in 0 <= begin < end <= total_rows=10"),
    ((2, 10, 0, 10, 2, 2), "CONE_SESSION_CERTIFIED libraries are not supported"),
    ((2, 10, 0, 10, 0, 2), "CONE_SESSION_CERTIFIED libraries are not supported"),
]


@pytest.mark.parametrize("case", range(len(MOVE_REFUSALS)))
def test_the_move_refuses_by_name_with_every_device_pointer_null(case):
    """Before a table, the stage, an arena or the handle is looked at: all of them are NULL here."""
    from cone_amd import _lib
    lib = _lib.load()
    (n_moves, total, begin, end, fs, fd), want = MOVE_REFUSALS[case]
    src, dst = _handle(fs), _handle(fd)
    rc = lib.cone_library_move_rows(None, ctypes.byref(src), ctypes.byref(dst), None, None, None, n_moves, total, begin, end, None, 0, None)
    msg = lib.cone_last_error().decode()
    assert rc == -1 and want in msg and msg.startswith("library_move: "), msg


def test_a_move_that_passes_the_host_values_is_refused_for_what_it_misses():
    """The later refusals in their order; the pointers are fakes that the host never reads through."""
    from cone_amd import _lib
    lib = _lib.load()
    m, other, tab = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)

    def call(src, dst, model=m, table=tab, total=10, stage=None, stage_bytes=0):
        rc = lib.cone_library_move_rows(model, ctypes.byref(src), ctypes.byref(dst), table, table, table, 2, total, 0, total, stage,
                                        stage_bytes, None)
        return rc, lib.cone_last_error().decode()

    ok = lambda **kw: _handle(fake=0x10000, **{"model": 0x1000, **kw})
    assert call(_handle(), _handle(), model=None) == (-1, "library_move: null argument")
    assert call(ok(), ok(), table=None) == (-1, "library_move: null argument")
    rc, msg = call(ok(capacity=9), ok())
    assert rc == -1 and "total_rows=10 > capacity=9 of the source" in msg
    for kw in (dict(flags=1), dict(v_dim=512), dict(hidden_dim=128), dict(model=0x2000)):
        rc, msg = call(ok(), ok(**kw))
        assert rc == -1 and "library_move: src and dst differ in model, flags or row widths" in msg, (kw, msg)
    rc, msg = call(ok(), ok(qkv_vid=None))                                          # a long-window arena and one with the layer-0 rows
    assert rc == -1 and "library_move: src and dst differ in which planes are present" in msg
    rc, msg = call(ok(), ok(), model=other)
    assert rc == -1 and "library_move: the libraries were opened with another handle" in msg
    rc, msg = call(ok(), ok(vproj=None))
    assert rc == -1 and "misses a region" in msg
    rc, msg = call(ok(), ok(), stage=ctypes.c_void_p(0x20010), stage_bytes=1 << 30)
    assert rc == -1 and "library_move: the staging buffer must be 256-B aligned" in msg
    need = lib.cone_library_move_stage_bytes(ctypes.byref(ok()), 10)
    rc, msg = call(ok(), ok(), stage=ctypes.c_void_p(0x20000), stage_bytes=need - 1)
    assert rc == -3 and f"library_move: staging buffer too small ({need - 1} < {need})" in msg


def test_stage_bytes_is_the_sum_of_the_present_planes_each_256_aligned():
    from cone_amd import _lib
    lib = _lib.load()
    size = lambda h, n: lib.cone_library_move_stage_bytes(ctypes.byref(h), n)
    fp32, bf16 = _handle(fake=0x10000), _handle(flags=1, fake=0x10000)
    long_, small = _handle(fake=0x10000, qkv_vid=None), _handle(fake=0x10000, hidden_dim=128)
    assert size(fp32, 1) == 1024 + 1024 + 1024 + 3072 and size(fp32, 900) == 900 * 6144            # 6 KiB per clip
    assert size(bf16, 3) == 3 * (1024 + 512 + 1024 + 3072) and size(bf16, 1) == 1024 + 512 + 1024 + 3072
    assert size(long_, 7) == 7 * 3072
    assert size(small, 1) == 1024 + 1024 + 512 + 1536 and size(small, 3) == 3072 + 3072 + 1536 + 4608
    odd = _handle(fake=0x10000, v_dim=32, hidden_dim=32)                                # 128-B rows: the planes are padded to 256 B
    assert size(odd, 1) == 256 * 3 + 512 and size(odd, 3) == 512 * 3 + 1280
    for h, n, want in ((fp32, 0, "n_rows=0 not in [1, 2^31)"), (_handle(flags=2, fake=0x10000), 5, "CONE_SESSION_CERTIFIED"),
                       (_handle(), 5, "misses a region")):
        assert size(h, n) == 0 and want in lib.cone_last_error().decode()
    assert lib.cone_library_move_stage_bytes(None, 5) == 0 and "null argument" in lib.cone_last_error().decode()


# ------------------------------------------------------------------------------------------------ the planner
def _check_plan(capacity, videos, stage_rows):
    from cone_amd.library import compaction_moves, plan_steps
    moves = compaction_moves(videos)
    assert moves == R.truth_moves(videos)                                                   # arena order, running sum
    assert [m[0] for m in moves] == sorted(m[0] for m in moves) and [m[1] for m in moves] == sorted(m[1] for m in moves)
    moving = [m for m in moves if m[0] != m[1]]
    steps = plan_steps(moves, stage_rows)
    total = sum(n for _, _, n in moving)
    assert [b for b, _, _ in steps] == [0] * bool(steps) + [e for _, e, _ in steps][:-1]     # the steps tile [0, total)
    assert (steps[-1][1] if steps else 0) == total and all(b < e for b, e, _ in steps)
    kinds = [staged for _, _, staged in steps]
    assert kinds == sorted(kinds, reverse=True)                                             # a staged prefix, a direct suffix
    for i, (b, e, staged) in enumerate(steps):
        src, dst = R.step_sets(moving, b, e)
        if staged:
            assert e - b <= stage_rows
        else:
            assert not (src & dst)
        later = set().union(*(R.step_sets(moving, b2, e2)[0] for b2, e2, _ in steps[i + 1:])) if i + 1 < len(steps) else set()
        assert not (dst & later)                                                            # no step overwrites what a later one reads
    planes = R.arena(capacity)
    want = R.memmove_truth(planes, moves)
    assert R.same(R.run_plan(planes, moves, steps), want)
    return moves, steps


@pytest.mark.parametrize("name", list(R.CASES))
def test_the_plan_of_every_named_case_equals_sequential_memmove(name):
    capacity, videos, stage_rows = R.CASES[name]
    moves, steps = _check_plan(capacity, videos, stage_rows)
    if name == "hole_end":
        assert steps == [] and all(s == d for s, d, _ in moves)
    if name == "mixed_plan":
        assert [s for _, _, s in steps] == [True, True, False, False, False] and steps[1][:2] == (16, 32) and steps[2][:2] == (32, 102)
    if name == "shift_700_by_1":
        assert steps == [(0, 700, True)]
    if name == "stage_below_video":
        assert steps == [(0, 30, True), (30, 60, True), (60, 90, True), (90, 100, True)]
    if name == "three_chained":
        for (_, d, n), (s0, _, n0) in zip(moves[1:], moves[:-1]):
            assert s0 <= d and d + n <= s0 + n0                                              # dst inside the predecessor's src
    if name.startswith("tile_"):
        assert videos[0][1] in (R.TILE - 1, R.TILE, R.TILE + 1, 2 * R.TILE + 1)


def test_random_histories_compact_like_sequential_memmove():
    rng = np.random.default_rng(20)
    some_moved = 0
    for trial in range(300):
        rows, videos = R.history(rng)
        stage_rows = int(rng.choice([1, 2, 7, 16, 33, 60, 400]))
        moves, steps = _check_plan(rows.capacity, videos, stage_rows)
        some_moved += bool(steps)
        assert sum(n for _, n in videos) + rows.free == rows.capacity
    assert some_moved > 200


def test_the_planner_refuses_what_is_no_compaction():
    from cone_amd.library import compaction_moves, plan_steps
    with pytest.raises(ValueError, match="rows of its own"):
        compaction_moves([(0, 10), (9, 5)])
    with pytest.raises(ValueError):
        compaction_moves([(0, 0)])
    with pytest.raises(ValueError, match="stage_rows=0 < 1"):
        plan_steps([(5, 0, 3)], 0)
    for bad in ([(0, 5, 3)], [(5, 0, 3), (20, 4, 3)], [(9, 0, 3), (11, 3, 3)]):         # upward; a gap in dst; a shrinking gap
        with pytest.raises(ValueError, match="not the moves of a compaction"):
            plan_steps(bad, 4)
    assert plan_steps([], 4) == [] and plan_steps([(0, 0, 5), (5, 5, 2)], 4) == []


def test_the_direct_model_fails_on_overlapping_sets():
    planes = R.arena(20)
    with pytest.raises(R.Overlap):
        R.apply_step(planes, [(1, 0, 10)], 0, 10, False)
    R.apply_step(planes, [(10, 0, 10)], 0, 10, False)


def test_which_named_case_catches_which_planted_error():
    from cone_amd.library import compaction_moves, plan_steps
    table = {}
    for planted in R.PLANTED:
        table[planted] = []
        for name, (capacity, videos, stage_rows) in R.CASES.items():
            moves = compaction_moves(videos)
            steps = plan_steps(moves, stage_rows)
            planes = R.arena(capacity)
            if not R.same(R.run_plan(planes, moves, steps, planted), R.memmove_truth(planes, moves)):
                table[planted].append(name)
    print("[library_compact] planted error -> named cases that catch it:")
    for planted, names in table.items():
        print(f"    {planted:22s} {', '.join(names) or '-'}")
    for planted, names in R.CATCHES.items():
        assert set(names) <= set(table[planted]), (planted, table[planted])
    assert "one_row_shift_1" not in table["direct_where_overlap"]      # a shift by a whole video overlaps nothing
    assert "hole_end" not in set().union(*table.values())              # nothing moves: nothing can go wrong
    assert set(R.CASES) >= {"tile_15", "tile_16", "tile_17", "tile_33", "one_row_shift_1", "shift_700_by_1", "three_chained",
                            "stage_below_video", "stage_video_minus_1", "stage_video_plus_1", "hole_front", "hole_middle", "hole_end",
                            "mixed_plan"}


# ------------------------------------------------------------------------------------------------ row ownership
def test_row_ranges_hold_one_hole_at_the_end_after_a_compaction():
    from cone_amd.library import RowRanges
    rng = np.random.default_rng(3)
    for _ in range(50):
        rows, videos = R.history(rng)
        used = sum(n for _, n in videos)
        rows.compacted()
        assert rows.holes == ([(used, rows.capacity - used)] if used < rows.capacity else []) and rows.free == rows.capacity - used
        if rows.free:
            assert rows.largest == rows.free and rows.take(rows.free) == used and rows.holes == []
    full = RowRanges(10)
    full.take(10)
    full.compacted()
    assert full.holes == []


# ------------------------------------------------------------------------------------------------ the wrapper
def _stub_library(capacity, videos):
    """A library on a stub localizer: no handle, no arena, no GPU -- what the wrapper decides before any GPU work."""
    from cone_amd.library import RowRanges, VideoLibrary
    handle = SimpleNamespace(value=1)
    model = SimpleNamespace(_handle=handle, _h=lambda: handle, _check_dim=lambda *a: None)
    lib = object.__new__(VideoLibrary)
    lib._loc = SimpleNamespace(args=SimpleNamespace(v_appear_feat_dim=256, v_motion_feat_dim=256, max_v_l=90, topk_window=20),
                               localizator=model, device="cpu")
    lib._handle_obj, lib._handle_value, lib._open = handle, 1, True
    lib.max_q_l, lib._rows, lib._videos, lib._next_id, lib._scan_cache = 20, RowRanges(capacity), {}, 1, None
    for row0, n in videos:
        rows = lib._rows.take(n)
        assert rows == row0
        lib._videos[lib._next_id] = (row0, n, 2)
        lib._next_id += 1
    return lib


def test_the_wrapper_refuses_before_any_gpu_work():
    lib = _stub_library(400, [(0, 100), (100, 60), (160, 200)])
    lib.remove(2)
    assert lib.free_clips == 100 and lib.largest_free == 60
    with pytest.raises(ValueError, match="resize: capacity_clips=299 is smaller than the 300 resident clips"):
        lib.resize(299)
    with pytest.raises(ValueError, match=r"no free range of 61 clips: the largest free hole has 60 \(100 of 400 clips are free"):
        lib.add(torch.zeros(61, 256))                                   # the default: as before, the existing message
    with pytest.raises(ValueError, match="no free range of 101 clips: the largest free hole has 60"):
        lib.add(torch.zeros(101, 256), compact=True)                    # more than is free in total: compacting would not help
    assert lib._videos == {1: (0, 100, 2), 3: (160, 200, 2)} and lib._rows.holes == [(100, 60), (360, 40)]
    lib.close()
    assert lib.largest_free == 0
    with pytest.raises(RuntimeError, match="closed"):
        lib.compact()
    with pytest.raises(RuntimeError, match="closed"):
        lib.resize(1000)


def test_a_compact_library_launches_nothing():
    lib = _stub_library(400, [(0, 100), (100, 60)])                      # no model, no arena: any launch would fail here
    assert lib.compact() == 0 and lib._rows.holes == [(160, 240)]
    assert _stub_library(50, []).compact() == 0
