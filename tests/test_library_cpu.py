"""Video libraries, the part that needs no GPU: the C ABI's declarations and binding, the refusals that fire on the host before
any pointer is read, row ownership against a first-principles model, and the wrapper's planning of calls."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import library_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "cone_hip.h")) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ header and binding
def test_header_binding_and_library_agree_on_the_new_entries():
    from cone_amd import _lib
    hdr = _header()
    assert re.search(r"#define\s+CONE_HIP_ABI_VERSION\s+8\b", hdr)
    declared = set(re.findall(r"\b(cone_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in R.NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert declared == set(_lib.EXPORTS)
    assert lib.cone_abi_version() == 8
    # the section sits between the sessions and the device metrics, cites the reference site per entry, states the contract
    at = hdr.index("video libraries (additive in ABI 8)")
    assert hdr.index("video sessions (additive in ABI 8)") < at < hdr.index("metrics on the device")
    section = hdr[at:hdr.index("metrics on the device")]
    assert section.count("run_on_video/cone_localizator.py:121-221") >= 5
    assert "the bits" in section and "predict_moment" in section and "CONE_SESSION_CERTIFIED" in section


def test_binding_mirrors_the_declared_struct_and_signatures():
    from cone_amd import _lib
    hdr = _header()
    body = re.search(r"typedef struct \{([^}]*)\} cone_library;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f for decl in body.split(";") for f in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert fields == [n for n, _ in _lib.Library._fields_]
    assert fields == ["model", "capacity", "flags", "v_dim", "hidden_dim", "vid_norm", "adapted", "adapted_bf16", "vproj", "qkv_vid"]
    assert ctypes.sizeof(_lib.Library) == 72
    assert ctypes.sizeof(_lib.Session) == 80 and ctypes.sizeof(_lib.SessionParams) == 32        # the sessions' stay as they are
    n_args = dict(cone_library_arena_bytes=3, cone_library_open=6, cone_library_add_workspace=2, cone_library_add=8,
                  cone_library_query_layout=17, cone_library_localize_workspace=8, cone_library_localize=15)
    for name, n in n_args.items():
        assert len(_lib._SIGNATURES[name][1]) == n, name
        decl = re.search(r"\b%s\(([^;]*)\);" % name, hdr).group(1)
        assert decl.count(",") + 1 == n, name
    for name in ("cone_library_arena_bytes", "cone_library_add_workspace", "cone_library_localize_workspace"):
        assert _lib._SIGNATURES[name][0] is ctypes.c_size_t


# ------------------------------------------------------------------------------------------------ host refusals
def _i32(v):
    return (ctypes.c_int32 * max(len(v), 1))(*v)


# (token lengths, q_ctx_l, q_row0, K) -> what the message must hold; capacity 10000 where there is one
REFUSALS = [
    (([], [], [], 20), "nq=0 not in [1, 64]"),
    (([3] * 65, [900] * 65, [0] * 65, 20), "nq=65 not in [1, 64]"),
    (([5, 0], [900, 900], [0, 0], 20), "tok_len[1]=0 not in [1, max_q_l=20]"),
    (([5, 20, 21], [900] * 3, [0] * 3, 20), "tok_len[2]=21 not in [1, max_q_l=20]"),
    (([5, 5], [900, 0], [0, 900], 20), "q_ctx_l[1]=0 < 1"),
    (([5, 5], [900, 900], [0, -1], 20), "q_row0[1]=-1 < 0"),
    (([5, 5, 5], [900, 900, 91], [0, 0, 900], 20), "K=20 not in [1, min(num_window=4, 256)] for query 2"),
    (([5], [900], [0], 0), "K=0 not in [1, min(num_window=21, 256)] for query 0"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_both_entries_refuse_by_name_with_null_outputs(case):
    """Before an output pointer, the arena or the handle is looked at: every device argument is NULL here."""
    from cone_amd import _lib
    lib = _lib.load()
    (lens, ctx, row0, K), want = REFUSALS[case]
    rc = lib.cone_library_query_layout(_i32(lens), _i32(row0), _i32(ctx), len(lens), 20, K, 5, 90, *([None] * 8), None)
    assert rc == -1 and want in lib.cone_last_error().decode(), lib.cone_last_error()
    assert "library_query_layout: " in lib.cone_last_error().decode()
    handle = _lib.Library(None, 10000, 0, 256, 256, None, None, None, None, None)
    p = _lib.SessionParams(90, 20, 0.5333, 0.5, 100, 5)
    n = lib.cone_library_localize_workspace(None, ctypes.byref(handle), _i32(row0), _i32(ctx), _i32(lens), len(lens), K, ctypes.byref(p))
    assert n == 0 and want in lib.cone_last_error().decode(), lib.cone_last_error()
    assert "library_localize: " in lib.cone_last_error().decode()


def test_row_ranges_are_checked_against_what_each_entry_knows():
    from cone_amd import _lib
    lib = _lib.load()
    p = _lib.SessionParams(90, 20, 0.5333, 0.5, 100, 5)
    handle = _lib.Library(None, 1000, 0, 256, 256, None, None, None, None, None)
    size = lambda row0, ctx: lib.cone_library_localize_workspace(None, ctypes.byref(handle), _i32(row0), _i32(ctx), _i32([5] * len(ctx)),
                                                                 len(ctx), 2, ctypes.byref(p))
    assert size([0, 901], [900, 100]) == 0          # row0 + ctx_l = capacity + 1
    assert "q_row0[1] + q_ctx_l[1] = 1001 > capacity=1000" in lib.cone_last_error().decode()
    assert size([0, 900], [900, 100]) == 0          # the pairs are fine: the next refusal is the missing handle
    assert "library_localize: null argument" in lib.cone_last_error().decode()
    # the layout entry knows no capacity: rows are int32
    layout = lambda row0, ctx: lib.cone_library_query_layout(_i32([5]), _i32([row0]), _i32([ctx]), 1, 20, 2, 5, 90, *([None] * 8), None)
    assert layout(R.INT32_MAX - 99, 100) == -1
    assert "= 2147483648 not below 2^31" in lib.cone_last_error().decode()
    assert layout(R.INT32_MAX - 100, 100) == -1
    assert "library_query_layout: null argument" in lib.cone_last_error().decode()      # (only the outputs were missing)
    # a certified library is out of scope and says so
    assert lib.cone_library_arena_bytes(None, 1000, _lib.SESSION_CERTIFIED) == 0
    assert "CONE_SESSION_CERTIFIED libraries are not supported" in lib.cone_last_error().decode()
    handle.flags = _lib.SESSION_CERTIFIED
    assert size([0], [900]) == 0 and "CONE_SESSION_CERTIFIED libraries are not supported" in lib.cone_last_error().decode()
    arena = ctypes.create_string_buffer(512)
    assert lib.cone_library_open(ctypes.c_void_p(1), 1000, _lib.SESSION_CERTIFIED, arena, 512, ctypes.byref(handle)) == -1
    assert "library_open: CONE_SESSION_CERTIFIED libraries are not supported" in lib.cone_last_error().decode()


# ------------------------------------------------------------------------------------------------ the layout model
def test_layout_cases_cover_what_the_issue_names():
    assert {255, 256, 257} <= {sum(c[0]) for c in R.LAYOUT_CASES}
    assert {len(c[0]) for c in R.LAYOUT_CASES} >= {1, 2, 64}
    assert any(r + c == R.INT32_MAX for _, ctx, row0, _ in R.LAYOUT_CASES for c, r in zip(ctx, row0))
    for lens, ctx, row0, K in R.LAYOUT_CASES:
        assert len(lens) == len(ctx) == len(row0)
        assert all(1 <= K <= min(R.num_windows(c), 256) for c in ctx)
        m = R.layout_model(lens, ctx, row0, K)
        assert m["q_vid_off"].tolist() == row0 and m["q_ctx_l"].tolist() == ctx and m["tok_off"][-1] == sum(lens)
    assert [R.num_windows(c) for c in (1, 45, 46, 91, 333, 900, 6000)] == [2, 2, 3, 4, 9, 21, 135]


# ------------------------------------------------------------------------------------------------ row ownership
def test_first_fit_free_list_follows_the_model_on_the_scripted_sequence():
    from cone_amd.library import RowRanges
    rows, model, owned = RowRanges(R.ROW_CAPACITY), R.RowModel(R.ROW_CAPACITY), {}
    assert rows.free == rows.largest == R.ROW_CAPACITY
    seen = set()
    for op, name, n in R.ROW_SCRIPT:
        if op == "add":
            start = rows.take(n)
            assert start == model.take(n), (op, name, n)
            owned[name] = (start, n)
        elif op == "remove":
            rows.release(*owned[name])
            model.release(*owned.pop(name))
        else:
            assert model.take(n) is None
            with pytest.raises(ValueError) as e:
                rows.take(n)
            largest = max([h[1] for h in model.holes()], default=0)
            assert f"no free range of {n} clips" in str(e.value) and f"largest free hole has {largest}" in str(e.value)
        assert rows.holes == model.holes(), (op, name, n)                   # sorted, coalesced
        assert rows.free == int((~model.used).sum()) and rows.largest == max([h[1] for h in model.holes()], default=0)
        seen.add(op)
    assert seen == {"add", "remove", "refuse"}
    with pytest.raises(ValueError, match="not an owned range"):
        RowRanges(10).release(2, 3)
    with pytest.raises(ValueError):
        RowRanges(0)


def test_first_fit_free_list_follows_the_model_on_random_traffic():
    from cone_amd.library import RowRanges
    rng = np.random.default_rng(5)
    rows, model, owned = RowRanges(257), R.RowModel(257), []
    for _ in range(600):
        if owned and rng.random() < 0.45:
            r = owned.pop(int(rng.integers(len(owned))))
            rows.release(*r)
            model.release(*r)
        else:
            n = int(rng.integers(1, 60))
            want = model.take(n)
            if want is None:
                with pytest.raises(ValueError, match=f"no free range of {n} clips"):
                    rows.take(n)
            else:
                assert rows.take(n) == want
                owned.append((want, n))
        assert rows.holes == model.holes()


# ------------------------------------------------------------------------------------------------ the wrapper
def _bare_library(videos):
    from cone_amd.library import VideoLibrary
    lib = object.__new__(VideoLibrary)         # no handle, no arena, no GPU: the refusals come first
    lib.max_q_l = 20
    lib._videos = dict(videos)
    return lib


def test_bad_pairs_are_refused_before_any_gpu_work():
    lib = _bare_library({1: (0, 900, 20), 3: (900, 91, 4)})
    q = lambda n: (torch.zeros(n, 768), torch.zeros(256))
    with pytest.raises(ValueError, match="unknown or removed video id 2"):
        lib.predict_moments([(1, q(5)), (2, q(5))])
    with pytest.raises(ValueError, match="unknown or removed video id 'a'"):
        lib.predict_moment("a", q(5))
    with pytest.raises(ValueError, match="query has 21 tokens > max_q_l=20"):
        lib.predict_moments([(1, q(5)), (3, q(21))])
    with pytest.raises(ValueError, match="query has 21 tokens > max_q_l=20"):
        lib.predict_moment(3, q(21))
    with pytest.raises(ValueError, match="query has 0 tokens"):
        lib.predict_moment(3, q(0))
    with pytest.raises(ValueError, match="unknown or removed video id 2"):
        lib.remove(2)
    assert lib.predict_moments([]) == []


@pytest.mark.parametrize("n_pairs,seed", [(1, 0), (7, 1), (64, 2), (65, 3), (200, 4)])
def test_planned_calls_cover_every_pair_once_with_one_k_and_consecutive_videos(n_pairs, seed):
    from cone_amd.library import inverse_order, plan_calls
    rng = np.random.default_rng(seed)
    k_of_video = {v: (3, 4, 9, 20)[v % 4] for v in range(11)}      # 11 videos, window counts of 46 / 91 / 333 / >= 900 clips
    video_of = [int(v) for v in rng.integers(0, 11, n_pairs)]
    calls = plan_calls(video_of, [k_of_video[v] for v in video_of])
    flat = [i for _, idx in calls for i in idx]
    assert sorted(flat) == list(range(n_pairs))                                   # every pair once
    for K, idx in calls:
        assert 1 <= len(idx) <= 64
        assert {k_of_video[video_of[i]] for i in idx} == {K}                      # one K a call
        vids = [video_of[i] for i in idx]
        runs = [v for j, v in enumerate(vids) if j == 0 or v != vids[j - 1]]
        assert len(runs) == len(set(runs))                                        # a video's pairs are consecutive
        for v in set(vids):
            mine = [i for i in idx if video_of[i] == v]
            assert mine == sorted(mine)                                           # ... in the caller's order
    # at most one call per group is short of 64
    for K in {k for k, _ in calls}:
        sizes = [len(idx) for k, idx in calls if k == K]
        assert all(s == 64 for s in sizes[:-1])
    where = inverse_order(calls, n_pairs)
    assert [flat[w] for w in where] == list(range(n_pairs))                       # the inverse permutation restores the order
    with pytest.raises(ValueError):
        inverse_order(calls + [(3, [0])], n_pairs)
    with pytest.raises(ValueError):
        inverse_order(calls[:-1], n_pairs)
