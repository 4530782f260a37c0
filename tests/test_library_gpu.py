"""Video libraries on the GPU: every answer of a library is compared with ``==`` against ``CONELocalizator.predict_moment`` on
the same video and query -- no tolerances.  (A library re-sequences the launchers ``predict_moment`` calls, per video where
the window ranking is concerned and once for everything after it; it computes nothing new.)"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import library_refs as R
from cone_amd import synth

pytestmark = pytest.mark.gpu

POISON = 0x7EADBEEF
QNAN = 0x7FC00000            # the arena's fill in the isolation test: a quiet NaN in every fp32, one in every pair of bf16


# ------------------------------------------------------------------------------------------------ fixtures
_LOCS, _REFS = {}, {}


def _localizer(kind="default", **extra):
    """One localizer per checkpoint kind for the whole module (tests/test_session_gpu.py's kinds)."""
    from cone_amd.localizator import CONELocalizator, LOCALIZER_OPT
    key = (kind, tuple(sorted(extra.items())))
    if key not in _LOCS:
        kw = dict(default={}, txt_pos=dict(use_txt_pos=True), pre_norm=dict(pre_norm=True), general=dict(hidden_dim=128, nheads=4),
                  long=dict(max_v_l=300, topk_window=5))[kind]
        sd = synth.make_state_dict(SimpleNamespace(**dict(LOCALIZER_OPT, **kw)), 5)
        _LOCS[key] = CONELocalizator(state_dict={k: torch.from_numpy(v) for k, v in sd.items()}, **kw, **extra)
    return _LOCS[key]


def _video(ctx_l, seed=0):
    return torch.randn(ctx_l, 256, generator=torch.Generator().manual_seed(1000 + seed + ctx_l)) * 2


def _queries(lens, seed=0):
    g = torch.Generator().manual_seed(77 + seed)
    return [(torch.randn(n, 768, generator=g), torch.randn(256, generator=g)) for n in lens]


def _mixed_lens(Q):
    return [(1, 7, 20, 12, 3)[i % 5] for i in range(Q)]


def _reference(loc, tag, videos, pairs):
    """predict_moment per (video index, query) pair, computed once per tag and never changed."""
    key = (id(loc), tag)
    if key not in _REFS:
        _REFS[key] = [loc.predict_moment(videos[v], q) for v, q in pairs]
        assert all(len(r) >= 1 for r in _REFS[key])
    return _REFS[key]


def _count_readbacks(monkeypatch):
    calls = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (calls.append(1) if t.is_cuda else None, real(t, *a, **k))[1])
    return calls


# ------------------------------------------------------------------------------------------------ mixed videos
MIXED_CLIPS = (1, 45, 46, 91, 333, 900, 6000)


def test_mixed_videos_in_one_call_each_equal_predict_moment():
    """Window counts 2, 2, 3, 4, 9, 21, 135, so K = 2, 2, 3, 4, 9, 20, 20: four groups of K, runs of one to three queries."""
    loc = _localizer()
    assert [min(R.TOPK_WINDOW, R.num_windows(n)) for n in MIXED_CLIPS] == [2, 2, 3, 4, 9, 20, 20]
    videos = [_video(n) for n in MIXED_CLIPS]
    queries = _queries(_mixed_lens(21), seed=3)
    pairs = [(i % 7, q) for i, q in enumerate(queries)]                    # interleaved: every video gets three queries
    want = _reference(loc, "mixed", videos, pairs)
    with loc.open_library(sum(MIXED_CLIPS) + 10) as lib:
        ids = [lib.add(v) for v in videos]
        assert lib.free_clips == 10 and lib.nbytes > 0
        assert [lib._videos[i][2] for i in ids] == [2, 2, 3, 4, 9, 20, 20]
        got = lib.predict_moments([(ids[v], q) for v, q in pairs])
        assert len(got) == 21
        for i in range(21):
            assert got[i] == want[i], (i, MIXED_CLIPS[pairs[i][0]])
        back = lib.predict_moments([(ids[v], q) for v, q in reversed(pairs)])
        assert back == want[::-1]
        v, q = pairs[12]
        assert lib.predict_moment(ids[v], q) == want[12]


# ------------------------------------------------------------------------------------------------ one video inside a call
def _batch_case():
    loc = _localizer()
    videos = [_video(900, seed=3), _video(901, seed=4), _video(1500, seed=5)]            # K = 20 each
    queries = _queries(_mixed_lens(65), seed=11)
    return loc, videos, queries


@pytest.mark.parametrize("Q", [1, 4, 5, 9])
def test_queries_of_one_video_across_the_four_query_launch_seam(Q):
    """Q queries on one video between two other videos' queries: its run is cut into launches of 4, 4 + 1, 4 + 4 + 1."""
    loc, videos, queries = _batch_case()
    want0 = _reference(loc, "one-video", videos, [(0, q) for q in queries])
    want1 = _reference(loc, "neighbours", videos, [(1, queries[0]), (2, queries[1])])
    with loc.open_library(900 + 901 + 1500) as lib:
        ids = [lib.add(v) for v in videos]
        got = lib.predict_moments([(ids[1], queries[0])] + [(ids[0], q) for q in queries[:Q]] + [(ids[2], queries[1])])
        assert got[0] == want1[0] and got[-1] == want1[1]
        for i in range(Q):
            assert got[1 + i] == want0[i], (Q, i)


def test_65_pairs_cross_the_call_limit_with_one_read_back(monkeypatch):
    loc, videos, queries = _batch_case()
    want0 = _reference(loc, "one-video", videos, [(0, q) for q in queries])
    three = [(i % 3, q) for i, q in enumerate(queries)]
    want3 = _reference(loc, "three-videos", videos, three)
    with loc.open_library(900 + 901 + 1500) as lib:
        ids = [lib.add(v) for v in videos]
        calls = _count_readbacks(monkeypatch)
        got0 = lib.predict_moments([(ids[0], q) for q in queries])
        assert len(calls) == 1
        got3 = lib.predict_moments([(ids[v], q) for v, q in three])
        assert len(calls) == 2
        monkeypatch.undo()
        assert got0 == want0
        assert got3 == want3


# ------------------------------------------------------------------------------------------------ kinds
@pytest.mark.parametrize("kind", ["txt_pos", "pre_norm", "general", "long"])
def test_checkpoint_kinds(kind):
    """--use_txt_pos, --pre_norm, a 128 / 4 handle (general path) and a long-window handle (no layer-0 row cache in the arena;
    max_v_l 300, topk_window 5: K = 5, 4, 5)."""
    loc = _localizer(kind)
    clips = (1000, 301, 700) if kind == "long" else (333, 91, 900)
    videos = [_video(n, seed=4) for n in clips]
    queries = _queries(_mixed_lens(6), seed=13)
    pairs = [(i % 3, q) for i, q in enumerate(queries)]
    want = _reference(loc, "kinds", videos, pairs)
    with loc.open_library(sum(clips)) as lib:
        ids = [lib.add(v) for v in videos]
        assert (not lib._cl.qkv_vid) == (kind == "long")
        assert lib.free_clips == 0
        assert lib.predict_moments([(ids[v], q) for v, q in pairs]) == want


def test_prefilter_bf16_library_equals_its_own_predict_moment():
    from cone_amd import _lib
    loc = _localizer(prefilter_bf16=True)
    queries = _queries(_mixed_lens(6), seed=17)
    videos = [_video(400, seed=5), _video(200, seed=6)]
    videos[0][130:133] = queries[0][1]
    pairs = [(i % 2, q) for i, q in enumerate(queries)]
    want = _reference(loc, "bf16", videos, pairs)
    with loc.open_library(700) as lib:
        assert lib._cl.flags == _lib.SESSION_BF16 and not lib._cl.adapted and lib._cl.adapted_bf16
        ids = [lib.add(v) for v in videos]
        assert lib.predict_moments([(ids[v], q) for v, q in pairs]) == want


# ------------------------------------------------------------------------------------------------ isolation and reuse
def _regions(lib):
    """(int32 view of the region, int32 words per row) of every region of the arena."""
    base, words = lib._arena.data_ptr(), lib._arena.view(torch.int32)
    cl, cap = lib._cl, lib._rows.capacity
    out = []
    for ptr, row_bytes in ((cl.vid_norm, cl.v_dim * 4), (cl.adapted, cl.v_dim * 4), (cl.adapted_bf16, cl.v_dim * 2),
                           (cl.vproj, cl.hidden_dim * 4), (cl.qkv_vid, cl.hidden_dim * 12)):
        if ptr:
            at = (ptr - base) // 4
            out.append((words[at:at + cap * row_bytes // 4], row_bytes // 4))
    return out


def _free_rows_hold(lib, pattern):
    for words, w in _regions(lib):
        for start, n in lib._rows.holes:
            if not bool((words[start * w:(start + n) * w] == pattern).all()):
                return False
    return True


@pytest.mark.parametrize("bf16", [False, True])
def test_add_and_localize_write_only_their_own_rows(bf16):
    """The arena starts as quiet NaNs everywhere; videos are added back to back and every second one removed, so every
    remaining video lies between NaN rows (stale rows of the removed videos are NaN-filled again).  The answers do not change
    and the free rows still hold the pattern bit for bit after the calls."""
    loc = _localizer(prefilter_bf16=True) if bf16 else _localizer()
    clips = (100, 60, 333, 50, 150)
    videos = [_video(n, seed=8) for n in clips]
    queries = _queries(_mixed_lens(6), seed=19)
    pairs = [((0, 2, 4)[i % 3], q) for i, q in enumerate(queries)]
    want = _reference(loc, ("isolation", bf16), videos, pairs)
    with loc.open_library(sum(clips) + 37) as lib:
        lib._arena.view(torch.int32).fill_(QNAN)
        assert sum(words.numel() for words, _ in _regions(lib)) * 4 <= lib.nbytes
        ids = [lib.add(v) for v in videos]
        for i in (1, 3):
            lib.remove(ids[i])
        assert lib._rows.holes == [(100, 60), (493, 50), (693, 37)]
        for words, w in _regions(lib):                      # the removed videos' rows: back to the pattern
            for start, n in lib._rows.holes[:2]:
                words[start * w:(start + n) * w] = QNAN
        assert _free_rows_hold(lib, QNAN)
        got = lib.predict_moments([(ids[v], q) for v, q in pairs])
        assert got == want
        assert _free_rows_hold(lib, QNAN)
        again = lib.add(videos[3])                          # first fit: into the first hole that holds 50 rows
        assert lib._videos[again][0] == 100 and lib._rows.holes == [(150, 10), (493, 50), (693, 37)]
        assert _free_rows_hold(lib, QNAN)
        assert lib.predict_moment(again, queries[0]) == loc.predict_moment(videos[3], queries[0])


def test_a_removed_videos_rows_are_reused_and_its_neighbours_do_not_change():
    loc = _localizer()
    clips = (200, 333, 150)
    videos = [_video(n, seed=9) for n in clips]
    shorter = _video(120, seed=9)
    queries = _queries(_mixed_lens(4), seed=23)
    pairs = [(0, queries[0]), (2, queries[1]), (0, queries[2]), (2, queries[3])]
    want = _reference(loc, "reuse", videos, pairs)
    with loc.open_library(sum(clips)) as lib:
        a, b, c = (lib.add(v) for v in videos)
        ask = [((a, c)[v // 2], q) for v, q in pairs]
        assert lib.predict_moments(ask) == want
        assert lib.predict_moment(b, queries[0]) == loc.predict_moment(videos[1], queries[0])
        with pytest.raises(ValueError, match="no free range of 1 clips: the largest free hole has 0"):
            lib.add(_video(1))
        lib.remove(b)
        assert lib.free_clips == 333
        with pytest.raises(ValueError, match="no free range of 334 clips: the largest free hole has 333"):
            lib.add(_video(334))
        d = lib.add(shorter)
        assert d not in (a, b, c) and lib._videos[d][:2] == (200, 120) and lib.free_clips == 213
        mixed = lib.predict_moments(ask + [(d, queries[1])])
        assert mixed[:4] == want
        assert mixed[4] == loc.predict_moment(shorter, queries[1])
        for call in (lambda: lib.predict_moment(b, queries[0]), lambda: lib.predict_moments(ask + [(b, queries[0])]),
                     lambda: lib.remove(b)):
            with pytest.raises(ValueError, match="unknown or removed video id"):
                call()


# ------------------------------------------------------------------------------------------------ the layout kernel
def _guarded(n, guard=64):
    buf = torch.full((n + 2 * guard,), POISON, dtype=torch.int32, device="cuda")
    return buf, buf[guard:guard + n]


@pytest.mark.parametrize("case", range(len(R.LAYOUT_CASES)))
def test_query_layout_kernel_matches_the_model_inside_guarded_buffers(case):
    from cone_amd import _lib
    lib = _lib.load()
    lens, ctx, row0, K = R.LAYOUT_CASES[case]
    want = R.layout_model(lens, ctx, row0, K)
    bufs = {k: _guarded(len(want[k])) for k in R.OUTPUTS}
    i32 = C.c_int32 * len(lens)
    _lib.check(lib.cone_library_query_layout(i32(*lens), i32(*row0), i32(*ctx), len(lens), R.MAX_Q_L, K, R.NUM_QUERIES, R.MAX_V_L,
                                             *(C.c_void_p(bufs[k][1].data_ptr()) for k in R.OUTPUTS), _lib.stream()))
    torch.cuda.synchronize()
    for k in R.OUTPUTS:
        whole, inner = bufs[k]
        assert np.array_equal(inner.cpu().numpy(), want[k]), (k, lens)
        assert bool((whole[:64] == POISON).all()) and bool((whole[64 + len(want[k]):] == POISON).all()), (k, lens)


def test_a_refused_layout_call_writes_nothing():
    from cone_amd import _lib
    lib = _lib.load()
    outs = [_guarded(64 * 20)[1] for _ in R.OUTPUTS]
    i32 = C.c_int32 * 2
    rc = lib.cone_library_query_layout(i32(4, 4), i32(0, 900), i32(900, 46), 2, 20, 4, 5, 90,
                                       *(C.c_void_p(o.data_ptr()) for o in outs), _lib.stream())
    assert rc == -1 and "K=4 not in [1, min(num_window=3, 256)] for query 1" in lib.cone_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool((o == POISON).all()) for o in outs)


# ------------------------------------------------------------------------------------------------ the C entries' own refusals
def test_c_entries_refuse_by_name():
    from cone_amd import _lib
    lib, loc = _lib.load(), _localizer()
    h = loc.localizator._h()
    other = _localizer("pre_norm").localizator._h()
    vid = _video(333).cuda()
    with loc.open_library(400) as L:
        cl, n_ws = L._cl, lib.cone_library_add_workspace(h, 333)
        ws = torch.empty(n_ws, dtype=torch.uint8, device="cuda")
        before = L._arena.clone()
        add = lambda m, row0, n, ws_bytes=n_ws: lib.cone_library_add(m, C.byref(cl), row0, _lib.ptr(vid), n, _lib.ptr(ws), ws_bytes,
                                                                     _lib.stream())
        assert add(h, 68, 333) == -1 and "rows [68, 68 + 333) are not inside [0, capacity=400)" in lib.cone_last_error().decode()
        assert add(h, -1, 10) == -1 and add(h, 0, 0) == -1
        assert add(other, 0, 333) == -1 and "opened with another handle" in lib.cone_last_error().decode()
        assert add(h, 0, 333, n_ws - 1) == -3 and "library_add: workspace too small" in lib.cone_last_error().decode()
        torch.cuda.synchronize()
        assert torch.equal(L._arena, before)                        # the refused calls wrote nothing
        assert add(h, 67, 333) == 0, lib.cone_last_error()
        i32, p = C.c_int32 * 1, L._params
        size = lambda m: lib.cone_library_localize_workspace(m, C.byref(cl), i32(67), i32(333), i32(7), 1, 9, C.byref(p))
        assert size(other) == 0 and "library_localize: the library was opened with another handle" in lib.cone_last_error().decode()
        n = size(h)
        assert n > 0
        q = _queries([7], seed=29)[0]
        tok, cls = q[0].cuda(), q[1].reshape(1, -1).cuda()
        lws = torch.empty(n, dtype=torch.uint8, device="cuda")
        kept = torch.full((3 * 5 * 5 * 8 + 3 * 4,), 0xA5, dtype=torch.uint8, device="cuda")
        call = lambda ws_bytes: lib.cone_library_localize(h, C.byref(cl), i32(67), i32(333), _lib.ptr(tok), i32(7), 1, _lib.ptr(cls), 9,
                                                          C.byref(p), C.c_void_p(kept.data_ptr()), C.c_void_p(kept.data_ptr() + 600),
                                                          _lib.ptr(lws), ws_bytes, _lib.stream())
        assert call(n - 1) == -3 and "library_localize: workspace too small" in lib.cone_last_error().decode()
        torch.cuda.synchronize()
        assert bool((kept == 0xA5).all())
        assert call(n) == 0, lib.cone_last_error()
        from cone_amd.session import VideoSession
        assert VideoSession.read_kept(kept.cpu(), 1) == [loc.predict_moment(vid.cpu(), q)]


# ------------------------------------------------------------------------------------------------ lifetime
def test_stale_handle_and_closed_library_are_refused():
    from cone_amd.localizator import CONELocalizator, LOCALIZER_OPT
    opt = SimpleNamespace(**LOCALIZER_OPT)
    sds = [{k: torch.from_numpy(v) for k, v in synth.make_state_dict(opt, seed).items()} for seed in (5, 6)]
    loc = CONELocalizator(state_dict=sds[0])
    vid = _video(333)
    q = _queries([7], seed=31)[0]
    lib = loc.open_library(400)
    a = lib.add(vid)
    before = lib.predict_moment(a, q)
    assert before == loc.predict_moment(vid, q)
    loc.localizator.load_state_dict(sds[1])
    for call in (lambda: lib.predict_moment(a, q), lambda: lib.predict_moments([(a, q), (a, q)]), lambda: lib.add(vid)):
        with pytest.raises(RuntimeError, match="VideoLibrary: load_state_dict replaced the model handle"):
            call()
    with loc.open_library(400) as lib2:
        after = lib2.predict_moment(lib2.add(vid), q)
    assert after == loc.predict_moment(vid, q) and after != before
    assert lib2.nbytes == 0 and lib2.free_clips == 0
    with pytest.raises(RuntimeError, match="closed"):
        lib2.predict_moment(1, q)
    with pytest.raises(RuntimeError, match="closed"):
        lib2.add(vid)
    lib.close()
    assert lib.nbytes == 0
