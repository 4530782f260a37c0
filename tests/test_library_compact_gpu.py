"""Library maintenance on the GPU.  The mover (cone_library_move_rows) runs on dictated, guarded arenas of row-unique integer
patterns and the WHOLE buffer, guards and plane padding included, is compared bit for bit with the model of tests/move_refs.py;
``compact`` / ``resize`` / ``add(compact=True)`` are compared with ``==`` against ``predict_moment`` on the raw videos, before
and after.  A copy is exact: no tolerance appears anywhere."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import move_refs as R
from cone_amd import synth

pytestmark = pytest.mark.gpu

POISON = 0x7EADBEEF
QNAN = 0x7FC00000
GUARD = 4096                # bytes of poison on either side of an arena / a staging buffer


# ------------------------------------------------------------------------------------------------ fixtures
_LOCS, _REFS = {}, {}


def _localizer(kind="default", **extra):
    """One localizer per checkpoint kind for the whole module (tests/test_library_gpu.py's kinds)."""
    from cone_amd.localizator import CONELocalizator, LOCALIZER_OPT
    key = (kind, tuple(sorted(extra.items())))
    if key not in _LOCS:
        kw = dict(default={}, txt_pos=dict(use_txt_pos=True), pre_norm=dict(pre_norm=True), general=dict(hidden_dim=128, nheads=4),
                  long=dict(max_v_l=300, topk_window=5))[kind]
        sd = synth.make_state_dict(SimpleNamespace(**dict(LOCALIZER_OPT, **kw)), 5)
        _LOCS[key] = CONELocalizator(state_dict={k: torch.from_numpy(v) for k, v in sd.items()}, **kw, **extra)
    return _LOCS[key]


def _kind(kind):
    return _localizer(prefilter_bf16=True) if kind == "prefilter_bf16" else _localizer(kind)


def _video(ctx_l, seed=0):
    return torch.randn(ctx_l, 256, generator=torch.Generator().manual_seed(2000 + seed + ctx_l)) * 2


def _queries(lens, seed=0):
    g = torch.Generator().manual_seed(177 + seed)
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


# ------------------------------------------------------------------------------------------------ kernel level
class Arena:
    """A library handle on a dictated arena between two guards; ``host`` mirrors the whole buffer as int32."""

    def __init__(self, loc, capacity, pattern=True):
        from cone_amd import _lib
        lib, self.h = _lib.load(), loc.localizator._h()
        flags = _lib.SESSION_BF16 if loc.prefilter_bf16 else 0
        n = lib.cone_library_arena_bytes(self.h, capacity, flags)
        assert n > 0 and n % 256 == 0
        self.capacity, self.cl = capacity, _lib.Library()
        self.host = np.full((n + 2 * GUARD) // 4, POISON, dtype=np.int32)
        self.buf = torch.from_numpy(self.host).cuda()
        base = self.buf.data_ptr()
        assert base % 256 == 0
        _lib.check(lib.cone_library_open(self.h, capacity, flags, C.c_void_p(base + GUARD), n, C.byref(self.cl)))
        cl = self.cl
        self.words = R.plane_words(cl.v_dim, cl.hidden_dim, bool(cl.adapted_bf16), bool(cl.qkv_vid))
        ptrs = [cl.vid_norm, cl.adapted_bf16 or cl.adapted, cl.vproj] + ([cl.qkv_vid] if cl.qkv_vid else [])
        self.at = [(p - base) // 4 for p in ptrs]
        assert all(GUARD // 4 <= a and a + capacity * w <= (GUARD + n) // 4 for a, w in zip(self.at, self.words))
        if pattern:
            R.fill(self.planes(self.host))
            self.buf.copy_(torch.from_numpy(self.host))

    def planes(self, host):
        """Views of the planes inside a mirror of the buffer."""
        return [host[a:a + self.capacity * w].reshape(self.capacity, w) for a, w in zip(self.at, self.words)]

    def equals(self, want):
        torch.cuda.synchronize()
        return np.array_equal(self.buf.cpu().numpy(), want)


def _stage(n_bytes):
    buf = torch.full((n_bytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, C.c_void_p(buf.data_ptr() + GUARD)


def _stage_untouched_outside(buf, n_bytes):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + n_bytes:] == 0xA5).all())


def _move(src, dst, moves, steps, m=None):
    """The steps as C calls on one uploaded table; a staged step gets a guarded staging buffer of exactly the bytes it needs.
    Returns the return codes."""
    from cone_amd import _lib
    lib, n = _lib.load(), len(moves)
    table = np.zeros(3 * n + 1, dtype=np.int64)
    table[:n], table[n:2 * n] = [mv[0] for mv in moves], [mv[1] for mv in moves]
    np.cumsum([mv[2] for mv in moves], out=table[2 * n + 1:])
    dev = torch.from_numpy(table).cuda()
    at = lambda k: C.c_void_p(dev.data_ptr() + 8 * k)
    rcs = []
    for begin, end, staged in steps:
        need = lib.cone_library_move_stage_bytes(C.byref(src.cl), end - begin) if staged else 0
        buf, ptr = _stage(need) if staged else (None, None)
        rcs.append(lib.cone_library_move_rows(m or src.h, C.byref(src.cl), C.byref(dst.cl), at(0), at(n), at(2 * n), n, int(table[-1]),
                                              begin, end, ptr, need, _lib.stream()))
        torch.cuda.synchronize()
        assert rcs[-1] != 0 or not staged or _stage_untouched_outside(buf, need)
    return rcs


def _expect_in_place(arena, moves):
    want = arena.host.copy()
    for view, plane in zip(arena.planes(want), R.memmove_truth(arena.planes(arena.host), moves)):
        view[:] = plane
    return want


KERNEL_KINDS = ("default", "prefilter_bf16", "long", "general")


@pytest.mark.parametrize("name", list(R.CASES))
@pytest.mark.parametrize("kind", KERNEL_KINDS)
def test_every_named_case_moves_like_the_model_inside_guarded_arenas(kind, name):
    """fp32 (6 KiB per clip), prefilter_bf16 (512-B bf16 rows, no ``adapted``), a long-window handle (no ``qkv_vid``), a 128 / 4
    handle (512-B ``vproj`` rows).  Three forms: ONE staged call over the whole list in place; the plan of ``plan_steps`` in
    place (staged and direct steps, seams inside moves); ONE direct call into a second arena."""
    from cone_amd.library import compaction_moves, plan_steps
    loc = _kind(kind)
    capacity, videos, stage_rows = R.CASES[name]
    moves = compaction_moves(videos)
    moving = [mv for mv in moves if mv[0] != mv[1]]
    total = sum(mv[2] for mv in moving)
    for steps in ([(0, total, True)], plan_steps(moves, stage_rows)):
        a = Arena(loc, capacity)
        assert len(a.words) == (3 if kind == "long" else 4) and a.words[1] == (128 if kind == "prefilter_bf16" else 256)
        want = _expect_in_place(a, moves)
        if moving:
            assert _move(a, a, moving, steps) == [0] * len(steps)
        assert a.equals(want), (kind, name, steps)
    used = sum(mv[2] for mv in moves)
    a, b = Arena(loc, capacity), Arena(loc, used + 3, pattern=False)
    want = b.host.copy()
    for view, plane in zip(b.planes(want), a.planes(a.host)):
        for s, d, n in moves:
            view[d:d + n] = plane[s:s + n]
    assert _move(a, b, moves, [(0, used, False)]) == [0]
    assert b.equals(want) and a.equals(a.host), (kind, name)


@pytest.mark.parametrize("staged", [False, True])
def test_a_move_that_leaves_the_capacity_is_skipped_whole_and_the_others_land(staged):
    loc = _localizer()
    for bad in ((95, 40, 10), (-2, 40, 10), (60, 95, 10), (60, -1, 10)):            # src / dst range outside [0, 100)
        moves = [(50, 0, 20), bad, (80, 20, 15)]
        a, b = Arena(loc, 100), Arena(loc, 100, pattern=False)
        dst = a if staged else b
        want = dst.host.copy()
        src_planes = [p.copy() for p in a.planes(a.host)]
        for view, plane in zip(dst.planes(want), src_planes):
            for s, d, n in (moves[0], moves[2]):
                view[d:d + n] = plane[s:s + n]
        assert _move(a, dst, moves, [(0, 45, staged)]) == [0]
        assert dst.equals(want), bad
        if not staged:
            assert a.equals(a.host)


def test_a_refused_move_writes_nothing():
    from cone_amd import _lib
    lib, loc = _lib.load(), _localizer()
    a = Arena(loc, 64)
    other = _localizer("pre_norm").localizator._h()
    moves = [(10, 0, 40)]
    assert _move(a, a, moves, [(0, 40, True)], m=other) == [-1]
    assert "library_move: the libraries were opened with another handle" in lib.cone_last_error().decode()
    assert _move(a, a, moves, [(0, 41, True)]) == [-1] and "rows [0, 41)" in lib.cone_last_error().decode()
    need = lib.cone_library_move_stage_bytes(C.byref(a.cl), 40)
    buf, ptr = _stage(need)
    table = torch.tensor([10, 0, 0, 40], dtype=torch.int64, device="cuda")
    at = lambda k: C.c_void_p(table.data_ptr() + 8 * k)
    rc = lib.cone_library_move_rows(a.h, C.byref(a.cl), C.byref(a.cl), at(0), at(1), at(2), 1, 40, 0, 40, ptr, need - 1, _lib.stream())
    assert rc == -3 and "library_move: staging buffer too small" in lib.cone_last_error().decode()
    assert a.equals(a.host) and bool((buf == 0xA5).all())
    b = Arena(_kind("long"), 64)                                                    # another model, other planes
    assert _move(a, b, moves, [(0, 40, False)]) == [-1]
    assert "src and dst differ" in lib.cone_last_error().decode() and b.equals(b.host)


# ------------------------------------------------------------------------------------------------ compact()
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


def _fill_free_rows(lib, pattern=QNAN):
    for words, w in _regions(lib):
        for start, n in lib._rows.holes:
            words[start * w:(start + n) * w] = pattern


FRAGMENTED = (100, 60, 333, 50, 150)


def _fragmented(lib, videos):
    """The case of test_add_and_localize_write_only_their_own_rows: NaNs everywhere, five videos, the second and fourth removed."""
    lib._arena.view(torch.int32).fill_(QNAN)
    ids = [lib.add(v) for v in videos]
    for i in (1, 3):
        lib.remove(ids[i])
    _fill_free_rows(lib)
    assert lib._rows.holes == [(100, 60), (493, 50), (693, 37)] and lib.largest_free == 60 and lib.free_clips == 147
    return ids


@pytest.mark.parametrize("stage_rows", [None, 80, 40])
def test_compact_a_fragmented_library(stage_rows):
    """The default buffer (one staged step of 483 rows), one of 80 rows (staged steps that cut the 333-clip video, one across the
    seam to the next video, then a direct step) and one of 40 rows (direct steps of 60 and 110 rows: every video is cut)."""
    loc = _localizer()
    videos = [_video(n, seed=8) for n in FRAGMENTED]
    late = _video(147, seed=9)
    queries = _queries(_mixed_lens(6), seed=19)
    pairs = [((0, 2, 4)[i % 3], q) for i, q in enumerate(queries)]
    want = _reference(loc, "fragmented", videos, pairs)
    want_late = _reference(loc, "late", [late], [(0, queries[1])])[0]
    with loc.open_library(sum(FRAGMENTED) + 37) as lib:
        ids = _fragmented(lib, videos)
        ask = [(ids[v], q) for v, q in pairs]
        assert lib.predict_moments(ask) == want
        with pytest.raises(ValueError, match="no free range of 147 clips: the largest free hole has 60"):
            lib.add(late)
        moved = lib.compact() if stage_rows is None else lib.compact(stage_bytes=stage_rows * 6144)
        assert moved == 333 + 150
        assert [lib._videos[ids[i]][:2] for i in (0, 2, 4)] == [(0, 100), (100, 333), (433, 150)]
        assert lib._rows.holes == [(583, 147)] and lib.free_clips == 147 and lib.largest_free == 147
        _fill_free_rows(lib)                                    # (vacated rows keep their old content: nobody may need it)
        assert lib.predict_moments(ask) == want
        new = lib.add(late)
        assert lib._videos[new][:2] == (583, 147) and lib.free_clips == 0 and new not in ids
        assert lib.predict_moment(new, queries[1]) == want_late
        assert lib.predict_moments(ask) == want


def test_add_with_compact_succeeds_where_the_default_raises():
    loc = _localizer()
    videos = [_video(n, seed=8) for n in FRAGMENTED]
    late = _video(147, seed=9)
    queries = _queries(_mixed_lens(6), seed=19)
    pairs = [((0, 2, 4)[i % 3], q) for i, q in enumerate(queries)]
    want = _reference(loc, "fragmented", videos, pairs)
    want_late = _reference(loc, "late", [late], [(0, queries[1])])[0]
    with loc.open_library(sum(FRAGMENTED) + 37) as lib:
        ids = _fragmented(lib, videos)
        with pytest.raises(ValueError, match=r"no free range of 147 clips: the largest free hole has 60 \(147 of 730 clips are free"):
            lib.add(late)
        with pytest.raises(ValueError, match="no free range of 148 clips"):
            lib.add(_video(148), compact=True)
        assert lib._rows.holes == [(100, 60), (493, 50), (693, 37)]            # neither attempt moved anything
        new = lib.add(late, compact=True)
        assert lib._videos[new][:2] == (583, 147) and lib._rows.holes == []
        assert lib.predict_moments([(ids[v], q) for v, q in pairs] + [(new, queries[1])]) == want + [want_late]


def test_compact_on_a_compact_library_returns_0_and_leaves_the_bits():
    loc = _localizer()
    with loc.open_library(300) as lib:
        lib._arena.view(torch.int32).fill_(QNAN)
        for n in (100, 60):
            lib.add(_video(n, seed=8))
        torch.cuda.synchronize()
        before = lib._arena.clone()
        assert lib.compact() == 0 and lib.compact(stage_bytes=1) == 0
        torch.cuda.synchronize()
        assert torch.equal(lib._arena.view(torch.int32), before.view(torch.int32)) and lib._rows.holes == [(160, 140)]
        gone = lib.add(_video(50, seed=8))
        lib.remove(gone)                                        # a hole at the end only: still compact
        assert lib.compact() == 0 and lib._rows.holes == [(160, 140)]
        first = next(iter(lib._videos))
        lib.remove(first)
        with pytest.raises(ValueError, match="stage_bytes=1000 holds no clip"):
            lib.compact(stage_bytes=1000)
        assert lib.compact() == 60


def test_rankings_and_searches_do_not_change_and_ties_keep_their_order():
    """Two pairs of byte-identical videos tie exactly; ``rank_videos`` breaks ties to the video that lies first in the arena, and
    a compaction keeps the arena order.  The first search after it must not use the scan table of the old rows: those rows are
    NaN-filled here."""
    loc = _localizer()
    clips = (120, 200, 91, 200, 60, 91, 333)
    videos = [_video(n, seed=3) for n in clips]                 # equal lengths share a seed: videos 1 / 3 and 2 / 5 are twins
    assert torch.equal(videos[1], videos[3]) and torch.equal(videos[2], videos[5])
    queries = _queries(_mixed_lens(5), seed=41)
    with loc.open_library(sum(clips) + 20) as lib:
        lib._arena.view(torch.int32).fill_(QNAN)
        ids = [lib.add(v) for v in videos]
        for i in (0, 4):
            lib.remove(ids[i])
        _fill_free_rows(lib)
        ranked, found = lib.rank_videos(queries), lib.search(queries, n_videos=4)
        for row in ranked:
            order = [v for v, _ in row]
            assert order.index(ids[1]) + 1 == order.index(ids[3]) and order.index(ids[2]) + 1 == order.index(ids[5])
            assert dict(row)[ids[1]] == dict(row)[ids[3]] and dict(row)[ids[2]] == dict(row)[ids[5]]
        assert lib._scan_cache is not None
        assert lib.compact() == sum(clips) - 120 - 60
        assert lib._scan_cache is None
        _fill_free_rows(lib)
        assert lib.search(queries, n_videos=4) == found
        assert lib.rank_videos(queries) == ranked
        assert lib.rank_videos(queries, n_videos=2, videos=[ids[5], ids[3], ids[6]]) == [
            [rv for rv in row if rv[0] in (ids[5], ids[3], ids[6])][:2] for row in ranked]


# ------------------------------------------------------------------------------------------------ resize()
def test_resize_up_and_down_keeps_ids_and_answers():
    loc = _localizer()
    videos = [_video(n, seed=8) for n in FRAGMENTED]
    late = _video(147, seed=9)
    queries = _queries(_mixed_lens(6), seed=19)
    pairs = [((0, 2, 4)[i % 3], q) for i, q in enumerate(queries)]
    want = _reference(loc, "fragmented", videos, pairs)
    want_late = _reference(loc, "late", [late], [(0, queries[1])])[0]
    with loc.open_library(sum(FRAGMENTED) + 37) as lib:
        ids = _fragmented(lib, videos)
        ask = [(ids[v], q) for v, q in pairs]
        small = lib.nbytes
        lib.resize(2000)                                        # up: compacts on the way
        assert lib.nbytes > 2 * small and lib._cl.capacity == 2000 and lib.free_clips == 2000 - 583 and lib.largest_free == 1417
        assert [lib._videos[ids[i]][:2] for i in (0, 2, 4)] == [(0, 100), (100, 333), (433, 150)]
        assert lib.predict_moments(ask) == want
        new = lib.add(late)
        assert lib._videos[new][:2] == (583, 147)               # behind the last video
        lib.remove(ids[2])
        with pytest.raises(ValueError, match="resize: capacity_clips=396 is smaller than the 397 resident clips"):
            lib.resize(396)
        assert lib._cl.capacity == 2000 and lib.predict_moment(new, queries[1]) == want_late        # still usable
        lib.resize(397)                                         # down to exactly the resident clips
        assert lib.nbytes < small and lib.free_clips == 0 and lib._rows.holes == [] and lib.largest_free == 0
        assert [lib._videos[v][:2] for v in (ids[0], ids[4], new)] == [(0, 100), (100, 150), (250, 147)]
        keep = [i for i, (v, _) in enumerate(pairs) if v != 2]
        assert lib.predict_moments([ask[i] for i in keep] + [(new, queries[1])]) == [want[i] for i in keep] + [want_late]
        with pytest.raises(ValueError, match="unknown or removed video id"):
            lib.predict_moment(ids[2], queries[0])
        with pytest.raises(ValueError, match="no free range of 1 clips"):
            lib.add(_video(1))


# ------------------------------------------------------------------------------------------------ kinds
@pytest.mark.parametrize("kind", ["txt_pos", "pre_norm", "general", "long", "prefilter_bf16"])
def test_checkpoint_kinds_answer_the_same_after_a_compaction(kind):
    loc = _kind(kind)
    clips = (310, 1000, 301, 50, 700) if kind == "long" else (40, 333, 91, 50, 400)
    videos = [_video(n, seed=4) for n in clips]
    queries = _queries(_mixed_lens(6), seed=13)
    pairs = [((1, 2, 4)[i % 3], q) for i, q in enumerate(queries)]
    want = _reference(loc, "kinds", videos, pairs)
    with loc.open_library(sum(clips) + 5) as lib:
        lib._arena.view(torch.int32).fill_(QNAN)
        ids = [lib.add(v) for v in videos]
        for i in (0, 3):
            lib.remove(ids[i])
        _fill_free_rows(lib)
        ask = [(ids[v], q) for v, q in pairs]
        assert lib.predict_moments(ask) == want
        row_bytes = lib._cl.v_dim * (4 + (2 if kind == "prefilter_bf16" else 4)) + lib._cl.hidden_dim * (4 if kind == "long" else 16)
        assert lib.compact(stage_bytes=64 * row_bytes) == sum(clips[i] for i in (1, 2, 4))       # g = 40, then 90: staged, then direct (long: g = 310, all direct)
        assert lib._rows.holes == [(sum(clips[i] for i in (1, 2, 4)), clips[0] + clips[3] + 5)]
        _fill_free_rows(lib)
        assert lib.predict_moments(ask) == want
        lib.resize(sum(clips))
        assert lib.predict_moments(ask) == want
