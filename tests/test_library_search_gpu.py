"""Library search on the GPU.

Kernel level: ``cone_library_scan`` on dictated arenas behind a hand-made ``cone_library``.  THE CONTRACT: for every (query,
video) the scan's window list equals ``cone_prefilter_scores`` (the streaming form: launches of at most 4 queries, as a
library call's stage A issues them) + ``cone_topk_windows_ws`` run on that video's rows ALONE -- compared bit for bit, as int32
words --, pads are -1 / -inf, and the ranking equals the stable top-k of the ``best`` row.  Every arena is a slice of a
1e30-filled buffer, holes are quiet NaNs, every output sits between guard words that are checked.

Through the model: every entry of ``VideoLibrary.search`` equals ``CONELocalizator.predict_moment`` on that video and query with
``==``, and its score is that video's best window score."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import search_refs as R
from cone_amd import synth

pytestmark = pytest.mark.gpu

POISON = 0x7EADBEEF
GUARD = 64
FAKE_HANDLE = 0x1000         # the scan compares the handle with the library's and never follows it


# ------------------------------------------------------------------------------------------------ kernel-level harness
def _device_arena(arena_np, guard_rows=8):
    """The arena as a slice of a 1e30-filled buffer: (whole buffer, the arena's rows)."""
    cap, dv = arena_np.shape
    whole = torch.full((cap + 2 * guard_rows, dv), 1e30, dtype=torch.float32, device="cuda")
    whole[guard_rows:guard_rows + cap] = torch.from_numpy(arena_np).cuda()
    return whole, whole[guard_rows:guard_rows + cap]


def _guarded(n, dtype):
    whole = torch.full((n + 2 * GUARD,), POISON, dtype=torch.int32, device="cuda")
    return whole, whole[GUARD:GUARD + n].view(dtype)


def _guards_hold(whole, n):
    return bool((whole[:GUARD] == POISON).all()) and bool((whole[GUARD + n:] == POISON).all())


def _scan(arena, videos, cls, W, K, n_rank, ws_short=0):
    """cone_library_scan over ``videos`` = [(row0, ctx_l), ...] of ``arena`` (device rows).  Returns the four outputs (slots by
    ascending row0) after checking every guard, and the return code."""
    from cone_amd import _lib
    from cone_amd.library import scan_table
    lib = _lib.load()
    S = W // 2
    order, row0, ctx, hb_off = scan_table(videos, S)
    V, nq, total_hb = len(videos), cls.shape[0], int(hb_off[-1])
    t_row0, t_ctx, t_off = (torch.from_numpy(x).cuda() for x in (row0, ctx, hb_off))
    handle = _lib.Library(FAKE_HANDLE, arena.shape[0], 0, arena.shape[1], 256, None, arena.data_ptr(), None, None, None)
    p = _lib.SessionParams(W, 20, 0.5333, 0.5, 100, 5)
    n_ws = lib.cone_library_scan_workspace(C.byref(handle), V, total_hb, nq, K, n_rank)
    assert n_ws > 0, lib.cone_last_error()
    ws_whole = torch.full((n_ws + 512,), 0x5A, dtype=torch.uint8, device="cuda")
    at = (-ws_whole.data_ptr()) % 256
    ws = ws_whole[at:at + n_ws]
    outs = [_guarded(nq * V * K, torch.int32), _guarded(nq * V * K, torch.float32), _guarded(nq * n_rank, torch.int32),
            _guarded(nq * n_rank, torch.float32)]
    rc = lib.cone_library_scan(C.c_void_p(FAKE_HANDLE), C.byref(handle), _lib.ptr(t_row0), _lib.ptr(t_ctx), _lib.ptr(t_off), V, total_hb,
                               _lib.ptr(cls, torch.float32), nq, K, n_rank, C.byref(p), *(C.c_void_p(o[1].data_ptr()) for o in outs),
                               C.c_void_p(ws.data_ptr()), n_ws - ws_short, _lib.stream())
    torch.cuda.synchronize()
    for (whole, inner) in outs:
        assert _guards_hold(whole, inner.numel())
    assert bool((ws_whole[:at] == 0x5A).all()) and bool((ws_whole[at + n_ws:] == 0x5A).all())        # the workspace's ends
    widx, wval, rslot, rval = (o[1] for o in outs)
    return rc, widx.view(nq, V, K), wval.view(nq, V, K), rslot.view(nq, n_rank), rval.view(nq, n_rank), order


def _reference(arena, videos, order, cls, W, K, n_rank):
    """The parent's way to the same lists: per video, on its rows alone, the streaming pre-filter in launches of at most 4
    queries and the stable top-k at K_v = min(K, num_window); -1 / -inf behind it; then the stable top-k of the best row."""
    from cone_amd import ops
    nq, V = cls.shape[0], len(videos)
    widx = torch.full((nq, V, K), -1, dtype=torch.int32, device="cuda")
    wval = torch.full((nq, V, K), float("-inf"), dtype=torch.float32, device="cuda")
    for slot, i in enumerate(order):
        row0, n = videos[i]
        rows = arena[row0:row0 + n]
        win = torch.cat([ops.prefilter_scores(rows, cls[g:g + 4], W, frame_scores=False)[1] for g in range(0, nq, 4)])
        k_v = min(K, R.num_windows(n, W))
        idx, val = ops.topk_windows(win, k_v)
        widx[:, slot, :k_v], wval[:, slot, :k_v] = idx, val
    rslot, rval = ops.topk_windows(wval[:, :, 0].contiguous(), n_rank)
    return widx, wval, rslot, rval


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_contract(arena, videos, cls, W, K, n_rank=None):
    n_rank = n_rank or len(videos)
    rc, widx, wval, rslot, rval, order = _scan(arena, videos, cls, W, K, n_rank)
    assert rc == 0
    want = _reference(arena, videos, order, cls, W, K, n_rank)
    assert torch.equal(widx, want[0])
    assert torch.equal(_bits(wval), _bits(want[1]))                 # as words: -inf pads and any NaN compare too
    assert torch.equal(rslot, want[2]) and torch.equal(_bits(rval), _bits(want[3]))
    for slot, i in enumerate(order):                                # pads exactly where the video runs out of windows
        nw = R.num_windows(videos[i][1], W)
        assert bool((widx[:, slot, :min(K, nw)] >= 0).all()) and bool((widx[:, slot, nw:] == -1).all())
        assert bool((wval[:, slot, nw:] == float("-inf")).all())
    return widx, wval, rslot, rval, order


def _queries(nq, dv, seed):
    return torch.from_numpy(R.unit_rows(nq, dv, 900 + seed)).cuda()


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("nq,K", [(1, 1), (4, 20), (5, 30), (64, 20)])
@pytest.mark.parametrize("dv,W", [(256, 90), (256, 125), (512, 90), (512, 125)])
def test_every_length_at_the_wave_workgroup_and_half_block_seams(dv, W, nq, K):
    """The sixteen lengths back to back without a gap, then again with gaps of 0 .. 3 rows: the 4-row wave slot (3, 4, 5), the
    16-row workgroup round (15, 16, 17), the half-block seam (44 .. 46, 89 .. 91); 1, 4, 5 and 64 queries (the 4-query pass
    seam, q0 > 0)."""
    lengths = list(R.KERNEL_LENGTHS)
    videos = R.stacked(lengths) + R.stacked(lengths[::-1], gaps=[i % 4 for i in range(16)], start=sum(lengths) + 2)
    arena_np = R.build_arena(videos, dv, seed=dv + W, capacity=videos[-1][0] + videos[-1][1] + 5)
    _, arena = _device_arena(arena_np)
    _assert_contract(arena, videos, _queries(nq, dv, nq), W, K, n_rank=min(len(videos), 7))


@pytest.mark.parametrize("V,nq", [(1, 5), (2, 5), (7, 5), (65, 5), (65, 64), (300, 5)])
def test_video_counts_across_the_64_mark(V, nq):
    """Videos of 1 .. 100 clips (the table's search over 1 .. 301 prefix sums), every third one behind a hole."""
    rng = np.random.default_rng(V)
    lengths = [int(n) for n in rng.integers(1, 101, V)]
    videos = R.stacked(lengths, gaps=[(i % 3 == 2) * int(rng.integers(1, 4)) for i in range(V)])
    _, arena = _device_arena(R.build_arena(videos, 256, seed=V))
    _assert_contract(arena, videos, _queries(nq, 256, V), 90, 20, n_rank=min(V, 10))


def test_a_video_of_1101_windows_takes_the_selection_loop():
    """45 x 1 100 clips between two short videos: more windows than the 1 024 the ranks are counted for in LDS."""
    videos = R.stacked([91, R.LONG_VIDEO, 333])
    assert R.num_windows(R.LONG_VIDEO, 90) == 1101
    _, arena = _device_arena(R.build_arena(videos, 256, seed=11))
    _assert_contract(arena, videos, _queries(5, 256, 3), 90, 30)


@pytest.mark.parametrize("W", [2, 3])
def test_more_than_4096_half_blocks_take_the_wave_per_half_block_form(W):
    """W = 2 / 3: S = 1, every clip is a half-block of its own -- 4 201 units: the scan leaves the workgroup-per-unit form
    (below 4 096 units) for a wave per unit; 1 201 and 1 202 windows: the selection loop with the odd term at every window."""
    videos = R.stacked([900, 901, 1200, 700, 500], gaps=[0, 0, 3, 0, 1])
    _, arena = _device_arena(R.build_arena(videos, 256, seed=W))
    _assert_contract(arena, videos, _queries(5, 256, W), W, 20)


# ------------------------------------------------------------------------------------------------ value families
@pytest.mark.parametrize("name", R.FAMILIES)
def test_value_families_against_the_per_video_path_and_the_float64_model(name):
    """Bit for bit against the per-video path, and against the float64 model of the reference's definition: every listed value
    within E of the model's score of that window, the list ordered (value descending, ties by index ascending), and no
    unlisted window above the list's last value by more than E.  E = dv 2^-24 |row| |query| bounds the rounding of an fp32
    dot product of dv terms in any summation order (rows and queries have norm <= 6 and 1).  Where the model's scores are
    more than 2 E apart (the planted peaks) the indices and the ranking must be the model's."""
    arena_np, videos, cls_np, W = R.family(name)
    K, V = 20, len(videos)
    _, arena = _device_arena(arena_np)
    widx, wval, rslot, rval, order = _assert_contract(arena, videos, torch.from_numpy(cls_np).cuda(), W, K)
    model = R.scan_truth(arena_np, videos, cls_np, W, K, V)
    assert list(order) == model["order"]
    E = arena_np.shape[1] * 2.0 ** -24 * 6.0
    widx, wval, rslot, rval = widx.cpu().numpy(), wval.cpu().numpy().astype(np.float64), rslot.cpu().numpy(), rval.cpu().numpy()
    for q in range(cls_np.shape[0]):
        for slot in range(V):
            win = model["win"][slot][q]
            n = min(K, len(win))
            idx, val = widx[q, slot, :n], wval[q, slot, :n]
            assert len(set(idx.tolist())) == n
            finite = np.isfinite(win[idx])
            assert np.array_equal(finite, np.isfinite(val)) and (np.abs(val[finite] - win[idx][finite]) <= E).all(), (name, q, slot)
            assert all(val[j] > val[j + 1] or (val[j] == val[j + 1] and idx[j] < idx[j + 1]) for j in range(n - 1))
            rest = np.delete(win, idx)
            assert rest.size == 0 or rest.max() <= val[-1] + E
            listed = model["wval"][q, slot, :n]
            if n > 1 and np.isfinite(listed).all() and (np.abs(np.diff(listed)) > 2 * E).all():
                assert idx.tolist() == model["widx"][q, slot, :n].tolist()
        ranked = np.isfinite(model["rank_val"][q])
        assert np.array_equal(ranked, np.isfinite(rval[q])) and (np.abs(rval[q][ranked] - model["rank_val"][q][ranked]) <= E).all()
    if name in ("seam", "seam_odd", "half_first", "twins", "all_nan"):
        assert widx[0, :, 0].tolist() == model["widx"][0, :, 0].tolist()
        assert rslot[0, :2].tolist() == model["rank_slot"][0, :2].tolist()
    if name == "twins":                                             # byte-identical videos: equal bits, the lower slot first
        assert np.array_equal(wval[:, 1], wval[:, 3]) and np.array_equal(widx[:, 1], widx[:, 3])
        for q in range(cls_np.shape[0]):
            r = rslot[q].tolist()
            assert r.index(1) + 1 == r.index(3)
    if name == "flat":                                              # equal rows: equal scores, the windows in index order
        assert widx[0, 1, :9].tolist() == list(range(9)) and len(set(wval[0, 1, :9].tolist())) == 1
    if name == "all_nan":
        assert widx[0, 1].tolist() == list(range(6)) + [-1] * 14 and (wval[:, 1] == -np.inf).all() and rslot[0, -1] == 1


def test_the_seam_between_adjacent_videos():
    """A peak in video 0's LAST row, a double peak in video 1's FIRST row, no row between them, W = 90 and 125 with video 0
    ending on and off a half-block boundary: video 0 scores the single peak in its last windows only, video 1 the double peak
    in windows 0 and 1 only, and neither sees the other's."""
    for W, len0 in [(90, 90), (90, 91), (90, 46), (125, 124), (125, 125), (125, 63)]:
        S = W // 2
        videos = R.stacked([len0, 3 * S + 1, 40])
        arena_np = R.build_arena(videos, 256, seed=W + len0)
        cls_np = R.unit_rows(2, 256, 5)
        arena_np[len0 - 1] = 3 * cls_np[0]
        arena_np[len0] = 6 * cls_np[0]
        _, arena = _device_arena(arena_np)
        widx, wval, rslot, rval, _ = _assert_contract(arena, videos, torch.from_numpy(cls_np).cuda(), W, 4)
        v0, v1 = wval[0, 0].cpu().numpy(), wval[0, 1].cpu().numpy()
        nw0 = R.num_windows(len0, W)
        last = [i for i in range(nw0) if max((i - 1) * S, 0) <= len0 - 1 < (i - 1) * S + W]       # windows that hold the last row
        assert abs(v0[0] - 3) < 1e-5 and (v0 < 3.5).all() and sorted(widx[0, 0, :len(last)].tolist()) == last, (W, len0)
        assert abs(v1[0] - 6) < 1e-5 and abs(v1[1] - 6) < 1e-5 and v1[2] < 1.5 and widx[0, 1, :2].tolist() == [0, 1], (W, len0)
        assert rslot[0, :2].tolist() == [1, 0]


# ------------------------------------------------------------------------------------------------ isolation
def test_holes_and_unsearched_videos_are_neither_written_nor_read():
    """Five videos with holes between them, three of them searched.  Holes are quiet NaNs; the run is repeated with the holes
    and the unsearched videos' rows overwritten by 1e30 (a read of any of them would score ~1e30): the outputs do not change by
    a bit, and the buffer -- arena, holes, the 1e30 frame around it -- is untouched by either scan."""
    videos = R.stacked([91, 200, 46, 333, 45], gaps=[2, 1, 0, 7, 3])
    arena_np = R.build_arena(videos, 256, seed=21, capacity=videos[-1][0] + 45 + 6)
    subset = [videos[3], videos[0], videos[2]]                          # out of order: the table sorts by row0
    cls = _queries(5, 256, 8)
    whole, arena = _device_arena(arena_np)
    before = whole.clone()
    got = _assert_contract(arena, subset, cls, 90, 20, n_rank=2)
    assert torch.equal(_bits(whole), _bits(before))
    keep = np.zeros(arena_np.shape[0], dtype=bool)
    for row0, n in subset:
        keep[row0:row0 + n] = True
    hostile = arena_np.copy()
    hostile[~keep] = 1e30
    whole2, arena2 = _device_arena(hostile)
    before2 = whole2.clone()
    again = _assert_contract(arena2, subset, cls, 90, 20, n_rank=2)
    assert torch.equal(_bits(whole2), _bits(before2))
    for a, b in zip(got[:4], again[:4]):
        assert torch.equal(_bits(a), _bits(b))
    assert float(got[1][torch.isfinite(got[1])].abs().max()) <= 1.0 + 1e-5     # unit rows only: nothing of the 1e30 got in


def test_a_refused_scan_writes_nothing():
    videos = R.stacked([91, 46])
    _, arena = _device_arena(R.build_arena(videos, 256, seed=2))
    rc, widx, wval, rslot, rval, _ = _scan(arena, videos, _queries(2, 256, 1), 90, 20, 2, ws_short=1)
    from cone_amd import _lib
    assert rc == -3 and "library_scan: workspace too small" in _lib.load().cone_last_error().decode()
    for t in (widx, wval, rslot, rval):
        assert bool((_bits(t) == POISON).all())


# ------------------------------------------------------------------------------------------------ through the model
_LOCS, _REFS = {}, {}


def _localizer(kind="default", **extra):
    """One localizer per checkpoint kind for the whole module (tests/test_library_gpu.py's kinds)."""
    from cone_amd.localizator import CONELocalizator, LOCALIZER_OPT
    key = (kind, tuple(sorted(extra.items())))
    if key not in _LOCS:
        kw = dict(default={}, txt_pos=dict(use_txt_pos=True), pre_norm=dict(pre_norm=True), general=dict(hidden_dim=128, nheads=4))[kind]
        sd = synth.make_state_dict(SimpleNamespace(**dict(LOCALIZER_OPT, **kw)), 5)
        _LOCS[key] = CONELocalizator(state_dict={k: torch.from_numpy(v) for k, v in sd.items()}, **kw, **extra)
    return _LOCS[key]


def _video(ctx_l, seed=0):
    return torch.randn(ctx_l, 256, generator=torch.Generator().manual_seed(1000 + seed + ctx_l)) * 2


def _text_queries(lens, seed=0):
    g = torch.Generator().manual_seed(77 + seed)
    return [(torch.randn(n, 768, generator=g), torch.randn(256, generator=g)) for n in lens]


def _moments(loc, tag, video, query):
    """predict_moment, computed once per (localizer, video, query) and never changed."""
    key = (id(loc), tag)
    if key not in _REFS:
        _REFS[key] = loc.predict_moment(video, query)
        assert len(_REFS[key]) >= 1
    return _REFS[key]


def _best_window_score(lib, vid_id, cls):
    """The video's best window score by the per-video path, on the library's own adapted rows."""
    from cone_amd import ops
    row0, n, _ = lib._videos[vid_id]
    cl = lib._cl
    at = (cl.adapted - lib._arena.data_ptr()) // 4
    rows = lib._arena.view(torch.float32)[at:at + lib._rows.capacity * cl.v_dim].view(-1, cl.v_dim)[row0:row0 + n]
    win = ops.prefilter_scores(rows, cls.reshape(1, -1).cuda(), lib._loc.args.max_v_l, frame_scores=False)[1]
    return float(ops.topk_windows(win, 1)[1][0, 0])


def _check_search(loc, lib, ids, videos, queries, tag, n_videos, subset=None):
    pool = list(ids) if subset is None else list(subset)
    got = lib.search(queries, n_videos=n_videos, videos=subset)
    assert len(got) == len(queries)
    for qi, (row, q) in enumerate(zip(got, queries)):
        assert len(row) == min(n_videos, len(pool))
        assert len({v for v, _, _ in row}) == len(row) and all(v in pool for v, _, _ in row)
        scores = {v: _best_window_score(lib, v, q[1]) for v in pool}
        assert [s for _, s, _ in row] == sorted(scores.values(), reverse=True)[:len(row)]     # the best of the pool, descending
        for v, score, moments in row:
            assert score == scores[v]
            assert moments == _moments(loc, (tag, ids.index(v), qi), videos[ids.index(v)], q), (qi, v)
    return got


MIXED_CLIPS = (1, 45, 46, 91, 333, 900, 6000)


def _count_readbacks(monkeypatch):
    calls = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (calls.append(1) if t.is_cuda else None, real(t, *a, **k))[1])
    return calls


def test_search_over_the_seven_mixed_videos_equals_predict_moment(monkeypatch):
    """Window counts 2 .. 135 (K = 2, 2, 3, 4, 9, 20, 20: one scan at K = 20 serves all); 1 and 5 queries, n_videos 1, 3, all, a
    subset; after remove + add into the hole; rank_videos lists every video once; two read-backs a search, one a ranking."""
    loc = _localizer()
    videos = [_video(n) for n in MIXED_CLIPS]
    queries = _text_queries([1, 7, 20, 12, 3], seed=3)
    with loc.open_library(sum(MIXED_CLIPS) + 10) as lib:
        ids = [lib.add(v) for v in videos]
        for qs in (queries[:1], queries):
            for n in (1, 3, 7):
                _check_search(loc, lib, ids, videos, qs, "mixed", n)
        _check_search(loc, lib, ids, videos, queries, "mixed", 2, subset=[ids[5], ids[0], ids[3]])
        _check_search(loc, lib, ids, videos, queries[:1], "mixed", 50, subset=[ids[6]])
        ranked = lib.rank_videos(queries, videos=ids)
        assert all(sorted(v for v, _ in row) == sorted(ids) for row in ranked)
        assert all(row == sorted(row, key=lambda e: -e[1]) for row in ranked)
        assert [r[:3] for r in lib.rank_videos(queries)] == lib.rank_videos(queries, n_videos=3)
        calls = _count_readbacks(monkeypatch)
        lib.search(queries, n_videos=3)
        assert len(calls) == 2
        lib.rank_videos(queries)
        assert len(calls) == 3
        monkeypatch.undo()
        # remove two videos, add another into the first hole: the cached table is rebuilt, the answers are the new library's
        lib.remove(ids[4])
        lib.remove(ids[1])
        newcomer = _video(300, seed=9)
        new_id = lib.add(newcomer)
        assert lib._videos[new_id][0] == lib._videos[ids[3]][0] + 91
        ids2 = [ids[0], ids[2], ids[3], new_id, ids[5], ids[6]]
        videos2 = [videos[0], videos[2], videos[3], newcomer, videos[5], videos[6]]
        got = _check_search(loc, lib, ids2, videos2, queries, "mixed-2", 6)
        assert all(ids[4] not in [v for v, _, _ in row] and ids[1] not in [v for v, _, _ in row] for row in got)
        with pytest.raises(ValueError, match="unknown or removed video id"):
            lib.search(queries, videos=[ids[4]])


@pytest.mark.parametrize("kind", ["txt_pos", "pre_norm", "general"])
def test_search_with_other_checkpoint_kinds(kind):
    loc = _localizer(kind)
    clips = (333, 91, 900)
    videos = [_video(n, seed=4) for n in clips]
    queries = _text_queries([7, 20, 3], seed=13)
    with loc.open_library(sum(clips)) as lib:
        ids = [lib.add(v) for v in videos]
        _check_search(loc, lib, ids, videos, queries, "kinds", 2)


def test_more_than_64_queries_are_cut_into_scans():
    loc = _localizer()
    videos = [_video(n, seed=6) for n in (333, 200)]
    queries = _text_queries([(1, 7, 20, 12, 3)[i % 5] for i in range(66)], seed=5)
    with loc.open_library(600) as lib:
        ids = [lib.add(v) for v in videos]
        got = lib.search(queries, n_videos=1)
        one_by_one = [lib.search([q], n_videos=1)[0] for q in (queries[0], queries[63], queries[64], queries[65])]
        assert [got[0], got[63], got[64], got[65]] == one_by_one
        for i in (0, 64, 65):
            v, _, moments = got[i][0]
            assert moments == loc.predict_moment(videos[ids.index(v)], queries[i])


def test_a_bf16_library_refuses_the_search_by_name():
    from cone_amd import _lib
    loc = _localizer(prefilter_bf16=True)
    q = _text_queries([7], seed=17)
    with loc.open_library(400) as lib:
        lib.add(_video(200, seed=6))
        for call in (lib.search, lib.rank_videos):
            with pytest.raises(_lib.ConeHipError, match="library_scan: CONE_SESSION_BF16 libraries are not supported"):
                call(q)
