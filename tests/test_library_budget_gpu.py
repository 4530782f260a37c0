"""Library window budgets on the GPU.

Kernel level: ``cone_library_budget`` on dictated lists (tests/budget_refs.py: hand-made, descending per list, decoupled from any
video), every output inside a poisoned, guarded buffer, compared bit for bit with ``budget_ref``.

The ragged call: ``predict_moments(..., windows=[k, ...])`` against the library's own uniform entry at that k (``lib._enqueue``:
code that was there before), and ``ragged=True`` against ``CONELocalizator.predict_moment`` -- with ``==``.

``search_windows``: the pairs and counts equal ``budget_ref`` on the scan's lists, the scores are ``rank_videos``', and the moments
of a video that receives k windows ``==`` a localizer of the same weights with ``topk_window = k``."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import budget_refs as R
from cone_amd import synth

pytestmark = pytest.mark.gpu

POISON = 0x7EADBEEF
GUARD = 64


# ------------------------------------------------------------------------------------------------ the budget kernel
def _guarded(n, dtype):
    whole = torch.full((n + 2 * GUARD,), POISON, dtype=torch.int32, device="cuda")
    return whole, whole[GUARD:GUARD + n].view(dtype)


def _budget(wval, W, ws_short=0):
    """cone_library_budget on device lists (nq, V, K): (rc, n_pairs, pair_slot, pair_k, pair_best as int32 words), after every
    guard and the workspace's ends have been checked."""
    from cone_amd import _lib
    lib = _lib.load()
    nq, V, K = wval.shape
    n_ws = lib.cone_library_budget_workspace(nq, V, K, W)
    assert n_ws > 0, lib.cone_last_error()
    ws_whole = torch.full((n_ws + 512,), 0x5A, dtype=torch.uint8, device="cuda")
    at = (-ws_whole.data_ptr()) % 256
    outs = [_guarded(nq, torch.int32), _guarded(nq * W, torch.int32), _guarded(nq * W, torch.int32), _guarded(nq * W, torch.float32)]
    rc = lib.cone_library_budget(_lib.ptr(wval, torch.float32), nq, V, K, W, *(C.c_void_p(o[1].data_ptr()) for o in outs),
                                 C.c_void_p(ws_whole.data_ptr() + at), n_ws - ws_short, _lib.stream())
    torch.cuda.synchronize()
    for whole, inner in outs:
        assert bool((whole[:GUARD] == POISON).all()) and bool((whole[GUARD + inner.numel():] == POISON).all())
    assert bool((ws_whole[:at] == 0x5A).all()) and bool((ws_whole[at + n_ws:] == 0x5A).all())
    n, slot, k, best = (o[1] for o in outs)
    return rc, n.cpu().numpy(), slot.view(nq, W).cpu().numpy(), k.view(nq, W).cpu().numpy(), best.view(torch.int32).view(nq, W).cpu().numpy()


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("V,K", R.SHAPES)
def test_budget_kernel_equals_the_model_bit_for_bit(V, K, family):
    """Every budget and query count of the issue on one (shape, family): the lists are generated for 64 queries and ranked once;
    1 and 5 queries are their first rows.  The two tie families put their tie at the W-th place: generated per W."""
    per_w = family.startswith("tie_at_w")
    made = None
    for W in R.BUDGETS:
        if made is None or per_w:
            wval_np, _ = R.dictated(V, K, 64, family, W)
            made = (wval_np, R.ranked_order(wval_np), torch.from_numpy(wval_np).cuda())
        wval_np, order, wval = made
        for nq in R.N_QUERIES:
            want = R.budget_ref(wval_np[:nq], W, order[:nq])
            rc, n, slot, k, best = _budget(wval[:nq], W)
            assert rc == 0
            assert np.array_equal(n, want[0]), (W, nq)
            assert np.array_equal(slot, want[1]) and np.array_equal(k, want[2]), (W, nq)
            assert np.array_equal(best, want[3].view(np.int32)), (W, nq)                # as words: -inf rows, +inf, the zeros' signs
    if family == "dead_slot" and V > 1:
        assert not (slot[:, :] == V // 2).any()


def test_a_tie_at_the_budgets_end_goes_to_the_lower_slot_and_a_window_of_nan_frames_is_never_chosen():
    """Hand-written: two identical lists (the odd window goes to slot 0), a -inf entry with a live index, -0.0 against +0.0."""
    ninf = float("-inf")
    wval = torch.tensor([[[5., 4., 3.], [5., 4., 3.], [1., ninf, ninf]],
                         [[0.0, -0.0, -1.], [-0.0, 0.0, ninf], [ninf, ninf, ninf]]], device="cuda")
    for W, want_k in ((1, [[1], [1]]), (3, [[2, 1], [2, 1]]), (4, [[2, 2], [2, 2]]), (9, [[3, 3, 1], [3, 2]])):
        rc, n, slot, k, best = _budget(wval, W)
        want = R.budget_ref(wval.cpu().numpy(), W)
        assert rc == 0 and np.array_equal(n, want[0]) and np.array_equal(slot, want[1]) and np.array_equal(k, want[2])
        assert np.array_equal(best, want[3].view(np.int32))
        assert [k[q, :n[q]].tolist() for q in range(2)] == want_k
        assert [slot[q, :n[q]].tolist() for q in range(2)] == [list(range(len(w))) for w in want_k]


def test_a_short_workspace_is_refused_and_nothing_is_written():
    from cone_amd import _lib
    wval = torch.from_numpy(R.dictated(3, 20, 5, "distinct", 20)[0]).cuda()
    rc, n, slot, k, best = _budget(wval, 20, ws_short=1)
    assert rc == -3 and "library_budget: workspace too small" in _lib.load().cone_last_error().decode()
    for t in (n, slot, k, best):
        assert (t == POISON).all()


# ------------------------------------------------------------------------------------------------ through the model
_LOCS, _REFS, _SD = {}, {}, {}


def _state_dict(kw):
    from cone_amd.localizator import LOCALIZER_OPT
    key = tuple(sorted(kw.items()))
    if key not in _SD:
        sd = synth.make_state_dict(SimpleNamespace(**dict(LOCALIZER_OPT, **kw)), 5)
        _SD[key] = {k: torch.from_numpy(v) for k, v in sd.items()}
    return _SD[key]


def _localizer(kind="default", **extra):
    """One localizer per (checkpoint kind, options) for the whole module; ``topk_window=k`` gives the yardstick of a pair that
    receives k windows: the same state dict, only the window count differs."""
    from cone_amd.localizator import CONELocalizator
    key = (kind, tuple(sorted(extra.items())))
    if key not in _LOCS:
        kw = dict(default={}, txt_pos=dict(use_txt_pos=True), pre_norm=dict(pre_norm=True), general=dict(hidden_dim=128, nheads=4),
                  long=dict(max_v_l=300, topk_window=5))[kind]
        _LOCS[key] = CONELocalizator(state_dict=_state_dict(kw), **dict(kw, **extra))
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


def _uniform(lib, vid_id, query, k):
    """The parent's own entry at K = k for one pair: cone_library_localize through lib._enqueue."""
    from cone_amd.session import VideoSession
    return VideoSession.read_kept(lib._enqueue(k, [(lib._videos[vid_id][:2], query)]).cpu(), 1)[0]


MIXED_CLIPS = (1, 45, 46, 91, 333, 900, 6000)
MIXED_K = (2, 2, 3, 4, 9, 20, 20)


def _mixed_library(loc):
    lib = loc.open_library(sum(MIXED_CLIPS) + 10)
    ids = [lib.add(_video(n)) for n in MIXED_CLIPS]
    assert [lib._videos[i][2] for i in ids] == list(MIXED_K)
    return lib, ids


# ---- windows=[k, ...] against the uniform entry
def test_a_window_count_per_pair_equals_the_uniform_entry_at_that_count(monkeypatch):
    """Every video of the mixed library at k = 1, 2, the middle, K - 1 and K, interleaved so that pairs of one video with
    different k sit next to each other in ONE call; one read-back."""
    from cone_amd import library
    loc = _localizer()
    queries = _queries(_mixed_lens(5), seed=3)
    with _mixed_library(loc)[0] as lib:
        ids = list(lib._videos)
        asks = [(v, k) for v, K in enumerate(MIXED_K) for k in sorted({1, 2, (K + 1) // 2, K - 1, K} - {0})]
        asks = asks[::2] + asks[1::2]                                          # the videos interleaved
        pairs = [(ids[v], queries[i % 5]) for i, (v, _) in enumerate(asks)]
        ks = [k for _, k in asks]
        plan = library.plan_ragged_calls([lib._videos[v][0] for v, _ in pairs], ks)
        assert len(plan) == 1 and len(pairs) == 26
        calls = _count_readbacks(monkeypatch)
        got = lib.predict_moments(pairs, windows=ks)
        assert len(calls) == 1
        monkeypatch.undo()
        for i, ((vid, q), k) in enumerate(zip(pairs, ks)):
            assert got[i] == _uniform(lib, vid, q, k), (i, asks[i])
        with pytest.raises(ValueError, match=r"windows\[0\]=3 not in \[1, 2\]"):
            lib.predict_moments([(ids[0], queries[0])], windows=[3])


SMALL_CLIPS = (91, 333)                                     # K = 4, 9
UNIFORM_WS_BYTES = 12500224                                 # cone_library_localize_workspace of the test's three pairs at K = 2, at d4d17cc


def _uniform_ws_bytes(lib, chunk, K):
    """cone_library_localize_workspace for ``chunk`` = [((row0, ctx_l), (tok, cls)), ...] at K windows a pair."""
    from cone_amd import _lib
    i32 = C.c_int32 * len(chunk)
    return _lib.load().cone_library_localize_workspace(
        lib._loc.localizator._h(), C.byref(lib._cl), i32(*(v[0] for v, _ in chunk)), i32(*(v[1] for v, _ in chunk)),
        i32(*(int(q[0].shape[0]) for _, q in chunk)), len(chunk), K, C.byref(lib._params))


def test_the_one_layout_kernel_serves_mixed_counts_in_a_run_and_leaves_the_uniform_workspace_as_it_was():
    """Three pairs on two short videos with counts [1, K, 2]: the second video's run has mixed counts, one pair has k = 1 -- the
    ragged outputs of the layout kernel (row_q / row_slot / cand_off, n_valid = k Nq) against the uniform entry at each k.  A
    uniform call passes none of the three: its workspace has the size the parent commit gave it."""
    loc = _localizer()
    queries = _queries([7, 20, 3], seed=29)
    with loc.open_library(sum(SMALL_CLIPS)) as lib:
        ids = [lib.add(_video(n, seed=9)) for n in SMALL_CLIPS]
        K = lib._videos[ids[1]][2]
        assert [lib._videos[i][2] for i in ids] == [4, K] and K == 9
        pairs, ks = [(ids[0], queries[0]), (ids[1], queries[1]), (ids[1], queries[2])], [1, K, 2]
        got = lib.predict_moments(pairs, windows=ks)
        for i, ((vid, q), k) in enumerate(zip(pairs, ks)):
            assert got[i] == _uniform(lib, vid, q, k), (i, k)
        n_ws = _uniform_ws_bytes(lib, [(lib._videos[v][:2], q) for v, q in pairs], 2)
        print("uniform workspace bytes:", n_ws)
        assert n_ws == UNIFORM_WS_BYTES


def test_65_ragged_pairs_cross_the_call_limit_and_a_lowered_window_limit_cuts_the_calls(monkeypatch):
    from cone_amd import library
    loc = _localizer()
    queries = _queries(_mixed_lens(65), seed=11)
    with _mixed_library(loc)[0] as lib:
        ids = list(lib._videos)
        vs = [(2, 3, 4)[i % 3] for i in range(65)]                             # K = 3, 4, 9
        ks = [1 + (i * 5) % MIXED_K[v] for i, v in enumerate(vs)]
        pairs = [(ids[v], q) for v, q in zip(vs, queries)]
        want = [_uniform(lib, vid, q, k) for (vid, q), k in zip(pairs, ks)]
        assert [len(c) for c in library.plan_ragged_calls([lib._videos[v][0] for v, _ in pairs], ks)] == [64, 1]
        calls = _count_readbacks(monkeypatch)
        assert lib.predict_moments(pairs, windows=ks) == want
        assert len(calls) == 1
        # the same list with at most 30 windows a call: the planner's other limit
        real, seen = library.plan_ragged_calls, []

        def lowered(video_of, k_of):
            seen.append(real(video_of, k_of, max_windows=30))
            return seen[-1]
        monkeypatch.setattr(library, "plan_ragged_calls", lowered)
        assert lib.predict_moments(pairs, windows=ks) == want
        assert len(calls) == 2 and len(seen[0]) > 5 and all(sum(ks[i] for i in idx) <= 30 for idx in seen[0])


# ---- ragged=True on existing ground
def test_ragged_mixed_videos_in_one_call_each_equal_predict_moment(monkeypatch):
    """tests/test_library_gpu.py's mixed case: K = 2, 2, 3, 4, 9, 20, 20 are five calls there (one per K) and one here."""
    from cone_amd import library
    loc = _localizer()
    videos = [_video(n) for n in MIXED_CLIPS]
    queries = _queries(_mixed_lens(21), seed=3)
    pairs = [(i % 7, q) for i, q in enumerate(queries)]
    want = _reference(loc, "mixed", videos, pairs)
    with _mixed_library(loc)[0] as lib:
        ids = list(lib._videos)
        ask = [(ids[v], q) for v, q in pairs]
        vids = [lib._videos[v] for v, _ in ask]
        assert len(library.plan_calls([v[0] for v in vids], [v[2] for v in vids])) == 5
        assert len(library.plan_ragged_calls([v[0] for v in vids], [v[2] for v in vids])) == 1
        calls = _count_readbacks(monkeypatch)
        got = lib.predict_moments(ask, ragged=True)
        assert len(calls) == 1
        monkeypatch.undo()
        for i in range(21):
            assert got[i] == want[i], (i, MIXED_CLIPS[pairs[i][0]])
        assert lib.predict_moments(ask[::-1], ragged=True) == want[::-1]
        assert lib.predict_moments(ask) == want                                 # the default stays the grouped plan, same answers


@pytest.mark.parametrize("kind", ["txt_pos", "pre_norm", "general", "long"])
def test_ragged_checkpoint_kinds(kind):
    loc = _localizer(kind)
    clips = (1000, 301, 700) if kind == "long" else (333, 91, 900)
    videos = [_video(n, seed=4) for n in clips]
    queries = _queries(_mixed_lens(6), seed=13)
    pairs = [(i % 3, q) for i, q in enumerate(queries)]
    want = _reference(loc, "kinds", videos, pairs)
    with loc.open_library(sum(clips)) as lib:
        ids = [lib.add(v) for v in videos]
        assert len({lib._videos[i][2] for i in ids}) >= 2                      # more than one K in the one call
        assert lib.predict_moments([(ids[v], q) for v, q in pairs], ragged=True) == want


def test_ragged_prefilter_bf16_library_runs_its_own_stage_a():
    from cone_amd import _lib
    loc = _localizer(prefilter_bf16=True)
    queries = _queries(_mixed_lens(6), seed=17)
    videos = [_video(400, seed=5), _video(91, seed=6)]
    videos[0][130:133] = queries[0][1]
    pairs = [(i % 2, q) for i, q in enumerate(queries)]
    want = _reference(loc, "bf16", videos, pairs)
    with loc.open_library(700) as lib:
        assert lib._cl.flags == _lib.SESSION_BF16
        ids = [lib.add(v) for v in videos]
        assert [lib._videos[i][2] for i in ids] == [10, 4]
        ask = [(ids[v], q) for v, q in pairs]
        assert lib.predict_moments(ask, ragged=True) == want
        got = lib.predict_moments(ask, windows=[3, 4, 10, 1, 1, 2])
        assert got[1] == want[1] and got[2] == want[2]
        assert [got[i] for i in (0, 3, 4, 5)] == [_uniform(lib, *ask[i], k) for i, k in ((0, 3), (3, 1), (4, 1), (5, 2))]
        with pytest.raises(_lib.ConeHipError, match="search_windows: CONE_SESSION_BF16 libraries are not supported"):
            lib.search_windows(queries[:1])


# ---- search_windows
SEARCH_CLIPS = (45, 200, 333, 333, 700, 900, 1500)          # windows 2, 6, 9, 9, 17, 21, 35; videos 2 and 3 are identical
# (query, video, clip, weight of the query's cls in the clip): every peak lies in two windows; the weights order the peaks
PEAKS = [(0, 5, 100, .95), (0, 5, 300, .9), (0, 5, 500, .85), (0, 5, 700, .8), (0, 2, 200, .75), (0, 6, 400, .7), (0, 6, 1000, .65),
         (0, 1, 100, .6), (0, 4, 350, .55),
         (1, 6, 100, .95), (1, 6, 500, .9), (1, 6, 900, .85), (1, 6, 1300, .8), (1, 4, 100, .75), (1, 5, 200, .7), (1, 5, 600, .65),
         (1, 1, 50, .6), (1, 2, 100, .55)]


def _search_case():
    queries = _queries([7, 20, 3], seed=41)
    videos = [_video(n, seed=20 + i) for i, n in enumerate(SEARCH_CLIPS)]
    for q, v, clip, t in PEAKS:
        videos[v][clip] = t * 16 * queries[q][1] / queries[q][1].norm() * 2 + (1 - t) * videos[v][clip]
    videos[3] = videos[2].clone()
    return queries, videos


def _search_library(loc, videos, spare=100):
    lib = loc.open_library(sum(SEARCH_CLIPS) + spare)
    return lib, lib.add_many(videos)


def _bits(x):
    return int(np.float32(x).view(np.int32))


def _check_windows(lib, ids, videos, queries, W, subset=None, tag="search"):
    """search_windows against (a) budget_ref on the scan's own lists, (b) rank_videos' scores, (c) a localizer with
    topk_window = k per entry."""
    got = lib.search_windows(queries, n_windows=W, videos=subset)
    sub, pool = lib._search_ids(subset)
    table = lib._table(sub, pool)
    _, wval, _ = lib._scan(table, queries, 1)
    V, K = len(table[0]), int(lib._loc.args.topk_window)
    n, slot, k, best = R.budget_ref(wval.cpu().numpy().reshape(len(queries), V, K), W)
    scores = [dict(row) for row in lib.rank_videos(queries, videos=subset)]
    distinct = set()
    assert len(got) == len(queries)
    for qi, row in enumerate(got):
        assert [(v, kk) for v, _, kk, _ in row] == [(table[0][s], int(c)) for s, c in zip(slot[qi, :n[qi]], k[qi, :n[qi]])], (W, qi)
        assert sum(kk for _, _, kk, _ in row) == min(W, int((wval.reshape(len(queries), -1)[qi] > float("-inf")).sum()))
        for at, (v, score, kk, moments) in enumerate(row):
            assert _bits(score) == _bits(scores[qi][v]) == _bits(best[qi, at])
            distinct.add(kk)
            i = ids.index(v)
            ref = _reference(_localizer(topk_window=kk), (tag, i, qi), videos, [(i, queries[qi])])[0]
            assert moments == ref, (W, qi, v, kk)
    assert len(distinct) <= 8
    return got


@pytest.mark.parametrize("W", [1, 5, 9, 20, 64])
def test_search_windows_spends_its_budget_where_the_peaks_are(W):
    """Budgets that split unevenly over seven videos of 45 .. 1 500 clips; at W = 9 the ninth window of query 0 is the first of a
    tie between the two identical videos and goes to the one that lies first in the arena."""
    loc = _localizer()
    queries, videos = _search_case()
    with _search_library(loc, videos)[0] as lib:
        ids = list(lib._videos)
        got = _check_windows(lib, ids, videos, queries[:2], W)
        row = got[0]
        if W == 1:
            assert [(v, k) for v, _, k, _ in row] == [(ids[5], 1)]
        if W == 9:
            assert [(v, k) for v, _, k, _ in row] == [(ids[5], 8), (ids[2], 1)]
        if W == 20:
            assert len(row) >= 3 and len({k for _, _, k, _ in row}) > 1        # an uneven split
            both = {v: k for v, _, k, _ in row}
            assert both.get(ids[2]) == both.get(ids[3]) and ids[2] in both      # the identical videos: the same share
            assert [v for v, _, _, _ in row].index(ids[2]) + 1 == [v for v, _, _, _ in row].index(ids[3])


def test_search_windows_over_a_subset_and_with_the_default_budget():
    loc = _localizer()
    queries, videos = _search_case()
    with _search_library(loc, videos)[0] as lib:
        ids = list(lib._videos)
        got = _check_windows(lib, ids, videos, queries[:2], 20, subset=[ids[5], ids[2], ids[6], ids[0]], tag="search")
        assert all(v in (ids[5], ids[2], ids[6], ids[0]) for row in got for v, _, _, _ in row)
        assert lib.search_windows(queries[:2]) == lib.search_windows(queries[:2], n_windows=20)     # None: topk_window


def test_a_budget_above_the_librarys_windows_is_search_over_every_video(monkeypatch):
    """Nothing of -inf is chosen: every video gets its own K, the moments are search's (== predict_moment); two read-backs."""
    loc = _localizer()
    queries, videos = _search_case()
    with _search_library(loc, videos)[0] as lib:
        ids = list(lib._videos)
        calls = _count_readbacks(monkeypatch)
        got = lib.search_windows(queries, n_windows=256)
        assert len(calls) == 2
        monkeypatch.undo()
        want = lib.search(queries, n_videos=len(ids))
        for row, ref in zip(got, want):
            assert [(v, s, m) for v, s, _, m in row] == ref
            assert [k for _, _, k, _ in row] == [lib._videos[v][2] for v, _, _, _ in row]
        small = lib.search_windows(queries[:1], n_windows=20, videos=[ids[0], ids[1], ids[2]])[0]   # 2 + 6 + 9 windows < 20
        assert sorted((v, k) for v, _, k, _ in small) == [(ids[0], 2), (ids[1], 6), (ids[2], 9)]
        v, q = 1, queries[0]
        assert dict((e[0], e[3]) for e in small)[ids[v]] == _reference(loc, ("search-full", v), videos, [(v, q)])[0]


def test_search_windows_keeps_ids_and_answers_when_slots_and_rows_change():
    """remove + add into the hole, a removed first video (every slot shifts), compact() (every row moves)."""
    loc = _localizer()
    queries, videos = _search_case()
    with _search_library(loc, videos)[0] as lib:
        ids = list(lib._videos)
        base = lib.search_windows(queries[:2], n_windows=20)
        assert all(v != ids[0] for row in base for v, _, _, _ in row)          # the 45-clip video holds no peak
        lib.remove(ids[0])
        newcomer = lib.add(_video(30, seed=77))
        assert lib._videos[newcomer][0] == 0                                    # into the hole
        assert lib.search_windows(queries[:2], n_windows=20) == base
        lib.remove(newcomer)
        slots_before = lib._table(None, list(lib._videos))[0]
        assert slots_before[0] == ids[1]                                        # every slot has shifted
        assert lib.search_windows(queries[:2], n_windows=20) == base
        assert lib.compact() == sum(SEARCH_CLIPS) - 45
        assert lib._videos[ids[1]][0] == 0
        assert lib.search_windows(queries[:2], n_windows=20) == base
        sub = lib.search_windows(queries[:1], n_windows=5, videos=[ids[5], ids[2]])[0]
        assert [(v, k) for v, _, k, _ in sub] == [(ids[5], 5)]
        assert sub[0][3] == lib.predict_moments([(ids[5], queries[0])], windows=[5])[0]


def test_65_queries_are_two_scans_and_two_read_backs(monkeypatch):
    loc = _localizer()
    queries, videos = _search_case()
    many = [queries[i % 3] for i in range(65)]
    with _search_library(loc, videos)[0] as lib:
        calls = _count_readbacks(monkeypatch)
        got = lib.search_windows(many, n_windows=5)
        assert len(calls) == 2
        monkeypatch.undo()
        one_by_one = [lib.search_windows([q], n_windows=5)[0] for q in queries]
        assert len(got) == 65 and all(got[i] == one_by_one[i % 3] for i in range(65))
        assert [sum(k for _, _, k, _ in row) for row in got] == [5] * 65
