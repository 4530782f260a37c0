"""Library moment search on the GPU.

Kernel level: ``cone_corpus_fuse_nms`` on dictated tables (tests/corpus_refs.py), every buffer a slice of a poisoned buffer with
guards, compared bit for bit with ``pool_ref``; a pool of one segment against the existing ``cone_fuse_nms``.

The candidates entry: ``cone_library_localize_candidates``' rows, pushed per pair through ``ops.fuse_nms``, are the ragged call's
answers with ``==``.

``search_moments``: the returned lists equal ``pool_ref`` on the read-back candidates of the pairs ``search_windows`` reports, and
on one video they are a localizer's ``predict_moment`` at ``topk_window`` = the video's share."""
import ctypes as C

import numpy as np
import pytest
import torch

import backend_refs as B
import corpus_refs as R
import test_library_budget_gpu as T            # its localizers, videos and queries: built once for both modules

pytestmark = pytest.mark.gpu

POISON = 0x7EADBEEF
GUARD = 64
PARAMS = ((0.5, 100, 5), (0.5, 100, 1), (0.5, 100, 100), (-1, 100, 5))      # (nms_thd, max_before, max_after)


# ------------------------------------------------------------------------------------------------ the pooled stage C
def _guarded(host, dtype):
    """``host`` (numpy) inside a poisoned device buffer: (whole int32 words, the slice viewed as ``dtype``)."""
    words = max(int(host.nbytes) // 4, 0)
    whole = torch.full((words + 2 * GUARD,), POISON, dtype=torch.int32, device="cuda")
    inner = whole[GUARD:GUARD + words]
    if words:
        inner.copy_(torch.from_numpy(np.ascontiguousarray(host).view(np.int32).reshape(-1)))
    return whole, inner.view(dtype)


def _intact(whole, n_words):
    return bool((whole[:GUARD] == POISON).all()) and bool((whole[GUARD + n_words:] == POISON).all())


def _corpus(cases, thd, mb, ma):
    """cone_corpus_fuse_nms on the queries ``cases``: per query (rows (ma, 5), seg (ma,), n), after every guard has been checked
    and every input found unchanged."""
    from cone_amd import _lib
    lib = _lib.load()
    flat, seg_off, seg_cand, seg_n, seg_tag, _ = R.assemble(cases)
    nq = len(cases)
    ins = [_guarded(flat, torch.float32), _guarded(seg_off, torch.int32), _guarded(seg_cand, torch.int64), _guarded(seg_n, torch.int32),
           _guarded(seg_tag, torch.int32)]
    before = [w.clone() for w, _ in ins]
    outs = [_guarded(np.zeros(nq * ma * 5, np.float64), torch.float64), _guarded(np.zeros(nq * ma, np.int32), torch.int32),
            _guarded(np.zeros(nq, np.int32), torch.int32)]
    for w, inner in outs:
        inner.view(torch.int32).fill_(POISON)
    rc = lib.cone_corpus_fuse_nms(*(C.c_void_p(i.data_ptr()) for _, i in ins), nq, len(seg_n), float(thd), mb, ma,
                                  *(C.c_void_p(o.data_ptr()) for _, o in outs), _lib.stream())
    assert rc == 0, lib.cone_last_error()
    torch.cuda.synchronize()
    for (w, i), b in zip(ins, before):
        assert torch.equal(w, b)
    for w, o in outs:
        assert _intact(w, o.view(torch.int32).numel())
    rows, seg, n = (o.cpu().numpy() for _, o in outs)
    rows, seg = rows.reshape(nq, ma, 5), seg.reshape(nq, ma)
    return [(rows[q], seg[q], int(n[q])) for q in range(nq)]


_POOL_REFS = {}


def _want(key, cand, segs, thd, mb, ma):
    """pool_ref of a named case, computed once."""
    k = (key, thd, mb, ma)
    if k not in _POOL_REFS:
        _POOL_REFS[k] = R.pool_ref(cand, segs, thd, mb, ma)
    return _POOL_REFS[k]


def _check(got, want, note):
    for q, (g, w) in enumerate(zip(got, want)):
        assert g[2] == w[2], (note, q, g[2], w[2])
        assert np.array_equal(g[1], w[1]), (note, q, g[1][:8], w[1][:8])
        assert np.array_equal(R.bits(g[0]), R.bits(w[0])), (note, q)


def _n_seg(n, i):
    """The segment count of a dictated pool of ``n`` candidates: 1, 2, 64, 256 by turns, at most one segment per candidate."""
    return min(n, (1, 2, 64, 256)[i % 4])


@pytest.mark.parametrize("family", R.FAMILIES)
def test_pooled_kernel_equals_the_model_at_every_pool_size(family):
    """The ten pool sizes of one family, cut into 1, 2, 64 or 256 segments, and a query without segments among them, in ONE
    launch per parameter set."""
    keys = [(family, n, _n_seg(n, i + R.FAMILIES.index(family))) for i, n in enumerate(R.POOL_SIZES)]
    cases = [R.pool_case(f, R.split(n, s, n)) for f, n, s in keys]
    cases.insert(3, (np.zeros((0, 4), np.float32), []))
    keys.insert(3, ("empty", 0, 0))
    for thd, mb, ma in PARAMS:
        got = _corpus(cases, thd, mb, ma)
        _check(got, [_want(k, c, s, thd, mb, ma) for k, (c, s) in zip(keys, cases)], (family, thd, mb, ma))
        assert got[3][2] == 0 and (got[3][1] == -1).all() and not got[3][0].any()


@pytest.mark.parametrize("family", ["distinct", "dup_in_segment", "span_under_every_tag", "fused_ties"])
def test_pooled_kernel_on_many_small_segments_and_on_uneven_ones(family):
    """1, 2, 64 and 256 segments of 1 - 4 rows each, and one query of three segments with 10 / 200 / 1 rows."""
    rng = np.random.default_rng(7)
    sizes = [rng.integers(1, 5, k).tolist() for k in (1, 2, 64, 256)] + [[10, 200, 1]]
    cases = [R.pool_case(family, s, seed=3, n_tags=2 + i) for i, s in enumerate(sizes)]
    for thd, mb, ma in PARAMS[:3]:
        got = _corpus(cases, thd, mb, ma)
        _check(got, [_want((family, "segs", i), c, s, thd, mb, ma) for i, (c, s) in enumerate(cases)], (family, thd, mb, ma))


def test_pooled_kernel_at_every_query_count_with_an_empty_query_among_them():
    cases, keys = [], []
    for i in range(65):
        family = R.FAMILIES[i % len(R.FAMILIES)]
        n = (5, 17, 64, 100, 3, 200, 1, 33)[i % 8]
        if i in (2, 64):
            cases.append((np.zeros((0, 4), np.float32), []))
        else:
            cases.append(R.pool_case(family, R.split(n, min(n, 1 + i % 7), i), seed=i))
        keys.append(("nq", i))
    for nq in (1, 5, 64, 65):
        got = _corpus(cases[:nq], 0.5, 100, 5)
        _check(got, [_want(k, c, s, 0.5, 100, 5) for k, (c, s) in zip(keys[:nq], cases[:nq])], nq)
        assert nq < 3 or got[2][2] == 0


def test_pooled_kernel_on_the_hand_made_tables():
    """The named tables of the CPU tests -- the span under two tags, identical spans in two videos, IoU exactly at and just above
    0.5, two segments of one tag, ties across segments, the cut before the NMS -- in one launch per parameter set."""
    names = sorted(R.HAND_MADE)
    cases = [R.HAND_MADE[n]() for n in names]
    for thd, mb, ma in PARAMS + ((0.5, 3, 5), (0.5, 4, 5)):
        got = _corpus(cases, thd, mb, ma)
        _check(got, [_want(("hand", n), c, s, thd, mb, ma) for n, (c, s) in zip(names, cases)], (thd, mb, ma))
    got = dict(zip(names, _corpus(cases, 0.5, 100, 5)))
    assert got["two_videos"][0][:4, 4].tolist() == [1.5, 0.75, 0.625, 0.5] and got["two_videos"][1].tolist() == [0, 1, 1, 0, -1]
    assert got["iou_edges"][2] == 4 and got["iou_edges"][0][:4, 1].tolist() == [10.0, 20.0, 19.9, 310.0]
    assert got["identical_spans_two_videos"][0][:2, :2].tolist() == [[0.0, 10.0], [0.0, 10.0]]


def test_a_cut_at_max_before_inside_a_run_of_ties_in_a_200_candidate_pool():
    cases = [R.pool_case("cut_in_ties", R.split(200, k, 5), seed=k) for k in (1, 7, 200)]
    got = _corpus(cases, 0.5, 100, 100)
    _check(got, [_want(("cut", i), c, s, 0.5, 100, 100) for i, (c, s) in enumerate(cases)], "cut")
    assert all(g[2] == 100 and len(set(g[0][90:, 4].tolist())) == 1 for g in got)


def test_a_table_above_the_cap_answers_for_its_first_1024_candidates():
    """The clamp that keeps a broken table in bounds (the wrapper never builds one): candidates are taken until the pool holds
    1 024, the segment that crosses the cap is truncated, the ones behind it are empty."""
    rng = np.random.default_rng(11)
    n = 1400
    st = np.round(rng.uniform(0, 5000, n), 2)
    cand = np.stack([st, st + 5, rng.uniform(0, 1, n), rng.uniform(0, 1, n)], 1).astype(np.float32)
    segs = [(0, 600, 1), (600, 300, 2), (900, 400, 1), (1300, 100, 3)]
    capped = [(0, 600, 1), (600, 300, 2), (900, 124, 1)]
    broken = [(cand, segs), (cand, [(0, 1024, 4), (1024, 376, 4)]), (cand, [(0, 100000, 1)]), (cand, [(0, -5, 1), (3, 10, 2)])]
    for thd, mb, ma in ((0.5, 100, 100), (-1, 100, 5)):
        got = _corpus(broken, thd, mb, ma)
        _check(got, [R.pool_ref(cand, capped, thd, mb, ma), R.pool_ref(cand, [(0, 1024, 4)], thd, mb, ma),
                     R.pool_ref(cand, [(0, 1024, 1)], thd, mb, ma), R.pool_ref(cand, [(0, -5, 1), (3, 10, 2)], thd, mb, ma)], "cap")
        assert (got[3][1][:got[3][2]] == 1).all()                              # the ordinal counts the empty segment


@pytest.mark.parametrize("n", [1, 100, 1024])
def test_one_segment_collapses_to_the_existing_kernel(n):
    """The same candidates through cone_fuse_nms: its fused rows and n equal the pooled kernel's on one segment, and with a segment
    per candidate (one tag) the segment ordinals are its idx."""
    from cone_amd import ops
    fams = sorted(B.STAGE_C_FAMILIES)
    cands = [B.stage_c_case(f, n)[0] for f in fams]
    dev = torch.from_numpy(np.stack(cands)).cuda()
    n_valid = torch.full((len(fams),), n, dtype=torch.int32, device="cuda")
    for thd, mb, ma in ((0.5, 100, 5), (0.5, 100, 100), (-1, 200, 5)):
        rows, kept, idx = ops.fuse_nms(dev, n_valid, thd, mb, ma)
        rows, kept, idx = rows[0].cpu().numpy(), kept[0].cpu().numpy(), idx[0].cpu().numpy()
        one = _corpus([(c, [(0, n, 5)]) for c in cands], thd, mb, ma)
        each = _corpus([(c, [(i, 1, 5) for i in range(n)]) for c in cands], thd, mb, ma)
        for q, f in enumerate(fams):
            for got in (one[q], each[q]):
                assert got[2] == kept[q] and np.array_equal(R.bits(got[0]), R.bits(rows[q])), (f, n, thd, mb, ma)
            assert np.array_equal(each[q][1], idx[q]), (f, n)
            assert one[q][1].tolist() == [0] * kept[q] + [-1] * (ma - kept[q])


# ------------------------------------------------------------------------------------------------ the candidates entry
def _candidates(lib, pairs, ks, scan=None, V=0, plan=None):
    """cone_library_localize_candidates on ``pairs`` = [(video id, query, scan query, slot), ...] through the planner's calls, all
    into ONE guarded buffer: (rows (sum k Nq, 4) on the host, first row of every pair)."""
    from cone_amd import library
    Nq = int(lib._loc.args.num_queries)
    vids = [lib._videos[p[0]] for p in pairs]
    calls = plan or library.plan_ragged_calls([v[0] for v in vids], ks)
    total = sum(ks) * Nq
    whole, cand = _guarded(np.zeros(total * 4, np.float32), torch.float32)
    cand.view(torch.int32).fill_(POISON)
    cand = cand.view(total, 4)
    row_of, at = [0] * len(pairs), 0
    for idx in calls:
        for i in idx:
            row_of[i] = at
            at += ks[i] * Nq
        lib._enqueue_ragged([(vids[i][:2], pairs[i][1], pairs[i][2], pairs[i][3]) for i in idx], [ks[i] for i in idx], scan, V,
                            cand=cand[row_of[idx[0]]:])
    torch.cuda.synchronize()
    assert _intact(whole, total * 4)
    host = cand.cpu()
    assert not bool((host.view(torch.int32) == POISON).any())                  # every row of every pair was written
    return host, row_of, calls


def _per_pair(host, row_of, ks, Nq):
    """The candidates of every pair through the existing stage C: predict_moment's lists."""
    from cone_amd import ops
    from cone_amd.session import MAX_AFTER, MAX_BEFORE, NMS_THD
    out = []
    for r0, k in zip(row_of, ks):
        rows, n, _ = ops.fuse_nms(host[r0:r0 + k * Nq].cuda().reshape(1, k * Nq, 4), torch.tensor([k * Nq], dtype=torch.int32, device="cuda"),
                                  NMS_THD, MAX_BEFORE, MAX_AFTER)
        rows, n = rows[0, 0].cpu().tolist(), int(n[0, 0])
        out.append([[r[0], r[1], r[4]] for r in rows[:n]])
    return out


def test_the_candidates_of_a_call_are_the_ragged_calls_before_its_stage_c():
    """The mixed library (1 .. 6 000 clips), pair counts from 1 up to K, the call's own stage A."""
    loc = T._localizer()
    queries = T._queries(T._mixed_lens(5), seed=3)
    with T._mixed_library(loc)[0] as lib:
        ids = list(lib._videos)
        asks = [(v, k) for v, K in enumerate(T.MIXED_K) for k in sorted({1, 2, (K + 1) // 2, K})]
        asks = asks[::2] + asks[1::2]
        pairs = [(ids[v], queries[i % 5], 0, 0) for i, (v, _) in enumerate(asks)]
        ks = [k for _, k in asks]
        host, row_of, calls = _candidates(lib, pairs, ks)
        assert len(calls) == 1
        want = lib.predict_moments([(p[0], p[1]) for p in pairs], windows=ks)
        assert _per_pair(host, row_of, ks, 5) == want
        # a refused call writes nothing: a workspace one byte short
        from cone_amd import _lib
        clib = _lib.load()
        whole, cand = _guarded(np.zeros(4 * 5 * 4, np.float32), torch.float32)
        cand.view(torch.int32).fill_(POISON)
        i32 = C.c_int32 * 1
        v = lib._videos[ids[5]]
        args = (loc.localizator._h(), C.byref(lib._cl), i32(v[0]), i32(v[1]))
        tok, cls = queries[0][0].cuda().contiguous(), queries[0][1].cuda().reshape(1, -1).contiguous()
        n = clib.cone_library_localize_candidates_workspace(*args, i32(tok.shape[0]), 1, i32(4), C.byref(lib._params), 0)
        ws = lib._ws.get(n, loc.device)
        rc = clib.cone_library_localize_candidates(*args, _lib.ptr(tok), i32(tok.shape[0]), 1, _lib.ptr(cls), i32(4), C.byref(lib._params),
                                                   None, None, None, None, 0, 0, 0, _lib.ptr(cand), _lib.ptr(ws), n - 1, _lib.stream())
        torch.cuda.synchronize()
        assert rc == -3 and "library_localize_candidates: workspace too small" in clib.cone_last_error().decode()
        assert bool((whole == POISON).all())


def test_the_candidates_entry_on_a_scans_lists_and_65_pairs_across_two_calls():
    loc = T._localizer()
    queries = T._queries(T._mixed_lens(3), seed=11)
    with T._mixed_library(loc)[0] as lib:
        ids = list(lib._videos)
        table = lib._table(None, ids)
        widx, wval, _ = lib._scan(table, queries, 1)
        scan = (0, queries, widx, wval)
        slot_of = {v: s for s, v in enumerate(table[0])}
        vs = [(2, 3, 4, 5, 6)[i % 5] for i in range(65)]                       # K = 3, 4, 9, 20, 20
        ks = [1 + (i * 5) % T.MIXED_K[v] for i, v in enumerate(vs)]
        pairs = [(ids[v], queries[i % 3], i % 3, slot_of[ids[v]]) for i, v in enumerate(vs)]
        host, row_of, calls = _candidates(lib, pairs, ks, scan, len(ids))
        assert [len(c) for c in calls] == [64, 1]
        own, own_rows, _ = _candidates(lib, pairs, ks)                         # the call's own stage A: the same bits
        assert own_rows == row_of and torch.equal(host.view(torch.int32), own.view(torch.int32))
        assert _per_pair(host, row_of, ks, 5) == lib.predict_moments([(p[0], p[1]) for p in pairs], windows=ks)


# ------------------------------------------------------------------------------------------------ search_moments
def _pool_of(lib, queries, W, subset=None):
    """Per query: (the pairs search_windows reports, pool_ref on their read-back candidates as search_moments' list)."""
    from cone_amd.session import MAX_BEFORE, NMS_THD
    rows = lib.search_windows(queries, n_windows=W, videos=subset)
    out = []
    for q, row in zip(queries, rows):
        pairs, ks = [(v, q, 0, 0) for v, _, _, _ in row], [k for _, _, k, _ in row]
        if not pairs:
            out.append((row, None))
            continue
        host, row_of, _ = _candidates(lib, pairs, ks)
        Nq = int(lib._loc.args.num_queries)
        segs = [(r0, k * Nq, i) for i, (r0, k) in enumerate(zip(row_of, ks))]
        out.append((row, lambda M, host=host, segs=segs, row=row: R.moments_of(
            *R.pool_ref(host.numpy(), segs, NMS_THD, MAX_BEFORE, M), [v for v, _, _, _ in row])))
    return out


@pytest.mark.parametrize("W", [1, 5, 20, 64])
def test_search_moments_is_the_pooled_stage_c_of_the_budgets_pairs(W):
    loc = T._localizer()
    queries, videos = T._search_case()
    with T._search_library(loc, videos)[0] as lib:
        pools = _pool_of(lib, queries[:2], W)
        if W == 20:
            assert all(len(row) >= 3 for row, _ in pools)                      # at least three videos receive windows
        for M in (5, 1, 100):
            got = lib.search_moments(queries[:2], n_windows=W, n_moments=M)
            for (row, ref), mine in zip(pools, got):
                assert mine == ref(M), (W, M)
                assert 1 <= len(mine) <= M and {v for v, _ in mine} <= {v for v, _, _, _ in row}
                assert [m[2] for _, m in mine] == sorted((m[2] for _, m in mine), reverse=True)
        if W >= 20:
            assert len({v for v, _ in lib.search_moments(queries[:1], n_windows=W, n_moments=100)[0]}) >= 3


def test_search_moments_on_one_video_is_predict_moment_at_the_videos_share():
    loc = T._localizer()
    queries, videos = T._search_case()
    with T._search_library(loc, videos)[0] as lib:
        ids = list(lib._videos)
        for i, W in ((5, 7), (1, 20), (0, 1)):                                 # K = 20, 6, 2: the share is min(W, K)
            k = min(W, lib._videos[ids[i]][2])
            want = T._reference(T._localizer(topk_window=k), ("moments", i), videos, [(i, queries[0])])[0]
            got = lib.search_moments(queries[:1], n_windows=W, n_moments=5, videos=[ids[i]])[0]
            assert [v for v, _ in got] == [ids[i]] * len(got) and [m for _, m in got] == want, (i, W)
    with loc.open_library(1000) as lib:
        vid = lib.add(videos[5])
        want = T._reference(T._localizer(topk_window=7), ("moments", 5), videos, [(5, queries[0])])[0]
        assert [m for _, m in lib.search_moments(queries[:1], n_windows=7, n_moments=5)[0]] == want
        assert lib.search_moments(queries[:1], n_windows=7)[0][0][0] == vid


def test_search_moments_over_a_subset_and_when_slots_and_rows_change():
    loc = T._localizer()
    queries, videos = T._search_case()
    with T._search_library(loc, videos)[0] as lib:
        ids = list(lib._videos)
        sub = [ids[5], ids[2], ids[6], ids[0]]
        (row, ref), = _pool_of(lib, queries[:1], 20, subset=sub)
        got = lib.search_moments(queries[:1], n_windows=20, videos=sub)[0]
        assert got == ref(5) and {v for v, _ in got} <= set(sub)
        assert lib.search_moments(queries[:2]) == lib.search_moments(queries[:2], n_windows=20, n_moments=5)      # the defaults
        base = lib.search_moments(queries[:2], n_windows=20, n_moments=10)
        lib.remove(ids[0])
        newcomer = lib.add(T._video(30, seed=77))
        assert lib._videos[newcomer][0] == 0                                    # into the hole
        assert lib.search_moments(queries[:2], n_windows=20, n_moments=10) == base
        lib.remove(newcomer)                                                    # every slot shifts
        assert lib.search_moments(queries[:2], n_windows=20, n_moments=10) == base
        assert lib.compact() == sum(T.SEARCH_CLIPS) - 45                        # every row moves
        assert lib.search_moments(queries[:2], n_windows=20, n_moments=10) == base


def test_65_queries_equal_one_by_one_calls_in_two_read_backs(monkeypatch):
    loc = T._localizer()
    queries, videos = T._search_case()
    many = [queries[i % 3] for i in range(65)]
    with T._search_library(loc, videos)[0] as lib:
        calls = T._count_readbacks(monkeypatch)
        got = lib.search_moments(many, n_windows=5)
        assert len(calls) == 2
        got1 = lib.search_moments(queries[:1], n_windows=20)
        assert len(calls) == 4
        monkeypatch.undo()
        one_by_one = [lib.search_moments([q], n_windows=5)[0] for q in queries]
        assert len(got) == 65 and all(got[i] == one_by_one[i % 3] for i in range(65))
        assert got1 == lib.search_moments(queries[:1], n_windows=20) and all(len(g) >= 1 for g in got)


def test_search_moments_on_a_general_checkpoint():
    loc = T._localizer("general")
    queries = T._queries(T._mixed_lens(2), seed=13)
    videos = [T._video(n, seed=4) for n in (333, 91, 900)]
    videos[2][400] = 32 * queries[0][1] / queries[0][1].norm()
    videos[0][100] = 24 * queries[0][1] / queries[0][1].norm()
    with loc.open_library(sum(v.shape[0] for v in videos)) as lib:
        ids = [lib.add(v) for v in videos]
        for (row, ref), mine in zip(_pool_of(lib, queries, 12), lib.search_moments(queries, n_windows=12, n_moments=8)):
            assert mine == ref(8) and len(row) >= 2 and {v for v, _ in mine} <= set(ids)
