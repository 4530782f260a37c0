"""Certified library budgets on the GPU, kernel level: ``cone_library_shadow_index`` against ``cone_prefilter_index_bf16`` and
``cone_library_scan_certified`` + ``cone_library_budget`` against ``cone_library_scan`` + ``cone_library_budget`` on the same table,
through the C entries, every output inside a poisoned, guarded buffer.  The models and the dictated inputs:
tests/certified_library_refs.py.

``test_the_bound_holds_on_the_devices_own_scores`` holds |coarse - exact| <= E on device scores per row family and records the
worst ratio (test_gpu_parity.record_measured, lines ``library_certified_bound``: profiles/library_certified_measured.txt)."""
import ctypes as C

import numpy as np
import pytest
import torch

import certified_library_refs as R
import prefilter_stage_refs as P

pytestmark = pytest.mark.gpu

POISON = 0x7EADBEEF
GUARD = 64
FAKE_HANDLE = 0x1000         # the entries compare the handle with the library's and never follow it


# ------------------------------------------------------------------------------------------------ harness
def _guarded(n, dtype):
    whole = torch.full((n + 2 * GUARD,), POISON, dtype=torch.int32, device="cuda")
    return whole, whole[GUARD:GUARD + n].view(dtype)


def _guards_hold(whole, n):
    return bool((whole[:GUARD] == POISON).all()) and bool((whole[GUARD + n:] == POISON).all())


def _aligned(n_bytes, fill=0x5A):
    whole = torch.full((n_bytes + 512,), fill, dtype=torch.uint8, device="cuda")
    at = (-whole.data_ptr()) % 256
    return whole, at, whole[at:at + n_bytes]


def _ends_hold(whole, at, n, fill=0x5A):
    return bool((whole[:at] == fill).all()) and bool((whole[at + n:] == fill).all())


class Lib:
    """A plain fp32 library handle over ``arena`` (capacity, dv) on the device -- only its adapted plane exists -- and a shadow
    arena filled with 0x5A bytes (bf16 1.5e16, measures 1.5e16: a row nobody indexed would win every list and spoil every proof)."""

    def __init__(self, arena):
        from cone_amd import _lib
        self.lib = _lib.load()
        self.arena = arena.contiguous().cuda()
        cap, dv = arena.shape
        self.handle = _lib.Library(FAKE_HANDLE, cap, 0, dv, 256, None, self.arena.data_ptr(), None, None, None)
        n = self.lib.cone_library_shadow_bytes(C.byref(self.handle))
        assert n == -(-cap * dv * 2 // 256) * 256 + -(-cap * 8 // 256) * 256, self.lib.cone_last_error()
        self.sh_whole, self.sh_at, self.sh_bytes = _aligned(n)
        self.sh = _lib.LibraryShadow()
        assert self.lib.cone_library_shadow_open(C.byref(self.handle), C.c_void_p(self.sh_bytes.data_ptr()), n, C.byref(self.sh)) == 0
        self.rows16 = self.sh_bytes[:cap * dv * 2].view(torch.int16).view(cap, dv)
        self.err = self.sh_bytes[self.sh.err - self.sh.rows_bf16:][:cap * 8].view(torch.float32).view(cap, 2)

    def index(self, row0, n):
        from cone_amd import _lib
        rc = self.lib.cone_library_shadow_index(C.c_void_p(FAKE_HANDLE), C.byref(self.handle), C.byref(self.sh), row0, n, _lib.stream())
        torch.cuda.synchronize()
        assert _ends_hold(self.sh_whole, self.sh_at, self.sh_bytes.numel())
        return rc

    def dictate(self, rows_bf16, err):
        """The shadow handed in is NOT the bf16 of the rows: coarse and exact scores are chosen independently."""
        self.rows16.copy_(rows_bf16.view(torch.int16).cuda())
        self.err.copy_(err.float().cuda())


def _table(videos, Wl):
    from cone_amd.library import certified_table
    order, row0, ctx, hb_off, win_off = certified_table(videos, Wl // 2, Wl)
    return order, [torch.from_numpy(x).cuda() for x in (row0, ctx, hb_off, win_off)], int(hb_off[-1]), win_off


def _params(Wl):
    from cone_amd import _lib
    return _lib.SessionParams(Wl, 20, 0.5333, 0.5, 100, 5)


def _scan_certified(L, videos, cls, Wl, K, W, n_cand=0, ws_short=0):
    from cone_amd import _lib
    order, (row0, ctx, hb_off, win_off_d), total_hb, win_off = _table(videos, Wl)
    V, nq, total_win, p = len(videos), cls.shape[0], int(win_off[-1]), _params(Wl)
    n_ws = L.lib.cone_library_scan_certified_workspace(C.byref(L.handle), V, total_hb, total_win, nq, K, W, n_cand)
    assert n_ws > 0, L.lib.cone_last_error()
    ws_whole, at, ws = _aligned(n_ws)
    outs = [_guarded(nq * V * K, torch.int32), _guarded(nq * V * K, torch.float32), _guarded(nq, torch.int32)]
    rc = L.lib.cone_library_scan_certified(C.c_void_p(FAKE_HANDLE), C.byref(L.handle), C.byref(L.sh), _lib.ptr(row0), _lib.ptr(ctx),
                                           _lib.ptr(hb_off), _lib.ptr(win_off_d), V, total_hb, total_win, _lib.ptr(cls, torch.float32),
                                           nq, K, W, n_cand, C.byref(p), *(C.c_void_p(o[1].data_ptr()) for o in outs),
                                           C.c_void_p(ws.data_ptr()), n_ws - ws_short, _lib.stream())
    torch.cuda.synchronize()
    for whole, inner in outs:
        assert _guards_hold(whole, inner.numel())
    assert _ends_hold(ws_whole, at, n_ws)
    widx, wval, cert = (o[1] for o in outs)
    return rc, widx.view(nq, V, K), wval.view(nq, V, K), cert, (order, win_off)


def _scan_plain(L, videos, cls, Wl, K):
    from cone_amd import _lib
    order, (row0, ctx, hb_off, _), total_hb, _ = _table(videos, Wl)
    V, nq, p = len(videos), cls.shape[0], _params(Wl)
    n_ws = L.lib.cone_library_scan_workspace(C.byref(L.handle), V, total_hb, nq, K, 1)
    assert n_ws > 0, L.lib.cone_last_error()
    ws = _aligned(n_ws)[2]
    widx = torch.empty(nq, V, K, dtype=torch.int32, device="cuda")
    wval = torch.empty(nq, V, K, dtype=torch.float32, device="cuda")
    rank = torch.empty(2, nq, dtype=torch.int32, device="cuda")
    assert L.lib.cone_library_scan(C.c_void_p(FAKE_HANDLE), C.byref(L.handle), _lib.ptr(row0), _lib.ptr(ctx), _lib.ptr(hb_off), V, total_hb,
                                   _lib.ptr(cls, torch.float32), nq, K, 1, C.byref(p), _lib.ptr(widx), _lib.ptr(wval),
                                   C.c_void_p(rank[0].data_ptr()), C.c_void_p(rank[1].data_ptr()), C.c_void_p(ws.data_ptr()), n_ws,
                                   _lib.stream()) == 0, L.lib.cone_last_error()
    return widx, wval


def _budget(wval, W):
    """cone_library_budget's four outputs as int32 words on the host."""
    from cone_amd import _lib
    lib = _lib.load()
    nq, V, K = wval.shape
    n_ws = lib.cone_library_budget_workspace(nq, V, K, W)
    ws = _aligned(n_ws)[2]
    out = torch.empty(nq + 3 * nq * W, dtype=torch.int32, device="cuda")
    at = lambda k: C.c_void_p(out.data_ptr() + 4 * (nq + k * nq * W))
    assert lib.cone_library_budget(_lib.ptr(wval.contiguous(), torch.float32), nq, V, K, W, C.c_void_p(out.data_ptr()), at(0), at(1), at(2),
                                   C.c_void_p(ws.data_ptr()), n_ws, _lib.stream()) == 0
    host = out.cpu().numpy()
    return host[:nq], host[nq:nq + nq * W].reshape(nq, W), host[nq + nq * W:nq + 2 * nq * W].reshape(nq, W), host[nq + 2 * nq * W:].reshape(nq, W)


def _words(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _assert_contract(L, videos, cls, Wl, K, W, n_cand=0, want_flags=None, all_certified=False):
    """The contract: for a certified query the budget on the emitted lists == the budget on the fp32 scan's lists, as words, and
    the chosen slots' prefixes are the scan's; every row is well-formed.  Returns the flags."""
    rc, widx, wval, cert, _ = _scan_certified(L, videos, cls, Wl, K, W, n_cand)
    assert rc == 0, L.lib.cone_last_error()
    flags = cert.cpu().numpy()
    assert set(flags.tolist()) <= {0, 1}
    pw, pv = _scan_plain(L, videos, cls, Wl, K)
    got, want = _budget(wval, W), _budget(pv, W)
    gi, gv, wi, wv = widx.cpu().numpy(), _words(wval).reshape(wval.shape), pw.cpu().numpy(), _words(pv).reshape(pv.shape)
    vals = wval.cpu().numpy()
    for q in range(len(flags)):
        if flags[q]:
            for a, b in zip(got, want):
                assert np.array_equal(a[q], b[q]), (q, a[q], b[q])
            for i in range(int(want[0][q])):
                s, k = int(want[1][q, i]), int(want[2][q, i])
                assert np.array_equal(gi[q, s, :k], wi[q, s, :k]) and np.array_equal(gv[q, s, :k], wv[q, s, :k]), (q, s, k)
        lists = np.where(np.isfinite(vals[q]), vals[q], -1e30).astype(np.float64)           # descending, padded behind
        assert (np.diff(lists, axis=1) <= 0).all() and not np.isnan(vals[q]).any()
        assert ((gi[q] == -1) <= (vals[q] == -np.inf)).all()
    if want_flags is not None:
        assert flags.tolist() == list(want_flags), (flags, want_flags)
    if all_certified:
        assert flags.all(), flags
    return flags


def _honest(lengths, dv, seed, gaps=None, scale=1.0):
    """N(0, 1) rows for videos of ``lengths`` (free rows of 1e30 between them with ``gaps``), the shadow indexed over exactly the
    videos' ranges."""
    videos, cap = R.stacked(lengths, gaps)
    g = torch.Generator().manual_seed(1234 + seed)
    arena = torch.full((cap + (gaps[-1] if gaps else 0) + 3, dv), 1e30)
    for r, n in videos:
        arena[r:r + n] = torch.randn(n, dv, generator=g) * scale
    L = Lib(arena)
    for r, n in videos:
        assert L.index(r, n) == 0
    return L, videos


def _unit_queries(nq, dv, seed):
    g = torch.Generator().manual_seed(99 + seed)
    q = torch.randn(nq, dv, generator=g)
    return (q / q.norm(dim=1, keepdim=True)).cuda()


# ------------------------------------------------------------------------------------------------ cone_library_shadow_index
@pytest.mark.parametrize("kind", ["unit", "midpoints", "subnormal", "f32max", "nan"])
@pytest.mark.parametrize("dv", [256, 768])
def test_shadow_index_equals_the_certified_index_row_by_row(dv, kind):
    """The bf16 bits are cone_prefilter_index_bf16's on the same rows, the max of the per-row measures is its err, bit for bit; rows
    outside the range keep their 0x5A bytes."""
    from cone_amd import _lib
    n, row0, cap = 333, 7, 350
    rows = P.index_rows(n, dv, kind, seed=dv)
    arena = torch.full((cap, dv), 1e30)
    arena[row0:row0 + n] = rows
    L = Lib(arena)
    assert L.index(row0, n) == 0
    want16 = torch.empty(n, dv, dtype=torch.int16, device="cuda")
    want_err = torch.empty(2, dtype=torch.float32, device="cuda")
    assert L.lib.cone_prefilter_index_bf16(_lib.ptr(L.arena[row0:row0 + n]), n, dv, _lib.ptr(want16), _lib.ptr(want_err), _lib.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(L.rows16[row0:row0 + n], want16)
    number = ~torch.isnan(rows)                                                # (a NaN's payload is the converter's business)
    assert torch.equal(want16.cpu()[number], rows.bfloat16().view(torch.int16)[number])
    err = L.err[row0:row0 + n]
    bits = err.contiguous().view(torch.int32)
    assert bool((bits >= 0).all())                                             # non-negative numbers or the positive quiet NaN: ordered like ints
    assert torch.equal(bits.max(dim=0).values, want_err.view(torch.int32))
    if kind == "nan":
        bad = torch.isnan(err).any(dim=1).nonzero().flatten().tolist()
        assert bad == [n // 3] and bool(torch.isnan(want_err).all())
    if kind == "f32max":
        assert bool(torch.isinf(err[n // 2]).all())
    model = R.row_measures(rows)
    fin = torch.isfinite(model).all(dim=1)
    assert bool((err.cpu().double()[fin] <= model[fin] * (1 + 2.0 ** -16) + 2.0 ** -54).all())
    v, vh = rows.double(), rows.bfloat16().double()
    assert bool((err.cpu().double()[fin, 0] >= (v - vh).norm(dim=1)[fin]).all())
    assert bool((err.cpu().double()[fin, 1] >= torch.maximum(v.norm(dim=1), vh.norm(dim=1))[fin]).all())
    for outside in (L.sh_bytes[:row0 * dv * 2], L.rows16[row0 + n:].view(torch.uint8), L.err[:row0].view(torch.uint8),
                    L.err[row0 + n:].view(torch.uint8)):
        assert bool((outside == 0x5A).all())


# ------------------------------------------------------------------------------------------------ honest arenas: shapes
@pytest.mark.parametrize("nq,K,W", [(1, 1, 1), (4, 20, 3), (5, 3, 20), (64, 20, 256), (5, 1, 20), (4, 3, 256), (4, 2, 5)])
@pytest.mark.parametrize("Wl,layout", [(4, "adjacent"), (5, "adjacent"), (4, "holes"), (5, "holes"), (5, "subset")])
def test_certified_budget_equals_the_fp32_budget_on_every_edge_length(Wl, layout, nq, K, W):
    S = Wl // 2
    lengths = [1, S, S + 1, 2 * S - 1, 2 * S + 1, 300, 2, 411, 1, 37]
    gaps = None if layout == "adjacent" else [(2 * i + 1) % 4 for i in range(len(lengths))]
    L, videos = _honest(lengths, 256, Wl + nq, gaps)
    if layout == "subset":
        every, videos = videos, [videos[i] for i in (8, 5, 0, 3, 7)]           # unlisted videos' rows must not be read
        for r, n in [v for v in every if v not in videos]:
            L.rows16[r:r + n] = 0x5A5A                                          # their shadow rows would win every list
            L.err[r:r + n] = 1e30
            L.arena[r:r + n] = 1e30
    # W <= 3: 128 candidates prove three windows; W = 256: every window of these tables is a candidate.  In between a slot's cap of
    # K < W windows can keep the walk from reaching W among 128 candidates: then the flag is 0 and nothing is claimed.
    _assert_contract(L, videos, _unit_queries(nq, 256, nq), Wl, K, W, all_certified=W <= 3 or W == 256)


@pytest.mark.parametrize("n_big,want_chunks", [(8180, 1), (8190, 2)])
def test_the_window_row_just_below_and_above_one_chunk(n_big, want_chunks):
    """total_win = 4 096 resp. 4 101 at S = 2: exactly one chunk of 4 096, then two."""
    lengths = [3, n_big, 1]
    L, videos = _honest(lengths, 256, n_big)
    total_win = sum(R.num_windows(n, 4) for n in lengths)
    assert -(-total_win // 4096) == want_chunks
    _assert_contract(L, videos, _unit_queries(5, 256, 3), 4, 20, 20, all_certified=True)


def test_the_multi_level_merge_2048_candidates_of_three_chunks():
    lengths = [5000, 7, 9000, 2500]
    L, videos = _honest(lengths, 256, 77)
    assert -(-sum(R.num_windows(n, 4) for n in lengths) // 4096) == 3
    _assert_contract(L, videos, _unit_queries(4, 256, 8), 4, 256, 256, n_cand=2048, all_certified=True)
    _assert_contract(L, videos, _unit_queries(2, 256, 9), 4, 20, 20, n_cand=4096, all_certified=True)      # the two-set merge of 8 192


def test_dv_768_and_a_short_workspace():
    from cone_amd import _lib
    L, videos = _honest([1, 45, 46, 91, 400], 768, 5, gaps=[0, 3, 0, 2, 1])
    cls = _unit_queries(5, 768, 4)
    _assert_contract(L, videos, cls, 90, 20, 20, all_certified=True)
    _assert_contract(L, videos, cls[:3], 125, 20, 60, all_certified=True)
    _assert_contract(L, videos, cls, 90, 20, 3, 5)                                # fewer candidates than windows: a real proof
    rc, widx, wval, cert, _ = _scan_certified(L, videos, cls, 90, 20, 20, ws_short=1)
    assert rc == -3 and "library_scan_certified: workspace too small" in _lib.load().cone_last_error().decode()
    assert bool((widx == POISON).all()) and bool((cert == POISON).all())


# ------------------------------------------------------------------------------------------------ dictated, decoupled arenas
def _dictated(coarse, exact, R_, N_, dv=256, hole_every=0):
    """One-clip videos: slot s has two windows (0 and 1: both cover its one clip), coarse score coarse[q][s], exact score
    exact[q][s]; every row's measures are (R_, N_).  Returns (L, videos, cls, flat coarse row, flat exact row, win_off)."""
    coarse, exact = torch.as_tensor(coarse, dtype=torch.float32), torch.as_tensor(exact, dtype=torch.float32)
    nq, V = coarse.shape
    videos, cap = R.stacked([1] * V, [hole_every] * V if hole_every else None)
    arena, shadow, cls = R.dictated_arenas(videos, cap + 2, [coarse[:, s:s + 1] for s in range(V)], [exact[:, s:s + 1] for s in range(V)], dv)
    L = Lib(arena)
    err = torch.full((cap + 2, 2), 1e30)
    for r, n in videos:
        err[r:r + n, 0], err[r:r + n, 1] = R_, N_
    L.dictate(shadow, err)
    flat = lambda x: np.repeat(np.where(np.isnan(x.numpy()), -np.inf, x.numpy()), 2, axis=1)
    return L, videos, cls.cuda(), flat(coarse), flat(exact), np.arange(0, 2 * V + 1, 2)


def _model_flags(coarse, exact, win_off, K, W, n_cand, E):
    _, _, flags, margin = R.certified_model(coarse, exact, win_off, K, W, n_cand, E)
    return flags, margin


@pytest.mark.parametrize("K", [1, 2])
def test_the_threshold_from_both_sides(K):
    """40 one-clip videos, W = 4 windows, 10 candidates (the five best videos' window pairs).  Query 0: margin 4 E, query 1: 2 E,
    query 2: 0 (t == c_last), query 3: negative.  Flags from the model; the margins are exact in fp32 by construction."""
    V, Wb, n_cand, N_ = 40, 4, 10, 1.0
    E1 = R.unit_query_bound(2.0 ** -6, N_, 256)
    unit = 2.0 ** -4                                                              # E1 ~ 2^-6: margins in multiples of 2^-4 >= 4 E
    coarse = np.tile(np.arange(V, 0, -1, dtype=np.float32) * 4, (4, 1))           # 160, 156, ...: candidates = slots 0 .. 4, c_last = 144
    exact = coarse.copy()
    n_take = 4 if K == 1 else 2                                                   # the walk's W-th window lies in slot 3 (K = 1) or 1 (K = 2)
    for q, m in enumerate((unit, 2 * E1 * 1.001, 0.0, -8.0)):
        exact[q, n_take - 1] = np.float32(144 + m)
        exact[q, n_take:5] = np.float32(144 + m) - np.arange(1, 6 - n_take, dtype=np.float32) * 2.0 ** -3
    L, videos, cls, fc, fe, win_off = _dictated(coarse, exact, 2.0 ** -6, N_)
    flags, margin = _model_flags(fc, fe, win_off, K, Wb, n_cand, E1)
    assert margin[0] >= 2 * E1 and margin[1] >= 2 * E1 and margin[2] == 0 and margin[3] < 0 and flags.tolist() == [1, 1, 0, 0]
    _assert_contract(L, videos, cls, 4, K, Wb, n_cand, want_flags=flags)


def test_ties_at_the_n_cand_th_coarse_place_and_across_a_chunk_seam():
    """Equal coarse scores at the set's edge: the lower flat index is the candidate.  4 200 one-clip videos put the tie's two
    windows into different chunks of 4 096.  The higher index holds the better exact score: were it chosen, the lists change."""
    V, K, Wb, seen = 4200, 2, 5, []
    coarse = np.full((1, V), 1.0, dtype=np.float32)
    coarse[0, [5, 9, 2047, 2048, 3000]] = [9, 8, 5, 5, 5]                         # flat windows 4094, 4095 | 4096, 4097 | 6000, 6001 tie at 5
    exact = coarse.copy()
    exact[0, 2048], exact[0, 3000] = 7.5, 7.75
    for n_cand in (5, 6, 7):                                                      # the edge inside slot 2047, between the chunks, inside slot 2048
        L, videos, cls, fc, fe, win_off = _dictated(coarse, exact, 2.0 ** -6, 1.0)
        flags, _ = _model_flags(fc, fe, win_off, K, Wb, n_cand, R.unit_query_bound(2.0 ** -6, 1.0, 256))
        rc, widx, wval, cert, _ = _scan_certified(L, videos, cls, 4, K, Wb, n_cand)
        assert rc == 0 and cert.cpu().tolist() == flags.tolist()
        seen += flags.tolist()
        mw, mv, _, _ = R.certified_model(fc, fe, win_off, K, Wb, n_cand, 1.0)
        assert np.array_equal(widx.cpu().numpy(), mw) and np.array_equal(_words(wval).reshape(mv.shape), mv.view(np.int32))
        assert (widx[0, 3000] == -1).all() and bool((widx[0, 2048, 0] >= 0) == (n_cand >= 7))
    assert seen == [0, 0, 1]            # t == 5 == c_last twice; with slot 2048's first window in the set t = 7.5 clears it


def test_two_identical_videos_do_not_certify_unless_every_window_is_a_candidate():
    lengths = [30, 30, 9]
    L, videos = _honest(lengths, 256, 11)
    L.arena[videos[1][0]:videos[1][0] + 30] = L.arena[videos[0][0]:videos[0][0] + 30]
    assert L.index(videos[1][0], 30) == 0
    cls = _unit_queries(4, 256, 2)
    total = sum(R.num_windows(n, 4) for n in lengths)                             # 16 + 16 + 6
    for W_, n_cand in ((1, 1), (3, 3), (5, 5)):                                   # an odd count: a twin is cut off at the set's edge, the
        flags = _assert_contract(L, videos, cls, 4, 20, W_, n_cand)               # last taken window IS the weakest candidate or its twin
        assert not flags.any(), (W_, n_cand, flags)
    _assert_contract(L, videos, cls, 4, 20, 3, 7)                                 # (the tie inside the set: whatever the flag, the contract)
    _assert_contract(L, videos, cls, 4, 20, 5, total, all_certified=True)


def test_a_video_of_nan_rows_is_never_chosen_and_nothing_certifies():
    lengths = [40, 25, 60]
    L, videos = _honest(lengths, 256, 13)
    L.arena[videos[1][0]:videos[1][0] + 25] = float("nan")
    assert L.index(videos[1][0], 25) == 0
    assert bool(torch.isnan(L.err[videos[1][0]:videos[1][0] + 25]).all())
    cls = _unit_queries(1, 256, 6)
    rc, widx, wval, cert, _ = _scan_certified(L, videos, cls, 4, 20, 5, 8)
    assert rc == 0 and cert.cpu().tolist() == [0]                                 # R is NaN: the sticky maximum
    assert bool((wval[0, 1] == float("-inf")).all())                              # its windows score -inf wherever they are listed
    n, slot, _, _ = _budget(wval, 5)
    assert 1 not in slot[0, :n[0]].tolist()
    total = sum(R.num_windows(n_, 4) for n_ in lengths)
    _assert_contract(L, videos, cls, 4, 20, 5, total, want_flags=[1])             # every window a candidate: no bound is needed


def test_an_all_minus_inf_query_and_fewer_finite_windows_than_the_budget():
    V = 30
    coarse = np.tile(np.arange(V, 0, -1, dtype=np.float32), (1, 1))
    exact = np.full((1, V), np.nan, dtype=np.float32)                             # every clip NaN in the fp32 arena: every exact window -inf
    L, videos, cls, fc, fe, win_off = _dictated(coarse, exact, 2.0 ** -6, 1.0)
    _assert_contract(L, videos, cls, 4, 2, 4, 10, want_flags=[0])
    rc, widx, wval, cert, _ = _scan_certified(L, videos, cls, 4, 2, 4, 2 * V)
    assert cert.cpu().tolist() == [1] and _budget(wval, 4)[0].tolist() == [0]     # all candidates; the budget spends nothing
    exact[0, :3] = [3.0, 2.0, 1.0]                                                # three finite videos (6 windows), a budget of 10
    L, videos, cls, fc, fe, win_off = _dictated(coarse, exact, 2.0 ** -6, 1.0)
    flags, _ = _model_flags(fc, fe, win_off, 2, 10, 20, R.unit_query_bound(2.0 ** -6, 1.0, 256))
    assert flags.tolist() == [0]
    _assert_contract(L, videos, cls, 4, 2, 10, 20, want_flags=[0])
    _assert_contract(L, videos, cls, 4, 2, 10, 2 * V, want_flags=[1])


@pytest.mark.parametrize("name", sorted(R.DICTATED))
def test_the_named_dictated_cases_equal_the_fault_free_model(name):
    """The cases of certified_library_refs.DICTATED -- the ones its ``catches()`` table is computed on -- on the device: flags and
    every list equal the model without a planted error.  ``threshold_eq`` / ``threshold_above`` sit AT the proof's threshold: with
    the dictated measures R = 2^-6, N = 0 and a query e_0, E = 2^-6 (1 + 2^-10) has the same bits in numpy and in the kernel's fp64
    (the 2^-113 term is below half an ulp), and the margins E and E + 2^-16 are exact fp32 differences."""
    case = R.DICTATED[name]
    coarse, exact, win_off, err = R.case_inputs(case)
    V = len(case["coarse"])
    videos, cap = R.stacked([1] * V)
    arena, shadow, cls = R.dictated_arenas(videos, cap + 2, [torch.tensor(case["coarse"][s:s + 1])[None] for s in range(V)],
                                           [torch.tensor(case["exact"][s:s + 1])[None] for s in range(V)])
    L = Lib(arena)
    L.dictate(shadow, torch.cat([err, torch.full((2, 2), 1e30)]))
    mw, mv, flags = R.run_case(case)
    rc, widx, wval, cert, _ = _scan_certified(L, videos, cls.cuda(), 4, case["K"], case["W"], case["n_cand"])
    assert rc == 0 and cert.cpu().tolist() == flags.tolist(), (name, cert, flags)
    assert np.array_equal(widx.cpu().numpy(), mw) and np.array_equal(_words(wval).reshape(mv.shape), mv.view(np.int32))


# ------------------------------------------------------------------------------------------------ the sweep
SWEEP_LENGTHS = [1, 2, 3, 5, 40, 37, 30, 2, 2, 15]


def sweep_case(seed, dv=256, nq=4):
    g = torch.Generator().manual_seed(4000 + seed)
    videos, cap = R.stacked(SWEEP_LENGTHS)
    arena = torch.randn(cap, dv, generator=g)
    cls = torch.randn(nq, dv, generator=g)
    return videos, arena, cls / cls.norm(dim=1, keepdim=True)


def sweep_model(seed, Wl=4, K=3, W=3):
    """The model's flags and margins for one seed at n_cand = W + 2, and E per query."""
    videos, arena, cls = sweep_case(seed)
    coarse, exact = R.honest_rows(arena, videos, cls, Wl)
    Rm, Nm = R.table_measures(R.row_measures(arena), videos)
    import prefilter_certified_ref as PC
    E = np.asarray([PC.device_bound(cls[q], Rm, Nm, arena.shape[1]) for q in range(cls.shape[0])])
    win_off = np.concatenate([[0], np.cumsum([R.num_windows(n, Wl) for _, n in videos])])
    _, _, flags, margin = R.certified_model(coarse, exact, win_off, K, W, W + 2, E)
    return flags, margin, E


def test_twenty_seeds_at_n_cand_w_plus_2():
    """N(0, 1) rows, unit queries, n_cand = W + 2: certified queries are compared with ==; the flags equal the model's wherever the
    model's margin lies outside [0, 2 E] (inside, the fp32 rounding of the scores may decide); both outcomes occur.  (The float64
    model alone gives both over these seeds: 57 queries certify, 23 do not, 38 margins lie outside [0, 2 E].)"""
    seen, decided = set(), 0
    for seed in range(20):
        videos, arena, cls = sweep_case(seed)
        L = Lib(arena)
        assert L.index(0, arena.shape[0]) == 0
        want, margin, E = sweep_model(seed)
        flags = _assert_contract(L, videos, cls.cuda(), 4, 3, 3, 5)
        for q in range(len(flags)):
            seen.add(int(flags[q]))
            if not np.isnan(margin[q]) and not 0 <= margin[q] <= 2 * E[q]:
                decided += 1
                assert flags[q] == want[q], (seed, q, margin[q], E[q])
    assert seen == {0, 1} and decided >= 20


# ------------------------------------------------------------------------------------------------ the bound, on device scores
BOUND_ROWS = 3000


def _bound_rows(kind, dv):
    g = torch.Generator().manual_seed(dv)
    rows = torch.randn(BOUND_ROWS, dv, generator=g) if kind == "normal" else P.index_rows(BOUND_ROWS, dv, kind, seed=dv)
    cls = torch.randn(4, dv, generator=g)
    return rows, cls / cls.norm(dim=1, keepdim=True)


@pytest.mark.parametrize("kind", ["unit", "midpoints", "subnormal", "normal"])
@pytest.mark.parametrize("dv", [256, 768])
def test_the_bound_holds_on_the_devices_own_scores(dv, kind):
    """|coarse - exact| <= E(q) for every window of 3 000 rows and 4 queries at max_v_l = 90: coarse = cone_prefilter_scores_bf16 on
    the shadow rows cone_library_shadow_index wrote, exact = cone_prefilter_scores on the fp32 rows -- the streaming forms, whose
    bits the two library scans carry --, E from the maxima of the shadow's per-row measures as lib_certify_kernel evaluates it.
    The worst ratio is recorded per family."""
    import prefilter_certified_ref as PC
    from cone_amd import ops
    from test_gpu_parity import record_measured
    rows, cls = _bound_rows(kind, dv)
    L = Lib(rows)
    assert L.index(0, BOUND_ROWS) == 0
    err = L.err.cpu().double()
    Rm, Nm = float(err[:, 0].max()), float(err[:, 1].max())
    assert np.isfinite(Rm) and np.isfinite(Nm)
    _, exact = ops.prefilter_scores(L.arena, cls.cuda(), 90, frame_scores=False)
    _, coarse = ops.prefilter_scores(L.rows16.view(torch.bfloat16), cls.cuda(), 90, frame_scores=False)
    gap = (coarse.double() - exact.double()).abs().cpu()
    E = torch.tensor([PC.device_bound(cls[q], Rm, Nm, dv) for q in range(4)], dtype=torch.float64)
    ratio = float((gap / E[:, None]).max())
    record_measured(f"library_certified_bound[{kind}-{dv}]", worst_gap_over_E=ratio, worst_gap=float(gap.max()), least_E=float(E.min()))
    assert ratio <= 1.0, (kind, dv, ratio)
    if kind != "subnormal":
        assert ratio > 1e-3                                                     # the two scorers do differ: the check is not idle
