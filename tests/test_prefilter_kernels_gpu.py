"""The exact-fp32 pre-filter scorers on the GPU against tests/prefilter_refs.py: every launch form of frame_score_kernel,
frame_score_mq_kernel, pf_split_queries_kernel + frame_score_mq3_kernel, frame_score_groups_kernel + window_max_seg_kernel and
window_combine_kernel, selected by shape through the public entries, under the derived bounds and the exact / bit-identity
claims of each case family.  EVERY run here is poisoned: the arena and the queries are slices of buffers whose other rows are
1e30, the outputs carry guard elements, the workspace starts as 1e30 (prefilter_refs: "Poison")."""
import ctypes as C

import pytest
import torch

import prefilter_bf16_ref as R
import prefilter_refs as F
import test_gpu_parity as P

pytestmark = pytest.mark.gpu

FAM_W, FAM_N = 35, 17 * 61 - 5           # S = 17 (a full tile + one lane), 61 half windows, the last one of 12 frames; n >= every dv
WORST = {}


def _note(tag, form, worst):
    key = f"{tag}/{form}"
    WORST[key] = max(WORST.get(key, 0.0), worst)


@pytest.fixture(scope="module", autouse=True)
def _record_worst():
    """The worst error / bound per (family, form) of the whole run, recorded once at the end."""
    yield
    for key in sorted(WORST):
        P.record_measured(f"prefilter_kernels[{key}]", worst_err_over_bound=WORST[key])


def _f32(numel, dev):
    return torch.full((numel,), F.POISON, dtype=torch.float32, device=dev)


def _run(case, W, want_fs=True, split=False):
    """One call of cone_prefilter_scores / cone_prefilter_scores_split on the poisoned case.  Returns (fs or None, win) on the
    CPU; the guards of both outputs are checked here."""
    from cone_amd import _lib
    lib, dev = _lib.load(), P._gpu()
    n, dv, nq, S = case.n, case.dv, case.nq, W // 2
    nw = F.n_half(n, W) + 1
    arena, pad = F.poisoned(case.ctx)
    arena = arena.to(dev)
    qbuf, qpad = F.poisoned(case.cls, 2)
    qbuf = qbuf.to(dev)
    vid, cls = arena[pad:pad + n], qbuf[qpad:qpad + nq]
    fsb = F.guarded(nq * n).to(dev) if want_fs else None
    winb = F.guarded(nq * nw).to(dev)
    nbytes = (lib.cone_prefilter_scores_split_workspace(n, nq, W, dv) if split else lib.cone_prefilter_scores_workspace(n, nq, W))
    ws = _f32(nbytes // 4 + 64, dev)
    fs_p = _lib.ptr(fsb[F.GUARD:F.GUARD + nq * n]) if want_fs else None
    win_p = _lib.ptr(winb[F.GUARD:F.GUARD + nq * nw])
    if split:
        assert not want_fs
        _lib.check(lib.cone_prefilter_scores_split(_lib.ptr(vid), n, dv, _lib.ptr(cls), nq, W, S, win_p, _lib.ptr(ws), nbytes,
                                                   _lib.stream()))
    else:
        _lib.check(lib.cone_prefilter_scores(_lib.ptr(vid), n, dv, _lib.ptr(cls), nq, W, S, fs_p, win_p, _lib.ptr(ws), nbytes,
                                             _lib.stream()))
    torch.cuda.synchronize()
    assert F.guards_intact(winb, nq * nw), "win: a guard element was written"
    assert bool((ws[(nbytes + 3) // 4:] == F.POISON).all()), "the workspace was written past its stated size"
    fs = None
    if want_fs:
        assert F.guards_intact(fsb, nq * n), "fs: a guard element was written"
        fs = fsb[F.GUARD:F.GUARD + nq * n].view(nq, n).cpu()
    return fs, winb[F.GUARD:F.GUARD + nq * nw].view(nq, nw).cpu()


def _check(case, W, form, tag, want_fs=True, split=False):
    """Run + verdict; with frame scores asked for, the run without them must give the same window bits."""
    fs, win = _run(case, W, want_fs, split)
    fails, worst = F.verdict(case, W, fs, win, split)
    print(f"[prefilter] {tag} {form} family={case.family} n={case.n} W={W} dv={case.dv} nq={case.nq}: worst={worst:.4g} {fails}")
    _note(case.family, form, worst)
    assert not fails, (tag, form, case.family, fails)
    if want_fs:
        assert F.same(_run(case, W, False, split)[1], win), (tag, "frame_scores=False changes the window bits")
    return fs, win


def _ctx_l(nh, W, short):
    """nh half windows; short: the last one one frame short of full (needs S >= 2), else full."""
    S = W // 2
    return nh * S - (1 if short and S >= 2 else 0)


# ------------------------------------------------------------------------------------------------ streaming form, 1 - 4 queries
def _alone_and_batched(case, W, tag):
    """The 4-query run under the verdict; the same queries alone and in batches of 2 and 3 (3 rides the 4-query launch) must
    have the bits they have in the batch of 4."""
    fs4, win4 = _check(case, W, "stream", tag)
    for rows in ([0], [3], [1, 2], [0, 1, 2], [3, 2, 1]):
        fs, win = _run(F.sub(case, rows), W)
        assert F.same(fs, fs4[rows]) and F.same(win, win4[rows]), (tag, rows)


@pytest.mark.parametrize("W,short", [(2, False), (3, False), (7, False), (7, True)])
@pytest.mark.parametrize("nh", F.STREAM_NH)
def test_streaming_form_across_the_launch_thresholds(nh, W, short):
    """dv 256 at nh = 2047 .. 8193: a workgroup per half window without (<= 2048) and with (2049 .. 4095) a grid-stride -- the
    barrier inside the stride loop --, a wave per half window without (4096 .. 8192) and with (8193) one."""
    _alone_and_batched(F.unit(_ctx_l(nh, W, short), 256, 4, seed=nh), W, f"thresholds[{nh},{W},{short}]")


@pytest.mark.parametrize("dv", [512, 768, 1024])
@pytest.mark.parametrize("nh", F.WIDE_NH)
def test_streaming_form_wide_rows_grid_stride(nh, dv):
    W = 7 if nh == 2049 else 3                      # (S = 3 with a short last half window; S = 1: the arena stays under 40 MB)
    _alone_and_batched(F.unit(_ctx_l(nh, W, True), dv, 4, seed=nh), W, f"wide[{nh},{dv}]")


@pytest.mark.parametrize("W", F.EDGE_W)
@pytest.mark.parametrize("nh", F.EDGE_NH)
def test_streaming_form_row_slot_edges(nh, W):
    """S = 45 / 62 with the last half window 0 .. 5 and S - 1 frames past a multiple of S: every row-slot count of RPW = 4,
    WPH = 4; the unit case with its batch identity and a peak at every structural frame."""
    for n in F.edge_ctx_ls(W, nh):
        _alone_and_batched(F.unit(n, 256, 4, seed=n), W, f"edges[{n},{W}]")
        for c in F.family_cases("peaks", n, 256, 4, W) + F.family_cases("nanrows", n, 256, 4, W):
            _check(c, W, "stream", f"edges[{n},{W}]")


@pytest.mark.parametrize("family", F.FAMILIES)
@pytest.mark.parametrize("dv", F.DVS)
def test_streaming_form_families(dv, family):
    """Every family at S = 17, 61 half windows (the last one short), 4 and 3 queries; pow2 must give the unscaled run's bits."""
    for c in F.family_cases(family, FAM_N, dv, 4, FAM_W):
        fs, win = _check(c, FAM_W, "stream", f"families[{dv}]")
        if family == "pow2":
            fb, wb = _run(F.pow2_base(FAM_N, dv, 4), FAM_W)
            assert F.same(fs, fb) and F.same(win, wb)
    if family in ("peaks", "nanrows"):              # ... and across the WPH switch / under the grid-stride
        for nh, W in ((2049, 7), (4097, 7), (8193, 3)):
            if dv == 256:
                for c in F.family_cases(family, _ctx_l(nh, W, True), dv, 4, W)[:2]:
                    _check(c, W, "stream", f"families[{dv},{nh}]")


def test_one_frame_video_and_frame_zero():
    for dv in F.DVS:
        for nq in (1, 4, 5, 8):
            c = F.peaks(1, dv, nq, [0])
            _check(c, 90, "stream" if nq < 5 else "mq", "one-frame")
            n1 = F.nanrows(1, dv, nq, 90)
            fs, win = _check(n1, 90, "stream" if nq < 5 else "mq", "one-frame-nan")
            assert bool(torch.isnan(fs).all()) and bool((win == float("-inf")).all())
            if nq >= 8:
                assert bool((_check(n1, 90, "split", "one-frame-nan", want_fs=False, split=True)[1] == float("-inf")).all())


# ------------------------------------------------------------------------------------------------ fp32 matrix cores, >= 5 queries
@pytest.mark.parametrize("dv,nq", [(dv, nq) for dv, nqs in F.MQ_NQ.items() for nq in nqs])
def test_matrix_core_form_query_counts(dv, nq):
    """16 / 32 / 64-query passes and the passes that start at q0 = 32 / 64 (dv > 512: 32 queries per launch), with and
    without the frame-score matrix.  The one-hot mirror makes every query its own channel: a pass that read the queries of
    q0 = 0 would be off by an exact mismatch."""
    n = 13 * 17 - 5
    _check(F.unit(n, dv, nq, seed=nq), FAM_W, "mq", f"nq[{dv},{nq}]")
    _check(F.onehot_mirror(n, dv, nq), FAM_W, "mq", f"nq[{dv},{nq}]")


@pytest.mark.parametrize("W", F.MQ_W)
def test_matrix_core_form_tile_edges(W):
    """S = 1 .. 62 at nh = 13 and 25 (12 waves: one and two workgroups, a last wave alone), a short last half window; a
    peak at every structural frame (lanes 16 t - 1, 16 t, the last valid lane of a partial tile)."""
    for nh in (13, 25):
        n = _ctx_l(nh, W, True)
        _check(F.unit(n, 512, 17, seed=W), W, "mq", f"tiles[{W},{nh}]")
        for c in F.family_cases("peaks", n, 512, 48, W) + F.family_cases("nanrows", n, 512, 17, W):
            _check(c, W, "mq", f"tiles[{W},{nh}]")


@pytest.mark.parametrize("nh", [1, 11, 12, 13])
def test_matrix_core_form_few_half_windows(nh):
    for dv in (512, 1024):
        _check(F.unit(_ctx_l(nh, 35, True), dv, 17, seed=nh), 35, "mq", f"nh[{nh},{dv}]")


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("W", [2, 7])
@pytest.mark.parametrize("k", range(4))
def test_matrix_core_form_grid_stride(k, W):
    """nh = 12 CUs - 1, 12 CUs, 12 CUs + 1, 24 CUs + 5: every wave owns one half window; one wave owns two; three rounds."""
    nh = F.mq_grid_nh(_n_cu())[k]
    c = F.unit(_ctx_l(nh, W, True), 512, 5, seed=k)
    _check(c, W, "mq", f"stride[{nh},{W}]")
    if k == 3:
        for fam in ("peaks", "nanrows"):
            _check(F.family_cases(fam, c.n, 512, 33, W)[0], W, "mq", f"stride[{nh},{W}]")


@pytest.mark.parametrize("family", F.FAMILIES)
@pytest.mark.parametrize("dv", F.DVS)
def test_matrix_core_form_families(dv, family):
    """33 queries: at dv > 512 the 33rd runs in the pass with q0 = 32.  The one-hot families must be exact: they pin the
    channel <-> k-slot map of v_mfma_f32_16x16x4_f32 on both operands."""
    for c in F.family_cases(family, FAM_N, dv, 33, FAM_W):
        fs, win = _check(c, FAM_W, "mq", f"families[{dv}]")
        if family == "pow2":
            fb, wb = _run(F.pow2_base(FAM_N, dv, 33), FAM_W)
            assert F.same(fs, fb) and F.same(win, wb)


# ------------------------------------------------------------------------------------------------ split form (opt-in), >= 8 queries
def _split(case, W, tag):
    return _check(case, W, "split", tag, want_fs=False, split=True)[1]


@pytest.mark.parametrize("dv", F.DVS)
@pytest.mark.parametrize("nq", F.SPLIT_NQ)
def test_split_form_query_counts(nq, dv):
    """One, two and three 64-query passes; 13 half windows: the workgroup of the 13th has eleven waves without a tile."""
    n = 13 * 17 - 5
    _split(F.unit(n, dv, nq, seed=nq), FAM_W, f"nq[{dv},{nq}]")
    _split(F.onehot_mirror(n, dv, nq), FAM_W, f"nq[{dv},{nq}]")


@pytest.mark.parametrize("W", F.MQ_W)
def test_split_form_tile_edges(W):
    for nh, dv in ((13, 256), (25, 768)):
        n = _ctx_l(nh, W, True)
        _split(F.unit(n, dv, 17, seed=W), W, f"tiles[{W},{nh}]")
        for c in F.family_cases("peaks", n, dv, 48, W) + F.family_cases("nanrows", n, dv, 17, W):
            _split(c, W, f"tiles[{W},{nh}]")


@pytest.mark.parametrize("dv", F.DVS)
def test_split_form_unequal_tile_counts(dv):
    """The tiles_of / slots bookkeeping on purpose: nh = 1 at S <= 16 (dv 256: two chunk steps, the smallest run of the ring),
    nh = 1 / 11 / 12 / 13, a last half window with fewer tiles (S = 33, ctx_l = 33 k + 1: 3 tiles against 1), and a grid-stride
    in which one wave owns two half windows and all others one (nh = 12 CUs + 1) or fewer rounds (24 CUs + 5)."""
    _split(F.unit(9, dv, 8), 32, f"smallest[{dv}]")
    _split(F.unit(16, dv, 17), 32, f"smallest[{dv}]")
    for nh in (1, 11, 12, 13):
        _split(F.unit(_ctx_l(nh, 35, True), dv, 17, seed=nh), 35, f"nh[{nh},{dv}]")
    for k in (1, 12, 13, 30):
        n = 33 * k + 1
        _split(F.unit(n, dv, 17, seed=k), 67, f"last-tiles[{k},{dv}]")
        _split(F.family_cases("peaks", n, dv, 64, 67)[0], 67, f"last-tiles[{k},{dv}]")
    for nh in F.mq_grid_nh(_n_cu()):
        for W in ((2, 7) if dv == 256 else (3,)):
            _split(F.unit(_ctx_l(nh, W, True), dv, 9, seed=nh), W, f"stride[{nh},{W},{dv}]")


@pytest.mark.parametrize("family", F.FAMILIES)
@pytest.mark.parametrize("dv", F.DVS)
def test_split_form_families(dv, family):
    """The three-piece bound per score; the one-hot families exact (h + m + l == x: test_prefilter_kernels_cpu); pow2 equal to
    the unscaled run bit for bit (pow2_safe: no piece goes subnormal); onehot2 under a bound of ONE product, which a lost
    partial product breaks."""
    for c in F.family_cases(family, FAM_N, dv, 17, FAM_W):
        win = _split(c, FAM_W, f"families[{dv}]")
        if family == "pow2":
            base = F.pow2_base(FAM_N, dv, 17)
            assert F.pow2_safe(base)
            assert F.same(win, _run(base, FAM_W, False, True)[1])


def test_split_entry_falls_back_to_the_fp32_forms_with_their_bits():
    """Fewer than 8 queries through the split entry: the streaming form (1 - 4) and the fp32 matrix-core form (5 - 7)."""
    for nq in (1, 3, 4, 5, 7):
        c = F.unit(13 * 17 - 5, 512, nq, seed=nq)
        assert F.same(_run(c, FAM_W, False, True)[1], _run(c, FAM_W, False, False)[1]), nq
    c = F.unit(13 * 17 - 5, 512, 8)
    assert not torch.equal(_run(c, FAM_W, False, True)[1], _run(c, FAM_W, False, False)[1])       # 8: the split form is on
    from cone_amd import ops
    dev = P._gpu()
    with pytest.raises(ValueError):             # frame scores are not on offer with the split form: refused, never silently fp32
        ops.prefilter_scores(c.ctx.to(dev), c.cls.to(dev), FAM_W, frame_scores=True, split_bf16=True)


# ------------------------------------------------------------------------------------------------ grouped form
def _run_grouped(cases, W):
    """cone_prefilter_batched over several videos (one dv) in ONE poisoned arena, PAD poison rows between them, up to 4
    queries per group.  Returns [(fs, win)] per video, on the CPU; guards checked."""
    from cone_amd import _lib
    lib, dev = _lib.load(), P._gpu()
    dv, S = cases[0].dv, W // 2
    rows, row0, at = [], [], F.PAD
    for c in cases:
        row0.append(at)
        at += c.n + F.PAD
    arena = torch.full((at, dv), F.POISON)
    for c, r in zip(cases, row0):
        arena[r:r + c.n] = c.ctx
    qbuf, qpad = F.poisoned(torch.cat([c.cls for c in cases]), 2)
    g_row0, g_ctx, g_q, q_fs, q_win, q_ctx = [], [], [], [], [], []
    fs_at = win_at = F.GUARD
    q = 0
    for c, r in zip(cases, row0):
        for g in range(0, c.nq, 4):
            live = list(range(q + g, q + min(g + 4, c.nq)))
            g_row0.append(r)
            g_ctx.append(c.n)
            g_q += live + [-1] * (4 - len(live))
        for _ in range(c.nq):
            q_fs.append(fs_at)
            q_win.append(win_at)
            q_ctx.append(c.n)
            fs_at += c.n
            win_at += F.n_half(c.n, W) + 1
        q += c.nq
    nq = q
    fsb, winb = _f32(fs_at + F.GUARD, dev), _f32(win_at + F.GUARD, dev)
    idx = torch.empty(nq, 1, dtype=torch.int32, device=dev)
    t = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)
    a, qb = arena.to(dev), qbuf.to(dev)
    args = (t(g_row0, torch.int64), t(g_ctx, torch.int32), t(g_q, torch.int32), t(q_fs, torch.int64), t(q_win, torch.int64),
            t(q_ctx, torch.int32))
    _lib.check(lib.cone_prefilter_batched(_lib.ptr(a), dv, _lib.ptr(qb[qpad:qpad + nq]), *(C.c_void_p(x.data_ptr()) for x in args[:3]),
                                          len(g_row0), max(c.n for c in cases), *(C.c_void_p(x.data_ptr()) for x in args[3:]), nq, W,
                                          S, _lib.ptr(fsb), _lib.ptr(winb), 1, _lib.ptr(idx), _lib.stream()))
    torch.cuda.synchronize()
    fsb, winb = fsb.cpu(), winb.cpu()
    assert F.guards_intact(fsb, fs_at - F.GUARD) and F.guards_intact(winb, win_at - F.GUARD), "grouped: a guard element was written"
    out, q = [], 0
    for c in cases:
        nw = F.n_half(c.n, W) + 1
        out.append((fsb[q_fs[q]:q_fs[q] + c.nq * c.n].view(c.nq, c.n), winb[q_win[q]:q_win[q] + c.nq * nw].view(c.nq, nw)))
        q += c.nq
    return out


def _check_grouped(cases, W, tag):
    for c, (fs, win) in zip(cases, _run_grouped(cases, W)):
        fails, worst = F.verdict(c, W, fs, win)
        print(f"[prefilter] {tag} grouped family={c.family} n={c.n} W={W} dv={c.dv} nq={c.nq}: worst={worst:.4g} {fails}")
        _note(c.family, "grouped", worst)
        assert not fails, (tag, c.family, fails)
        for g in range(0, c.nq, 4):                         # the single-video streaming entry, bit for bit
            rows = list(range(g, min(g + 4, c.nq)))
            sfs, swin = _run(F.sub(c, rows), W)
            assert F.same(sfs, fs[rows]) and F.same(swin, win[rows]), (tag, c.family, rows)


@pytest.mark.parametrize("dv", F.DVS)
def test_grouped_form_short_videos_and_live_slots(dv):
    """ctx_l = 1 .. 17 with 1 .. 5 and 8 queries (groups of 1 - 4 live slots), odd and even W; NaN rows."""
    for n in F.GROUP_CTX:
        for nq in F.GROUP_NQ:
            W = 5 if (n + nq) % 2 else 4
            _check_grouped([F.unit(n, dv, nq, seed=n)], W, f"short[{dv}]")
        _check_grouped([F.nanrows(n, dv, 3, 5)], 5, f"short-nan[{dv}]")
    from cone_amd import ops
    dev = P._gpu()
    for nq in F.GROUP_NQ:                           # ... and the wrapper that builds the one-video plan: the same bits
        c = F.unit(17, dv, nq, seed=17)
        got = ops.prefilter_window_scores(c.ctx.to(dev), c.cls.to(dev), 5).cpu()
        assert F.same(got, _run_grouped([c], 5)[0][1]), (dv, nq)
    for family in F.FAMILIES:
        _check_grouped(F.family_cases(family, FAM_N, dv, 5, FAM_W)[:1], FAM_W, f"families[{dv}]")


def test_grouped_form_two_videos_share_a_launch():
    a, b = F.unit(333, 256, 5, seed=1), F.nanrows(47, 256, 3, 7, seed=2)
    _check_grouped([a, b, F.peaks(18, 256, 4, [0, 2, 16, 17])], 7, "two-videos")
    _check_grouped([b, a], 6, "two-videos")


def test_grouped_form_grid_stride():
    """32 768 + 9 clips: the 2 048 workgroups of 16 rows take a second round."""
    n = F.GROUP_STRIDE_CLIPS
    _check_grouped([F.unit(n, 256, 2, seed=5)], 90, "stride")
    c = F.peaks(n, 256, 4, [32767, 32768, n - 1, 32770])
    _check_grouped([c], 125, "stride")


# ------------------------------------------------------------------------------------------------ the bf16 scorers' thresholds
@pytest.mark.parametrize("nh", F.STREAM_NH)
def test_bf16_streaming_form_across_the_launch_thresholds(nh):
    """launch_frame_scores_bf16 copies the thresholds of launch_frame_scores: the same nh list under the bf16 contract's own
    bound (prefilter_bf16_ref)."""
    from cone_amd import ops
    dev = P._gpu()
    W = 7 if nh % 2 else 2
    c = F.unit(_ctx_l(nh, W, True), 256, 3, seed=nh)
    _, got = ops.prefilter_scores(ops.rows_to_bf16(c.ctx.to(dev)), c.cls.to(dev), W, frame_scores=False)
    torch.cuda.synchronize()
    win, ab = R.window_scores(c.ctx, c.cls, W)
    bound = R.accumulation_bound(win, ab, 256)
    err = (got.cpu().double() - win).abs()
    _note("unit", "bf16-stream", float((err / bound).max()))
    assert got.shape == win.shape and bool((err <= bound).all()), (nh, float((err / bound).max()))
