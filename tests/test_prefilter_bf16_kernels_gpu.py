"""The bf16 pre-filter scorers on the GPU against tests/prefilter_stage_refs.py (part A): every instantiation of
frame_score_bf16_kernel, frame_score_mq_bf16_kernel<1|2|4> and frame_score_groups_bf16_kernel<1|2> (with win_fill_seg_kernel
and topk_seg_kernel), selected by shape through cone_prefilter_scores_bf16 / cone_prefilter_batched_bf16 -- the entries
behind ops.prefilter_scores and ops.prefilter_batched on a bf16 arena.  Reference: float64 on the bf16-rounded operands;
tolerance: prefilter_bf16_ref.accumulation_bound; the quantum and dictated families must return the float64 value itself.
EVERY run is poisoned: the arena and the queries are slices of buffers whose other rows are 1e30, the outputs carry guards,
the workspace starts as 1e30 and is checked behind its stated size."""
import ctypes as C

import pytest
import torch

import prefilter_refs as F
import prefilter_stage_refs as G
import test_gpu_parity as P

pytestmark = pytest.mark.gpu

WORST, RAN = {}, {}
DVS_STREAM = (32, 96, 256, 480, 512, 544, 992, 1024)
DVS_MQ = (32, 96, 256, 288, 480, 512, 544, 1024)
NQ_MQ = (5, 16, 17, 32, 33, 64, 65, 129)


@pytest.fixture(scope="module", autouse=True)
def _record():
    """Once, at the end: the worst error / bound per (form, family) and the first case that ran each instantiation."""
    yield
    for key in sorted(WORST):
        P.record_measured(f"prefilter_bf16_kernels[{key}]", worst_err_over_bound=WORST[key])
    for inst in sorted(RAN):
        P.record_measured(f"prefilter_bf16_kernels.ran[{inst}]", first_case=RAN[inst][0], cases=RAN[inst][1])


def _ran(inst, tag):
    first, n = RAN.get(inst, (tag, 0))
    RAN[inst] = (first, n + 1)


def _note_launches(case, W, tag):
    nh = F.n_half(case.n, W)
    if case.nq >= 5:
        for q0 in range(0, case.nq, 64):
            rem = case.nq - q0
            _ran(f"frame_score_mq_bf16_kernel<{4 if rem > 32 else 2 if rem > 16 else 1}>", tag)
        return
    rem = case.nq
    while rem > 0:
        qg = 4 if rem >= 3 else rem
        _ran(G.instantiation(qg, case.dv, nh), tag)
        rem -= qg


_ARENA = {}


def _arena16(case):
    """The case's rows rounded to bf16 (torch: round to nearest even) inside a poisoned device buffer; kept for the sub-runs."""
    key = (case.ctx.data_ptr(), tuple(case.ctx.shape))
    if key not in _ARENA:
        _ARENA.clear()
        buf = torch.full((2 * F.PAD + case.n, case.dv), F.POISON).bfloat16()
        buf[F.PAD:F.PAD + case.n] = case.ctx.bfloat16()
        _ARENA[key] = (case.ctx, buf.to(P._gpu()))
    return _ARENA[key][1]


def _f32(numel, dev):
    return torch.full((numel,), F.POISON, dtype=torch.float32, device=dev)


def _run(case, W):
    """cone_prefilter_scores_bf16 on the poisoned case -> win (nq, nw) on the CPU; guards and the workspace tail checked."""
    from cone_amd import _lib
    lib, dev = _lib.load(), P._gpu()
    n, dv, nq, S = case.n, case.dv, case.nq, W // 2
    nw = G.n_windows(n, W)
    vid = _arena16(case)[F.PAD:F.PAD + n]
    qbuf, qpad = F.poisoned(case.cls, 2)
    qbuf = qbuf.to(dev)
    winb = F.guarded(nq * nw).to(dev)
    nbytes = lib.cone_prefilter_scores_bf16_workspace(n, nq, W)
    ws = _f32(nbytes // 4 + 64, dev)
    _lib.check(lib.cone_prefilter_scores_bf16(_lib.ptr(vid), n, dv, _lib.ptr(qbuf[qpad:qpad + nq]), nq, W, S,
                                              _lib.ptr(winb[F.GUARD:F.GUARD + nq * nw]), _lib.ptr(ws), nbytes, _lib.stream()))
    torch.cuda.synchronize()
    assert F.guards_intact(winb, nq * nw), "win: a guard element was written"
    assert bool((ws[(nbytes + 3) // 4:] == F.POISON).all()), "the workspace was written past its stated size"
    return winb[F.GUARD:F.GUARD + nq * nw].view(nq, nw).cpu()


def _check(case, W, form, tag):
    win = _run(case, W)
    fails, worst = G.scorer_verdict(case, W, win)
    print(f"[prefilter16] {tag} {form} family={case.family} n={case.n} W={W} dv={case.dv} nq={case.nq}: worst={worst:.4g} {fails}")
    if case.family not in G.EXACT_FAMILIES:
        WORST[f"{form}/{case.family}"] = max(WORST.get(f"{form}/{case.family}", 0.0), worst)
    _note_launches(case, W, tag)
    assert not fails, (tag, form, case.family, fails)
    return win


def _ctx_l(nh, W, tail):
    """nh half windows, the last one of ``tail`` frames (0: full)."""
    S = W // 2
    return (nh - 1) * S + (tail if 0 < tail < S else S)


# ------------------------------------------------------------------------------------------------ streaming form, 1 - 4 queries
STREAM_NH = (1, 2047, 2048, 2049, 4095, 4096, 8192, 8193)
ROTATION = ((1, 256), (2, 96), (3, 544), (4, 1024), (1, 992), (2, 512), (4, 480), (3, 32))


@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("nh", STREAM_NH)
def test_streaming_form_across_the_launch_thresholds(nh, W):
    """nh = 1 .. 8193 at S = 1: a workgroup per half window (WPH 4) without (<= 2048) and with (2049 .. 4095) a grid-stride,
    a wave per half window (WPH 1) without (4096 .. 8192) and with (8193) one; four (nq, dv) pairs per point, rotated so that
    the eight points meet every QG and both VPL in both forms; quantum and dictated exact, unit under the bound."""
    at = STREAM_NH.index(nh)
    for j in range(4):
        nq, dv = ROTATION[(at + 2 * j + (W & 1)) % 8]
        tag = f"thresholds[{nh},{W}]"
        _check(G.quantum(nh, dv, nq, seed=nh), W, "stream", tag)
        if j == 0:
            _check(G.unit(nh, dv, nq, seed=nh), W, "stream", tag)
            _check(G.scorer_case("dictated", nh, dv, nq, W, seed=W), W, "stream", tag)


@pytest.mark.parametrize("dv", DVS_STREAM)
@pytest.mark.parametrize("nh", [2049, 8193])
def test_streaming_form_every_width_and_query_group_under_the_grid_stride(nh, dv):
    """Both grid-stride regimes x every dv (VPL 1 and 2 with idle lanes on both: 32 .. 480, 544 .. 992) x nq 1 .. 4."""
    W = 5                                                               # S = 2, the last half window of one frame
    n = _ctx_l(nh, W, 1)
    for nq in (1, 2, 3, 4):
        _check(G.quantum(n, dv, nq, seed=dv + nq), W, "stream", f"widths[{nh},{dv}]")
    _check(G.scorer_case("dictated", n, dv, 3, W, seed=1), W, "stream", f"widths[{nh},{dv}]")


@pytest.mark.parametrize("S", [1, 2, 3, 4, 5, 15, 16, 17, 45])
def test_streaming_form_row_slot_edges(S):
    """The row slots of RPW = 4 and the four-wave stride of 16 rows: S = 1 .. 45, odd and even W (the first-frame plane), the
    last half window of 1 and of S - 1 frames, 13 half windows (the dictated family's NaN-only and -inf-only windows)."""
    for W in (2 * S, 2 * S + 1):
        for tail in sorted({1, S - 1} - {0}) if S > 1 else [0]:
            n = _ctx_l(13, W, tail)
            dv = 256 if tail == 1 else 544
            tag = f"slots[{S},{W},{tail}]"
            for fam in ("quantum", "dictated", "unit", "raw"):
                _check(G.scorer_case(fam, n, dv, 3, W, seed=S), W, "stream", tag)
            _check(G.scorer_case("dictated", n, dv, 4, W, seed=S + 1), W, "stream", tag)
    for n in (1, S):                                                    # one frame; one full half window
        for fam in ("quantum", "dictated"):
            _check(G.scorer_case(fam, n, 96, 2, 2 * S + 1), 2 * S + 1, "stream", f"slots[{S},n={n}]")


@pytest.mark.parametrize("dv", [96, 256, 544, 1024])
@pytest.mark.parametrize("nh", [100, 4100])
def test_a_querys_bits_do_not_depend_on_the_launch_it_shares(nh, dv):
    """unit rows (inexact sums): each query alone (QG 1), in pairs (QG 2), in threes (QG 4, one dead slot) and in the batch of
    four has the same bits, in both WPH forms -- and so does quantum x 2^+-20 against quantum."""
    W = 7
    c = G.unit(_ctx_l(nh, W, 2), dv, 4, seed=nh)
    win4 = _check(c, W, "stream", f"bits[{nh},{dv}]")
    for rows in ([0], [1], [2], [3], [1, 2], [2, 1], [0, 1, 2], [3, 2, 1]):      # every slot of QG 1, 2 and 4
        assert F.same(_run(G.sub(c, rows), W), win4[rows]), (nh, dv, rows)
    a, b = G.quantum(c.n, dv, 4, seed=3), G.quantum_up(c.n, dv, 4, seed=3)
    assert torch.equal(_check(a, W, "stream", "bits-quantum"), _check(b, W, "stream", "bits-quantum"))


# ------------------------------------------------------------------------------------------------ bf16 matrix cores, >= 5 queries
@pytest.mark.parametrize("dv", DVS_MQ)
@pytest.mark.parametrize("nq", NQ_MQ)
def test_matrix_core_form_query_counts_and_widths(nq, dv):
    """QT 1 / 2 / 4 and the second and third pass (q0 = 64, 128) with a nearly empty last tile, at every width: one block
    of k-steps (32 .. 256), a SHORT second block (288: 1 of 8 k-steps, 480: 7), two full blocks (512), a short third (544)
    and four (1024).  S = 17: a full tile and one lane; 13 half windows, the last one short."""
    W, n = 35, 13 * 17 - 5
    tag = f"mq[{nq},{dv}]"
    _check(G.quantum(n, dv, nq, seed=nq), W, "mq", tag)
    _check(G.unit(n, dv, nq, seed=nq), W, "mq", tag)
    _check(G.scorer_case("dictated", n, dv, nq, W, seed=nq), W, "mq", tag)
    if dv in (288, 544):
        _check(G.raw(n, dv, nq, seed=nq), W, "mq", tag)


@pytest.mark.parametrize("dv", [288, 544])
@pytest.mark.parametrize("S", [1, 15, 16, 17, 33])
def test_matrix_core_form_tile_edges(S, dv):
    """16-frame tiles: S = 15, 16, 17 (one lane short, full, one lane over), 33 (three tiles), 1; odd and even W; 13 and 25
    half windows (12 waves: a second workgroup of one wave), the last one of one frame."""
    for W in (2 * S, 2 * S + 1):
        for nh, nq in ((13, 17), (25, 33)):
            n = _ctx_l(nh, W, 1)
            for fam in ("quantum", "dictated", "unit"):
                _check(G.scorer_case(fam, n, dv, nq, W, seed=S), W, "mq", f"tiles[{S},{W},{nh},{dv}]")


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("W", [2, 5])
@pytest.mark.parametrize("k", [-1, 0, 1])
def test_matrix_core_form_grid_stride(k, W):
    """nh = 12 CUs - 1, 12 CUs, 12 CUs + 1: every wave owns at most one half window; exactly one; one wave owns two."""
    nh = 12 * _n_cu() + k
    n = _ctx_l(nh, W, 1)
    for fam in ("quantum", "dictated", "unit"):
        _check(G.scorer_case(fam, n, 288, 5, W, seed=k + 2), W, "mq", f"stride[{nh},{W}]")
    _check(G.quantum(n, 544, 33, seed=k + 2), W, "mq", f"stride[{nh},{W}]")


@pytest.mark.parametrize("dv", [96, 288, 544, 1024])
def test_both_forms_give_the_same_bits_on_exact_inputs(dv):
    """quantum: the first four of five queries through the streaming form and all five through the matrix cores."""
    W, n = 35, 13 * 17 - 5
    c = G.quantum(n, dv, 5, seed=dv)
    mq = _check(c, W, "mq", f"forms[{dv}]")
    assert torch.equal(_check(G.sub(c, range(4)), W, "stream", f"forms[{dv}]"), mq[:4])
    assert torch.equal(_run(G.sub(c, [4]), W), mq[4:])


def test_the_ops_wrappers_reach_the_same_entries():
    from cone_amd import ops
    dev = P._gpu()
    for nq in (3, 17):
        c = G.unit(13 * 17 - 5, 288, nq, seed=nq)
        arena = _arena16(c)[F.PAD:F.PAD + c.n]
        fs, win = ops.prefilter_scores(arena, c.cls.to(dev), 35, frame_scores=False)
        assert fs is None and F.same(win.cpu(), _run(c, 35))
        assert torch.equal(ops.rows_to_bf16(c.ctx.to(dev)).view(torch.int16), arena.view(torch.int16))


# ------------------------------------------------------------------------------------------------ grouped form
def _run_grouped(cases, W, k=3):
    """cone_prefilter_batched_bf16 over several videos (one dv) in ONE poisoned bf16 arena, PAD poison rows between them, up
    to 4 queries per group (dead slots -1).  Returns [(win, idx)] per video on the CPU; guards checked."""
    from cone_amd import _lib
    lib, dev = _lib.load(), P._gpu()
    dv, S = cases[0].dv, W // 2
    row0, at = [], F.PAD
    for c in cases:
        row0.append(at)
        at += c.n + F.PAD
    arena = torch.full((at, dv), F.POISON).bfloat16()
    for c, r in zip(cases, row0):
        arena[r:r + c.n] = c.ctx.bfloat16()
    qbuf, qpad = F.poisoned(torch.cat([c.cls for c in cases]), 2)
    g_row0, g_ctx, g_q, q_win, q_ctx = [], [], [], [], []
    win_at, q = F.GUARD, 0
    for c, r in zip(cases, row0):
        for g in range(0, c.nq, 4):
            live = list(range(q + g, q + min(g + 4, c.nq)))
            g_row0.append(r)
            g_ctx.append(c.n)
            g_q += live + [-1] * (4 - len(live))
        for _ in range(c.nq):
            q_win.append(win_at)
            q_ctx.append(c.n)
            win_at += G.n_windows(c.n, W)
        q += c.nq
    nq = q
    winb = _f32(win_at + F.GUARD, dev)
    idxb = torch.full((F.GUARD + nq * k + F.GUARD,), -77, dtype=torch.int32, device=dev)
    t = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)
    a, qb = arena.to(dev), qbuf.to(dev)
    args = (t(g_row0, torch.int64), t(g_ctx, torch.int32), t(g_q, torch.int32), t(q_win, torch.int64), t(q_ctx, torch.int32))
    p = lambda x: C.c_void_p(x.data_ptr())
    _lib.check(lib.cone_prefilter_batched_bf16(_lib.ptr(a), dv, _lib.ptr(qb[qpad:qpad + nq]), p(args[0]), p(args[1]), p(args[2]),
                                               len(g_row0), max(c.n for c in cases), p(args[3]), p(args[4]), nq, W, S,
                                               _lib.ptr(winb), k, _lib.ptr(idxb[F.GUARD:F.GUARD + nq * k]), _lib.stream()))
    torch.cuda.synchronize()
    winb, idxb = winb.cpu(), idxb.cpu()
    assert F.guards_intact(winb, win_at - F.GUARD), "grouped: a window guard element was written"
    assert bool((idxb[:F.GUARD] == -77).all()) and bool((idxb[F.GUARD + nq * k:] == -77).all()), "grouped: an index guard was written"
    idx = idxb[F.GUARD:F.GUARD + nq * k].view(nq, k)
    out, q = [], 0
    for c in cases:
        nw = G.n_windows(c.n, W)
        out.append((winb[q_win[q]:q_win[q] + c.nq * nw].view(c.nq, nw), idx[q:q + c.nq]))
        q += c.nq
    return out


def _check_grouped(cases, W, tag, k=3):
    for c, (win, idx) in zip(cases, _run_grouped(cases, W, k)):
        fails, worst = G.scorer_verdict(c, W, win)
        print(f"[prefilter16] {tag} groups family={c.family} n={c.n} W={W} dv={c.dv} nq={c.nq}: worst={worst:.4g} {fails}")
        if c.family not in G.EXACT_FAMILIES:
            WORST[f"groups/{c.family}"] = max(WORST.get(f"groups/{c.family}", 0.0), worst)
        _ran(f"frame_score_groups_bf16_kernel<{1 if c.dv <= 512 else 2}>", tag)
        assert not fails, (tag, c.family, fails)
        for g in range(0, c.nq, 4):                         # the single-video streaming form, bit for bit
            rows = list(range(g, min(g + 4, c.nq)))
            assert torch.equal(_run(G.sub(c, rows), W), win[rows]), (tag, c.family, rows)
        for q in range(c.nq):                               # topk_seg_kernel on these scores: the stable order, -1 padded
            want = G._stable_desc(win[q].numpy())[:k].tolist()
            assert idx[q].tolist() == want + [-1] * (k - len(want)), (tag, c.family, q)


@pytest.mark.parametrize("dv", [256, 544])
@pytest.mark.parametrize("W", [4, 5, 34, 35])
def test_grouped_form_short_videos_and_live_slots(W, dv):
    """Videos of 1, S - 1, S and S + 1 half windows (the last one short) with 1, 2, 3, 4 and 5 queries -- groups of 1 - 4 live
    slots -- in ONE launch; the dictated family's all-negative, +-0 and -inf scores go through both branches of pf_atomic_max
    (a NaN is dropped), and every window must equal the single-video streaming form's."""
    S = W // 2
    nhs = sorted({1, max(S - 1, 1), S, S + 1})
    for fam in ("dictated", "quantum", "unit"):
        cases = [G.scorer_case(fam, _ctx_l(nh, W, 1), dv, 1 + (j + S) % 5, W, seed=nh + j) for j, nh in enumerate(nhs)]
        _check_grouped(cases, W, f"short[{W},{dv}]")
    _check_grouped([G.scorer_case("dictated", _ctx_l(13, W, 1), dv, nq, W, seed=nq) for nq in (1, 2, 3, 4)], W, f"slots[{W},{dv}]")


@pytest.mark.parametrize("W,dv", [(2, 256), (3, 544), (5, 256)])
def test_grouped_form_block_cap(W, dv):
    """max_nh > 8192: the 2 048 workgroups of four waves take a second round; a short video shares the launch."""
    n = _ctx_l(8200, W, 1)
    _check_grouped([G.scorer_case("dictated", n, dv, 3, W, seed=2), G.quantum(7, dv, 2, seed=1)], W, f"cap[{W},{dv}]")
    _check_grouped([G.unit(n, dv, 2, seed=3)], W, f"cap[{W},{dv}]")


def test_the_batched_wrapper_reaches_the_grouped_entry():
    from cone_amd import ops
    dev = P._gpu()
    c = G.unit(100, 544, 5, seed=9)
    got = ops.prefilter_window_scores(_arena16(c)[F.PAD:F.PAD + c.n], c.cls.to(dev), 7).cpu()
    assert F.same(got, _run_grouped([c], 7)[0][0])
