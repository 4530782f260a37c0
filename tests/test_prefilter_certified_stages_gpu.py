"""pf_index_kernel (part B) and the stages of the certified pre-filter (part C) on the GPU against
tests/prefilter_stage_refs.py, through cone_prefilter_index_bf16 and cone_prefilter_topk_certified.

Part C uses the entry's three independent pointers as an instrument: with DICTATED arenas (frame f of query q is x e_q in the
fp32 arena, c e_q in the bf16 arena, the query a e_q, a hand-written err = (R, N)) every coarse and every exact frame score
is chosen exactly and independently, and the device must return the Python model's idx, val and certified.  The honest runs
(rescore) compare with the exact-fp32 streaming form of each query alone.  EVERY run is poisoned: arenas and queries are
slices of buffers whose other rows are 1e30, outputs carry guards, the workspace starts as 1e30."""
import numpy as np
import pytest
import torch

import prefilter_certified_ref as C
import prefilter_refs as F
import prefilter_stage_refs as G
import test_gpu_parity as P

pytestmark = pytest.mark.gpu

I_GUARD = -77


def _f32(numel, dev):
    return torch.full((numel,), F.POISON, dtype=torch.float32, device=dev)


def _i32(numel, dev):
    return torch.full((numel,), I_GUARD, dtype=torch.int32, device=dev)


def _int_guards_intact(buf, numel):
    b = buf.cpu()
    return bool((b[:F.GUARD] == I_GUARD).all()) and bool((b[F.GUARD + numel:] == I_GUARD).all())


# ------------------------------------------------------------------------------------------------ B: pf_index_kernel
def _index(x):
    """cone_prefilter_index_bf16 on a poisoned slice -> (bits (n_rows, dim) int16, R, N) on the CPU; guards checked."""
    from cone_amd import _lib
    lib, dev = _lib.load(), P._gpu()
    n_rows, dim = x.shape
    xin, pad = F.poisoned(x, 4)
    xin = xin.to(dev)
    outb = torch.full((F.GUARD + n_rows * dim + F.GUARD,), 0x5555, dtype=torch.int16, device=dev)
    errb = F.guarded(2).to(dev)
    _lib.check(lib.cone_prefilter_index_bf16(_lib.ptr(xin[pad:pad + n_rows]), n_rows, dim, _lib.ptr(outb[F.GUARD:F.GUARD + n_rows * dim]),
                                             _lib.ptr(errb[F.GUARD:F.GUARD + 2]), _lib.stream()))
    torch.cuda.synchronize()
    assert F.guards_intact(errb, 2), "err: a guard element was written"
    ob = outb.cpu()
    assert bool((ob[:F.GUARD] == 0x5555).all()) and bool((ob[F.GUARD + n_rows * dim:] == 0x5555).all()), "out: a guard was written"
    R_, N_ = (float(v) for v in errb[F.GUARD:F.GUARD + 2].cpu().double())
    return ob[F.GUARD:F.GUARD + n_rows * dim].view(n_rows, dim), R_, N_


RATIO, PAYLOAD = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _record_index():
    """Once, at the end: the largest measured R / R64 and N / N64 per row kind, and the NaN payloads (device -> torch)."""
    yield
    for key in sorted(RATIO):
        P.record_measured(f"prefilter_index[{key}]", worst_over_f64=RATIO[key])
    for dev_bits, torch_bits in PAYLOAD.items():
        P.record_measured("prefilter_index_nan_payload", device=dev_bits, torch_cpu=torch_bits)


INDEX_SHAPES = [(r, d) for r in (1, 3, 4, 5) for d in (4, 252, 256, 260, 16384)] + [(65537, 4)]


@pytest.mark.parametrize("n_rows,dim", INDEX_SHAPES)
def test_index_bits_and_norms(n_rows, dim):
    """Every row content at every shape: 1 - 5 rows (a workgroup of four waves: fewer rows than waves, as many, one more),
    65 537 rows of dim 4 (the first count past the 16 384-workgroup cap: wave 0 takes rows 0 and 65 536), dim 4 (one lane),
    252 / 256 / 260 (63 lanes, 64, 64 + a second round of one) and 16 384.  out == torch's round to nearest even, bit for bit;
    finite rows: R64 <= R <= R64 (1 + 2^-10)(1 + 2^-16) + 2^-54 and the same for N; non-finite rows as stated below.  (A NaN's
    payload differs: the device stores the quiet NaN 0x7fc0, torch's CPU conversion 0xffff -- compared as NaN, recorded.)"""
    for kind in ("unit", "midpoints", "subnormal", "negzero", "f32max", "nan"):
        x = G.index_rows(n_rows, dim, kind, seed=dim)
        bits, got_R, got_N = _index(x)
        want, R64, N64 = G.index_ref(x)
        nan = torch.isnan(x)
        assert torch.equal(bits[~nan], want[~nan]), (kind, "bf16 bits differ from round-to-nearest-even")
        if bool(nan.any()):                             # a NaN stays a NaN; its payload is recorded, not asserted
            assert bool(torch.isnan(bits[nan].view(torch.bfloat16).float()).all()), kind
            PAYLOAD[hex(int(bits[nan][0]) & 0xffff)] = hex(int(want[nan][0]) & 0xffff)
        if kind == "nan":
            assert got_R != got_R and got_N != got_N, (kind, got_R, got_N)
        elif kind == "f32max":                          # fp32 max -> bf16 +inf: x - bf16(x) = -inf, both norms +inf
            assert got_R == float("inf") and got_N == float("inf"), (kind, got_R, got_N)
        else:
            for name, got, ref in (("R", got_R, R64), ("N", got_N, N64)):
                if ref > 2.0 ** -40:                    # (below: the absolute 2^-55 dominates, a ratio says nothing)
                    RATIO[f"{kind}/{name}"] = max(RATIO.get(f"{kind}/{name}", 0.0), got / ref)
            assert R64 <= got_R <= R64 * G.INDEX_INFLATE + G.INDEX_TINY, (kind, got_R, R64)
            assert N64 <= got_N <= N64 * G.INDEX_INFLATE + G.INDEX_TINY, (kind, got_N, N64)


# ------------------------------------------------------------------------------------------------ C: the certified entry
_DEV, _HELD = {}, []


def _device_arenas(key, make):
    """(vid_f32 slice, vid_bf16 slice) of one case on the device, poisoned around; the last case stays for its reruns."""
    if key not in _DEV:
        _DEV.clear()
        v32, v16 = make()
        dev = P._gpu()
        a32, pad = F.poisoned(v32)
        a16 = torch.full((2 * F.PAD + v16.shape[0], v16.shape[1]), F.POISON).bfloat16()
        a16[F.PAD:F.PAD + v16.shape[0]] = v16
        n = v32.shape[0]
        _DEV[key] = (a32.to(dev)[pad:pad + n], a16.to(dev)[F.PAD:F.PAD + n])
    return _DEV[key][:2]


def _topk(v32, v16, err, cls, W, k, n_cand):
    """cone_prefilter_topk_certified on device slices -> (idx (nq, k), val (nq, k), certified (nq,)) on the CPU; guards and
    the workspace tail checked."""
    from cone_amd import _lib
    lib, dev = _lib.load(), P._gpu()
    n, dv = v32.shape
    nq = cls.shape[0]
    qbuf, qpad = F.poisoned(cls, 2)
    qbuf = qbuf.to(dev)
    errt = torch.tensor([err[0], err[1]], dtype=torch.float32, device=dev)
    idxb, valb, certb = _i32(2 * F.GUARD + nq * k, dev), F.guarded(nq * k).to(dev), _i32(2 * F.GUARD + nq, dev)
    nbytes = lib.cone_prefilter_topk_certified_workspace(n, nq, W, k, n_cand)
    assert nbytes > 0
    ws = _f32(nbytes // 4 + 64, dev)
    sl = lambda b, m: b[F.GUARD:F.GUARD + m]
    _lib.check(lib.cone_prefilter_topk_certified(_lib.ptr(v32), _lib.ptr(v16), n, dv, _lib.ptr(qbuf[qpad:qpad + nq]), nq, W, W // 2, k,
                                                 n_cand, _lib.ptr(errt), _lib.ptr(sl(idxb, nq * k)), _lib.ptr(sl(valb, nq * k)),
                                                 _lib.ptr(sl(certb, nq)), _lib.ptr(ws), nbytes, _lib.stream()))
    torch.cuda.synchronize()
    assert _int_guards_intact(idxb, nq * k) and _int_guards_intact(certb, nq) and F.guards_intact(valb, nq * k), "a guard was written"
    assert bool((ws[(nbytes + 3) // 4:] == F.POISON).all()), "the workspace was written past its stated size"
    return sl(idxb, nq * k).view(nq, k).cpu(), sl(valb, nq * k).view(nq, k).cpu(), sl(certb, nq).cpu()


def _check_dictated(case, R=None, N=None, want_cert=None):
    """The device against the stage model on one dictated case (R, N: this run's err, default the case's)."""
    R = case.R if R is None else R
    N = case.N if N is None else N
    v32, v16 = _device_arenas(id(case), lambda: G.dictated_arenas(case))
    _HELD[:] = [case]                                   # (the cached arenas' case stays alive: its id stays its own)
    idx, val, cert = _topk(v32, v16, (R, N), case.cls, case.W, case.k, case.n_cand)
    m_idx, m_val, m_cert, _ = G.stage_model(case, R=R, N=N)
    print(f"[certified] {case.name} R={R} N={N}: certified={cert.tolist()} model={m_cert.tolist()}")
    assert cert.tolist() == m_cert.tolist(), (case.name, R, N)
    assert torch.equal(idx, m_idx), (case.name, "idx", cert.tolist())
    assert torch.equal(val, m_val), (case.name, "val", cert.tolist())
    if want_cert is not None:
        assert cert.tolist() == want_cert, (case.name, R, N)
    return idx, val, cert


# ---- the candidate set made visible -------------------------------------------------------------------------------------
_SMALL = G.visible_cases_small()


@pytest.mark.parametrize("case", _SMALL, ids=[c.name for c in _SMALL])
def test_candidate_set_is_the_stable_order_first_n_cand(case):
    """k = n_cand, exact above coarse and in its own order, R = N = 0: idx lists exactly the chosen set.  num_window = n_cand
    + 1, 700 and 4 095 - 4 097 (one chunk, one chunk to the last slot, two); every coarse pattern; n_cand 1 .. 256."""
    idx, _, cert = _check_dictated(case)
    if "neg_inf" not in case.name:
        assert cert.tolist() == [1] * case.nq
        assert sorted(idx[0].tolist()) == G.candidate_set(G.windows_of(case.coarse_fs, 2)[0].numpy(), case.n_cand)[0].tolist()
    else:
        assert cert.tolist() == [0] * case.nq           # a set that had to take -inf windows: c_last = -inf


LONG = [("tie_at_seam", 8193, 64, 1), ("tie_at_seam", 8193, 255, 1), ("tie_at_ncand", 8193, 256, 1), ("zeros_mixed", 8193, 65, 1),
        ("tie_at_seam", 65536, 256, 1), ("tie_at_ncand", 65536, 256, 1), ("all_equal", 65536, 256, 1), ("neg_inf", 8193, 128, 1),
        ("tie_at_ncand", 4097, 64, 3), ("tie_at_seam", 8193, 128, 5), ("all_equal", 4097, 63, 5)]


@pytest.mark.parametrize("pattern,nw,n_cand,nq", LONG)
def test_candidate_set_over_chunk_seams(pattern, nw, n_cand, nq):
    """Ties across windows 4095 | 4096 (the chosen windows lie on both sides, the tie group goes on behind them); 3 and 16
    chunks -- at 65 536 windows and n_cand = 256 sixteen chunk sets exactly fill the merge workgroup --; 3 and 5 queries (5:
    the coarse scan on the matrix cores)."""
    case = G.visible_case(pattern, nw, n_cand, seed=nw % 97, nq=nq)
    idx, _, cert = _check_dictated(case)
    if pattern != "neg_inf":
        assert cert.tolist() == [1] * nq
        if pattern == "tie_at_seam":
            assert min(idx[0].tolist()) < 4096 <= max(i for i in idx[0].tolist() if i < 4096 + n_cand)


@pytest.mark.parametrize("nw,n_cand,k", [(8193, 1366, 256), (69633, 256, 256)])
def test_candidate_list_route_agrees(nw, n_cand, k):
    """n_cand x chunks > 4 096 (3 x 1 366; 18 x 256): the candidates come from cone_topk_windows_ws, an ordered list instead
    of a set -- the same windows, the same answer."""
    _check_dictated(G.visible_case("tie_at_ncand", nw, n_cand, seed=7, k=k))
    if nw < 10000:
        _check_dictated(G.visible_case("tie_at_seam", nw, n_cand - 1, seed=8, k=k))         # 3 x 1 365 = 4 095: the set route


# ---- the proof's comparison ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", [1.0, 1 + 2.0 ** -12])
@pytest.mark.parametrize("dv", [256, 1024])
def test_certify_threshold_sits_where_the_header_puts_it(dv, a):
    """g = t - c_last exact; R0 solves E(R0) == g.  R = fp32(R0 (1 - 2^-20)) must certify, fp32(R0 (1 + 2^-20)) must not:
    2^-20 is far above the fp64 evaluation error of E (a few 2^-53) and fp32's spacing of R (2^-24).  a = 1 + 2^-12 is not a
    bf16 value: |qh - q| = 2^-12 and N |qh - q| is part of E."""
    case = G.comparison_case(dv=dv, a=a, name=f"comparison/{dv}/{a}")
    R0 = G.solve_R0(case, 0, case.g)
    below, above = float(np.float32(R0 * (1 - 2.0 ** -20))), float(np.float32(R0 * (1 + 2.0 ** -20)))
    P.record_measured(f"prefilter_certify_threshold[{dv},{a}]", g=case.g, R0=R0)
    _check_dictated(case, R=below, want_cert=[1])
    _check_dictated(case, R=above, want_cert=[0])
    _check_dictated(case, R=float("inf"), want_cert=[0])
    _check_dictated(case, R=below, N=float("nan"), want_cert=[0])
    _check_dictated(case, R=0.0, N=float("inf"), want_cert=[0])


def test_certify_is_strict_and_exact_at_R_N_zero():
    """R = N = 0: E = 2^-113 exactly.  t == c_last must not certify, t = nextafter(c_last) must; t - c_last == E exactly (t =
    2^-113 over c_last = 0) must not (strict), the next float must."""
    one_up = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
    e_up = float(np.nextafter(np.float32(2.0 ** -113), np.float32(1.0)))
    _check_dictated(G.threshold_case(1.0, name="threshold/t==c_last"), want_cert=[0])
    _check_dictated(G.threshold_case(one_up, name="threshold/nextafter"), want_cert=[1])
    _check_dictated(G.threshold_case(2.0 ** -113, c_last=0.0, name="threshold/gap==E"), want_cert=[0])
    _check_dictated(G.threshold_case(e_up, c_last=0.0, name="threshold/gap>E"), want_cert=[1])
    _check_dictated(G.threshold_case(-1.0, c_last=-1.0, name="threshold/negative"), want_cert=[0])


def test_every_window_a_candidate_certifies_whatever_err_says():
    """num_window == n_cand certifies even with err = NaN; num_window == n_cand + 1 does not."""
    nan = float("nan")
    for nc in (2, 64, 200):
        all_in = G.visible_case("distinct", nc, nc, seed=nc, k=min(nc, 8))
        _check_dictated(all_in, R=nan, N=nan, want_cert=[1])
        one_out = G.visible_case("distinct", nc + 1, nc, seed=nc, k=min(nc, 8))
        _check_dictated(one_out, R=nan, N=nan, want_cert=[0])
        _check_dictated(one_out, want_cert=[1])


# ---- rescore ------------------------------------------------------------------------------------------------------------
def _exact_path(vid, cls, W, k):
    """The exact-fp32 path on the device: the streaming form with each query ALONE, then cone_topk_windows."""
    from cone_amd import ops
    nq = cls.shape[0]
    idx = torch.full((nq, k), -1, dtype=torch.int32)
    val = torch.full((nq, k), float("-inf"))
    for q in range(nq):
        _, win = ops.prefilter_scores(vid, cls[q:q + 1].contiguous(), W, frame_scores=False)
        ke = min(k, win.shape[1])
        i, v = ops.topk_windows(win, ke)
        idx[q, :ke], val[q, :ke] = i[0].cpu(), v[0].cpu()
    return idx, val


@pytest.mark.parametrize("dv", [256, 512, 768, 1024])
@pytest.mark.parametrize("W", [2, 3, 5, 63, 64, 65, 127, 128, 129])
def test_rescore_windows_have_the_streaming_forms_bits(W, dv):
    """Honest arenas (unit and raw rows, the shadow and err from cone_prefilter_index_bf16): 40 half windows, the last window
    of 1 frame and of S - 1 frames, n_cand = 16 of 41 windows; planted peaks put window 0 and the last window into the
    top-k.  W = 63 .. 65, 127 .. 129: sixteen waves x four rows = 64 frames per round of pf_rescore_kernel."""
    from cone_amd import _lib
    lib, dev = _lib.load(), P._gpu()
    S, k, n_cand, nq = W // 2, 8, 16, 3
    for fam, tail in ((G.unit, 1), (G.raw, max(S - 1, 1))):
        n = 39 * S + min(tail, S)
        c = fam(n, dv, nq, seed=W)
        amp = float(c.ctx.norm(dim=1).max())
        c.ctx[0] = 2 * amp * c.cls[0]
        c.ctx[n - 1] = 1.5 * amp * c.cls[0] + amp * c.cls[1]
        v32 = F.poisoned(c.ctx)[0].to(dev)[F.PAD:F.PAD + n]
        v16 = torch.full((2 * F.PAD + n, dv), F.POISON, device=dev).bfloat16()[F.PAD:F.PAD + n]      # the shadow: a slice too
        err = torch.empty(2, device=dev)
        _lib.check(lib.cone_prefilter_index_bf16(_lib.ptr(v32), n, dv, _lib.ptr(v16), _lib.ptr(err), _lib.stream()))
        idx, val, cert = _topk(v32, v16, tuple(err.tolist()), c.cls, W, k, n_cand)
        want_idx, want_val = _exact_path(v32, c.cls.to(dev), W, k)
        assert torch.equal(idx, want_idx) and torch.equal(val, want_val), (W, dv, fam.__name__, cert.tolist())
        assert {0, 40} <= set(idx[0].tolist()) and 40 in idx[1].tolist(), (idx.tolist(), cert.tolist())
        P.record_measured(f"prefilter_rescore[{fam.__name__},{W},{dv}]", certified=int(cert.sum()), queries=nq)


def test_rescore_skips_nan_frames_and_a_window_of_nan_scores_minus_inf():
    idx, val, cert = _check_dictated(G.nan_frames_case(4), want_cert=[1])
    _check_dictated(G.nan_frames_case(8), want_cert=[0])
    assert not bool(torch.isnan(val).any())


# ---- fallback -----------------------------------------------------------------------------------------------------------
DVS = (256, 512, 768, 1024)
FLAGS = {1: [(0,), (1,)], 4: [(1, 0, 0, 1), (0, 1, 1, 0)], 5: [(1, 1, 1, 1, 0), (0, 0, 1, 0, 1)],
         9: [(0, 1, 1, 1, 1, 1, 1, 1, 0), (1, 1, 1, 1, 0, 1, 0, 0, 1)]}


@pytest.mark.parametrize("k", [1, 64, 65, 256])
@pytest.mark.parametrize("nq", [1, 4, 5, 9])
def test_fallback_runs_for_exactly_the_uncertified_queries(nq, k):
    """Per query, certified or not by construction (prefilter_stage_refs.mixed_case); in both kinds the largest exact score
    lies OUTSIDE the candidate set, so the certified list and the fallback's differ: a gated-off group (queries 0 - 3 of the
    first 5-query layout, 4 - 7 of the first 9-query one) keeps the certified rows, an uncertified query gets every window's
    top-k.  Then err = +inf forces the fallback for all.  W = 2 and 3 and the four row widths (frame_score_gated_kernel<1..4>,
    the wide form: 2 999 half windows) in turn."""
    for j, flags in enumerate(FLAGS[nq]):
        case = G.mixed_case(flags, 3000, k, W=2 + (j + k) % 2, dv=DVS[(nq + j + k) % 4])
        _check_dictated(case, want_cert=list(flags))
        _check_dictated(case, R=float("inf"), want_cert=[0] * nq)


@pytest.mark.parametrize("k,W,dv", [(64, 2, 256), (65, 3, 512), (256, 2, 768), (256, 5, 1024)])
def test_fallback_merges_ties_across_the_chunk_seam(k, W, dv):
    """8 193 windows = three chunk lists; the uncertified queries' exact scores tie across windows 4095 | 4096, and the k
    best take the tie's lowest indices from both chunks.  8 192 half windows: the narrow form of frame_score_gated_kernel."""
    case = G.mixed_case((0, 1, 0), 8193, k, W=W, seam=True, dv=dv, name="seam")
    idx, _, _ = _check_dictated(case, want_cert=[0, 1, 0])
    got = idx[0].tolist()
    assert any(3600 <= i < 4096 for i in got) and any(4096 <= i < 4600 for i in got), got
    _check_dictated(case, R=float("inf"), want_cert=[0, 0, 0])


def test_fallback_two_merge_levels_with_seam_ties():
    """70 001 windows, k = 256: 18 chunk lists of 256 exceed one merge workgroup (two levels, as the 140 000-row case of
    test_prefilter_certified_gpu.py) -- here with exact ties across the first seam and the outsider in the last chunk."""
    case = G.mixed_case((0, 1), 70001, 256, W=2, seam=True, name="seam2")
    _check_dictated(case, want_cert=[0, 1])
    _check_dictated(case, N=float("inf"), want_cert=[0, 0])
