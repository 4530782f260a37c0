"""The certified pre-filter on the GPU (cone_prefilter_index_bf16, cone_prefilter_topk_certified, ops.PrefilterIndex): the
index against the float64 restatement (tests/prefilter_certified_ref.py), and the top-k against the exact-fp32 path -- the
streaming form run with each query ALONE, then cone_topk_windows -- bit for bit, whatever the proof says; inputs that must
certify, that must not, a mix of both in one call, a soundness sweep, non-finite rows, graph capture."""
import pytest
import torch

import prefilter_certified_ref as C
import test_gpu_parity as P

pytestmark = pytest.mark.gpu

BASE = (3000, 90, 256, 3, 30)           # (ctx_l, W, dv, nq, k): every axis is taken through its cases around this point


def _unit_rows(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g)
    return x / x.norm(dim=1, keepdim=True)


_CASES = {}


def _case(ctx_l, dv):
    """N(0,1) unit rows and 17 unit queries of one (ctx_l, dv), made once, on the device."""
    if (ctx_l, dv) not in _CASES:
        dev = P._gpu()
        _CASES[(ctx_l, dv)] = (_unit_rows(ctx_l, dv, 21).to(dev), _unit_rows(17, dv, 22).to(dev))
    return _CASES[(ctx_l, dv)]


def _exact(vid, cls, W, k):
    """The exact-fp32 path: per query alone (the streaming form), its stable top-min(k, windows), padded with (-1, -inf)."""
    from cone_amd import ops
    nq = cls.shape[0]
    idx = torch.full((nq, k), -1, dtype=torch.int32, device=vid.device)
    val = torch.full((nq, k), float("-inf"), device=vid.device)
    for q in range(nq):
        _, win = ops.prefilter_scores(vid, cls[q:q + 1].contiguous(), W, frame_scores=False)
        ke = min(k, win.shape[1])
        idx[q, :ke], val[q, :ke] = (t[0] for t in ops.topk_windows(win, ke))
    return idx, val


def _assert_exact(vid, cls, W, k, got, tag):
    idx, val, cert = got
    torch.cuda.synchronize()
    want_idx, want_val = _exact(vid, cls, W, k)
    assert idx.dtype == torch.int32 and cert.dtype == torch.int32 and idx.shape == val.shape == (cls.shape[0], k)
    assert torch.equal(idx, want_idx), (tag, cert.tolist())
    assert torch.equal(val, want_val), (tag, cert.tolist())
    assert bool(((cert == 0) | (cert == 1)).all())
    return cert.tolist()


@pytest.mark.parametrize("n_rows,dim", [(1, 256), (4097, 256), (1000, 1024)])
def test_index_stores_rows_to_bf16_bits_and_measures_the_shadow(n_rows, dim):
    from cone_amd import _lib, ops
    dev = P._gpu()
    x = (_unit_rows(n_rows, dim, 5) * torch.linspace(0.5, 3.0, n_rows)[:, None]).to(dev)
    out = torch.empty(n_rows, dim, dtype=torch.bfloat16, device=dev)
    err = torch.full((2,), float("nan"), device=dev)            # the entry initialises it
    _lib.check(_lib.load().cone_prefilter_index_bf16(_lib.ptr(x), n_rows, dim, _lib.ptr(out), _lib.ptr(err), _lib.stream()))
    assert torch.equal(out.view(torch.int16), ops.rows_to_bf16(x).view(torch.int16))
    R, N = C.index_norms(x.cpu())
    got_R, got_N = (float(v) for v in err.cpu().double())
    P.record_measured(f"prefilter_certified_index[{n_rows},{dim}]", R_over_f64=got_R / R, N_over_f64=got_N / N)
    assert R <= got_R <= 1.01 * R and N <= got_N <= 1.01 * N, (got_R, R, got_N, N)
    index = ops.PrefilterIndex(x)
    assert torch.equal(index.vid16.view(torch.int16), out.view(torch.int16)) and torch.equal(index.err, err)


def _axis_cases():
    c, w, d, q, k = BASE
    S = w // 2
    out = [(c, w, x, q, k) for x in (256, 512, 768, 1024)]
    out += [(c, x, d, q, k) for x in (4, 5)]                    # 1 501 windows: the proof decides; 5: the odd-W first-frame term
    out += [(x, w, d, q, k) for x in (1, S - 1)]                # 2 windows: k larger than the number of windows
    out += [(16400, 4, d, q, k)]                                # 8 201 windows: the two-level top-k
    out += [(c, 4, d, x, k) for x in (1, 5, 17)]                # 5, 17: the matrix-core coarse form
    out += [(c, 4, d, q, 1), (c, w, d, q, 1), (c, w, d, q, 200)]        # k = 1; k = 200 > 68 windows
    out += [(c, 4, x, q, k) for x in (768, 1024)]               # the proof decides (E with gamma(dv)) at the wide rows too
    return out


@pytest.mark.parametrize("ctx_l,W,dv,nq,k", _axis_cases())
def test_topk_equals_the_exact_path_bit_for_bit(ctx_l, W, dv, nq, k):
    from cone_amd import ops
    vid, cls = _case(ctx_l, dv)
    index = ops.PrefilterIndex(vid)
    q = cls[:nq].contiguous()
    cert = _assert_exact(vid, q, W, k, index.topk(q, W, k), (ctx_l, W, dv, nq, k))
    P.record_measured(f"prefilter_certified_equal[{ctx_l},{W},{dv},{nq},{k}]", certified=sum(cert), queries=nq)
    if ops.num_windows(ctx_l, W) <= max(4 * k, 128):            # every window is a candidate
        assert cert == [1] * nq


@pytest.mark.parametrize("ctx_l,n_cand", [(3000, 64), (3000, 1000), (3000, 1501), (16400, 1365), (16400, 2000)])
def test_topk_equals_the_exact_path_for_explicit_candidate_counts(ctx_l, n_cand):
    """n_cand past 256 fills more than one register slot per thread of the certify kernel; 1 501 = every window; 16 400 clips
    are 3 chunks: 3 x 1 365 <= 4 096 is the last count the set selection takes, 2 000 goes through cone_topk_windows_ws."""
    from cone_amd import ops
    W, dv, nq, k = 4, 256, 3, 30
    vid, cls = _case(ctx_l, dv)
    q = cls[:nq].contiguous()
    cert = _assert_exact(vid, q, W, k, ops.PrefilterIndex(vid).topk(q, W, k, n_cand=n_cand), (ctx_l, n_cand))
    assert cert == [1] * nq         # N(0,1) rows: 30th against the n_cand-th of >= 1 501 windows is far more than E apart


def _planted(ctx_l, dv, q, base, frames, seed):
    """Rows = `base` (one row for all: ties) or unit noise orthogonal to q (base None), with frame frames[j] replaced by
    a_j q + sqrt(1 - a_j^2) (that row), a_j = 0.9 - 0.05 j: well separated peaks along q."""
    if base is None:
        noise = _unit_rows(ctx_l, dv, seed)
        noise = noise - (noise @ q)[:, None] * q[None, :]
        vid = noise / noise.norm(dim=1, keepdim=True)
    else:
        vid = base[None, :].repeat(ctx_l, 1)
    for j, f in enumerate(frames):
        a = 0.9 - 0.05 * j
        vid[f] = a * q + (1 - a * a) ** 0.5 * vid[f]
    return vid


@pytest.mark.parametrize("nq", [1, 5])
def test_planted_peaks_must_certify(nq):
    """k / 2 planted frames in k / 2 separate half windows (W = 4: a frame lights the two windows that share its half):
    the k-th fp32 score clears the (n_cand + 1)-th by more than 2 E on the CPU, so the device has to certify."""
    from cone_amd import ops
    dev = P._gpu()
    ctx_l, W, dv, k, n_cand = 3000, 4, 256, 8, 128
    q = _unit_rows(1, dv, 31)[0]
    vid = _planted(ctx_l, dv, q, None, (100, 700, 1300, 2222), 32)
    win = C.window_scores((vid @ q)[None, :], W)[0]                         # fp32 scores on the CPU
    order = C.stable_desc(win)
    R, N = C.index_norms(vid)
    E = C.device_bound(q, R * C.INFLATE + 2.0 ** -55, N * C.INFLATE + 2.0 ** -55, dv)
    assert float(win[order[k - 1]] - win[order[n_cand]]) > 2 * E, (float(win[order[k - 1]]), float(win[order[n_cand]]), E)
    cls = torch.cat([q[None, :], -q[None, :], _unit_rows(3, dv, 33)])[:nq].contiguous().to(dev)       # (the others: whatever)
    vid = vid.to(dev)
    got = ops.PrefilterIndex(vid).topk(cls, W, k)
    cert = _assert_exact(vid, cls, W, k, got, ("planted", nq))
    assert cert[0] == 1
    assert sorted(got[0][0].tolist()) == [50, 51, 350, 351, 650, 651, 1111, 1112]


@pytest.mark.parametrize("dv", [256, 512, 768, 1024])
def test_a_video_of_identical_rows_must_not_certify(dv):
    """Every window ties: t - c_last is a rounding difference, <= E for any valid bound.  The fallback (the gated scan of
    every row width) lists 0 .. k-1."""
    from cone_amd import ops
    dev = P._gpu()
    W, k = 4, 30
    rows = _unit_rows(4, dv, 41)
    vid = rows[:1].repeat(600, 1).to(dev)                                   # 301 windows > n_cand = 128
    cls = rows[1:4].contiguous().to(dev)
    got = ops.PrefilterIndex(vid).topk(cls, W, k)
    assert _assert_exact(vid, cls, W, k, got, "identical") == [0, 0, 0]
    assert got[0].tolist() == [list(range(k))] * 3


@pytest.mark.parametrize("layout", [(0, 1), (0, 0, 0, 0, 1, 0)])
def test_certified_and_uncertified_queries_share_a_call(layout):
    """A video of one base row b with planted peaks along q0, q0 orthogonal to b.  Query q0 (0 in `layout`): the peaks
    stand out of a floor of exact ties -> certified.  Query b (1): every window scores 1.0 -> not certified.  (0, 1): one
    launch group holds both; the six-query layout has a first group that is gated off and a second that runs."""
    from cone_amd import ops
    dev = P._gpu()
    ctx_l, W, dv, k = 3000, 4, 256, 8
    b, q0 = _unit_rows(2, dv, 51)
    q0 = q0 - (q0 @ b) * b
    q0 = q0 / q0.norm()
    vid = _planted(ctx_l, dv, q0, b, (100, 700, 1300, 2222), 0).to(dev)
    cls = torch.stack([b if f else q0 for f in layout]).contiguous().to(dev)
    got = ops.PrefilterIndex(vid).topk(cls, W, k)
    cert = _assert_exact(vid, cls, W, k, got, ("mixed", layout))
    assert cert == [1 - f for f in layout]
    for row, f in zip(got[0].tolist(), layout):
        assert row == (list(range(k)) if f else [50, 51, 350, 351, 650, 651, 1111, 1112])


SWEEP = dict(ctx_l=3998, W=4, dv=256, nq=3, k=2)        # 2 000 windows, n_cand = k + 2


def test_soundness_sweep_over_20_seeds():
    """n_cand = k + 2: the proof has almost no candidates to spare, so it fails often -- and every row must still be the exact
    path's, certified or not.  By the float64 model (prefilter_certified_ref.margin) these seeds hold queries far on either
    side of E: a sweep in which all queries certify, or none, would show nothing, and fails."""
    from cone_amd import ops
    dev = P._gpu()
    s, flags = SWEEP, []
    for seed in range(20):
        vid, cls = _unit_rows(s["ctx_l"], s["dv"], 1000 + seed).to(dev), _unit_rows(s["nq"], s["dv"], 2000 + seed).to(dev)
        got = ops.PrefilterIndex(vid).topk(cls, s["W"], s["k"], n_cand=s["k"] + 2)
        flags += _assert_exact(vid, cls, s["W"], s["k"], got, ("sweep", seed))
    P.record_measured("prefilter_certified_sweep", certified=sum(flags), queries=len(flags))
    assert 1 <= sum(flags) <= len(flags) - 1, flags


def test_non_finite_rows_are_never_certified_and_still_exact():
    """One row holds a NaN, one holds fp32 max (bf16: +inf): R and N are non-finite, no query certifies, and the answer is the
    exact path's (whose window max skips NaN frame scores)."""
    from cone_amd import ops
    dev = P._gpu()
    ctx_l, W, dv, k = 3000, 4, 256, 30
    vid = _unit_rows(ctx_l, dv, 61)
    vid[1234, 7] = float("nan")
    vid[2000, 100] = torch.finfo(torch.float32).max
    vid, cls = vid.to(dev), _unit_rows(3, dv, 62).to(dev)
    index = ops.PrefilterIndex(vid)
    assert not bool(torch.isfinite(index.err).any())
    assert _assert_exact(vid, cls, W, k, index.topk(cls, W, k), "non-finite") == [0, 0, 0]


def test_fallback_merges_its_chunk_lists_in_two_levels():
    """70 001 windows, k = 256: 18 chunk lists of 256 exceed one merge workgroup's 4 096 values.  n_cand = k leaves the proof
    nothing to spare, so the fallback runs."""
    from cone_amd import ops
    dev = P._gpu()
    g = torch.Generator(device=dev).manual_seed(7)
    vid = torch.randn(140000, 256, device=dev, generator=g)
    vid = vid / vid.norm(dim=1, keepdim=True)
    cls = _unit_rows(2, 256, 71).to(dev)
    got = ops.PrefilterIndex(vid).topk(cls, 4, 256, n_cand=256)
    assert _assert_exact(vid, cls, 4, 256, got, "two-level merge") == [0, 0]


def test_named_checks():
    from cone_amd import _lib, ops
    dev = P._gpu()
    index = ops.PrefilterIndex(_unit_rows(400, 256, 81).to(dev))
    cls = _unit_rows(1, 256, 82).to(dev)
    with pytest.raises(_lib.ConeHipError, match="n_cand"):
        index.topk(cls, 4, 8, n_cand=4)                 # fewer candidates than k
    with pytest.raises(_lib.ConeHipError, match="n_cand"):
        index.topk(cls, 4, 8, n_cand=202)               # more than the 201 windows
    with pytest.raises(_lib.ConeHipError, match="k=257"):
        index.topk(cls, 4, 257)
    with pytest.raises(_lib.ConeHipError, match="feature dim"):
        ops.PrefilterIndex(_unit_rows(8, 128, 83).to(dev)).topk(_unit_rows(1, 128, 84).to(dev), 4, 2)


def test_topk_is_captured_in_a_graph_and_replays_on_new_queries():
    from cone_amd import ops
    dev = P._gpu()
    ctx_l, W, dv, k = 3000, 4, 256, 30
    vid, cls = _case(ctx_l, dv)
    index = ops.PrefilterIndex(vid)
    buf = cls[:3].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        index.topk(buf, W, k)                           # warm-up: one-time kernel setup and the workspace, outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = index.topk(buf, W, k)
    new = cls[5:8].contiguous()
    buf.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    eager = index.topk(new, W, k)
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
    _assert_exact(vid, new, W, k, out, "graph")
