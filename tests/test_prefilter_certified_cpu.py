"""The certified pre-filter, the parts that need no GPU: the header and the binding, and the error bound E(q) of
tests/prefilter_certified_ref.py held against fp32 scores computed on the CPU -- on the inputs for which the bound has to be
MEASURED rather than assumed (rounding midpoints, subnormals)."""
import os
import re

import pytest
import torch

import prefilter_certified_ref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cone_prefilter_index_bf16", "cone_prefilter_topk_certified_workspace", "cone_prefilter_topk_certified")


def test_header_declares_the_certified_entries_and_stays_abi_8():
    from cone_amd import _lib
    with open(os.path.join(ROOT, "include", "cone_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"#define\s+CONE_HIP_ABI_VERSION\s+8\b", hdr)
    declared = set(re.findall(r"\b(cone_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, name
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    assert "2^-8 / (1 + 2^-8)" in hdr           # the rounding figure the bound does NOT rely on is stated right


def test_lib_binds_the_certified_entries():
    import ctypes
    from cone_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS, name
    res, args = _lib._SIGNATURES["cone_prefilter_topk_certified"]
    assert res is ctypes.c_int and len(args) == 17          # vid_f32 .. stream, as declared
    assert len(_lib._SIGNATURES["cone_prefilter_index_bf16"][1]) == 6
    assert _lib._SIGNATURES["cone_prefilter_topk_certified_workspace"][0] is ctypes.c_size_t
    from cone_amd import ops
    assert callable(ops.PrefilterIndex.topk)


def _unit(x):
    return x / x.norm(dim=1, keepdim=True)


def _midpoint_rows(n, dv, seed, unit=True):
    """Every element is sign * (1 + 2^-8) * 2^e: a bf16 rounding midpoint (ties to even: down to 2^e), relative error
    2^-8 / (1 + 2^-8).  Unit rows: all exponents equal to -log2(sqrt(dv)) (dv a power of four)."""
    g = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, (n, dv), generator=g).float() * 2 - 1
    e = torch.full((n, dv), -0.5 * torch.log2(torch.tensor(float(dv))).item()) if unit else \
        torch.randint(-6, 3, (n, dv), generator=g).float()
    return sign * (1 + 2.0 ** -8) * torch.exp2(e)


def _inputs(kind, dv, seed):
    g = torch.Generator().manual_seed(100 + seed)
    if kind == "unit":
        return _unit(torch.randn(64, dv, generator=g)), _unit(torch.randn(4, dv, generator=g))
    if kind == "midpoint":
        v = _midpoint_rows(64, dv, seed)
        return v, torch.cat([v[:2], -v[2:3], _midpoint_rows(1, dv, seed + 1, unit=False)])      # the worst query: a row itself
    if kind == "subnormal":     # unit rows with a third of the elements replaced by subnormals (and a row of nothing else)
        v, q = _unit(torch.randn(64, dv, generator=g)), _unit(torch.randn(4, dv, generator=g))
        tiny = torch.randn(64, dv, generator=g) * 2.0 ** -135
        v = torch.where(torch.rand(64, dv, generator=g) < 1 / 3, tiny, v)
        v[0] = tiny[0]
        q[1] = torch.randn(dv, generator=g) * 2.0 ** -130
        return v, q
    raise ValueError(kind)


@pytest.mark.parametrize("dv", [256, 1024])
@pytest.mark.parametrize("kind", ["unit", "midpoint", "subnormal"])
def test_bound_holds_for_every_frame_on_the_cpu(kind, dv):
    """E(q) >= |fp32 score of the bf16-rounded operands - fp32 score of the originals| for every (frame, query)."""
    v, q = _inputs(kind, dv, dv)
    R, N = C.index_norms(v)
    coarse = v.bfloat16().float() @ q.bfloat16().float().T              # fp32 products and sums, torch's order
    exact = v @ q.T
    diff = (coarse.double() - exact.double()).abs()
    worst = 0.0
    for j in range(q.shape[0]):
        E = C.cert_bound(q[j], R, N, dv)
        assert E > 0 and bool((diff[:, j] <= E).all()), (kind, dv, j, float(diff[:, j].max()), E)
        worst = max(worst, float(diff[:, j].max()) / E)
    print(f"[prefilter_certified] {kind} dv={dv}: R={R:.3e} N={N:.3e} worst |coarse - exact| / E = {worst:.3f}")
    if kind == "midpoint":
        assert worst > 0.9                      # the bound is not slack where it matters: a midpoint row as its own query


@pytest.mark.parametrize("dv", [256, 1024])
def test_two_to_the_minus_nine_per_operand_is_violated_by_midpoint_rows(dv):
    """Why R is measured: a bf16 operand's relative error reaches 2^-8 / (1 + 2^-8), twice the "up to 2^-9" of the bf16 mode's
    notes.  On midpoint rows both the per-row residual and the score error exceed what 2^-9 reasoning allows (the
    mode's eps for unit rows: 2^-8 (1 + 2^-9) + dv 2^-23), while the measured bound holds."""
    v = _midpoint_rows(8, dv, 3)
    assert torch.allclose(v.norm(dim=1), torch.full((8,), 1 + 2.0 ** -8))       # unit rows up to the midpoint factor
    assert float(torch.tensor(1 + 2.0 ** -8).bfloat16()) == 1.0                # ties to even: down
    res = (v.double() - C.bf16(v)).norm(dim=1) / v.double().norm(dim=1)
    assert bool((res > 2.0 ** -9 * 1.9).all()) and abs(float(res[0]) - C.U_BF16) < 1e-12
    eps9 = (2.0 ** -8 * (1 + 2.0 ** -9) + dv * 2.0 ** -23) * (1 + 2.0 ** -8) ** 2     # scaled to these rows' norms
    err = ((v.bfloat16().float() * v.bfloat16().float()).sum(1).double() - (v * v).sum(1).double()).abs()    # query = the row
    assert bool((err > eps9).all()), (float(err.min()), eps9)
    R, N = C.index_norms(v)
    for j in range(8):
        assert float(err[j]) <= C.cert_bound(v[j], R, N, dv)


def test_margin_tells_planted_peaks_from_ties():
    """The float64 model used to choose the GPU tests' inputs: planted, well separated peaks clear E by far; a video of
    identical rows has margin ~0 <= E."""
    g = torch.Generator().manual_seed(0)
    dv, W, k = 256, 4, 4
    q = _unit(torch.randn(1, dv, generator=g))[0]
    noise = torch.randn(400, dv, generator=g)
    noise = _unit(noise - (noise @ q)[:, None] * q[None, :])
    vid = noise.clone()
    for j, f in enumerate((40, 200)):
        a = 0.9 - 0.1 * j
        vid[f] = a * q + (1 - a * a) ** 0.5 * noise[f]
    m, E = C.margin(vid, q, W, k, 16)
    assert m > 100 * E and 1e-3 < E < 1e-2, (m, E)
    m, E = C.margin(noise[:1].repeat(400, 1), noise[0], W, k, 16)
    assert abs(m) <= E, (m, E)
