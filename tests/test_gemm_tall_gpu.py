"""The tall form of the row GEMM (cone_amd/csrc/gemm_tall.hip: K = 256, persistent 128-row tiles, the layer tail's weight ring)
against the 8-wave row tile it stands in for.

Every comparison is ``torch.equal`` against ``cone_test_gemm`` forced to family 3 on the same inputs (``_reference``): the tall form walks the same
k-ordered fma chain per output element and the same epilogue arithmetic, so not a bit may differ.  One case per flag set is also
held against the float64 bound of tests/row_refs.py, which pins the form to the truth as well as to its sibling.

Rows are passed with strides (lda = 260, ldc = N + 4) whose padding columns hold NaN, and C carries 32 NaN rows past M: an input
read out of its row poisons the result, a store out of its place destroys a canary."""
import functools

import numpy as np
import pytest
import torch

import inputs as gi
import row_refs as RR
from cone_amd import _lib, synth
from cone_amd.config import make_opt

pytestmark = pytest.mark.gpu

K = 256
LDA = 260
GUARD = 32
M_WALK = 5 * 128 + 37           # n_cu = 2: a workgroup walks three tiles, the last one partial
RELU, RES, LN = 1, 2, 4


def _gpu():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _operands(N, k=K):
    """One draw per (N, K), shared by every test and never modified: 1024 rows of A and R, W, bias."""
    g = torch.Generator().manual_seed(7919 * N + k)
    dev = _gpu()
    mk = lambda *s: torch.randn(*s, generator=g)
    return dict(A=mk(1024, k).to(dev), W=(mk(N, k) / k ** 0.5).to(dev), bias=mk(N).to(dev), R=mk(1024, N).to(dev))


def _rows_tile(A, M, N, flags, bias, R, A2=None, a2_mod=0, ln=None, variant=3, k=K, W=None):
    """cone_test_gemm on contiguous operands, forced to `variant`."""
    lib, P = _lib.load(), _lib.ptr
    C = torch.full((M, N), float("nan"), device=A.device)
    _lib.check(lib.cone_test_gemm(P(A), P(A2), a2_mod, P(W), P(bias), P(R) if flags & RES else None, P(ln[0]) if ln else None,
                                  P(ln[1]) if ln else None, P(C), None, None, M, N, k, flags | (variant << 8), _lib.stream()))
    return C


@functools.lru_cache(maxsize=None)
def _reference(M, N, flags, with_bias):
    """Family 3 exists for N % 256 == 0 only (any other N silently takes the square tiles, whose k order is another one), so W,
    bias and R are padded with zero rows / columns to the next multiple of 256 and the first N columns are the reference: a
    column of the row tile is a function of its own W row alone."""
    d = _operands(N)
    Np = (N + 255) // 256 * 256
    W, bias, R = torch.zeros(Np, K, device=_gpu()), torch.zeros(Np, device=_gpu()), torch.zeros(M, Np, device=_gpu())
    W[:N], bias[:N], R[:, :N] = d["W"], d["bias"], d["R"][:M]
    return _rows_tile(d["A"][:M].contiguous(), M, Np, flags, bias if with_bias else None, R, W=W)[:, :N].contiguous()


def _padded(t, ld):
    """t's rows at row stride ld, NaN in the padding columns."""
    out = torch.full((t.shape[0], ld), float("nan"), device=t.device)
    out[:, :t.shape[1]] = t
    return out


def _tall(A, W, bias, R, M, N, flags, n_cu, M_dev=None, variant=4, lda=LDA, pad_c=4, k=K, A2=None, ln=None):
    """cone_test_gemm_tall on strided operands -> the whole C buffer (M + GUARD rows of N + pad_c floats, NaN before the call)."""
    lib, P = _lib.load(), _lib.ptr
    ldc = N + pad_c
    Ap = _padded(A[:max(M, 1)], lda) if lda != k else A[:max(M, 1)].contiguous()
    Rp = _padded(R[:max(M, 1)], ldc) if (flags & RES) else None
    C = torch.full((M + GUARD, ldc), float("nan"), device=A.device)
    md = torch.tensor([M_dev], dtype=torch.int32, device=A.device) if M_dev is not None else None
    _lib.check(lib.cone_test_gemm_tall(P(Ap), P(A2), 0, P(W), P(bias), P(Rp), P(ln[0]) if ln else None, P(ln[1]) if ln else None,
                                       P(C), None, None, M, N, k, flags | (variant << 8), lda, ldc, P(md), n_cu, _lib.stream()))
    torch.cuda.synchronize()
    return C


def _check(M, N, flags, with_bias, n_cu, M_dev=None):
    d = _operands(N)
    C = _tall(d["A"], d["W"], d["bias"] if with_bias else None, d["R"], M, N, flags, n_cu, M_dev=M_dev)
    rows = M if M_dev is None else min(M, M_dev)
    ref = _reference(M, N, flags, with_bias)
    assert torch.equal(C[:rows, :N], ref[:rows]), (M, N, flags, with_bias, n_cu, M_dev)
    assert bool(torch.isnan(C[:, N:]).all()), "a store reached C's padding columns"
    assert bool(torch.isnan(C[rows:]).all()), "a store reached a row past the row count"


@pytest.mark.parametrize("M", [1, 15, 16, 17, 127, 128, 129, M_WALK])
@pytest.mark.parametrize("N", [96, 256])
def test_rows(M, N):
    """One wave active, an idle upper half, a partial last group, and a workgroup walking three tiles with the ring running on
    across them (n_cu = 2)."""
    _check(M, N, 0, True, 2)


def test_one_workgroup_walks_every_tile():
    _check(3 * 128, 96, 0, True, 1)
    _check(3 * 128, 256, RELU, True, 1)


@pytest.mark.parametrize("N", [32, 96, 256, 768])
def test_columns(N):
    """96: three chunks per tile, the ring's stage phase moves from tile to tile; 32: fewer chunks than ring stages."""
    _check(M_WALK, N, 0, True, 2)
    _check(17, N, 0, True, 2)


@pytest.mark.parametrize("flags", [0, RELU, RES, RELU | RES])
@pytest.mark.parametrize("with_bias", [False, True])
def test_flags(flags, with_bias):
    _check(M_WALK, 96, flags, with_bias, 2)
    _check(129, 256, flags, with_bias, 2)


@pytest.mark.parametrize("M_dev", [0, 1, 100, M_WALK])
def test_device_row_count(M_dev):
    """*M_dev wins over M: rows at and past it are neither computed into C nor touched."""
    _check(M_WALK, 96, RELU | RES, True, 2, M_dev=M_dev)
    _check(M_WALK, 256, 0, True, 2, M_dev=M_dev)


def test_dispatcher():
    """Family 4 through launch_gemm equals family 3 on an eligible shape; what the tall form cannot run is refused by name at
    family 4 and runs the old form at family 0."""
    dev = _gpu()
    M, N = 300, 256
    d = _operands(N)
    A = d["A"][:M].contiguous()
    C = _tall(d["A"], d["W"], d["bias"], d["R"], M, N, RELU, 0)
    assert torch.equal(C[:M, :N], _reference(M, N, RELU, True))
    g = torch.Generator().manual_seed(5)
    ln = ((torch.rand(N, generator=g) + 0.5).to(dev), torch.randn(N, generator=g).to(dev))
    A2 = torch.randn(M, K, generator=g).to(dev)
    d512 = _operands(N, 512)
    cases = [
        ("LayerNorm", dict(flags=RES | LN, ln=ln), dict(A=A, W=d["W"], k=K)),
        ("A2", dict(flags=0, A2=A2), dict(A=A, W=d["W"], k=K)),
        ("K must be 256", dict(flags=0), dict(A=d512["A"][:M].contiguous(), W=d512["W"], k=512)),
    ]
    for name, kw, op in cases:
        flags = kw["flags"]
        call = lambda variant: _tall(op["A"], op["W"], d["bias"], d["R"], M, N, flags, 0, variant=variant, lda=op["k"], pad_c=0,
                                     k=op["k"], A2=kw.get("A2"), ln=kw.get("ln"))
        with pytest.raises(_lib.ConeHipError, match=name):
            call(4)
        old = _rows_tile(op["A"], M, N, flags, d["bias"], d["R"][:M].contiguous(), A2=kw.get("A2"), ln=kw.get("ln"), variant=0,
                         k=op["k"], W=op["W"])
        assert torch.equal(call(0)[:M], old), name


@pytest.mark.parametrize("flags", [0, RELU, RES, RELU | RES])
def test_float64_bound(flags):
    """The derived elementwise bound of row_refs (any summation order of the nz products + the epilogue's roundings)."""
    dev = _gpu()
    M, N = 257, 96
    c = RR.gemm_case("benign", M, N, K)
    C = _tall(c.A.to(dev), c.W.to(dev), c.bias.to(dev), c.R.to(dev), M, N, flags, 2)
    ref, bound, _ = RR.gemm_ref_bound(c, flags)
    worst = RR.worst_ratio(C[:M, :N].cpu(), ref, bound)
    print(f"[gemm_tall] flags={flags}: worst |err| / bound = {worst:.4f}")
    assert worst <= 1.0, worst


def test_forward_path_bits_do_not_depend_on_the_threshold():
    """cone_forward_packed on a 6-window batch with every eligible launch on the tall form (threshold 1) against the default."""
    from cone_amd.model import build_model
    dev = _gpu()
    opt = make_opt("ego4d")
    model, _ = build_model(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(opt, 11).items()})
    rng = np.random.default_rng(6)
    lens_v = [opt.max_v_l] + [int(x) for x in rng.integers(1, opt.max_v_l + 1, 5)]
    lens_q = [opt.max_q_l] + [int(x) for x in rng.integers(1, opt.max_q_l + 1, 5)]
    inp = gi.stage_b_inputs(opt, 41, lens_v, lens_q)
    vid = np.concatenate([inp["src_vid"][b, :lens_v[b]] for b in range(6)], 0)
    txt = np.concatenate([inp["src_txt"][b, :lens_q[b]] for b in range(6)], 0)
    i32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=dev)
    vrow0, trow0 = i32(np.concatenate([[0], np.cumsum(lens_v)[:-1]])), i32(np.concatenate([[0], np.cumsum(lens_q)[:-1]]))
    tok_index = i32(np.concatenate([np.arange(n) for n in lens_q]))

    def run():
        vproj, tproj = model.project(0, torch.from_numpy(vid).to(dev)), model.project(1, torch.from_numpy(txt).to(dev))
        out = model.forward_packed(vproj, vrow0, i32(lens_v), tproj, trow0, i32(lens_q), opt.max_v_l, opt.max_q_l,
                                   l0=model.layer0_cache(vproj, tproj, opt.max_v_l, tok_index=tok_index), saliency=True, aux=True)
        torch.cuda.synchronize()
        flat = {k: v.clone() for k, v in out.items() if k != "aux_outputs"}
        # (the entry writes a window's own clips only)
        flat["saliency_scores"] = torch.cat([flat["saliency_scores"][b, :lens_v[b]] for b in range(6)])
        for i, a in enumerate(out.get("aux_outputs", [])):
            flat.update({f"aux{i}_{k}": v.clone() for k, v in a.items()})
        return flat

    try:
        model.set_option("gemm_tall_min_rows", 0)
        old = run()
        model.set_option("gemm_tall_min_rows", -1)
        default = run()
        model.set_option("gemm_tall_min_rows", 1)
        tall = run()
    finally:
        model.set_option("gemm_tall_min_rows", -1)
    assert set(old) == set(default) == set(tall) and len(old) >= 3
    for k in old:
        assert torch.equal(old[k], tall[k]), k
        assert torch.equal(old[k], default[k]), k
