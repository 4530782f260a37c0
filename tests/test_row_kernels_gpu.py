"""The row kernels on hostile value distributions: every form of the fp32 GEMM family, the fused layer tails (exact fp32,
three-piece split, single piece), gemm_bf16 and the row LayerNorm / L2 normalisation against float64, ELEMENTWISE, inside
bounds derived from the inputs (tests/row_refs.py: families, references, derivations).  That a plain evaluation stays inside
those bounds, that every LayerNorm row has one, that every planted error leaves them by >= 10 bounds and that the pow2
scales are exact is shown on the CPU in tests/test_row_kernels_cpu.py.

Every launch fills its outputs with NaN plus 3 spare rows; finiteness is asserted first, then |out - ref| <= bound for every
element, then that the spare rows are untouched.  The exact checks use torch.equal: pow2 (the scaled run = the scaled base
run), constant (= ln_b), onehot with a_i = 1 and flags 0 (= W[:, k] + bias, one rounding), row isolation (a row of +Inf, or
with one NaN channel, changes no other row's bits).  The worst err / bound per (kernel, form, family) is recorded
(test_gpu_parity.record_measured; the committed table: profiles/row_kernels_measured.txt).

Which test enters which kernel or form:
  cone_test_gemm, automatic             test_gemm_families[N-K-flags] form "auto": M = 1, 17: gemm_rows_spread_kernel without
                                        LayerNorm, gemm_rows_small_kernel with it; M = 130, 257 the same (<= 64 row groups)
  cone_test_gemm | 0x100                ... form "square": gemm_f32_kernel<128, 128> / <64, 256> (LayerNorm)
  cone_test_gemm | 0x200, | 0x300       ... forms "rows4" / "rows8": gemm_rows_kernel<16> / gemm_rows16_kernel
  cone_test_gemm | 8                    ... form "nospread": gemm_rows_small_kernel without LayerNorm too
  (256, 96)                             the spread form's short last pass
  A2 / a2_mod                           test_gemm_second_operand (gemm_f32_kernel<128, 128, true>)
  cone_test_layernorm                   test_layernorm_families[dim]
  cone_test_tail_form ROWS128 / ROWS64 / WIDE / SPREAD, pre 0 | 1 (OUT and OUT2), cone_test_proj_ffn, cone_test_ffn
                                        test_fp32_tail_families[ff-M] (SPREAD: ff = 1024; ROWS64: post-norm only)
  cone_test_ffn_split, cone_test_proj_ffn_split, CONE_TEST_PACK [| CONE_TEST_SINGLE_PIECE]
                                        test_matrix_core_tail_families[mode-ff-M]
                                        (ffn_split_kernel<false, false> / <true, false>, ffn_bf16_kernel<false, false, false> /
                                        <true, false, false>, one tile per workgroup, dense rows, no M_dev)
  cone_test_tail_mc                     tests/test_tail_mc_forms_gpu.py: the same kernels and ffn_split_kernel<true, true>,
                                        ffn_bf16_kernel<true, true, false> (the q | k | v ride) and <true, false, true> (pre-norm,
                                        OUT2 set or NULL), with r_idx / R2, M_dev, padded strides, and walked (n_cu = 2, 1 at
                                        677 rows) as well as un-walked; its docstring names the test per kernel
  cone_test_rows_mc                     ... rows256_split_kernel / rows256_bf16_kernel walked and un-walked, ldx / ldc, M_dev
  cone_test_rows_split, both modes      test_matrix_core_row_gemm_families[mode-N] (pow2 at s = -40, 40, -80; tiny measured)
  cone_test_gemm_bf16                   test_gemm_bf16_families[N-K]
  cone_l2_normalize_rows                test_l2_normalize_families[dim]
  row isolation of each of the above    test_row_isolation_*"""
import itertools

import pytest
import torch

import row_refs as R
from test_gpu_parity import record_measured

pytestmark = pytest.mark.gpu

SPARE = 3
FORMS = (("auto", 0), ("square", 0x100), ("rows4", 0x200), ("rows8", 0x300), ("nospread", 8))
SAME_BITS_AS_AUTO = ("rows8", "nospread")
TAIL_ROWS128, TAIL_ROWS64, TAIL_WIDE, TAIL_LADDER, TAIL_SPREAD = range(5)          # CONE_TAIL_FORM_*
TAIL_FORMS = (("rows128", TAIL_ROWS128), ("rows64", TAIL_ROWS64), ("wide", TAIL_WIDE), ("spread", TAIL_SPREAD))
PACK, SINGLE = 1, 2                                                                 # CONE_TEST_PACK, CONE_TEST_SINGLE_PIECE
PACK_OF = {"split": PACK, "bf16": PACK | SINGLE}


def _gpu():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda", 0)


def _lib():
    from cone_amd import _lib
    return _lib.load(), _lib.ptr, _lib


class Worst:
    """Worst err / bound per (form, family) of one kernel; recorded when the test ends well."""

    def __init__(self, kernel):
        self.kernel, self.w = kernel, {}

    def note(self, form, family, ratio):
        k = (form, family)
        self.w[k] = max(self.w.get(k, 0.0), ratio)

    def record(self):
        for (form, family), r in sorted(self.w.items()):
            record_measured("row_kernels", kernel=self.kernel, form=form, family=family, err_over_bound=float(r))


def _dev(c, **over):
    """The case's fp32 tensors on the device (uploaded once per case); over: replacements for this launch."""
    if not hasattr(c, "_d"):
        c._d = {k: v.to(_gpu()).contiguous() for k, v in vars(c).items() if isinstance(v, torch.Tensor)}
    d = dict(c._d)
    d.update(over)
    return d


def _nan(M, N):
    return torch.full((M + SPARE, N), float("nan"), device=_gpu())


def _hold(out, M, ref, bound, what):
    """Finite first, then every element inside its bound, then the spare rows untouched.  -> worst err / bound."""
    o = out.detach().cpu()
    fin = torch.isfinite(ref)
    assert bool(torch.isfinite(o[:M][fin]).all()), (what, "not finite")
    assert bool(torch.isnan(o[:M][~fin]).all()), (what, "finite where the reference is not")
    assert bool(torch.isnan(o[M:]).all()), (what, "spare rows written")
    err = (o[:M].double() - ref).abs()
    ok = (err <= bound) | ~fin
    ratio = R.worst_ratio(o[:M][fin], ref[fin], bound[fin])
    assert bool(ok.all()), (what, f"{int((~ok).sum())} elements outside their bound, worst err / bound {ratio:.3g}",
                            f"worst err {float(err[fin].max()):.3g}")
    return ratio


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ launchers
def run_gemm(c, flags, form=0, **over):
    lib, P, L = _lib()
    d = _dev(c, **over)
    out = _nan(c.M, c.N)
    L.check(lib.cone_test_gemm(P(d["A"]), P(d.get("A2")), c.a2_mod, P(d["W"]), P(d["bias"]), P(d["R"]) if flags & 2 else None,
                               P(d["lg"]), P(d["lb"]), P(out), None, None, c.M, c.N, c.K, flags | form, L.stream()))
    return out


_img = {}


def _scratch(key, nbytes):
    if key not in _img:
        _img[key] = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=_gpu())
    return _img[key]


def run_gemm_bf16(c, flags, **over):
    lib, P, L = _lib()
    d = _dev(c, **over)
    nbytes = lib.cone_test_gemm_bf16_image_bytes(c.N, c.K)
    assert nbytes > 0, (c.N, c.K)
    out = _nan(c.M, c.N)
    L.check(lib.cone_test_gemm_bf16(P(d["A"]), None, 0, P(d["W"]), P(d["bias"]), P(d["R"]) if flags & 2 else None, None, None,
                                    P(out), None, None, c.M, c.N, c.K, flags, P(_scratch(("gb", c.N, c.K), nbytes)), 0, 0, None,
                                    L.stream()))
    return out


def run_rows_split(c, mode, **over):
    lib, P, L = _lib()
    d = _dev(c, **over)
    nbytes = lib.cone_test_rows_split_image_bytes(c.N)
    assert nbytes > 0 and c.K == 256
    out = _nan(c.M, c.N)
    L.check(lib.cone_test_rows_split(P(d["A"]), P(d["W"]), P(d["bias"]), P(out), c.M, c.N, P(_scratch(("rs", c.N), nbytes)),
                                     PACK_OF[mode], L.stream()))
    return out


def run_tail_form(c, form, pre, **over):
    """-> (OUT, OUT2 or None)."""
    lib, P, L = _lib()
    d = _dev(c, **over)
    out, out2 = _nan(c.M, 256), (_nan(c.M, 256) if pre else None)
    scratch = _scratch(("spread", c.ff), lib.cone_test_proj_ffn_spread_scratch_bytes(c.ff))
    L.check(lib.cone_test_tail_form(P(d["A"]), P(d["Wo"]), P(d["bo"]), P(d["R"]), P(d["pg"]), P(d["pb"]), P(d["W1"]), P(d["b1"]),
                                    P(d["W2"]), P(d["b2"]), P(d["lg"]), P(d["lb"]), P(out), c.M, c.ff, None, None, None, int(pre),
                                    P(out2), form, 0, P(scratch), L.stream()))
    return out, out2


def run_proj_ffn(c, **over):
    lib, P, L = _lib()
    d = _dev(c, **over)
    out = _nan(c.M, 256)
    L.check(lib.cone_test_proj_ffn(P(d["A"]), P(d["Wo"]), P(d["bo"]), P(d["R"]), P(d["pg"]), P(d["pb"]), P(d["W1"]), P(d["b1"]),
                                   P(d["W2"]), P(d["b2"]), P(d["lg"]), P(d["lb"]), P(out), c.M, c.ff, L.stream()))
    return out, None


def run_ffn(c, **over):
    lib, P, L = _lib()
    d = _dev(c, **over)
    out = _nan(c.M, 256)
    L.check(lib.cone_test_ffn(P(d["R"]), P(d["W1"]), P(d["b1"]), P(d["W2"]), P(d["b2"]), P(d["lg"]), P(d["lb"]), P(out), c.M, c.ff,
                              L.stream()))
    return out, None


def run_ffn_mc(c, mode, proj, **over):
    """The matrix-core tails: cone_test_ffn_split / cone_test_proj_ffn_split in mode "split" or "bf16"."""
    lib, P, L = _lib()
    d = _dev(c, **over)
    nbytes = lib.cone_test_ffn_split_image_bytes(c.ff)
    assert nbytes > 0, c.ff
    img = _scratch(("ffn", c.ff), nbytes)
    out = _nan(c.M, 256)
    if proj:
        wo = _scratch(("wo",), lib.cone_test_proj_split_image_bytes())
        L.check(lib.cone_test_proj_ffn_split(P(d["A"]), P(d["Wo"]), P(d["bo"]), P(d["R"]), P(d["pg"]), P(d["pb"]), P(d["W1"]),
                                             P(d["b1"]), P(d["W2"]), P(d["b2"]), P(d["lg"]), P(d["lb"]), P(out), c.M, c.ff, P(img),
                                             P(wo), PACK_OF[mode], L.stream()))
    else:
        L.check(lib.cone_test_ffn_split(P(d["R"]), P(d["W1"]), P(d["b1"]), P(d["W2"]), P(d["b2"]), P(d["lg"]), P(d["lb"]), P(out),
                                        c.M, c.ff, P(img), PACK_OF[mode], L.stream()))
    return out, None


def run_layernorm(c, **over):
    lib, P, L = _lib()
    d = _dev(c, **over)
    out = _nan(c.M, c.dim)
    L.check(lib.cone_test_layernorm(P(d["x"]), P(d["g"]), P(d["b"]), P(out), c.M, c.dim, L.stream()))
    return out


def run_l2(c, eps, clamp, **over):
    lib, P, L = _lib()
    d = _dev(c, **over)
    out = _nan(c.M, c.dim)
    L.check(lib.cone_l2_normalize_rows(P(d["x"]), c.M, c.dim, eps, clamp, P(out), L.stream()))
    return out


# ------------------------------------------------------------------------------------------------ fp32 GEMM family
@pytest.mark.parametrize("N,K,flags", [(N, K, f) for N, K, fs in R.GEMM_SHAPES for f in fs])
def test_gemm_families(N, K, flags):
    """Every family that applies, M = 1, 17, 130, 257, every form; the automatic form, the 8-wave row tile and the
    workgroup-per-16-rows form must also agree bit for bit (the launcher's promise that a row's bits do not depend on the
    batch it sits in; the square tiles and the 4-wave row tile walk k in another order and are held to float64 only).  pow2 (no LayerNorm): the base run is held to float64 and the scaled
    runs are the base run times 2^s exactly.  constant (flags 2 | 4): exactly ln_b.  onehot, a_i = 1, flags 0: exactly
    W[:, k] + bias."""
    worst = Worst("cone_test_gemm")
    for M in R.GEMM_MS:
        fams = R.gemm_families(M, K, flags) + ([] if flags & 4 else ["pow2base"])
        for fam in fams:
            c = R.gemm_case(fam, M, N, K)
            ref, bound, _ = R.gemm_ref_bound(c, flags)
            first = None
            for name, bits in FORMS:
                out = run_gemm(c, flags, bits)
                worst.note(name, fam, _hold(out, M, ref, bound, (fam, M, N, K, flags, name)))
                if first is None:
                    first = out
                elif name in SAME_BITS_AS_AUTO:
                    assert _same_bits(first[:M], out[:M]), (fam, M, name, "differs from the automatic form")
                if fam == "pow2base":
                    for s in R.POW2_SCALES:
                        scaled = run_gemm(R.gemm_case("pow2", M, N, K, scale=s), flags, bits)
                        assert torch.equal(scaled[:M], out[:M] * 2.0 ** s), ("pow2", s, M, name)
                        assert bool(torch.isnan(scaled[M:]).all())
        if flags == 6:
            c = R.gemm_case("constant", M, N, K)
            for name, bits in FORMS:
                out = run_gemm(c, flags, bits)
                assert torch.equal(out[:M].cpu(), c.lb.expand(M, N)), ("constant", M, name)
                assert bool(torch.isnan(out[M:]).all())
        if flags == 0 and M >= K:
            c = R.gemm_case("onehot1", M, N, K)
            want = c.W.t()[torch.arange(M) % K] + c.bias
            for name, bits in FORMS:
                out = run_gemm(c, flags, bits)
                assert torch.equal(out[:M].cpu(), want), ("onehot, a = 1", M, name)
    worst.record()


@pytest.mark.parametrize("a2", ["full", "mod5"])
def test_gemm_second_operand(a2):
    """(A + A2) W^T, A2 a full matrix or 5 rows indexed m % 5 (gemm_f32_kernel<128, 128, true>), N = 512, flags relu."""
    worst = Worst("cone_test_gemm")
    for M, fam in itertools.product(R.GEMM_MS, ("benign", "spike", "cancel")):
        c = R.gemm_case(fam, M, 512, 256, a2=a2)
        ref, bound, _ = R.gemm_ref_bound(c, 1)
        worst.note("A2 " + a2, fam, _hold(run_gemm(c, 1), M, ref, bound, (fam, M, a2)))
    worst.record()


# ------------------------------------------------------------------------------------------------ row LayerNorm, L2
@pytest.mark.parametrize("dim", R.LN_DIMS)
def test_layernorm_families(dim):
    worst = Worst("cone_test_layernorm")
    for fam in R.FAMILIES_LN:
        c = R.ln_case(fam, R.LN_ROWS, dim)
        ref, bound, _ = R.ln_kernel_ref_bound(c)
        worst.note(str(dim), fam, _hold(run_layernorm(c), c.M, ref, bound, (fam, dim)))
    c = R.ln_case("constant", R.LN_ROWS, dim)
    out = run_layernorm(c)
    assert torch.equal(out[:c.M].cpu(), c.b.expand(c.M, dim)), "constant rows (all-zero rows among them) must give ln_b exactly"
    assert bool(torch.isnan(out[c.M:]).all())
    worst.record()


@pytest.mark.parametrize("dim", R.L2_DIMS)
def test_l2_normalize_families(dim):
    """eps 0 | 1e-5, clamp 0 | 1; a zero row is NaN with eps = 0 and 0 with eps > 0, as the float64 evaluation of the formula."""
    worst = Worst("cone_l2_normalize_rows")
    for fam, eps, clamp in itertools.product(R.L2_FAMILIES, (0.0, 1e-5), (0, 1)):
        c = R.l2_case(fam, 6, dim)
        ref, bound = R.l2_ref_bound(c.x, eps, clamp)
        worst.note(f"{dim} eps={eps:g} clamp={clamp}", fam, _hold(run_l2(c, eps, clamp), c.M, ref, bound, (fam, dim, eps, clamp)))
    worst.record()


# ------------------------------------------------------------------------------------------------ fp32 layer tail
def _fp32_tail_launches(ff):
    """(name, proj, pre, launcher) of every entry and form of the exact-fp32 tail at this ff."""
    for name, form in TAIL_FORMS:
        if form == TAIL_SPREAD and ff % 256:
            continue
        yield name, True, False, (lambda c, form=form, **o: run_tail_form(c, form, False, **o))
        if form != TAIL_ROWS64:
            yield name + " pre", True, True, (lambda c, form=form, **o: run_tail_form(c, form, True, **o))
    yield "proj_ffn", True, False, run_proj_ffn
    yield "ffn", False, False, run_ffn


@pytest.mark.parametrize("ff,M", list(itertools.product(R.TAIL_FFS["f32"], R.TAIL_MS)))
def test_fp32_tail_families(ff, M):
    """Every forced form, post- and pre-norm (OUT = the stream, OUT2 = its LayerNorm), cone_test_proj_ffn and cone_test_ffn.
    `dead`: the reference is LN(X + b2) and the bound carries nothing of the hidden path.  constant: exactly ln_b."""
    worst = Worst("fp32 tail")
    for fam, m in R.tail_cases(M):
        c = R.tail_case(fam, m, ff)
        for name, proj, pre, launch in _fp32_tail_launches(ff):
            rb = R.tail_ref_bound(c, "f32", proj, pre)
            out, out2 = launch(c)
            r = _hold(out, m, *rb["OUT"], (fam, m, ff, name))
            if pre:
                r = max(r, _hold(out2, m, *rb["OUT2"], (fam, m, ff, name, "OUT2")))
            worst.note(name, fam, r)
    c = R.tail_case("constant", M, ff)
    for name, proj, pre, launch in _fp32_tail_launches(ff):
        out, out2 = launch(c)
        assert torch.equal((out2 if pre else out)[:M].cpu(), c.lb.expand(M, 256)), ("constant", name)
        if pre:
            assert torch.equal(out[:M].cpu(), c.R), ("constant: the stream is the residual", name)
    worst.record()


@pytest.mark.parametrize("mode,ff,M", [(mode, ff, M) for mode in ("split", "bf16") for ff in R.TAIL_FFS[mode] for M in R.TAIL_MS])
def test_matrix_core_tail_families(mode, ff, M):
    """cone_test_ffn_split / cone_test_proj_ffn_split with CONE_TEST_PACK (three pieces: fp32-accurate, the split bound) and
    CONE_TEST_PACK | CONE_TEST_SINGLE_PIECE (against float64 on operands rounded once to bf16)."""
    worst = Worst(f"{mode} tail")
    for fam, m in R.tail_cases(M):
        c = R.tail_case(fam, m, ff)
        for proj in (False, True):
            rb = R.tail_ref_bound(c, mode, proj, False)
            out, _ = run_ffn_mc(c, mode, proj)
            worst.note("proj_ffn" if proj else "ffn", fam, _hold(out, m, *rb["OUT"], (mode, fam, m, ff, proj)))
    c = R.tail_case("constant", M, ff)
    for proj in (False, True):
        out, _ = run_ffn_mc(c, mode, proj)
        assert torch.equal(out[:M].cpu(), c.lb.expand(M, 256)), ("constant", mode, proj)
    worst.record()


# ------------------------------------------------------------------------------------------------ matrix-core row GEMMs
@pytest.mark.parametrize("mode,N", list(itertools.product(("split", "bf16"), R.ROWS_SPLIT_NS)))
def test_matrix_core_row_gemm_families(mode, N):
    """cone_test_rows_split in both modes.  pow2 at s = -40, 40 and -80 (exact).  tiny: inside the fp32 bound plus the flush
    allowance; what the matrix cores did with the subnormal pieces is MEASURED against the two emulations (pieces kept /
    pieces below 2^-126 flushed) and recorded, not asserted."""
    worst = Worst(f"cone_test_rows_split {mode}")
    for M in R.GEMM_MS:
        for fam in R.gemm_families(M, 256, 0) + ["pow2base"]:
            c = R.gemm_case(fam, M, N, 256)
            ref, bound, _ = R.gemm_ref_bound(c, 0, mode)
            out = run_rows_split(c, mode)
            worst.note(str(N), fam, _hold(out, M, ref, bound, (mode, fam, M, N)))
            if fam == "pow2base":
                for s in R.POW2_SCALES_SPLIT:
                    scaled = run_rows_split(R.gemm_case("pow2", M, N, 256, scale=s), mode)
                    assert torch.equal(scaled[:M], out[:M] * 2.0 ** s), ("pow2", mode, s, M, N)
            if fam == "tiny" and mode == "split" and M == 130:
                o = out[:M].cpu()
                keep = R.eval_gemm(c, 0, R.mm_split, torch.float32)
                flushed = R.eval_gemm(c, 0, lambda a, W: R.mm_split(a, W, flush=True), torch.float32)
                unit = 2.0 ** -126
                record_measured("row_kernels_tiny", kernel="cone_test_rows_split", N=N,
                                err_vs_float64_in_2p126=float((o.double() - ref).abs().max()) / unit,
                                dist_to_emulation_keeping_subnormal_pieces_in_2p126=float((o - keep).abs().max()) / unit,
                                dist_to_emulation_flushing_them_in_2p126=float((o - flushed).abs().max()) / unit,
                                emulations_apart_in_2p126=float((keep - flushed).abs().max()) / unit)
        if M >= 256:
            c = R.gemm_case("onehot1", M, N, 256)
            if mode == "bf16":
                want = (R.bf(c.W).t()[torch.arange(M) % 256] + c.bias.double()).float()
                assert torch.equal(run_rows_split(c, mode)[:M].cpu(), want), "onehot, a = 1: bf16(W[:, k]) + bias, one rounding"
    worst.record()


@pytest.mark.parametrize("N,K", R.GEMM_BF16_SHAPES)
def test_gemm_bf16_families(N, K):
    worst = Worst("cone_test_gemm_bf16")
    for M, flags in itertools.product(R.GEMM_MS, (0, 1, 2, 3)):
        for fam in R.gemm_families(M, K, flags) + ["pow2base"]:
            c = R.gemm_case(fam, M, N, K)
            ref, bound, _ = R.gemm_ref_bound(c, flags, "bf16")
            out = run_gemm_bf16(c, flags)
            worst.note(f"{N}x{K} flags={flags}", fam, _hold(out, M, ref, bound, (fam, M, N, K, flags)))
            if fam == "pow2base":
                for s in R.POW2_SCALES:
                    scaled = run_gemm_bf16(R.gemm_case("pow2", M, N, K, scale=s), flags)
                    assert torch.equal(scaled[:M], out[:M] * 2.0 ** s), ("pow2", s, M, flags)
    worst.record()


# ------------------------------------------------------------------------------------------------ row isolation
def _isolation(what, M, rowwise, run):
    """run(**over) -> tuple of outputs.  Row r of every row-wise input in turn all +Inf, then NaN in one channel: every row
    other than r keeps the bits of the clean run (spare rows included: they stay NaN with the fill's bits)."""
    clean = [o for o in run() if o is not None]
    torch.cuda.synchronize()
    for r in sorted({0, 15, 16, M - 1}):
        if r >= M:
            continue
        for kind in ("inf", "nan"):
            over = {}
            for name, t in rowwise.items():
                p = t.clone()
                if kind == "inf":
                    p[r] = float("inf")
                else:
                    p[r, (7 * r + 3) % p.shape[1]] = float("nan")
                over[name] = p
            outs = [o for o in run(**over) if o is not None]
            keep = torch.ones(M + SPARE, dtype=torch.bool, device=_gpu())
            keep[r] = False
            for i, (a, b) in enumerate(zip(clean, outs)):
                assert _same_bits(a[keep], b[keep]), (what, f"row {r} {kind} changed another row of output {i}")


def _rowwise(c, names):
    d = _dev(c)
    return {k: d[k] for k in names}


@pytest.mark.parametrize("N,K,flags", [(256, 256, 0), (256, 256, 7), (256, 256, 6), (512, 256, 3), (256, 1024, 2), (256, 96, 1)])
def test_row_isolation_gemm(N, K, flags):
    for M in (17, 130):
        c = R.gemm_case("benign", M, N, K)
        for name, bits in FORMS:
            _isolation(("gemm", N, K, flags, M, name), M, _rowwise(c, ["A", "R"] if flags & 2 else ["A"]),
                       lambda bits=bits, **o: (run_gemm(c, flags, bits, **o),))
    c = R.gemm_case("benign", 130, 512, 256, a2="full")
    _isolation(("gemm A2",), 130, _rowwise(c, ["A"]), lambda **o: (run_gemm(c, 1, 0, **o),))


def test_row_isolation_layernorm_and_l2():
    for dim in R.LN_DIMS:
        c = R.ln_case("benign", R.LN_ROWS, dim)
        _isolation(("layernorm", dim), c.M, _rowwise(c, ["x"]), lambda **o: (run_layernorm(c, **o),))
    for dim in R.L2_DIMS:
        c = R.l2_case("benign", 6, dim)
        for eps, clamp in ((0.0, 0), (1e-5, 1)):
            _isolation(("l2", dim, eps, clamp), c.M, _rowwise(c, ["x"]), lambda **o: (run_l2(c, eps, clamp, **o),))


@pytest.mark.parametrize("ff,M", list(itertools.product(R.TAIL_FFS["f32"], R.TAIL_MS)))
def test_row_isolation_fp32_tail(ff, M):
    """r = M - 1 is the row the padding lanes of the last group re-read (TB_LD_ROW / min(row, M - 1))."""
    c = R.tail_case("benign", M, ff)
    for name, proj, pre, launch in _fp32_tail_launches(ff):
        _isolation(("fp32 tail", ff, M, name), M, _rowwise(c, ["A", "R"] if proj else ["R"]), lambda **o: launch(c, **o))


@pytest.mark.parametrize("mode", ["split", "bf16"])
def test_row_isolation_matrix_core_kernels(mode):
    for ff, M in itertools.product(R.TAIL_FFS[mode], R.TAIL_MS):
        c = R.tail_case("benign", M, ff)
        for proj in (False, True):
            _isolation((mode, "tail", ff, M, proj), M, _rowwise(c, ["A", "R"] if proj else ["R"]),
                       lambda **o: run_ffn_mc(c, mode, proj, **o))
    for N, M in itertools.product(R.ROWS_SPLIT_NS, (17, 130)):
        c = R.gemm_case("benign", M, N, 256)
        _isolation((mode, "rows", N, M), M, _rowwise(c, ["A"]), lambda **o: (run_rows_split(c, mode, **o),))
    if mode == "bf16":
        for (N, K), flags in itertools.product(R.GEMM_BF16_SHAPES, (0, 3)):
            for M in (17, 130):
                c = R.gemm_case("benign", M, N, K)
                _isolation(("gemm_bf16", N, K, flags, M), M, _rowwise(c, ["A", "R"] if flags & 2 else ["A"]),
                           lambda **o: (run_gemm_bf16(c, flags, **o),))
