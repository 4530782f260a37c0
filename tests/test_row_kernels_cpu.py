"""CPU half of the row-kernel suite (tests/row_refs.py holds the families, the float64 references and the derived bounds;
tests/test_row_kernels_gpu.py holds the kernels to them):

  * a plain fp32 evaluation (matmul + epilogue; for the split and single-piece kernels their torch emulation) stays inside the
    bound of the float64 reference on every family and every shape the GPU suite runs, and every LayerNorm row of every case
    has a bound (first-order domain max(delta) / s <= 0.05, or the non-linearised bound's ds <= s / 2);
  * every planted wrong version is put at least 10 bounds away by at least one family of its kernel class -- those of the
    matrix-core tails' ride, gather and pre-norm forms included (one table per mode);
  * the pow2 scales are exact: nothing overflows or goes subnormal for the chosen s.

Run with -s to see the tables (worst err / bound per family, the family that catches each planted error)."""
import itertools

import pytest
import torch

import row_refs as R

F32 = torch.float32
POWER = 10.0


def _tail_runs(mode):
    for ff in R.TAIL_FFS[mode]:
        for M in R.TAIL_MS:
            for fam, m in R.tail_cases(M):
                yield fam, m, ff


def _tail_forms(mode):
    """(proj, pre) of the hooks: the fp32 and the single-piece tail have all three (cone_test_tail_form / cone_test_tail_mc);
    the three-piece split has no pre-norm kernel.  The ride and gather forms of the matrix-core tails: row_refs.mc_forms."""
    return ((True, False), (False, False)) if mode == "split" else ((True, False), (True, True), (False, False))


MM = {"f32": R.mm32, "split": R.mm_split, "bf16": R.mm32_bf}


def _table(title, worst):
    print(f"\n{title}")
    for k in sorted(worst):
        print(f"  {k:<28s} worst err / bound {worst[k]:.3g}")


def _note(worst, key, ratio):
    worst[key] = max(worst.get(key, 0.0), ratio)


def _domain_ok(info, what):
    assert info["rig"] <= R.LN_RIG_VALID, (what, info, "a LayerNorm row without a bound")


# ------------------------------------------------------------------------------------------------ the reference alone
def test_fp32_gemm_reference_stays_inside_every_bound():
    worst, first = {}, {}
    for (N, K, flagset), M in itertools.product(R.GEMM_SHAPES, R.GEMM_MS):
        for flags in flagset:
            for fam in R.gemm_families(M, K, flags):
                c = R.gemm_case(fam, M, N, K)
                ref, bound, info = R.gemm_ref_bound(c, flags)
                out = R.eval_gemm(c, flags, R.mm32, F32)
                assert bool(torch.isfinite(out).all())
                _note(worst, fam, R.worst_ratio(out, ref, bound))
                # ONE LayerNorm behind one GEMM: every row lies in the first-order domain of the issue's bound
                assert info["first"] <= R.LN_VALID, (fam, M, N, K, flags, info)
                _note(first, fam, info["first"])
    for a2 in ("full", "mod5"):
        c = R.gemm_case("benign", 130, 512, 256, a2=a2)
        ref, bound, _ = R.gemm_ref_bound(c, 1)
        _note(worst, "benign+A2", R.worst_ratio(R.eval_gemm(c, 1, R.mm32, F32), ref, bound))
    _table("fp32 GEMM family, plain fp32 evaluation vs float64", worst)
    _table("  max(delta) / s of the LayerNorm epilogue (<= 0.05)", first)
    assert max(worst.values()) <= 1.0


def test_constant_rows_are_exact_in_fp32():
    """W = 0, bias = 0, constant residual rows (<= 12 significant bits): every partial sum of the mean is exact, the centred
    row is exactly 0 and the output exactly ln_b -- in fp32 as in float64."""
    for M in R.GEMM_MS:
        c = R.gemm_case("constant", M, 256, 256)
        out = R.eval_gemm(c, 6, R.mm32, F32)
        assert torch.equal(out, c.lb.expand(M, 256))
    for dim in R.LN_DIMS:
        c = R.ln_case("constant", R.LN_ROWS, dim)
        assert torch.equal(R.eval_ln(c, F32), c.b.expand(R.LN_ROWS, dim))
    for proj, pre in _tail_forms("f32"):
        c = R.tail_case("constant", 17, 128)
        out, out2 = R.eval_tail(c, R.mm32, F32, proj, pre)
        assert torch.equal(out2 if pre else out, c.lb.expand(17, 256))


@pytest.mark.parametrize("mode", ["f32", "split", "bf16"])
def test_tail_reference_stays_inside_every_bound(mode):
    worst, dom = {}, {}
    for fam, M, ff in _tail_runs(mode):
        for proj, pre in _tail_forms(mode):
            c = R.tail_case(fam, M, ff)
            rb = R.tail_ref_bound(c, mode, proj, pre)
            out, out2 = R.eval_tail(c, MM[mode], F32, proj, pre)
            what = (mode, fam, M, ff, proj, pre)
            _domain_ok(rb["valid"], what)
            assert bool(torch.isfinite(rb["OUT"][1]).all()), what
            if not proj and mode == "f32":
                assert rb["valid"]["first"] <= R.LN_VALID, (what, rb["valid"])          # one LayerNorm: first-order domain
            key = f"{fam}{'/proj' if proj else ''}{'/pre' if pre else ''}"
            _note(worst, key, R.worst_ratio(out, *rb["OUT"]))
            if pre:
                _note(worst, key, R.worst_ratio(out2, *rb["OUT2"]))
            _note(dom, key, rb["valid"]["first"])
    _table(f"layer tail, mode {mode}: its torch emulation vs float64", worst)
    _table("  worst max(delta) / s over the LayerNorms (beyond 0.05: the non-linearised bound)", dom)
    assert max(worst.values()) <= 1.0


def test_split_tail_reference_refuses_the_pre_norm_form():
    with pytest.raises(ValueError, match="no pre-norm form"):
        R.tail_ref_bound(R.tail_case("benign", 17, 64), "split", True, True)


def test_gathered_rows_are_the_residual_rows():
    """tail_mc_case: the two source matrices and the index row reproduce R bit for bit, both signs occur, no row sits at its
    own index (M > 2), and what a wrong gather would read differs from R."""
    for M in (1, 17) + R.MC_MS:
        c = R.tail_mc_case("benign", M, 64, 96)
        assert c.r_idx.dtype == torch.int32 and c.Rg.shape == c.R2.shape == (M, 256)
        assert torch.equal(R.gather_rows(c), c.R)
        if M > 2:
            assert bool((c.r_idx < 0).any()) and bool((c.r_idx >= 0).any())
            for fault in R.GATHER_FAULTS:
                assert not torch.equal(R.gather_rows(c, fault), c.R), fault


def _mc_cases(mode):
    for M, ff, nq in R.mc_runs(mode):
        for fam in R.mc_families(mode, M):
            yield fam, M, ff, nq
    for fam in R.MC_EDGE_FAMILIES:
        yield fam, R.MC_MS[0], *R.MC_EDGE


@pytest.mark.parametrize("mode", ["split", "bf16"])
def test_mc_tail_forms_reference_stays_inside_every_bound(mode):
    """The ride, gather and pre-norm forms on every case tests/test_tail_mc_forms_gpu.py runs.  Two conditions per case: every
    element of OUT, OUT2 and QKV has a FINITE bound (every LayerNorm row inside LN_RIG_VALID), and the mode's plain torch
    emulation in fp32 stays inside every bound.  Left out by name (row_refs.MC_LEFT_OUT): `cancel` in mode "split", one row of
    which has no LayerNorm bound at ff = 128 and 677 rows (ds / s = 0.53).  Nothing is left out in mode "bf16": the ride's bound
    carries OUT's bound through |Wq| and through the one rounding (`flip` adds 1.5 spacings where a rounding boundary lies
    within OUT's bound), which is finite wherever OUT's is, and the emulation meets it on every family.  The ff = 1024 edge
    runs row_refs.MC_EDGE_FAMILIES (benign and cancel have no bound there)."""
    worst = {}
    for fam, M, ff, nq in _mc_cases(mode):
        c = R.tail_mc_case(fam, M, ff, nq)
        what = (mode, fam, M, ff, nq)
        rb = R.tail_ref_bound(c, mode, True, False, ride=True)
        _domain_ok(rb["valid"], what)
        assert bool(torch.isfinite(rb["OUT"][1]).all()) and bool(torch.isfinite(rb["QKV"][1]).all()), what
        out, _, qkv = R.eval_tail(c, MM[mode], F32, True, False, ride=True, gather=True)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(qkv).all()), what
        _note(worst, f"{fam}/ride OUT", R.worst_ratio(out, *rb["OUT"]))
        _note(worst, f"{fam}/ride QKV {nq}", R.worst_ratio(qkv, *rb["QKV"]))
        if mode == "bf16" and nq == R.MC_NQKV[0]:
            rb = R.tail_ref_bound(c, mode, True, True)
            _domain_ok(rb["valid"], what + ("pre",))
            assert bool(torch.isfinite(rb["OUT"][1]).all()) and bool(torch.isfinite(rb["OUT2"][1]).all()), what
            out, out2 = R.eval_tail(c, MM[mode], F32, True, True, gather=True)
            _note(worst, f"{fam}/pre", max(R.worst_ratio(out, *rb["OUT"]), R.worst_ratio(out2, *rb["OUT2"])))
    _table(f"matrix-core tail forms, mode {mode}: its torch emulation vs float64", worst)
    assert max(worst.values()) <= 1.0


def test_dead_tail_reference_is_the_layernorm_of_the_residual():
    """`dead`: the float64 reference the kernels are held to IS LN(X + b2), and its bound carries nothing of the hidden path."""
    c = R.tail_case("dead", 17, 128)
    rb = R.tail_ref_bound(c, "f32", False, False)
    y = c.R.double() + c.b2.double()
    want = torch.nn.functional.layer_norm(y, (256,), c.lg.double(), c.lb.double(), 1e-5)
    assert float((rb["OUT"][0] - want).abs().max()) < 1e-13
    assert float(rb["OUT"][1].max()) < 64 * R.U * float(want.abs().max() + 4)


@pytest.mark.parametrize("mode", ["split", "bf16"])
def test_matrix_core_row_gemm_emulation_stays_inside_every_bound(mode):
    worst = {}
    for N, M in itertools.product(R.ROWS_SPLIT_NS, R.GEMM_MS):
        for fam in R.gemm_families(M, 256, 0):
            c = R.gemm_case(fam, M, N, 256)
            ref, bound, _ = R.gemm_ref_bound(c, 0, mode)
            _note(worst, fam, R.worst_ratio(R.eval_gemm(c, 0, MM[mode], F32), ref, bound))
    if mode == "bf16":
        for (N, K), M, flags in itertools.product(R.GEMM_BF16_SHAPES, R.GEMM_MS, (0, 1, 2, 3)):
            for fam in R.gemm_families(M, K, flags):
                c = R.gemm_case(fam, M, N, K)
                ref, bound, _ = R.gemm_ref_bound(c, flags, mode)
                _note(worst, fam + "/gemm_bf16", R.worst_ratio(R.eval_gemm(c, flags, MM[mode], F32), ref, bound))
    _table(f"row GEMM on the bf16 matrix cores, mode {mode}: torch emulation vs float64", worst)
    assert max(worst.values()) <= 1.0


def test_layernorm_and_l2_reference_stay_inside_every_bound():
    worst = {}
    for dim in R.LN_DIMS:
        for fam in R.FAMILIES_LN:
            c = R.ln_case(fam, R.LN_ROWS, dim)
            ref, bound, info = R.ln_kernel_ref_bound(c)
            assert info["first"] <= R.LN_VALID, (fam, dim, info)
            _note(worst, "layernorm/" + fam, R.worst_ratio(R.eval_ln(c, F32), ref, bound))
    for dim, fam, eps, clamp in itertools.product(R.L2_DIMS, R.L2_FAMILIES, (0.0, 1e-5), (0, 1)):
        c = R.l2_case(fam, 6, dim)
        assert R.in_l2_domain(c.x)
        ref, bound = R.l2_ref_bound(c.x, eps, clamp)
        out = R.eval_l2(c.x, eps, clamp, F32)
        zero = (c.x == 0).all(-1)
        if eps == 0:
            assert bool(torch.isnan(ref[zero]).all()) and bool(torch.isnan(out[zero]).all())
        else:
            assert bool((ref[zero] == 0).all()) and bool((out[zero] == 0).all())
        _note(worst, "l2/" + fam, R.worst_ratio(out[~zero], ref[~zero], bound[~zero]))
    _table("row LayerNorm and L2 normalisation, plain fp32 vs float64", worst)
    assert max(worst.values()) <= 1.0


# ------------------------------------------------------------------------------------------------ power
def _catch(title, faults, attempts):
    """attempts(fault) yields (label, faulty output, ref, bound).  Every fault must be >= POWER bounds away somewhere."""
    print(f"\n{title}")
    for fault in faults:
        best = (0.0, None)
        for label, out, ref, bound in attempts(fault):
            r = R.worst_ratio(out, ref, bound)
            if not bool(torch.isfinite(out).all()):
                r = float("inf")
            if r > best[0]:
                best = (r, label)
        print(f"  {fault:<16s} caught by {best[1]} at {best[0]:.3g} bounds")
        assert best[0] >= POWER, (title, fault, best)


def test_every_planted_error_is_caught_gemm_class():
    """The faulty versions are evaluated in float64: the distance to the reference is the fault's alone.  (The one-pass
    variance E[x^2] - mean^2 is exact in float64: it is an fp32 fault and is evaluated in fp32.)"""
    def attempts(fault):
        dt, mm = (F32, R.mm32) if fault == "one_pass" else (torch.float64, R.mm64)
        for flags in ((3, 7) if fault == "relu_after_res" else (6, 7) if fault in R.LN_FAULTS else (2, 6)):
            for M in (130, 257):
                for fam in R.gemm_families(M, 256, flags):
                    c = R.gemm_case(fam, M, 256, 256)
                    ref, bound, _ = R.gemm_ref_bound(c, flags)
                    yield f"{fam}[M={M}, flags={flags}]", R.eval_gemm(c, flags, mm, dt, fault).double(), ref, bound
    _catch("fp32 GEMM + epilogue", R.LN_FAULTS + R.EPI_FAULTS, attempts)


def test_every_planted_error_is_caught_layernorm_class():
    def attempts(fault):
        for dim in R.LN_DIMS:
            for fam in R.FAMILIES_LN:
                c = R.ln_case(fam, R.LN_ROWS, dim)
                ref, bound, _ = R.ln_kernel_ref_bound(c)
                # the one-pass variance is an fp32 fault (it is exact in float64)
                yield f"{fam}[{dim}]", R.eval_ln(c, F32 if fault == "one_pass" else torch.float64, fault).double(), ref, bound
    _catch("row LayerNorm", R.LN_FAULTS, attempts)


@pytest.mark.parametrize("proj,pre", [(True, False), (True, True), (False, False)])
def test_every_planted_error_is_caught_tail_class(proj, pre):
    def attempts(fault):
        for M, ff in ((17, 128), (257, 128)):
            for fam in R.tail_families(M):
                c = R.tail_case(fam, M, ff)
                rb = R.tail_ref_bound(c, "f32", proj, pre)
                dt = F32 if fault == "one_pass" else torch.float64
                out, out2 = R.eval_tail(c, R.mm32 if dt == F32 else R.mm64, dt, proj, pre, fault)
                yield f"{fam}[M={M}]", out.double(), *rb["OUT"]
                if pre:
                    yield f"{fam}[M={M}] OUT2", out2.double(), *rb["OUT2"]
    _catch(f"fp32 layer tail, proj={proj} pre={pre}", R.LN_FAULTS + R.EPI_FAULTS, attempts)


MM64 = {"split": R.mm64, "bf16": R.mm64_bf}


@pytest.mark.parametrize("mode", ["split", "bf16"])
def test_every_planted_error_is_caught_mc_forms(mode):
    """The faults of the ride, the gather and the pre-norm form, evaluated in float64 on the mode's operands (mode "bf16":
    rounded once), so that the distance is the fault's alone: the same evaluation without a fault stays inside every bound.
    The pre-norm faults exist in the single-piece mode only: the split has no such kernel (tail_ref_bound refuses it)."""
    def attempts(fault):
        pre = fault in R.PRE_FAULTS
        for M, ff, nq in ((R.MC_MS[0], R.MC_WALK_FF[mode], 96), (R.MC_MS[1], R.MC_WALK_FF[mode], 96)):
            for fam in R.mc_families(mode, M):
                c = R.tail_mc_case(fam, M, ff, nq)
                rb = R.tail_ref_bound(c, mode, True, pre, ride=not pre)
                outs = R.eval_tail(c, MM64[mode], torch.float64, True, pre, fault, ride=not pre, gather=True)
                for name, o in zip(("OUT", "OUT2", "QKV"), outs):
                    if o is not None:
                        yield f"{fam}[M={M}, ff={ff}] {name}", o, *rb[name]
    faults = (None,) + R.RIDE_FAULTS + R.GATHER_FAULTS + (R.PRE_FAULTS if mode == "bf16" else ())
    clean = max(R.worst_ratio(o, ref, bound) for _, o, ref, bound in attempts(None))
    assert clean <= 1.0, ("the evaluation without a fault leaves its bound", mode, clean)
    if mode == "bf16":
        c = R.tail_mc_case("benign", R.MC_MS[0], R.MC_WALK_FF[mode], 96)
        rb = R.tail_ref_bound(c, mode, True, True)
        out, out2 = R.eval_tail(c, MM64[mode], torch.float64, True, True, gather=True)
        assert max(R.worst_ratio(out, *rb["OUT"]), R.worst_ratio(out2, *rb["OUT2"])) <= 1.0
    _catch(f"matrix-core tail forms, mode {mode} (ride, gather{', pre-norm' if mode == 'bf16' else '; no pre-norm kernel'})",
           faults[1:], attempts)


def test_every_planted_error_is_caught_split_class():
    """The split's own faults, on the row GEMM (the tails run the same six-product unit): a lost mm product is at most 2^-16
    of a product and a lost third piece likewise, so only a family with ONE product per output (onehot) can see them."""
    def attempts(fault):
        drop = {"drop_mm": ("mm",), "drop_l": ("l",)}[fault]
        for N in R.ROWS_SPLIT_NS:
            for fam in R.gemm_families(257, 256, 0):
                c = R.gemm_case(fam, 257, N, 256)
                ref, bound, _ = R.gemm_ref_bound(c, 0, "split")
                out = R.eval_gemm(c, 0, lambda a, W: R.mm_split(a, W, drop), F32)
                yield f"{fam}[N={N}]", out.double(), ref, bound
    _catch("three-piece split row GEMM", R.SPLIT_FAULTS, attempts)

    def epi(fault):
        for fam in R.gemm_families(257, 256, 0):
            c = R.gemm_case(fam, 257, 64, 256)
            ref, bound, _ = R.gemm_ref_bound(c, 0, "split")
            yield fam, R.eval_gemm(c, 0, R.mm64, torch.float64, fault), ref, bound
    _catch("three-piece split row GEMM, layout faults", ("k_swap", "bias_last32"), epi)


def test_single_piece_bound_tells_one_rounding_from_none_and_from_two_pieces():
    """The single-piece reference is bf16 arithmetic: the unrounded float64 product and the two-piece product (h + m) are both
    >= 10 bounds away on onehot, so the bound separates the contract from its neighbours."""
    c = R.gemm_case("onehot", 257, 64, 256)
    ref, bound, _ = R.gemm_ref_bound(c, 0, "bf16")
    full = R.eval_gemm(c, 0, R.mm64, torch.float64)
    assert R.worst_ratio(full, ref, bound) >= POWER

    def two(a, W):
        ah, am, _ = R.split3(a)
        wh, wm, _ = R.split3(W)
        return (ah + am) @ (wh + wm).t()
    assert R.worst_ratio(R.eval_gemm(c, 0, two, F32), ref, bound) >= POWER


# ------------------------------------------------------------------------------------------------ pow2
def test_pow2_scales_are_exact():
    """(a) the proof of row_refs.pow2_is_safe for every shape and scale the GPU suite scales; (b) the consequence, on the CPU:
    the fp32 / split / single-piece evaluation of the scaled case is the scaled evaluation of the base case, bit for bit."""
    for (N, K, _), M in itertools.product(R.GEMM_SHAPES, (17, 257)):
        base = R.gemm_case("pow2base", M, N, K)
        for s in R.POW2_SCALES:
            assert R.pow2_is_safe(base, s), (M, N, K, s)
            sc = R.gemm_case("pow2", M, N, K, scale=s)
            for flags in (0, 1, 2, 3):
                assert torch.equal(R.eval_gemm(sc, flags, R.mm32, F32), R.eval_gemm(base, flags, R.mm32, F32) * 2.0 ** s)
    for N in R.ROWS_SPLIT_NS + (128,):
        base = R.gemm_case("pow2base", 130, N, 256)
        for s in R.POW2_SCALES_SPLIT:
            assert R.pow2_is_safe(base, s), (N, s)
            sc = R.gemm_case("pow2", 130, N, 256, scale=s)
            for mm in (R.mm_split, R.mm32_bf):
                assert torch.equal(R.eval_gemm(sc, 0, mm, F32), R.eval_gemm(base, 0, mm, F32) * 2.0 ** s)
    assert not R.pow2_is_safe(R.gemm_case("pow2base", 17, 256, 256), -110)       # the proof can fail: 2^-24 2^-110 is subnormal
    assert not R.pow2_is_safe(R.gemm_case("benign", 17, 256, 256), -40)          # and needs the quantised draw
