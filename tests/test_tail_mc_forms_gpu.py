"""The matrix-core layer tails (three-piece split: ffn_split.hip; single piece: ffn_bf16.hip) and their K = 256 row GEMM in the
forms only whole-model tests reached before: the q | k | v ride, the pre-norm form (single piece only) with and without OUT2,
the gathered residual, a device-side row count, padded row strides, and the TILE WALK -- one workgroup running several
128-row tiles with the weight ring running on across them -- at a few hundred rows, through cone_test_tail_mc /
cone_test_rows_mc and their n_cu (the CU count that sizes the persistent grid).

Every launch: outputs NaN-filled with 3 spare rows and padded strides (lda = ldr = ldo = ldo2 = 260, ldq = n_qkv + 4, NaN in
the padding of inputs and outputs); finiteness first, then |out - float64| <= the DERIVED bound elementwise (tests/row_refs.py;
that the references satisfy their own bounds and that every planted fault of these forms leaves them by >= 10 bounds is shown
on the CPU, tests/test_row_kernels_cpu.py), then spare rows and padding columns untouched.  The worst err / bound per (mode,
form, family) is recorded (profiles/row_kernels_measured.txt); the thresholds are the bounds.

The walk is pinned by BIT identities: a launch's rows do not depend on n_cu (0 = one tile per workgroup, 2 = three tiles per
workgroup at 677 = 5 * 128 + 37 rows, 1 = all six; the last tile is partial, five of its waves idle).  For every walked tail
launch the test asserts that the slots a tile consumes, G = NP + 2 ff / 32 + n_qkv / 32, are NO multiple of the ring depth, so
the ring phase really moves from tile to tile; that is what picks ff = 64 for the single-piece mode and ff = 128 for the split
(row_refs.MC_WALK_FF).

Which test launches which kernel (w = walked, u = un-walked; every test is parametrised by mode):
  ffn_split_kernel<false, false>, ffn_bf16_kernel<false, false, false>     A = NULL: test_rows_do_not_depend_on_the_grid (w, u),
                                                                           test_new_entries_give_the_bits_of_the_old_hooks (u)
  ffn_split_kernel<true, false>, ffn_bf16_kernel<true, false, false>       test_forms_against_float64 "gather" (w, u),
                                                                           test_rows_do_not_depend_on_the_grid "proj", "gather" (w, u)
  ffn_split_kernel<true, true>, ffn_bf16_kernel<true, true, false>         test_forms_against_float64 "ride", "gather ride" (w, u),
                                                                           test_rows_do_not_depend_on_the_grid (w, u),
                                                                           test_ride_at_the_lds_edge (u), test_ride_identities (w, u)
  ffn_bf16_kernel<true, false, true>                                       test_forms_against_float64 "pre", "pre, no OUT2" (w, u),
                                                                           test_rows_do_not_depend_on_the_grid (w, u)
  rows256_split_kernel, rows256_bf16_kernel                                test_rows_do_not_depend_on_the_grid (w, u),
                                                                           test_ride_identities (w, u), test_device_row_count (w)"""
import functools

import pytest
import torch

import row_refs as R
from test_row_kernels_gpu import PACK_OF, SPARE, Worst, _dev, _gpu, _hold, _lib, _same_bits, _scratch, run_ffn_mc, run_rows_split

pytestmark = pytest.mark.gpu

MODES = ("split", "bf16")
PAD = 4                                                  # floats of NaN padding behind every row
NSLOT = {"bf16": 8, "split": 3}                          # BF_NSLOT (ffn_bf16.hip), SP_NSLOT (ffn_split.hip): the ring depth
WALK_M, WALK_CU = R.MC_MS[1], 2                          # 677 rows = six tiles, three per workgroup
NAN = float("nan")


def slots_per_tile(proj, ff, n_qkv):
    """G of the kernels: NP = 8 slots of the output projection (PROJ), two per 32-unit hidden chunk, one per 32 q | k | v
    outputs (ffn_split_kernel / ffn_bf16_kernel: `const int G = NP + 2 * nc + NQ`)."""
    return (8 if proj else 0) + 2 * (ff // 32) + n_qkv // 32


def _phase_moves(mode, proj, ff, n_qkv):
    g = slots_per_tile(proj, ff, n_qkv)
    assert g % NSLOT[mode] != 0, (mode, proj, ff, n_qkv, g, "the ring phase would not move from tile to tile")


def _padded(t, pad):
    """t's rows in a buffer of row stride t.shape[1] + pad, NaN in the padding."""
    if not pad:
        return t.contiguous()
    buf = torch.full((t.shape[0], t.shape[1] + pad), NAN, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf


def _out(M, N, pad):
    return torch.full((M + SPARE, N + pad), NAN, device=_gpu())


class Launch:
    """The outputs of one launch: the padded buffers (OUT, OUT2, QKV: None where the form has none) and their widths."""

    def __init__(self, **bufs):
        self.bufs = bufs

    def __getitem__(self, name):
        """The output's columns: (M + SPARE, N)."""
        buf = self.bufs[name]
        return buf[:, :buf.shape[1] - self.pad]

    def padding_untouched(self, what):
        for name, buf in self.bufs.items():
            if buf is not None and self.pad:
                assert bool(torch.isnan(buf[:, -self.pad:]).all()), (what, name, "padding columns written")

    def names(self):
        return [k for k, v in self.bufs.items() if v is not None]


def run_tail(c, mode, *, proj=True, pre=False, out2=True, ride=False, gather=False, pad=PAD, n_cu=0, m_dev=None, M=None,
             R_rows=None):
    """cone_test_tail_mc on the case's operands.  pad = 0: dense strides.  M: the host row count (default c.M); m_dev: the
    device-side one.  R_rows: another residual matrix (the gathered rows materialised)."""
    lib, P, L = _lib()
    d = _dev(c)
    M = c.M if M is None else M
    img = _scratch(("mc ffn", c.ff), lib.cone_test_ffn_split_image_bytes(c.ff))
    wo = _scratch(("mc wo",), lib.cone_test_proj_split_image_bytes())
    nq = c.n_qkv if ride else 0
    qimg = _scratch(("mc q", nq), lib.cone_test_rows_split_image_bytes(nq)) if ride else None
    res = Launch(OUT=_out(M, 256, pad), OUT2=_out(M, 256, pad) if pre and out2 else None, QKV=_out(M, nq, pad) if ride else None)
    res.pad = pad
    A = _padded(d["A"], pad) if proj else None
    if gather:
        Rm, R2, ridx = _padded(d["Rg"], pad), _padded(d["R2"], pad), d["r_idx"]
    else:
        Rm, R2, ridx = _padded(d["R"] if R_rows is None else R_rows, pad), None, None
    mdev = None if m_dev is None else torch.tensor([m_dev], dtype=torch.int32, device=_gpu())
    ld = 256 + pad if pad else 0
    L.check(lib.cone_test_tail_mc(P(A), P(d["Wo"]), P(d["bo"]), P(Rm), P(d["pg"]), P(d["pb"]), P(d["W1"]), P(d["b1"]), P(d["W2"]),
                                  P(d["b2"]), P(d["lg"]), P(d["lb"]), P(res.bufs["OUT"]), M, c.ff, P(ridx), P(R2), P(mdev), int(pre),
                                  P(res.bufs["OUT2"]), P(d["Wq"]) if ride else None, P(d["qb"]) if ride else None,
                                  P(res.bufs["QKV"]), nq, ld, ld, ld, ld, nq + pad if pad and ride else 0, n_cu, P(img), P(wo),
                                  P(qimg), PACK_OF[mode], L.stream()))
    return res


def run_rows(mode, X, ldx, W, bias, M, N, *, pad=PAD, n_cu=0, m_dev=None):
    """cone_test_rows_mc: C (M, N) = X W^T + bias, X a buffer of row stride ldx (0: 256).  -> the padded output buffer."""
    lib, P, L = _lib()
    out = _out(M, N, pad)
    mdev = None if m_dev is None else torch.tensor([m_dev], dtype=torch.int32, device=_gpu())
    L.check(lib.cone_test_rows_mc(P(X), P(W), P(bias), P(out), M, N, P(_scratch(("mc rows", N), lib.cone_test_rows_split_image_bytes(N))),
                                  PACK_OF[mode], ldx, N + pad if pad else 0, P(mdev), n_cu, L.stream()))
    return out


@functools.lru_cache(maxsize=None)
def _ref(mode, fam, M, ff, nq, pre):
    """The float64 reference and bounds of one case, computed once and shared (never modified)."""
    return R.tail_ref_bound(R.tail_mc_case(fam, M, ff, nq), mode, True, pre, ride=not pre)


def _hold_launch(res, M, rb, what):
    """Every output of the launch inside its bound; padding untouched.  -> worst err / bound."""
    worst = 0.0
    for name in res.names():
        worst = max(worst, _hold(res[name], M, *rb[name], what + (name,)))
    res.padding_untouched(what)
    return worst


FORMS = {"ride": dict(ride=True), "gather": dict(gather=True), "gather ride": dict(ride=True, gather=True),
         "proj": dict(), "ffn": dict(proj=False), "pre": dict(pre=True), "pre, no OUT2": dict(pre=True, out2=False)}


def _forms(mode, plain=False):
    names = [n for n, *_ in R.mc_forms(mode)] + (["pre, no OUT2"] if mode == "bf16" else [])
    return names + (["proj", "ffn"] if plain else [])


# ------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("mode,M,ff,nq", [(mode, *run) for mode in MODES for run in R.mc_runs(mode)])
def test_forms_against_float64(mode, M, ff, nq):
    """Ride (OUT and QKV), gathered residual (proj and ride forms), pre-norm (OUT un-normalised, OUT2 normalised; and with OUT2 =
    NULL: OUT carries the same bits) on every family of row_refs.mc_families: 130 rows un-walked, 677 rows with n_cu = 2."""
    walked = M == WALK_M
    n_cu = WALK_CU if walked else 0
    worst = Worst(f"{mode} tail forms")
    for fam in R.mc_families(mode, M):
        c = R.tail_mc_case(fam, M, ff, nq)
        for form in _forms(mode):
            kw = FORMS[form]
            pre = kw.get("pre", False)
            if pre and nq != R.MC_NQKV[0]:
                continue                                  # the pre-norm form has no ride: once per (M, ff)
            if walked:
                _phase_moves(mode, True, ff, nq if kw.get("ride") else 0)
            res = run_tail(c, mode, n_cu=n_cu, **kw)
            worst.note(form, fam, _hold_launch(res, M, _ref(mode, fam, M, ff, nq, pre), (mode, fam, M, ff, nq, form)))
            if form == "pre, no OUT2":
                both = run_tail(c, mode, n_cu=n_cu, **FORMS["pre"])
                assert _same_bits(res.bufs["OUT"], both.bufs["OUT"]), (mode, fam, M, ff, "OUT depends on OUT2 being there")
    worst.record()


@pytest.mark.parametrize("mode", MODES)
def test_ride_at_the_lds_edge(mode):
    """The shipped layout, ff = 1024 and n_qkv = 768: the split mode's ring, b1, parameter rows and q | k | v bias take 157 of
    the 160 KiB of LDS (the qkv_fits edge).  Float64 on the two families that have a bound there (row_refs.MC_EDGE_FAMILIES);
    OUT has the bits of the launch without the ride (cone_test_proj_ffn_split)."""
    ff, nq = R.MC_EDGE
    M = R.MC_MS[0]
    lib = _lib()[0]
    assert lib.cone_test_ffn_split_image_bytes(ff) > 0
    worst = Worst(f"{mode} tail forms")
    for fam in R.MC_EDGE_FAMILIES:
        c = R.tail_mc_case(fam, M, ff, nq)
        res = run_tail(c, mode, ride=True)
        worst.note("ride ff=1024", fam, _hold_launch(res, M, _ref(mode, fam, M, ff, nq, False), (mode, fam, "edge")))
        old, _ = run_ffn_mc(c, mode, True)
        assert _same_bits(res["OUT"], old), (mode, fam, "the ride changed OUT")
    worst.record()


# ------------------------------------------------------------------------------------------------ the walk
def _same_launch(a, b, what):
    for name in a.names():
        assert _same_bits(a.bufs[name], b.bufs[name]), (what, name)


@pytest.mark.parametrize("mode", MODES)
def test_rows_do_not_depend_on_the_grid(mode):
    """Walked vs un-walked: the buffers of one launch at n_cu = 0 (a tile per workgroup), 2 and 1 are identical, bit for bit,
    padding and spare rows included -- every form of the tails at the ff where the ring phase moves (asserted), and the row
    GEMM at N = 96 and 768 (whose G = 3 and 24 are multiples of both ring depths: the phase stays) and N = 160 (G = 5: it
    moves, asserted).  130 rows with n_cu = 1: two tiles, the second with two rows."""
    ff = R.MC_WALK_FF[mode]
    for M in (WALK_M, R.MC_MS[0]):
        for nq in R.MC_NQKV:
            c = R.tail_mc_case("benign", M, ff, nq)
            for form in _forms(mode, plain=True):
                kw = FORMS[form]
                if not kw.get("ride") and nq != R.MC_NQKV[0]:
                    continue
                _phase_moves(mode, kw.get("proj", True), ff, nq if kw.get("ride") else 0)
                base = run_tail(c, mode, n_cu=0, **kw)
                assert bool(torch.isfinite(base["OUT"][:M]).all()), (mode, form, M)
                for n_cu in (2, 1):
                    _same_launch(base, run_tail(c, mode, n_cu=n_cu, **kw), (mode, form, M, nq, f"n_cu = {n_cu} changed the bits"))
        for N in (96, 768, 160):
            g = R.gemm_case("benign", M, N, 256)
            d = _dev(g)
            X = _padded(d["A"], PAD)
            base = run_rows(mode, X, 256 + PAD, d["W"], d["bias"], M, N)
            assert bool(torch.isfinite(base[:M, :N]).all()) and bool(torch.isnan(base[M:]).all()) and bool(torch.isnan(base[:, N:]).all())
            if N == 160:
                assert (N // 32) % NSLOT[mode] != 0
            for n_cu in (2, 1):
                assert _same_bits(base, run_rows(mode, X, 256 + PAD, d["W"], d["bias"], M, N, n_cu=n_cu)), (mode, "rows", N, M, n_cu)
            if N != 160:                                  # and the bits of the old hook (dense)
                assert _same_bits(base[:M, :N], run_rows_split(g, mode)[:M]), (mode, "rows", N, M, "strided vs cone_test_rows_split")


@pytest.mark.parametrize("mode", MODES)
def test_strided_and_dense_operands_give_the_same_rows(mode):
    """Padded strides (260, n_qkv + 4) against dense ones, M = 1, 17, 130 and 677 walked: identical rows."""
    for M in (1, 17) + R.MC_MS:
        ff = R.MC_WALK_FF[mode]
        n_cu = WALK_CU if M == WALK_M else 0
        c = R.tail_mc_case("benign", M, ff, R.MC_NQKV[0])
        for form in _forms(mode, plain=True):
            a, b = run_tail(c, mode, n_cu=n_cu, **FORMS[form]), run_tail(c, mode, n_cu=n_cu, pad=0, **FORMS[form])
            a.padding_untouched((mode, form, M))
            for name in a.names():
                assert bool(torch.isfinite(b[name][:M]).all()) and bool(torch.isnan(b[name][M:]).all()), (mode, form, M, name)
                assert _same_bits(a[name], b[name]), (mode, form, M, name, "the strides changed the bits")


@pytest.mark.parametrize("mode", MODES)
def test_device_row_count(mode):
    """M_dev = 0, 1, 100, 677 under a host bound of 677 rows and n_cu = 2: rows below M_dev carry the bits of the plain launch,
    rows from M_dev on of OUT, OUT2 and QKV (and of the row GEMM's C) stay NaN, M_dev = 0 writes nothing."""
    M, ff, nq = WALK_M, R.MC_WALK_FF[mode], R.MC_NQKV[0]
    c = R.tail_mc_case("benign", M, ff, nq)
    g = R.gemm_case("benign", M, 160, 256)
    d = _dev(g)
    X = _padded(d["A"], PAD)
    plain_rows = run_rows(mode, X, 256 + PAD, d["W"], d["bias"], M, 160, n_cu=WALK_CU)
    for form in ["gather ride"] + (["pre"] if mode == "bf16" else []):
        plain = run_tail(c, mode, n_cu=WALK_CU, **FORMS[form])
        for m_dev in (0, 1, 100, M):
            res = run_tail(c, mode, n_cu=WALK_CU, m_dev=m_dev, **FORMS[form])
            for name in res.names():
                assert _same_bits(res.bufs[name][:m_dev], plain.bufs[name][:m_dev]), (mode, form, m_dev, name)
                assert bool(torch.isnan(res.bufs[name][m_dev:]).all()), (mode, form, m_dev, name, "rows past M_dev written")
    for m_dev in (0, 1, 100, M):
        out = run_rows(mode, X, 256 + PAD, d["W"], d["bias"], M, 160, n_cu=WALK_CU, m_dev=m_dev)
        assert _same_bits(out[:m_dev], plain_rows[:m_dev]) and bool(torch.isnan(out[m_dev:]).all()), (mode, "rows", m_dev)


@pytest.mark.parametrize("mode", MODES)
def test_gathered_rows_are_the_same_rows_read_from_another_place(mode):
    """The gathered residual (r_idx over two source matrices, both signs) against the same rows materialised contiguously."""
    ff, nq = R.MC_WALK_FF[mode], R.MC_NQKV[0]
    for M in R.MC_MS:
        n_cu = WALK_CU if M == WALK_M else 0
        c = R.tail_mc_case("benign", M, ff, nq)
        assert torch.equal(R.gather_rows(c), c.R)
        for form in ["proj", "ride"] + (["pre"] if mode == "bf16" else []):
            _same_launch(run_tail(c, mode, n_cu=n_cu, **FORMS[form]), run_tail(c, mode, n_cu=n_cu, gather=True, **FORMS[form]),
                         (mode, form, M, "the gather changed the bits"))


@pytest.mark.parametrize("mode", MODES)
def test_ride_identities(mode):
    """Ride vs no ride: identical OUT.  QKV = the row-GEMM entry run on that OUT with Wq's image -- the same products in the
    same order, in both modes: the ride converts (splits) the registers that hold the stored OUT exactly as the row GEMM
    converts the rows it loads, and both run the same slot loop on the same image."""
    ff = R.MC_WALK_FF[mode]
    for M in R.MC_MS:
        n_cu = WALK_CU if M == WALK_M else 0
        for nq in R.MC_NQKV:
            c = R.tail_mc_case("benign", M, ff, nq)
            d = _dev(c)
            ride, plain = run_tail(c, mode, n_cu=n_cu, ride=True), run_tail(c, mode, n_cu=n_cu)
            assert _same_bits(ride.bufs["OUT"], plain.bufs["OUT"]), (mode, M, nq, "the ride changed OUT")
            qkv = run_rows(mode, ride.bufs["OUT"], 256 + PAD, d["Wq"], d["qb"], M, nq, n_cu=n_cu)
            assert _same_bits(ride.bufs["QKV"], qkv), (mode, M, nq, "the ride's QKV is not the row GEMM of its OUT")


@pytest.mark.parametrize("mode", MODES)
def test_new_entries_give_the_bits_of_the_old_hooks(mode):
    """Dense strides, no ride, no pre-norm, n_cu = 0: cone_test_tail_mc = cone_test_ffn_split / cone_test_proj_ffn_split and
    cone_test_rows_mc = cone_test_rows_split."""
    for ff in R.TAIL_FFS[mode]:
        for M in (1, 17) + R.MC_MS:
            c = R.tail_mc_case("benign", M, ff, R.MC_NQKV[0])
            for proj in (False, True):
                new = run_tail(c, mode, proj=proj, pad=0)
                old, _ = run_ffn_mc(c, mode, proj)
                assert _same_bits(new.bufs["OUT"], old), (mode, ff, M, proj)
    for N in R.ROWS_SPLIT_NS:
        for M in (1, 17) + R.MC_MS:
            g = R.gemm_case("benign", M, N, 256)
            d = _dev(g)
            assert _same_bits(run_rows(mode, d["A"], 0, d["W"], d["bias"], M, N, pad=0), run_rows_split(g, mode)), (mode, N, M)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_by_name():
    """Each refused before anything is launched: the outputs stay NaN."""
    lib, P, L = _lib()
    c = R.tail_mc_case("benign", 17, 64, 96)

    def refused(match, mode="split", **kw):
        with pytest.raises(L.ConeHipError, match=match):
            run_tail(c, mode, **kw)

    refused("no pre-norm form", pre=True)
    refused("negative CU count", n_cu=-1)
    refused("negative CU count", mode="bf16", n_cu=-1, proj=False)
    d = _dev(c)
    dev = _gpu()

    def call(mode, *, ridx=None, R2=None, lda=0, ff=64, nq=0, Wq=None, b1=None, pack=None):
        out, qkv = _out(17, 256, 0), _out(17, max(nq, 32), 0)
        rc = lib.cone_test_tail_mc(P(d["A"]), P(d["Wo"]), P(d["bo"]), P(d["R"]), P(d["pg"]), P(d["pb"]), P(d["W1"]),
                                   P(d["b1"] if b1 is None else b1), P(d["W2"]), P(d["b2"]), P(d["lg"]), P(d["lb"]), P(out), 17, ff,
                                   P(ridx), P(R2), None, 0, None, P(Wq), P(d["qb"]) if Wq is not None else None,
                                   P(qkv) if Wq is not None else None, nq, lda, 0, 0, 0, 0, 0,
                                   P(_scratch(("mc ffn", 64), lib.cone_test_ffn_split_image_bytes(64))),
                                   P(_scratch(("mc wo",), lib.cone_test_proj_split_image_bytes())),
                                   P(_scratch(("mc q", 96), lib.cone_test_rows_split_image_bytes(96))),
                                   PACK_OF[mode] if pack is None else pack, L.stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(qkv).all()), "a refused launch wrote"
        return rc, lib.cone_last_error().decode()

    for mode in MODES:
        rc, msg = call(mode, ridx=d["r_idx"])
        assert rc != 0 and "needs both source matrices" in msg, msg
        rc, msg = call(mode, lda=258)
        assert rc != 0 and "multiples of 4" in msg, msg
    # a ride that does not fit the LDS: split mode, ff = 2048 with n_qkv = 768 needs 161 KiB.  pack = 0 keeps the (split) mode and
    # builds no image: the launcher refuses ahead of the launch, so the ff = 64 scratch is never read as a larger image
    b1 = torch.zeros(2048, device=dev)
    Wq = torch.zeros(768, 256, device=dev)
    rc, msg = call("split", ff=2048, nq=768, Wq=Wq, b1=b1, pack=0)
    assert rc != 0 and "exceed 160 KiB" in msg, msg
    g = R.gemm_case("benign", 17, 96, 256)
    gd = _dev(g)
    for mode in MODES:
        with pytest.raises(L.ConeHipError, match="negative CU count"):
            run_rows(mode, gd["A"], 0, gd["W"], gd["bias"], 17, 96, n_cu=-1)
