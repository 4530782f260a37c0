"""Every instantiation of the shipped model's attention cores against float64 at its tile edges, through the kernel-level
hooks (cone_test_enc_attn / cone_test_enc_attn_txt, cone_test_dec_cross / cone_test_dec_cross_ex, cone_test_small_attn).
References and batches: tests/attention_refs.py; that every window of these batches can FAIL (a key or a table row off by
one moves the float64 result by >= 10 TOL) is proved on the CPU in tests/test_attention_cores_cpu.py.

Every test fills OUT with NaN plus spare rows, asserts that the real rows are finite and within TOL = 2e-5 of float64 (the
bound of every kernel-level attention test of this project) and that the spare rows are untouched, and prints its worst
distance.

Which test enters which launcher case (attention.hip, dec_cross.hip, dec_cross_mfma.hip):
  CONE_ATTN16(6 .. 12) / CONE_ATTN16D(13 .. 16), modes packed / gather / pos-add / gather | 4 / pos-add | 4
                                        test_encoder_core_matches_float64[n-mode]; Lmax = 1 on the 6-wave build: [6-*]
                                        test_encoder_core_saturated_scores (NKT 7, 10, 12, 16; packed and pos-add)
  CONE_ATTNW(6 .. 9)                    test_encoder_wave_form_is_bit_identical (equal bits with the workgroup form, which
                                        the test above holds against float64 on the same batches)
  launch_mfma_one<2, true> (5 slots)    test_decoder_cross_beyond_128_keys[variant 2 | 3, also 4 beyond 110 tokens]
                                        test_decoder_cross_saliency_ride[150]
  launch_mfma_one<1, true> / launch_x_one<true>
                                        test_decoder_cross_saliency_ride[110] (per-window / shared queries, variant 2)
  launch_mfma_one<2, false>             test_decoder_cross_xp_operand[150, variants 2 | 3 | 4]
  launch_mfma_one<1, false>             test_decoder_cross_xp_operand[110 | 128, variants 2 | 3; 128, variant 4]
  launch_res_one<false>                 test_decoder_cross_xp_operand[110, variant 4]
  launch_dec_cross above 128 keys       test_decoder_cross_beyond_128_keys[variant 1] (launch_one<5, 3, true>)
  launch_dec_cross with XP              test_decoder_cross_xp_operand[variant 1] (launch_one<5, 2 | 3, false>)
  the saliency ride                     test_decoder_cross_saliency_ride
  refusals by name                      test_decoder_cross_refuses_by_name, test_small_cross_attention_refuses_193_keys
  dec_self_attn_kernel<3 | 5 | 8 | 10>  test_small_self_attention_matches_float64[nq-256] for those nq
  small_attn_kernel<8 | 16>, self form  test_small_self_attention_matches_float64[nq-257] (every nq), [nq-256] (other nq)
  small_attn_kernel<8 | 16>, cross form test_small_cross_attention_matches_float64"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import attention_refs as R

pytestmark = pytest.mark.gpu

TOL = R.TOL
SENTINEL = 12345.0


def _gpu():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda", 0)


def maxdiff(a, b):
    return float((a.detach().cpu().double() - torch.as_tensor(b).double()).abs().max())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _dev(c, names):
    """The case's tensors on the device, uploaded once per case (the position tables are tens of MiB)."""
    if not hasattr(c, "_d"):
        c._d = {}
    dev = _gpu()
    for k in names:
        if k not in c._d:
            v = getattr(c, k)
            if isinstance(v, np.ndarray):
                v = torch.from_numpy(v)
            elif isinstance(v, list):
                v = torch.tensor(v, dtype=torch.int32)
            c._d[k] = v.to(dev).contiguous()
    return c._d


def _check_rows(out, ref, n_real, what):
    """Real rows finite and within TOL, spare rows untouched; -> the worst distance."""
    assert bool(torch.isfinite(out[:n_real]).all()), what
    assert bool(torch.isnan(out[n_real:]).all()), (what, "spare rows written")
    worst = maxdiff(out[:n_real], ref)
    print(f"{what}: worst distance to float64 {worst:.3g}")
    assert worst < TOL, (what, worst)
    return worst


# ------------------------------------------------------------------------------------------------ encoder core
def _enc_run(c, mode, txt_hook, packed="QKV"):
    """One launch over case c; txt_hook: None = cone_test_enc_attn, "null" / "rows" = cone_test_enc_attn_txt without / with
    the text position rows.  mode may carry the 0x200 form bit.  -> OUT (M + 2, 256) on the device."""
    from cone_amd import _lib
    lib = _lib.load()
    d = _dev(c, [packed, "qkv_vid", "qkv_txt", "pos", "txt_pos", "vrow0", "vl", "trow0", "off"])
    out = torch.full((c.M + 2, 256), float("nan"), device=_gpu())
    P = _lib.ptr
    if txt_hook is None:
        rc = lib.cone_test_enc_attn(mode, P(d[packed]), P(d["qkv_vid"]), P(d["qkv_txt"]), P(d["pos"]), P(d["vrow0"]), P(d["vl"]),
                                    P(d["trow0"]), P(d["off"]), P(out), c.B, c.Lmax, c.zrow, _lib.stream())
    else:
        rc = lib.cone_test_enc_attn_txt(mode & ~4, P(d[packed]), P(d["qkv_vid"]), P(d["qkv_txt"]), P(d["pos"]),
                                        P(d["txt_pos"]) if txt_hook == "rows" else None, P(d["vrow0"]), P(d["vl"]),
                                        P(d["trow0"]), P(d["off"]), P(out), c.B, c.Lmax, c.zrow, _lib.stream())
    _lib.check(rc)
    torch.cuda.synchronize()
    return out


def _enc_hook(mode):
    return "rows" if mode & 4 else ("null" if mode == 0 else None)


@pytest.mark.parametrize("n,mode", [(n, m) for n in range(6, 17) for m in R.MODES])
def test_encoder_core_matches_float64(n, mode):
    """enc_attn16_kernel<n, mode>: the batch of R.enc_lengths(n) has Lmax = 16 n exactly, so launch_enc_attn_t picks that
    build.  Modes 0 and the two | 4 forms go through cone_test_enc_attn_txt, modes 1 and 2 through cone_test_enc_attn -- and
    through the new hook without text rows, which must give the same bits.  n = 6 also runs the batch with Lmax = 1."""
    for c in ([R.enc_case(n), R.enc_case(n, short=True)] if n == 6 else [R.enc_case(n)]):
        ref = R.enc_ref64(R.enc_rows(mode, c), c.off)
        out = _enc_run(c, mode, _enc_hook(mode))
        _check_rows(out, ref, c.M, f"enc_attn16<{n}, {mode}> Lmax={c.Lmax}")
        if mode in (1, 2):
            again = _enc_run(c, mode, "null")
            assert torch.equal(_bits(out[:c.M]), _bits(again[:c.M])), "the two hooks disagree on a mode both reach"


@pytest.mark.parametrize("n,mode", [(n, m) for n in range(6, 10) for m in (0, 1, 2)])
def test_encoder_wave_form_is_bit_identical(n, mode):
    """enc_attn_wave_kernel<n, mode> (mode | 0x200): the bits of the workgroup form on the batches of the test above."""
    for c in ([R.enc_case(n), R.enc_case(n, short=True)] if n == 6 else [R.enc_case(n)]):
        wg = _enc_run(c, mode, None)
        wave = _enc_run(c, mode | 0x200, None)
        assert bool(torch.isfinite(wave[:c.M]).all()) and bool(torch.isnan(wave[c.M:]).all())
        assert torch.equal(_bits(wg[:c.M]), _bits(wave[:c.M]))
        print(f"enc_attn_wave<{n}, {mode}> Lmax={c.Lmax}: equal bits; distance to float64 "
              f"{maxdiff(wave[:c.M], R.enc_ref64(R.enc_rows(mode, c), c.off)):.3g}")


@pytest.mark.parametrize("lv,lt", R.SAT_WINDOWS)
@pytest.mark.parametrize("mode", [0, 2])
def test_encoder_core_saturated_scores(mode, lv, lt):
    """Scores of about +-60 with every row's maximum at the LAST key, on the cores that carry their scores in the log2 domain
    (kQScaleLog2, exp2) and normalise after P.V: windows of 110 / 150 / 192 / 256 tokens = NKT 7, 10, 12, 16."""
    c = R.enc_saturated_case(lv, lt)
    ref = R.enc_ref64(R.saturated_rows(mode, c), c.off)
    out = _enc_run(c, mode, "null", packed="QKV" if mode == 0 else "QKV_table")
    _check_rows(out, ref, c.M, f"saturated, {lv + lt} tokens, mode {mode}")


# ------------------------------------------------------------------------------------------------ folded decoder cross-attention
@functools.lru_cache(maxsize=8)
def _dec_ref(Lmax, shared, use_xp):
    return R.dec_cross64(R.dec_case(Lmax, 5, shared), use_xp)


def _dec_run(c, variant, slabs, use_xp=False, ride=0, old_hook=False):
    """-> (rc, OUT (B nq + 2, 256), sal (B + 1, ride) or None).  ride = sal_ld (0: no saliency ride)."""
    from cone_amd import _lib
    lib = _lib.load()
    dev = _gpu()
    if not hasattr(c, "WvT"):
        c.WvT = c.Wv.t().contiguous()
    d = _dev(c, ["DQ", "XP", "X", "pos", "vl", "off", "Wk", "WvT", "bv", "sal_w", "sal_b"])
    P = _lib.ptr
    out = torch.full((c.B * c.nq + 2, 256), float("nan"), device=dev)
    sl = torch.empty(lib.cone_test_dec_cross_slab_floats(), device=dev) if slabs else None
    sal = torch.full((c.B + 1, ride), SENTINEL, device=dev) if ride else None
    if old_hook:
        assert not use_xp and not ride
        rc = lib.cone_test_dec_cross(P(d["DQ"]), P(d["X"]), P(d["pos"]), P(d["vl"]), P(d["off"]), P(d["Wk"]), P(d["WvT"]),
                                     P(d["bv"]), P(out), c.B, c.nq, c.Lmax, variant, P(sl), _lib.stream())
    else:       # with XP the table and the clip counts are not handed over at all
        rc = lib.cone_test_dec_cross_ex(P(d["DQ"]), P(d["XP"]) if use_xp else None, P(d["X"]), None if use_xp else P(d["pos"]),
                                        None if use_xp else P(d["vl"]), P(d["off"]), P(d["Wk"]), P(d["WvT"]), P(d["bv"]),
                                        P(out), c.B, c.nq, c.Lmax, variant, P(sl), P(d["sal_w"]) if ride else None,
                                        P(d["sal_b"]) if ride else None, P(sal), ride, _lib.stream())
    torch.cuda.synchronize()
    return rc, out, sal


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("variant,Lmax", [(v, L) for v in (2, 3, 1, 4) for L in (129, 150, 192)] +
                         [(v, L) for v in (2, 3) for L in (193, 241, 256)])
def test_decoder_cross_beyond_128_keys(variant, Lmax, shared):
    """5 slots, windows of more than 128 tokens: dec_cross_mfma_kernel<2, true> (variants 2, 3; variant 4 beyond its 110
    tokens takes the same two-read form), where wave w owns key tiles w and w + 8, and the VALU kernel's 192-key build
    (variant 1).  One batch mixes Lmax, 1, 16, 17, 128, 129, 143, 144, 145 (240, 241): waves with and without a second tile
    and one-key tiles in one launch.  ``shared``: the same query rows for every window (matrix-core forms: the operand slabs
    built once; the VALU kernel has no such form and reads the repeated rows)."""
    from cone_amd import _lib
    c = R.dec_case(Lmax, 5, shared)
    rc, out, _ = _dec_run(c, variant, slabs=shared and variant != 1, old_hook=True)
    _lib.check(rc)
    _check_rows(out, _dec_ref(Lmax, shared, False)[0], c.B * 5, f"dec cross variant {variant} Lmax={Lmax} shared={shared}")


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("variant", [2, 3, 4, 1])
@pytest.mark.parametrize("Lmax", [110, 128, 150])
def test_decoder_cross_xp_operand(Lmax, variant, shared):
    """The precomputed memory + pos operand (the --use_txt_pos decoder): K = XP Wk^T, V = X Wv^T + bv.  XP = X + table rows
    + a perturbation, and neither the table nor the clip counts are handed over: reading X for the keys cannot pass."""
    from cone_amd import _lib
    c = R.dec_case(Lmax, 5, shared)
    rc, out, _ = _dec_run(c, variant, slabs=shared and variant != 1, use_xp=True)
    _lib.check(rc)
    _check_rows(out, _dec_ref(Lmax, shared, True)[0], c.B * 5, f"dec cross XP variant {variant} Lmax={Lmax} shared={shared}")


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("variant", [2, 3])
@pytest.mark.parametrize("Lmax", [110, 150])
def test_decoder_cross_saliency_ride(Lmax, variant, shared):
    """The saliency head riding in the cross-attention launch: sal[b, p] = <raw memory row p, sal_w> + sal_b for p < lv, the
    rest of the row and the spare row untouched, sal_ld < lv clips, and the attention output keeps its bits."""
    from cone_amd import _lib
    c = R.dec_case(Lmax, 5, shared)
    ref, sal_ref = _dec_ref(Lmax, shared, False)
    rc, plain, _ = _dec_run(c, variant, slabs=shared)
    _lib.check(rc)
    _check_rows(plain, ref, c.B * 5, f"dec cross variant {variant} Lmax={Lmax} shared={shared}")
    wide, narrow = max(c.vl) + 3, 40
    assert sum(v > narrow for v in c.vl) >= 2 and sum(0 < v < narrow for v in c.vl) >= 2
    for ld in (wide, narrow):
        rc, out, sal = _dec_run(c, variant, slabs=shared, ride=ld)
        _lib.check(rc)
        assert torch.equal(_bits(out), _bits(plain)), "the ride changed the attention output"
        sal = sal.cpu()
        worst = 0.0
        for b in range(c.B):
            n = min(c.vl[b], ld)
            assert bool(torch.isfinite(sal[b, :n]).all())
            if n:
                worst = max(worst, maxdiff(sal[b, :n], sal_ref[b][:n]))
            assert bool((sal[b, n:] == SENTINEL).all()), (b, "entries past the window's clips written")
        assert bool((sal[c.B] == SENTINEL).all())
        print(f"saliency ride variant {variant} Lmax={Lmax} shared={shared} sal_ld={ld}: worst distance to float64 {worst:.3g}")
        assert worst < TOL


def test_decoder_cross_refuses_by_name():
    """A Lmax beyond a form's limit is refused by name and does not run: the VALU form at 193 keys, 10 slots at 129 (and the
    saliency ride on forms that have none)."""
    from cone_amd import _lib
    lib = _lib.load()
    for c, variant, kw, text in ((R.dec_case(193, 5, False), 1, {}, "nq=5 Lmax=193 unsupported"),
                                 (R.dec_case(129, 10, False), 2, {}, "nq=10 Lmax=129 unsupported"),
                                 (R.dec_case(129, 10, False), 3, dict(old_hook=True), "nq=10 Lmax=129 unsupported"),
                                 (R.dec_case(110, 5, False), 4, dict(ride=96), "saliency"),
                                 (R.dec_case(110, 5, False), 1, dict(ride=96), "saliency"),
                                 (R.dec_case(110, 5, False), 3, dict(ride=96, use_xp=True), "saliency")):
        rc, out, sal = _dec_run(c, variant, slabs=False, **kw)
        assert rc < 0, (variant, c.Lmax, c.nq)
        assert text in lib.cone_last_error().decode(), lib.cone_last_error().decode()
        assert bool(torch.isnan(out).all()), "a refused call wrote"
        assert sal is None or bool((sal == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ the decoder's small attentions
def _off_ptr(t, floats):
    return C.c_void_p(t.data_ptr() + 4 * floats)


@pytest.mark.parametrize("ldo", [256, 257])
@pytest.mark.parametrize("nq", list(range(1, 17)))
def test_small_self_attention_matches_float64(nq, ldo):
    """Self-attention over the nq slots of B windows from a packed q | k | v buffer (ld = 768): with ldo = 256 the slot counts
    3 / 5 / 8 / 10 run dec_self_attn_kernel<nq> (four windows per workgroup: B = 1, 3, 4, 5, 9 leave partial last workgroups),
    every other count -- and every count with an output stride that is no multiple of 4 -- small_attn_kernel<8 | 16>."""
    from cone_amd import _lib
    lib = _lib.load()
    dev = _gpu()
    qkv = R.small_self_case(nq)
    qd = qkv.to(dev)
    worst = 0.0
    for B in R.SMALL_SELF_B:
        rows = B * nq
        ref = torch.cat([R.small_self_window64(qkv, nq, b) for b in range(B)])
        out = torch.full((rows + 2, ldo), float("nan"), device=dev)
        _lib.check(lib.cone_test_small_attn(_lib.ptr(qd), 768, _off_ptr(qd, 256), 768, _off_ptr(qd, 512), 768, _lib.ptr(out),
                                            ldo, None, B, nq, nq, _lib.stream()))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out[:rows, :256]).all()), (nq, B)
        assert bool(torch.isnan(out[rows:]).all()) and bool(torch.isnan(out[:, 256:]).all()), (nq, B, "spare rows / columns written")
        worst = max(worst, maxdiff(out[:rows, :256], ref))
    print(f"small self-attention nq={nq} ldo={ldo}: worst distance to float64 {worst:.3g}")
    assert worst < TOL


def _small_cross_run(c, Lmax):
    from cone_amd import _lib
    lib = _lib.load()
    d = _dev(c, ["Q", "KD", "VD", "off"])
    out = torch.full((c.B * c.nq + 2, 256), float("nan"), device=_gpu())
    ld = R.D * R.SMALL_ND
    rc = lib.cone_test_small_attn(_lib.ptr(d["Q"]), 256, _off_ptr(d["KD"], R.D), ld, _off_ptr(d["VD"], R.D), ld, _lib.ptr(out), 256,
                                  _lib.ptr(d["off"]), c.B, c.nq, Lmax, _lib.stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("nq", [1, 5, 8, 9, 16])
def test_small_cross_attention_matches_float64(nq):
    """small_attn_kernel<8 | 16>, cross form: a ragged batch with 1, 63, 64, 65, 127, 128, 129, 191 and 192 keys (the kernel
    walks keys in three rounds of 64 lanes), K / V strided as the unfolded decoder passes them: the second layer's 256-column
    slice of rows with ld = 256 nd."""
    from cone_amd import _lib
    c = R.small_cross_case(nq)
    rc, out = _small_cross_run(c, c.Lmax)
    _lib.check(rc)
    ref = torch.cat([R.small_cross_window64(c, b) for b in range(c.B)])
    _check_rows(out, ref, c.B * nq, f"small cross-attention nq={nq}")


def test_small_cross_attention_refuses_193_keys():
    from cone_amd import _lib
    rc, out = _small_cross_run(R.small_cross_case(5), 193)
    assert rc < 0 and "193 keys > 192" in _lib.load().cone_last_error().decode()
    assert bool(torch.isnan(out).all()), "a refused call wrote"
