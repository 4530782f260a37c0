"""The stage-B front end and glue kernels at their workgroup, wave and lane edges, each through the launcher the forward path
calls (the cone_test_* entries of include/cone_hip.h and the public cone_pos_tables, cone_mask_lengths, cone_window_table,
cone_layer0_text_positions).  References, case families, bounds: tests/glue_refs.py; that the references deserve trust and
that every planted error is seen: tests/test_glue_kernels_cpu.py.

Every output buffer is filled with a NaN pattern first (glue_refs.poison) and carries SPARE rows behind its last one; every
test checks the values inside the expected write set AND that nothing outside it changed.  Integers, gathers and copies are
compared bit for bit; dots against row_refs.gemm_delta; LayerNorm rows against row_refs.ln_ref_bound; sine rows against
glue_refs.sine_bound() (8 x the CPU's fp32 sin / cos error on the table's own arguments: not taken from the device).  The
device's worst sine distances are recorded (test_gpu_parity.record_measured; profiles/glue_kernels_measured.txt).

Which test enters which kernel:
  scan_lengths_kernel                    test_scan_lengths[B-kind] (qlen given and NULL)
  compact_index_kernel                   test_compact_index[B-Lv_pad-Lq_pad]
  row_index_kernel                       test_row_index
  pack_pos_kernel                        test_pack_pos[tpe] (tpe NULL / given), test_pack_pos_long_windows
  gen_pack_pos_kernel                    test_gen_pack_pos[d-tpe]
  pack_l0_kernel                         test_pack_l0[qk-pos] (QK, POS each NULL or not)
  add_pos_rows_kernel                    test_add_pos_rows[txt_pos]
  pos_rows_kernel, gen_pos_rows_kernel   test_pos_tables[d-max_v_l] (+ the zero row, pos_qk), test_pos_tables_prefix_and_refusals
  txt_pos_rows_kernel, gen_txt_pos_rows_kernel
                                         test_txt_pos_rows[d-n], test_layer0_text_positions_same_bits[d]
  saliency_kernel, gen_saliency_kernel   test_saliency_and_memory_tap[d-dLv-dLq]
  rowdot_kernel, gen_rowdot_kernel       test_heads[d-n_rows]
  tile_rows_kernel, tile_rows2_kernel    test_tile_rows[period]
  mask_lengths_kernel                    test_mask_lengths[L]
  window_table_kernel, window_pad_kernel test_window_table[W-eval_bsz-K-sparse], test_window_table_refusals
  the B > maxGridSize[1] refusal         test_forward_refuses_more_windows_than_the_grid_holds"""
import itertools

import numpy as np
import pytest
import torch

import glue_refs as G
import row_refs as R
from test_gpu_parity import record_measured

pytestmark = pytest.mark.gpu

SPARE = 3


def _gpu():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda", 0)


def _lib():
    from cone_amd import _lib
    return _lib.load(), _lib.ptr, _lib


_ALIVE = []


@pytest.fixture(autouse=True)
def _release_uploads():
    yield
    _ALIVE.clear()


def dv(a, dtype=None):
    """numpy / torch -> a contiguous device tensor (int arrays as int32, float arrays as fp32).  It stays alive until the test
    ends: a raw pointer handed to the library keeps nothing alive, and the caching allocator hands the block of a temporary
    that died inside an argument list to the very next upload of the same list."""
    t = torch.as_tensor(np.ascontiguousarray(a)) if not isinstance(a, torch.Tensor) else a
    if dtype is None:
        dtype = torch.float32 if t.is_floating_point() else torch.int32
    t = t.to(dtype).contiguous().to(_gpu())
    _ALIVE.append(t)
    return t


def P_(*shape, dtype=torch.float32):
    return G.poison(*shape, dtype=dtype, device=_gpu())


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def rows_written(n, total):
    m = np.zeros(total, bool)
    m[:n] = True
    return m


def hold(out, ref, bound, what):
    """Every element finite and inside its bound.  -> the worst |out - ref| and the worst err / bound."""
    out = np.asarray(out, np.float64)
    assert np.isfinite(out).all(), (what, "not finite")
    err = np.abs(out - ref)
    bad = err > bound
    ratio = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)))) if err.size else 0.0
    assert not bad.any(), (what, f"{int(bad.sum())} elements outside their bound, worst err {float(err.max()):.3g}, "
                                 f"worst err / bound {ratio:.3g}")
    return (float(err.max()) if err.size else 0.0), ratio


_MODELS = {}
HEADS = {256: 8, 128: 4, 512: 8}


def get_model(d):
    """A --use_txt_pos handle of width d (random weights)."""
    from cone_amd import synth
    from cone_amd.config import make_opt
    from cone_amd.model import build_model
    if d not in _MODELS:
        opt = make_opt("ego4d", hidden_dim=d, nheads=HEADS[d], use_txt_pos=True)
        sd = synth.make_state_dict(opt, 40 + d)
        m, _ = build_model(opt)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        _MODELS[d] = (m, opt, sd)
    return _MODELS[d]


# ------------------------------------------------------------------------------------------------ scan, compaction
@pytest.mark.parametrize("kind", G.SCAN_KINDS)
@pytest.mark.parametrize("B", G.SCAN_BS)
def test_scan_lengths(B, kind):
    lib, P, L = _lib()
    v, q = G.scan_case(B, kind)
    dvl, dql = dv(v), dv(q)
    for ql, dq in ((q, dql), (None, None)):
        off = P_(B + 1 + SPARE, dtype=torch.int32)
        L.check(lib.cone_test_scan_lengths(P(dvl), P(dq), B, P(off), L.stream()))
        o = host(off)
        assert np.array_equal(o[:B + 1], G.scan_ref(v, ql)), (B, kind, ql is None)
        assert G.untouched(off, rows_written(B + 1, B + 1 + SPARE))


@pytest.mark.parametrize("Lv_pad,Lq_pad", G.COMPACT_PADS)
@pytest.mark.parametrize("B", [b for b in G.SCAN_BS if b <= 1025])
def test_compact_index(B, Lv_pad, Lq_pad):
    lib, P, L = _lib()
    v, q = G.compact_case(B, Lv_pad, Lq_pad)
    voff, toff, vidx, tidx = G.compact_ref(v, q, Lv_pad, Lq_pad)
    ov, ot = P_(len(vidx) + SPARE, dtype=torch.int32), P_(len(tidx) + SPARE, dtype=torch.int32)
    L.check(lib.cone_test_compact_index(P(dv(v)), P(dv(voff)), Lv_pad, P(ov), P(dv(q)), P(dv(toff)), Lq_pad, P(ot), B, L.stream()))
    assert np.array_equal(host(ov)[:len(vidx)], vidx) and np.array_equal(host(ot)[:len(tidx)], tidx)
    # the rows past off[B] are nobody's
    assert G.untouched(ov, rows_written(len(vidx), len(vidx) + SPARE)) and G.untouched(ot, rows_written(len(tidx), len(tidx) + SPARE))


# ------------------------------------------------------------------------------------------------ row index, packing
def _pack_dev(c):
    if not hasattr(c, "_d"):
        c._d = {k: dv(getattr(c, k)) for k in ("vproj", "vrow0", "vlen", "tproj", "trow0", "qlen", "off")}
    return c._d


_CASES = {}


def pack_case(d, **kw):
    key = (d,) + tuple(sorted(kw.items()))
    if key not in _CASES:
        _CASES[key] = G.pack_case(d, **kw)
    return _CASES[key]


def _row_mask(c, rows=None, width=None):
    m = np.zeros((c.M + SPARE, width or c.d), bool)
    m[:c.M] = True if rows is None else rows[:, None]
    return m


def _dim_t(d):
    """The table the model hands the library (cone_amd.model); glue_refs builds its own from the formula."""
    from cone_amd.model import _dim_t_table
    return dv(_dim_t_table(d))


def _tpe_case(c):
    """Text position operands for the packing kernels: an embedding row per token index of the longest query."""
    g = torch.Generator().manual_seed(9 + c.d)
    E = torch.randn(int(c.qlen.max()) + 1, c.d, generator=g) * 0.5
    return E, torch.rand(c.d, generator=g) + 0.5, torch.randn(c.d, generator=g)


def _check_pack(c, X, POS, XP, tpe, what):
    """X: the gather, bit for bit.  POS: sine rows inside the sine bound, text rows +0.0 or LayerNorm(x + E[t]) inside its
    bound.  XP = X + POS: that bound plus the rounding of the one add.  Nothing behind row M.  -> worst sine distance."""
    Xr = G.pack_x_ref(c)
    assert G.same_bits(host(X)[:c.M], Xr), (what, "X is not the gather")
    pos = host(POS)[:c.M]
    ref = G.pack_pos64(c)
    bound = np.full(ref.shape, G.sine_bound())
    txt = ~c.kind
    if tpe is None:
        assert not G.bits(pos[txt]).any(), (what, "a text token's position row is not +0.0")
        bound[txt] = 0.0
    elif txt.any():
        E, g, b = tpe
        x = torch.as_tensor(Xr[txt]).double() + E.double()[torch.as_tensor(c.pos[txt])]
        r, bd, info = R.ln_ref_bound(x, G.U * x.abs(), g, b, own_sum=R.LN_OWN_SUM)
        assert info["first"] <= R.LN_VALID
        ref[txt], bound[txt] = r.numpy(), bd.numpy()
    hold(pos[txt], ref[txt], bound[txt], (what, "POS, text rows"))
    worst, _ = hold(pos[c.kind], ref[c.kind], bound[c.kind], (what, "POS, clip rows"))
    assert G.untouched(X, _row_mask(c)) and G.untouched(POS, _row_mask(c)), (what, "rows behind the batch written")
    if XP is not None:
        s = Xr.astype(np.float64) + ref
        hold(host(XP)[:c.M], s, bound + G.U * np.abs(s), (what, "XP"))
        assert G.untouched(XP, _row_mask(c))
    return worst


def test_row_index():
    lib, P, L = _lib()
    c = pack_case(256)
    d = _pack_dev(c)
    ridx = P_(c.M + SPARE, dtype=torch.int32)
    L.check(lib.cone_test_row_index(P(d["vrow0"]), P(d["vlen"]), P(d["trow0"]), P(d["qlen"]), P(d["off"]), P(ridx), c.B, c.Lmax, L.stream()))
    assert np.array_equal(host(ridx)[:c.M], G.row_index_ref(c.vrow0, c.vlen, c.trow0, c.qlen))
    assert G.untouched(ridx, rows_written(c.M, c.M + SPARE))


@pytest.mark.parametrize("tpe", [False, True])
def test_pack_pos(tpe):
    lib, P, L = _lib()
    c = pack_case(256)
    assert c.Lmax == int((c.vlen + c.qlen).max())            # Lmax is exactly the longest window
    d = _pack_dev(c)
    t = _tpe_case(c) if tpe else None
    td = [dv(x) for x in t] if tpe else [None] * 3
    X, POS, XP = (P_(c.M + SPARE, 256) for _ in range(3))
    L.check(lib.cone_test_pack_pos(P(d["vproj"]), P(d["vrow0"]), P(d["vlen"]), P(d["tproj"]), P(d["trow0"]), P(d["qlen"]), P(d["off"]),
                                   P(_dim_t(256)), P(X), P(POS), P(XP), c.B, c.Lmax, P(td[0]), P(td[1]), P(td[2]), L.stream()))
    worst = _check_pack(c, X, POS, XP, t, ("pack_pos", tpe))
    record_measured("glue_kernels", kernel="pack_pos", lv_max=int(c.vlen.max()), tpe=tpe, worst_sine_err_e9=worst * 1e9, bound_e9=G.sine_bound() * 1e9)


def test_pack_pos_long_windows():
    """The tables stop at 255 clips; longer windows live on this kernel's own sinf / cosf."""
    lib, P, L = _lib()
    c = pack_case(256, windows=tuple((lv, 1 + i) for i, lv in enumerate(G.LONG_LVS)), n_clips=1100)
    d = _pack_dev(c)
    X, POS, XP = (P_(c.M + SPARE, 256) for _ in range(3))
    L.check(lib.cone_test_pack_pos(P(d["vproj"]), P(d["vrow0"]), P(d["vlen"]), P(d["tproj"]), P(d["trow0"]), P(d["qlen"]), P(d["off"]),
                                   P(_dim_t(256)), P(X), P(POS), P(XP), c.B, c.Lmax, None, None, None, L.stream()))
    worst = _check_pack(c, X, POS, XP, None, "pack_pos, long windows")
    record_measured("glue_kernels", kernel="pack_pos", lv_max=1023, tpe=False, worst_sine_err_e9=worst * 1e9, bound_e9=G.sine_bound() * 1e9)


@pytest.mark.parametrize("tpe", [False, True])
@pytest.mark.parametrize("d", [64, 128, 320, 512])
def test_gen_pack_pos(d, tpe):
    lib, P, L = _lib()
    c = pack_case(d)
    dd = _pack_dev(c)
    t = _tpe_case(c) if tpe else None
    td = [dv(x) for x in t] if tpe else [None] * 3
    X, POS = P_(c.M + SPARE, d), P_(c.M + SPARE, d)
    L.check(lib.cone_test_gen_pack_pos(P(dd["vproj"]), P(dd["vrow0"]), P(dd["vlen"]), P(dd["tproj"]), P(dd["trow0"]), P(dd["qlen"]),
                                       P(dd["off"]), P(_dim_t(d)), P(X), P(POS), d, c.B, c.Lmax, P(td[0]), P(td[1]), P(td[2]),
                                       L.stream()))
    worst = _check_pack(c, X, POS, None, t, ("gen_pack_pos", d, tpe))
    record_measured("glue_kernels", kernel="gen_pack_pos", d=d, tpe=tpe, worst_sine_err_e9=worst * 1e9, bound_e9=G.sine_bound() * 1e9)


@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("with_qk", [False, True])
def test_pack_l0(with_qk, with_pos):
    lib, P, L = _lib()
    c = pack_case(256)
    d = _pack_dev(c)
    rng = np.random.default_rng(5)
    n_tab = G.table_row_count(255)
    qkv_vid = rng.standard_normal((c.vproj.shape[0], 768), dtype=np.float32)
    qkv_txt = rng.standard_normal((c.tproj.shape[0], 768), dtype=np.float32)
    pos_qk = rng.standard_normal((n_tab, 512), dtype=np.float32)
    X, POS, QK, V = P_(c.M + SPARE, 256), P_(c.M + SPARE, 256), P_(c.M + SPARE, 512), P_(c.M + SPARE, 256)
    L.check(lib.cone_test_pack_l0(P(d["vproj"]), P(d["vrow0"]), P(d["vlen"]), P(d["tproj"]), P(d["trow0"]), P(d["qlen"]), P(d["off"]),
                                  P(_dim_t(256)), P(dv(qkv_vid)), P(dv(qkv_txt)), P(dv(pos_qk)), P(X), P(POS) if with_pos else None,
                                  P(QK) if with_qk else None, P(V) if with_qk else None, c.B, c.Lmax, L.stream()))
    what = ("pack_l0", with_qk, with_pos)
    assert G.same_bits(host(X)[:c.M], G.pack_x_ref(c)) and G.untouched(X, _row_mask(c)), what
    if with_pos:
        pos = host(POS)[:c.M]
        assert not G.bits(pos[~c.kind]).any(), (what, "a text token's position row is not +0.0")
        hold(pos[c.kind], G.pack_pos64(c)[c.kind], G.sine_bound(), (what, "POS"))
        assert G.untouched(POS, _row_mask(c))
    else:
        assert G.untouched(POS), (what, "POS written though NULL was passed")
    if with_qk:
        k, t = c.kind, ~c.kind
        qk = np.empty((c.M, 512), np.float32)
        # one fp32 add per element (IEEE: the same bits in numpy); a text token's row is its cache row unchanged
        qk[k] = qkv_vid[c.src[k], :512] + pos_qk[c.lv[k] * (c.lv[k] - 1) // 2 + c.pos[k]]
        qk[t] = qkv_txt[c.src[t], :512]
        v = np.where(k[:, None], qkv_vid[np.minimum(c.src, len(qkv_vid) - 1), 512:], qkv_txt[np.minimum(c.src, len(qkv_txt) - 1), 512:])
        assert G.same_bits(host(QK)[:c.M], qk), (what, "QK")
        assert G.same_bits(host(V)[:c.M], v), (what, "V")
        assert G.untouched(QK, _row_mask(c, width=512)) and G.untouched(V, _row_mask(c))
    else:
        assert G.untouched(QK) and G.untouched(V), (what, "QK / V written though NULL was passed")


@pytest.mark.parametrize("with_txt", [False, True])
def test_add_pos_rows(with_txt):
    lib, P, L = _lib()
    c = pack_case(256)
    d = _pack_dev(c)
    rng = np.random.default_rng(6)
    MEM = rng.standard_normal((c.M, 256), dtype=np.float32)
    tab = rng.standard_normal((G.table_row_count(255), 256), dtype=np.float32)
    tp = rng.standard_normal((c.tproj.shape[0], 256), dtype=np.float32)
    XP = P_(c.M + SPARE, 256)
    L.check(lib.cone_test_add_pos_rows(P(dv(MEM)), P(d["off"]), P(d["vlen"]), P(dv(tab)), P(XP), c.B, c.Lmax,
                                       P(dv(tp)) if with_txt else None, P(d["trow0"]) if with_txt else None, L.stream()))
    k, t = c.kind, ~c.kind
    ref = MEM.copy()
    ref[k] = MEM[k] + tab[c.lv[k] * (c.lv[k] - 1) // 2 + c.pos[k]]          # one fp32 add: the same bits
    if with_txt:
        ref[t] = MEM[t] + tp[c.src[t]]
    assert G.same_bits(host(XP)[:c.M], ref) and G.untouched(XP, _row_mask(c))


# ------------------------------------------------------------------------------------------------ position tables
def _pos_tables(model, max_v_l, d, n_enc):
    lib, P, L = _lib()
    rows = G.table_row_count(max_v_l)
    assert lib.cone_pos_table_rows(max_v_l) == rows
    pr, pq = P_(rows + SPARE, d), P_(n_enc * rows + SPARE, 2 * d)
    rc = lib.cone_pos_tables(model._h(), max_v_l, P(pr), P(pq), L.stream())
    return rc, rows, pr, pq


@pytest.mark.parametrize("d,max_v_l", [(256, 255), (128, 64), (512, 64)])
def test_pos_tables(d, max_v_l):
    model, opt, sd = get_model(d)
    n_enc = opt.enc_layers
    rc, rows, pr, pq = _pos_tables(model, max_v_l, d, n_enc)
    assert rc == 0
    got = host(pr)
    ref = G.table_rows64(max_v_l, d)
    kernel = "pos_rows" if d == 256 else "gen_pos_rows"
    worst, _ = hold(got[:rows - 1], ref[:-1], G.sine_bound(), (kernel, d, max_v_l))       # every row
    record_measured("glue_kernels", kernel=kernel, d=d, max_v_l=max_v_l, worst_sine_err_e9=worst * 1e9, bound_e9=G.sine_bound() * 1e9)
    assert not G.bits(got[rows - 1]).any(), "the zero row of pos_rows is not +0.0"
    assert G.untouched(pr, rows_written(rows, rows + SPARE)[:, None])
    qk = host(pq)[:n_enc * rows].reshape(n_enc, rows, 2 * d)
    assert G.untouched(pq, rows_written(n_enc * rows, n_enc * rows + SPARE)[:, None])
    a = torch.as_tensor(ref)
    for l in range(n_enc):
        W = torch.as_tensor(sd[f"transformer.encoder.layers.{l}.self_attn.in_proj_weight"][:2 * d]).double()
        want = torch.as_tensor(G.pos_qk64(ref, [sd[f"transformer.encoder.layers.{l}.self_attn.in_proj_weight"]])[0])
        # the fp32 sum bound of the row-kernel suite; the GEMM's input rows are the device's own sine rows: within
        # sine_bound of the reference's (da)
        bound = R.gemm_delta(a, W, torch.zeros_like(want), "f32", da=torch.full_like(a, G.sine_bound()))
        assert not (qk[l, rows - 1] != 0).any(), (l, "the zero row of pos_qk is not zero")
        hold(qk[l], want.numpy(), bound.numpy(), ("pos_qk", d, l))


def test_pos_tables_prefix_and_refusals():
    lib, P, L = _lib()
    model, opt, _ = get_model(256)
    n_enc = opt.enc_layers
    rc, rows, pr, pq = _pos_tables(model, 255, 256, n_enc)
    assert rc == 0
    rc, rows90, pr90, pq90 = _pos_tables(model, 90, 256, n_enc)
    assert rc == 0
    # row lv (lv - 1) / 2 + p is the same row whatever the bound
    assert G.same_bits(host(pr90)[:rows90 - 1], host(pr)[:rows90 - 1])
    big, small = host(pq)[:n_enc * rows].reshape(n_enc, rows, 512), host(pq90)[:n_enc * rows90].reshape(n_enc, rows90, 512)
    assert G.same_bits(small[:, :rows90 - 1], big[:, :rows90 - 1])
    for bad in (0, 256):
        a, b = P_(8, 256), P_(8, 512)
        assert lib.cone_pos_tables(model._h(), bad, P(a), P(b), L.stream()) != 0
        assert b"pos_tables" in lib.cone_last_error()
        torch.cuda.synchronize()
        assert G.untouched(a) and G.untouched(b)


# ------------------------------------------------------------------------------------------------ text positions
def _txt_launch(c, d, tok, src, mod, n_dev, ops=None, n_emb=None):
    lib, P, L = _lib()
    E, g, b = ops if ops is not None else (dv(c.E), dv(c.g), dv(c.b))
    out = P_(c.n + SPARE, d)
    nd = None if n_dev is None else dv(np.asarray([n_dev]))
    x = dv(c.x)
    n_emb = n_emb or c.n_emb
    if d == 256:
        L.check(lib.cone_test_txt_pos_rows(P(x), P(tok), P(src), mod, n_emb, P(E), P(g), P(b), c.n, P(nd), P(out), L.stream()))
    else:
        L.check(lib.cone_test_gen_txt_pos_rows(P(x), P(tok), P(src), mod, n_emb, P(E), P(g), P(b), c.n, P(nd), d, P(out), L.stream()))
    return out


@pytest.mark.parametrize("n", G.TXT_NS)
@pytest.mark.parametrize("d", [256, 128, 512])
def test_txt_pos_rows(d, n):
    c = G.txt_case(d, n)
    forms = [("tok", c.tok, None, 1, nd) for nd in (None, 0, n - 1, n, n + 5)]
    forms += [("mod", None, c.src_row, mod, None) for mod in G.TXT_MODS]
    for name, tok, src, mod, n_dev in forms:
        cnt, j = G.txt_index(tok, src, mod, c.n_emb, n, n_dev)
        out = _txt_launch(c, d, None if tok is None else dv(tok), None if src is None else dv(src), mod, n_dev)
        what = (d, n, name, mod, n_dev)
        assert G.untouched(out, rows_written(cnt, n + SPARE)[:, None]), (what, "rows past the device count written")
        if cnt:
            ref, bound, info = G.txt_ref_bound(c, j)
            assert info["first"] <= R.LN_VALID, info
            hold(host(out)[:cnt], ref.numpy(), bound.numpy(), what)


@pytest.mark.parametrize("d", [256, 128, 512])
def test_layer0_text_positions_same_bits(d):
    """The public entry on the model's own embedding table: the same launch, the same bits."""
    lib, P, L = _lib()
    model, opt, sd = get_model(d)
    n = 257
    c = G.txt_case(d, n)
    pre = "txt_position_embed."
    E = model._sd[pre + "position_embeddings.weight"]
    g, b = model._sd[pre + "LayerNorm.weight"], model._sd[pre + "LayerNorm.bias"]
    n_emb = int(E.shape[0])
    tok = dv(c.tok)
    via_hook = _txt_launch(c, d, tok, None, 1, None, ops=(E, g, b), n_emb=n_emb)
    out, qk = P_(n + SPARE, d), torch.empty(opt.enc_layers * n, 2 * d, device=_gpu())
    L.check(lib.cone_layer0_text_positions(model._h(), P(dv(c.x)), P(tok), n, P(out), P(qk), L.stream()))
    assert G.same_bits(host(out), host(via_hook))
    _, j = G.txt_index(c.tok, None, 1, n_emb, n)
    ref = G.txt_pos64(c.x.numpy(), sd[pre + "position_embeddings.weight"], j, sd[pre + "LayerNorm.weight"], sd[pre + "LayerNorm.bias"])
    assert float(np.abs(host(out)[:n] - ref).max()) < 1e-4        # (the elementwise bound is held in test_txt_pos_rows)


# ------------------------------------------------------------------------------------------------ saliency, memory tap
@pytest.mark.parametrize("dLv,dLq", [(0, 0), (3, 2), (0, 2), (3, 0)])
@pytest.mark.parametrize("d", [256, 128, 512])
def test_saliency_and_memory_tap(d, dLv, dLq):
    lib, P, L = _lib()
    c = G.sal_case(d)
    assert (c.vlen == 0).any() and (c.qlen == 0).any()
    Lv, Lq = c.lv_max + dLv, c.lq_max + dLq
    ops = [dv(x) for x in (c.MEM, c.off, c.vlen, c.qlen, c.w, c.bias)]
    ref = G.saliency64(c.MEM, c.off, c.vlen, c.w, c.bias, Lv)
    valid = np.arange(Lv)[None, :] < c.vlen[:, None]
    bound = np.zeros(ref.shape)
    for b_ in range(c.B):
        lv = int(c.vlen[b_])
        bound[b_, :lv] = G.dot_bound(c.MEM[c.off[b_]:c.off[b_] + lv], c.w, c.bias)[:, 0]
    tap_ref = G.mem_tap_ref(c.MEM, c.off, c.vlen, c.qlen, Lv, Lq)
    for with_sal, with_tap in itertools.product((True, False), repeat=2):
        sal, tap = P_(c.B + SPARE, Lv), P_(c.B + SPARE, Lv + Lq, d)
        args = [P(o) for o in ops] + [P(sal) if with_sal else None, Lv, P(tap) if with_tap else None, Lq, c.B]
        if d == 256:
            L.check(lib.cone_test_saliency(*args, L.stream()))
        else:
            L.check(lib.cone_test_gen_saliency(*args, d, L.stream()))
        what = (d, Lv, Lq, with_sal, with_tap)
        if with_sal:
            s = host(sal)[:c.B]
            hold(s[valid], ref[valid], bound[valid], what)
            assert not G.bits(s[~valid]).any(), (what, "padding entries are not +0.0")
            assert G.untouched(sal, rows_written(c.B, c.B + SPARE)[:, None])
        else:
            assert G.untouched(sal), what
        if with_tap:
            # bit copies of the valid clip and token rows, +0.0 rows in the padding of both halves
            assert G.same_bits(host(tap)[:c.B], tap_ref), what
            assert G.untouched(tap, rows_written(c.B, c.B + SPARE)[:, None, None])
        else:
            assert G.untouched(tap), what


# ------------------------------------------------------------------------------------------------ heads
@pytest.mark.parametrize("n_rows", G.HEAD_ROWS)
@pytest.mark.parametrize("d", [256, 128, 512])
def test_heads(d, n_rows):
    lib, P, L = _lib()
    for nout, act in itertools.product((1, 2), (0, 1)):
        c = G.head_case(d, n_rows, nout)
        ldo = nout + 1
        out = P_(n_rows + SPARE, ldo)
        args = [P(dv(c.xbuf)), c.ldx, P(dv(c.W)), P(dv(c.b)), P(out), ldo, n_rows, nout, act]
        if d == 256:
            L.check(lib.cone_test_rowdot(*args, L.stream()))
        else:
            L.check(lib.cone_test_gen_rowdot(*args, d, L.stream()))
        what = (d, n_rows, nout, act)
        written = np.zeros((n_rows + SPARE, ldo), bool)
        written[:n_rows, :nout] = True
        assert G.untouched(out, written), (what, "the gap columns or the spare rows were written")
        o = host(out)[:n_rows, :nout]
        ref, _ = G.rowdot64(c.x, c.W, c.b, act)
        hold(o, ref, G.rowdot_bound(c.x, c.W, c.b, act), what)      # (finite first: no NaN at the saturating logits)
        if act == 1:
            for r, t in c.sat:
                if abs(t) == 90.0:
                    assert o[r, 0] == (1.0 if t > 0 else 0.0), (what, r, t, float(o[r, 0]))
                if t == 30.0:
                    assert o[r, 0] == 1.0, (what, r, t)


# ------------------------------------------------------------------------------------------------ tilers
@pytest.mark.parametrize("period", G.TILE_PERIODS)
def test_tile_rows(period):
    lib, P, L = _lib()
    rng = np.random.default_rng(period)
    for n_rows in G.tile_rows_of(period):
        src = rng.standard_normal((period, 256), dtype=np.float32)
        x = P_(n_rows + SPARE, 256)
        x[:period] = dv(src)
        L.check(lib.cone_test_tile_rows(P(x), period, n_rows, L.stream()))
        assert G.same_bits(host(x)[:n_rows], G.tile_ref(src, n_rows)), (period, n_rows)      # (rows < period: the source, unchanged)
        assert G.untouched(x, rows_written(n_rows, n_rows + SPARE)[:, None])                 # (n_rows == period: nothing is written)
        src1 = rng.standard_normal((period, 256), dtype=np.float32)
        s0, s1 = dv(src), dv(src1)
        d0, d1 = P_(n_rows + SPARE, 256), P_(n_rows + SPARE, 256)
        L.check(lib.cone_test_tile_rows2(P(d0), P(s0), P(d1), P(s1), period, n_rows, L.stream()))
        assert G.same_bits(host(d0)[:n_rows], G.tile_ref(src, n_rows)) and G.same_bits(host(d1)[:n_rows], G.tile_ref(src1, n_rows))
        assert G.untouched(d0, rows_written(n_rows, n_rows + SPARE)[:, None]) and G.untouched(d1, rows_written(n_rows, n_rows + SPARE)[:, None])
        assert G.same_bits(host(s0), src) and G.same_bits(host(s1), src1)
    # fewer rows than the period: tile_rows launches nothing
    x = P_(period + SPARE, 256)
    L.check(lib.cone_test_tile_rows(P(x), period + 1, period, L.stream()))
    torch.cuda.synchronize()
    assert G.untouched(x)


# ------------------------------------------------------------------------------------------------ mask lengths
@pytest.mark.parametrize("Lm", G.MASK_LS)
def test_mask_lengths(Lm):
    lib, P, L = _lib()
    for B, kind in itertools.product(G.MASK_BS, ("ones", "zeros", "prefix")):
        m = G.mask_case(B, Lm, kind)
        out = P_(B + SPARE, dtype=torch.int32)
        L.check(lib.cone_mask_lengths(P(dv(m)), B, Lm, P(out), L.stream()))
        assert np.array_equal(host(out)[:B], G.mask_lengths_ref(m)), (B, Lm, kind)
        assert G.untouched(out, rows_written(B, B + SPARE))


# ------------------------------------------------------------------------------------------------ window table
WT_COLS = ("vid_row0", "vid_len", "video_start", "pad_len", "txt_row0", "txt_len", "cls_row")


def _window_table(c, q_base, nb, batch_pad, derive, n_rows=None, row_q="case", row_slot="case", n_batches=None):
    lib, P, L = _lib()
    n_rows = c.n_rows if n_rows is None else n_rows
    outs = [P_(c.n_rows + SPARE, dtype=torch.int32) for _ in WT_COLS]
    rq = (None if c.row_q is None else dv(c.row_q)) if isinstance(row_q, str) else row_q
    rs = (None if c.row_slot is None else dv(c.row_slot)) if isinstance(row_slot, str) else row_slot
    rc = lib.cone_window_table(P(dv(c.win_idx)), c.nq, c.K, P(rq), P(rs), n_rows, P(dv(c.q_ctx_l)), P(dv(c.q_vid_off)), P(dv(c.tok_off)),
                               P(dv(c.tok_len)), q_base, c.eval_bsz, c.W, P(batch_pad), derive, nb if n_batches is None else n_batches,
                               *(P(o) for o in outs), L.stream())
    torch.cuda.synchronize()
    return rc, dict(zip(WT_COLS, outs))


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("eval_bsz,K", G.WT_BATCHING)
@pytest.mark.parametrize("W", G.WT_WS)
def test_window_table(W, eval_bsz, K, sparse):
    c = G.wt_case(W, eval_bsz, K, sparse=sparse)
    for q_base in G.wt_q_bases(eval_bsz):
        nb, kw = G.wt_view(c, q_base)
        ref = G.window_table_ref(**kw)
        # the padding derived from the windows themselves
        pad = P_(nb + SPARE, dtype=torch.int32)
        rc, got = _window_table(c, q_base, nb, pad, 1)
        assert rc == 0
        what = (W, eval_bsz, K, sparse, q_base)
        assert np.array_equal(host(pad)[:nb], ref["batch_pad"]), (what, "batch_pad")
        assert G.untouched(pad, rows_written(nb, nb + SPARE))
        for k in WT_COLS:
            assert np.array_equal(host(got[k])[:c.n_rows], ref[k]), (what, k)
            assert G.untouched(got[k], rows_written(c.n_rows, c.n_rows + SPARE)), (what, k)
        # the split's table handed in (a table no view could derive: it has to be READ, and left as it is)
        given = ref["batch_pad"] + 3
        ref2 = G.window_table_ref(**kw, batch_pad=given)
        pad = dv(given)
        rc, got = _window_table(c, q_base, nb, pad, 0)
        assert rc == 0 and np.array_equal(host(pad), given), (what, "a given batch_pad was changed")
        for k in WT_COLS:
            assert np.array_equal(host(got[k])[:c.n_rows], ref2[k]), (what, k, "given table")
            assert G.untouched(got[k], rows_written(c.n_rows, c.n_rows + SPARE)), (what, k)


def test_window_table_refusals():
    lib, _, _ = _lib()
    c = G.wt_case(90, 4, 4, sparse=True)
    nb, _ = G.wt_view(c, 0)

    def refused(needle, **kw):
        pad = P_(nb + SPARE, dtype=torch.int32)
        rc, got = _window_table(c, 0, nb, pad, 1, **kw)
        assert rc != 0 and needle in lib.cone_last_error(), (needle, lib.cone_last_error())
        assert G.untouched(pad) and all(G.untouched(o) for o in got.values()), needle

    refused(b"batch_pad holds", n_batches=nb - 1)
    refused(b"come together", row_slot=None)
    refused(b"come together", row_q=None)
    refused(b"does not fit", n_rows=c.nq * c.K + 1)
    refused(b"does not fit", n_rows=c.nq * c.K - 1, row_q=None, row_slot=None)      # the dense list has exactly nq K rows


# ------------------------------------------------------------------------------------------------ the grid limit
def test_forward_refuses_more_windows_than_the_grid_holds():
    """The per-window kernels put the window index in gridDim.y: one window more than the device's maxGridSize[1] is refused by
    name before anything is launched or written (every operand is allocated in full all the same)."""
    lib, P, L = _lib()
    model, opt, _ = get_model(256)
    limit = lib.cone_test_grid_limit_y()
    assert limit >= 65535, limit
    if limit + 1 >= 2 ** 23:          # B * L < 2^24 tokens refuses such a batch first: the grid limit is out of reach
        pytest.fail(f"maxGridSize[1] = {limit}: the grid refusal cannot be reached, review the contract in include/cone_hip.h")
    B, nq = limit + 1, opt.num_queries
    h = model._h()
    ones, zeros = torch.ones(B, dtype=torch.int32, device=_gpu()), torch.zeros(B, dtype=torch.int32, device=_gpu())
    row = torch.zeros(4, 256, device=_gpu())

    def outputs():
        return P_(B, nq, 2), P_(B, nq, 2), P_(B, 1)

    # the arena entry: every window is clip row 0 + token row 0
    nbytes = lib.cone_forward_packed_workspace(h, B, 1, 1, None)
    assert nbytes < 2 ** 34, nbytes
    ws = torch.empty(nbytes, dtype=torch.uint8, device=_gpu())
    lo, sp, sa = outputs()
    rc = lib.cone_forward_packed(h, P(row), P(zeros), P(ones), P(row), P(zeros), P(ones), B, 1, 1, P(lo), P(sp), P(sa), None, None,
                                 P(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"grid limit" in lib.cone_last_error() and str(limit).encode() in lib.cone_last_error(), lib.cone_last_error()
    assert G.untouched(lo) and G.untouched(sp) and G.untouched(sa)
    del ws
    # the padded entry
    a = model.args
    vid, txt = torch.zeros(B, 1, a.v_motion_feat_dim, device=_gpu()), torch.zeros(B, 1, a.t_feat_dim, device=_gpu())
    nbytes = lib.cone_forward_workspace(h, B, 1, 1)
    assert nbytes < 2 ** 34, nbytes
    ws = torch.empty(nbytes, dtype=torch.uint8, device=_gpu())
    lo, sp, sa = outputs()
    rc = lib.cone_forward_windows(h, P(vid), P(ones), P(txt), P(ones), B, 1, 1, P(lo), P(sp), P(sa), None, P(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"grid limit" in lib.cone_last_error(), lib.cone_last_error()
    assert G.untouched(lo) and G.untouched(sp) and G.untouched(sa)
