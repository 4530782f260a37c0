"""The packed fp32 weight streams (cone_amd/csrc/tail_pack.hip) and the two weight-ring kernels on them: the persistent row kernel
of the exact-fp32 layer tail (ffn.hip) and the tall row GEMM (gemm_tall.hip).

1. The pack kernel against a numpy model of the layout, written here from the layout's formula and compared bit for bit:
       image[chunk g][slab s][lane l][4 floats],  row = l / 4,  ch = (l % 4) ^ swz(row),  swz(row) = (0x1230 >> 4 ((row / 4) % 4)) & 3
       projection format, chunk c of W (N, 256):  slab s      = W[32 c + 16 (s / 16) + row][16 (s % 16) + 4 ch ..]
       feed-forward format, chunk c:              slab s < 16 = W1[16 c + row][16 s + 4 ch ..]
                                                  slab 16 + t = W2[16 t + row][16 c + 4 ch ..]
   The image sits between two poisoned guards, which must survive.
2. Both kernels streaming the image against the same kernels streaming the row-major matrices: ``torch.equal`` (the LDS
   contents are the same bytes, so not a bit may differ), the row-major result held against the float64 bounds of
   tests/row_refs.py, and rows past M poisoned and checked.
3. A model whose weights are reloaded runs on the images of the NEW weights.

Weights are N(0, 1) draws plus a counter pattern (every element its own value): a slab in another slab's place cannot cancel."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import inputs as gi
import row_refs as RR
from cone_amd import _lib, synth
from cone_amd.config import make_opt

pytestmark = pytest.mark.gpu

GUARD = 32                      # poisoned rows past M
PAD = 4096                      # poisoned bytes on either side of an image
FF_ODD = 144                    # 9 feed-forward chunks: 17 chunks per projecting tile, the ring's stage phase moves from tile to tile
FF_MIN = 32                     # the smallest ff the row kernel accepts (ffn_fused_supported): 2 feed-forward chunks
RELU, RES = 1, 2


def _gpu():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda", 0)


def _distinct(t, step):
    """+ a counter pattern: element i gets i * step on top of its draw."""
    return (t + torch.arange(t.numel(), dtype=torch.float32).reshape(t.shape) * step).contiguous()


# ------------------------------------------------------------------------------------------------ the layout, in numpy
_L = np.arange(64)
_ROW = _L >> 2
_CH = (_L & 3) ^ ((0x1230 >> (((_ROW >> 2) & 3) * 4)) & 3)
_Q = np.arange(4)


def _model_proj(W):
    """(N, 256) -> (N / 32, 32, 64, 4)"""
    N = W.shape[0]
    img = np.empty((N // 32, 32, 64, 4), np.float32)
    for c in range(N // 32):
        for s in range(32):
            rows = 32 * c + 16 * (s // 16) + _ROW
            cols = 16 * (s % 16) + 4 * _CH
            img[c, s] = W[rows[:, None], cols[:, None] + _Q[None, :]]
    return img


def _model_ffn(W1, W2):
    """(ff, 256), (256, ff) -> (ff / 16, 32, 64, 4)"""
    ff = W1.shape[0]
    img = np.empty((ff // 16, 32, 64, 4), np.float32)
    for c in range(ff // 16):
        for s in range(16):
            img[c, s] = W1[(16 * c + _ROW)[:, None], (16 * s + 4 * _CH)[:, None] + _Q[None, :]]
            img[c, 16 + s] = W2[(16 * s + _ROW)[:, None], (16 * c + 4 * _CH)[:, None] + _Q[None, :]]
    return img


def _model_tail(Wo, W1, W2, Wq):
    parts = ([_model_proj(Wo)] if Wo is not None else []) + [_model_ffn(W1, W2)] + ([_model_proj(Wq)] if Wq is not None else [])
    return np.concatenate(parts, 0)


@functools.lru_cache(maxsize=None)
def _weights(ff, n_qkv=768):
    """One draw per ff, shared by every test and never modified (CPU tensors)."""
    g = torch.Generator().manual_seed(104729 * ff + n_qkv)
    mk = lambda *s: torch.randn(*s, generator=g)
    return SimpleNamespace(Wo=_distinct(mk(256, 256) / 16, 2.0 ** -20), W1=_distinct(mk(ff, 256) / 16, 2.0 ** -22),
                           W2=_distinct(mk(256, ff) / ff ** 0.5, 2.0 ** -22), Wq=_distinct(mk(n_qkv, 256) / 16, 2.0 ** -21))


def _guarded(nbytes):
    """A device buffer of PAD + nbytes + PAD bytes, every byte 0xA5 -> (whole buffer as uint8, the image's slice)."""
    buf = torch.full((nbytes + 2 * PAD,), 0xA5, dtype=torch.uint8, device=_gpu())
    return buf, buf[PAD:PAD + nbytes]


def _check_image(buf, img, model):
    torch.cuda.synchronize()
    got = img.cpu().numpy().view(np.int32)
    want = np.ascontiguousarray(model).view(np.int32).reshape(-1)
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} words differ, first at {int(np.argmax(got != want))}"
    assert bool((buf[:PAD] == 0xA5).all()) and bool((buf[-PAD:] == 0xA5).all()), "the pack kernel wrote outside its image"


@pytest.mark.parametrize("ff", [1024, FF_MIN])
@pytest.mark.parametrize("proj", [False, True])
@pytest.mark.parametrize("ride", [False, True])
def test_pack_tail(ff, proj, ride):
    lib, P, dev = _lib.load(), _lib.ptr, _gpu()
    w = _weights(ff)
    nbytes = lib.cone_test_f32_pack_tail_bytes(ff, int(proj), 768 if ride else 0)
    assert nbytes == ((8 if proj else 0) + ff // 16 + (24 if ride else 0)) * 32768
    buf, img = _guarded(nbytes)
    Wo, W1, W2, Wq = (t.to(dev) for t in (w.Wo, w.W1, w.W2, w.Wq))
    _lib.check(lib.cone_test_f32_pack_tail(P(Wo) if proj else None, P(W1), P(W2), ff, P(Wq) if ride else None, 768, P(img),
                                           _lib.stream()))
    _check_image(buf, img, _model_tail(w.Wo.numpy() if proj else None, w.W1.numpy(), w.W2.numpy(), w.Wq.numpy() if ride else None))


@pytest.mark.parametrize("N", [768, 32])
def test_pack_rows(N):
    lib, P, dev = _lib.load(), _lib.ptr, _gpu()
    W = _weights(1024).Wq[:N].contiguous()
    nbytes = lib.cone_test_f32_pack_rows_bytes(N)
    assert nbytes == N // 32 * 32768
    buf, img = _guarded(nbytes)
    Wd = W.to(dev)
    _lib.check(lib.cone_test_f32_pack_rows(P(Wd), N, P(img), _lib.stream()))
    _check_image(buf, img, _model_proj(W.numpy()))


def test_pack_refusals():
    lib = _lib.load()
    assert lib.cone_test_f32_pack_tail_bytes(24, 1, 0) == 0 and lib.cone_test_f32_pack_tail_bytes(128, 1, 40) == 0
    assert lib.cone_test_f32_pack_rows_bytes(48) == 0 and lib.cone_test_f32_pack_rows_bytes(0) == 0


# ------------------------------------------------------------------------------------------------ the layer tail
@functools.lru_cache(maxsize=None)
def _tail_case(ff, n_qkv=768):
    """row_refs' benign tail operands at 1024 rows with this module's weights; CPU, shared, never modified."""
    c = RR.tail_case("benign", 1024, ff)
    w = _weights(ff, n_qkv)
    c = SimpleNamespace(**vars(c))
    c.Wo, c.W1, c.W2, c.Wq = w.Wo, w.W1, w.W2, w.Wq
    g = torch.Generator().manual_seed(31 * ff + n_qkv)
    c.qb = torch.randn(n_qkv, generator=g)
    return c


@functools.lru_cache(maxsize=None)
def _tail_dev(ff, n_qkv=768):
    c, dev = _tail_case(ff, n_qkv), _gpu()
    return {k: v.to(dev) for k, v in vars(c).items() if torch.is_tensor(v)}


@functools.lru_cache(maxsize=None)
def _tail_image(ff, proj, n_qkv):
    lib, P = _lib.load(), _lib.ptr
    d = _tail_dev(ff, n_qkv or 768)
    buf, img = _guarded(lib.cone_test_f32_pack_tail_bytes(ff, int(proj), n_qkv))
    _lib.check(lib.cone_test_f32_pack_tail(P(d["Wo"]) if proj else None, P(d["W1"]), P(d["W2"]), ff, P(d["Wq"]) if n_qkv else None,
                                           n_qkv, P(img), _lib.stream()))
    torch.cuda.synchronize()
    return buf, img


def _tail(M, ff, packed, proj=True, pre=False, out2=True, n_qkv=0, nw=8, n_cu=2):
    """cone_test_tail_packed -> (OUT, OUT2 | None, QKV | None): M + GUARD rows each, NaN before the call."""
    lib, P, dev = _lib.load(), _lib.ptr, _gpu()
    d = _tail_dev(ff, n_qkv or 768)
    nan = lambda n: torch.full((M + GUARD, n), float("nan"), device=dev)
    OUT, OUT2, QKV = nan(256), nan(256) if pre and out2 else None, nan(n_qkv) if n_qkv else None
    img = _tail_image(ff, proj, n_qkv)[1] if packed else None
    A, R = d["A"][:M].contiguous(), d["R"][:M].contiguous()
    _lib.check(lib.cone_test_tail_packed(P(A) if proj else None, P(d["Wo"]), P(d["bo"]), P(R), P(d["pg"]), P(d["pb"]), P(d["W1"]),
                                         P(d["b1"]), P(d["W2"]), P(d["b2"]), P(d["lg"]), P(d["lb"]), P(OUT), M, ff, int(pre), P(OUT2),
                                         P(d["Wq"]) if n_qkv else None, P(d["qb"]) if n_qkv else None, P(QKV), n_qkv, nw, n_cu,
                                         P(img), _lib.stream()))
    torch.cuda.synchronize()
    return OUT, OUT2, QKV


def _check_tail(M, ff, bound=False, **kw):
    """Packed == row-major, bit for bit, rows past M untouched in both; bound: the row-major result inside row_refs' bound."""
    old, new = _tail(M, ff, False, **kw), _tail(M, ff, True, **kw)
    for name, a, b in zip(("OUT", "OUT2", "QKV"), old, new):
        assert (a is None) == (b is None)
        if a is None:
            continue
        assert not bool(torch.isnan(a[:M]).any()), (name, M, ff, kw)
        assert torch.equal(a[:M], b[:M]), (name, M, ff, kw)
        assert bool(torch.isnan(a[M:]).all()) and bool(torch.isnan(b[M:]).all()), f"{name}: a store reached a row past M"
    if bound:
        c = SimpleNamespace(**vars(_tail_case(ff, kw.get("n_qkv") or 768)))
        c.A, c.R, c.M = c.A[:M], c.R[:M], M
        rb = RR.tail_ref_bound(c, proj=kw.get("proj", True), pre=kw.get("pre", False))
        for name, out in (("OUT", new[0]), ("OUT2", new[1])):
            if out is None or rb[name] is None:
                continue
            worst = RR.worst_ratio(out[:M].cpu(), *rb[name])
            print(f"[tail_packed] M={M} ff={ff} {kw} {name}: worst |err| / bound = {worst:.4f}")
            assert worst <= 1.0, (name, worst)


@pytest.mark.parametrize("M", [1, 15, 16, 17, 127, 128, 129])
def test_tail_rows(M):
    """One wave active, an idle upper half, a partial last group, a second tile."""
    _check_tail(M, FF_ODD, bound=M == 129)


def test_tail_half_tile_round():
    """Grid of 4: 4 full tiles + 100 rows = a last round in half-tile mode (one tile <= half the grid); + 3 tiles: not."""
    _check_tail(4 * 128 + 100, FF_ODD, n_cu=4)
    _check_tail(4 * 128 + 3 * 128 - 5, FF_ODD, n_cu=4)


@pytest.mark.parametrize("ff", [FF_MIN, FF_ODD, 1024])
def test_tail_walks_three_tiles(ff):
    """Grid of 2, 2 * 128 * 2 + 129 rows: every workgroup walks three tiles, the ring runs on across the boundaries and the
    chunk offset wraps twice (ff = 144: 17 chunks per tile, so the stage phase differs in every tile)."""
    _check_tail(2 * 128 * 2 + 129, ff, bound=ff == FF_ODD)


@pytest.mark.parametrize("M", [1, 17, 63, 64, 65, 3 * 64 + 9, 6 * 64 + 1])
def test_tail_nw4(M):
    """The 64-row form (8 pieces per wave per chunk) through its row range; the last two walk two / four tiles per workgroup."""
    _check_tail(M, FF_ODD, nw=4, bound=M == 65)


@pytest.mark.parametrize("out2", [False, True])
def test_tail_prenorm(out2):
    _check_tail(129, FF_ODD, pre=True, out2=out2, bound=True)
    _check_tail(2 * 128 * 2 + 129, FF_ODD, pre=True, out2=out2)


@pytest.mark.parametrize("n_qkv", [96, 768])
def test_tail_ride(n_qkv):
    """The q | k | v ride: its chunks trail the feed-forward ones in the image (96: 3 chunks, 20 per tile)."""
    _check_tail(129, FF_ODD, n_qkv=n_qkv)
    _check_tail(2 * 128 * 2 + 129, FF_ODD, n_qkv=n_qkv)
    d = _tail_dev(FF_ODD, n_qkv)
    OUT, _, QKV = _tail(129, FF_ODD, True, n_qkv=n_qkv)
    ref = OUT[:129].double() @ d["Wq"].double().t() + d["qb"].double()
    bnd = (256 + 6) * RR.U * (OUT[:129].double().abs() @ d["Wq"].double().abs().t() + d["qb"].double().abs())
    assert RR.worst_ratio(QKV[:129].cpu(), ref.cpu(), bnd.cpu()) <= 1.0


@pytest.mark.parametrize("nw", [8, 4])
def test_tail_block_alone(nw):
    """Without the projection: an image without Wo chunks."""
    _check_tail(129, FF_ODD, proj=False, nw=nw, bound=True)
    _check_tail(2 * 128 * 2 + 129, FF_ODD, proj=False, nw=nw)
    _check_tail(300, FF_MIN, proj=False, nw=nw)


# ------------------------------------------------------------------------------------------------ the tall row GEMM
@functools.lru_cache(maxsize=None)
def _gemm_case(N):
    c = RR.gemm_case("benign", 1024, N, 256)
    c = SimpleNamespace(**vars(c))
    c.W = _distinct(c.W, 2.0 ** -21)
    return c


@functools.lru_cache(maxsize=None)
def _gemm_dev(N):
    lib, P, dev = _lib.load(), _lib.ptr, _gpu()
    d = {k: v.to(dev) for k, v in vars(_gemm_case(N)).items() if torch.is_tensor(v)}
    d["buf"], d["img"] = _guarded(lib.cone_test_f32_pack_rows_bytes(N))
    _lib.check(lib.cone_test_f32_pack_rows(P(d["W"]), N, P(d["img"]), _lib.stream()))
    torch.cuda.synchronize()
    return d


def _tall(M, N, flags, with_bias, packed, n_cu=2, M_dev=None):
    lib, P, dev = _lib.load(), _lib.ptr, _gpu()
    d = _gemm_dev(N)
    C = torch.full((M + GUARD, N), float("nan"), device=dev)
    md = torch.tensor([M_dev], dtype=torch.int32, device=dev) if M_dev is not None else None
    _lib.check(lib.cone_test_gemm_tall_packed(P(d["A"][:M].contiguous()), P(d["W"]), P(d["bias"]) if with_bias else None,
                                              P(d["R"][:M].contiguous()) if flags & RES else None, P(C), M, N, flags, P(md), n_cu,
                                              P(d["img"]) if packed else None, _lib.stream()))
    torch.cuda.synchronize()
    return C


def _check_tall(M, N, flags=0, with_bias=True, bound=False, **kw):
    old, new = _tall(M, N, flags, with_bias, False, **kw), _tall(M, N, flags, with_bias, True, **kw)
    rows = M if kw.get("M_dev") is None else min(M, kw["M_dev"])
    assert not bool(torch.isnan(old[:rows]).any())
    assert torch.equal(old[:rows], new[:rows]), (M, N, flags, with_bias, kw)
    assert bool(torch.isnan(old[rows:]).all()) and bool(torch.isnan(new[rows:]).all()), "a store reached a row past the row count"
    if bound:
        c = SimpleNamespace(**vars(_gemm_case(N)))
        c.A, c.R, c.M = c.A[:M], c.R[:M], M
        if not with_bias:
            c.bias = torch.zeros(N)
        ref, bnd, _ = RR.gemm_ref_bound(c, flags)
        worst = RR.worst_ratio(new[:M].cpu(), ref, bnd)
        print(f"[gemm_tall_packed] M={M} N={N} flags={flags} bias={with_bias}: worst |err| / bound = {worst:.4f}")
        assert worst <= 1.0, worst


@pytest.mark.parametrize("M", [1, 15, 16, 17, 127, 128, 129, 2 * 128 * 2 + 129])
@pytest.mark.parametrize("N", [32, 96, 768])
def test_tall_rows(M, N):
    """32: fewer chunks than ring stages; 96: the stage phase moves from tile to tile; the last row count: three tiles per
    workgroup on a grid of 2, the chunk offset wraps twice."""
    _check_tall(M, N)


@pytest.mark.parametrize("flags", [0, RELU, RES, RELU | RES])
@pytest.mark.parametrize("with_bias", [False, True])
def test_tall_flags(flags, with_bias):
    _check_tall(2 * 128 * 2 + 129, 96, flags, with_bias, bound=True)
    _check_tall(129, 768, flags, with_bias)


def test_tall_device_row_count():
    _check_tall(2 * 128 * 2 + 129, 96, RELU | RES, M_dev=300)
    _check_tall(2 * 128 * 2 + 129, 768, 0, M_dev=0)


# ------------------------------------------------------------------------------------------------ the model handle
def test_reloaded_weights_rebuild_the_images():
    """A batch large enough for the tail's row kernel (> 768 row groups) with the tall GEMM forced on: packed == row-major on
    one set of weights, then -- the SAME model object, other weights -- packed == row-major again, and not the first result."""
    from cone_amd.model import build_model
    dev = _gpu()
    opt = make_opt("ego4d")
    model, _ = build_model(opt)
    B = 128
    lens_v, lens_q = [opt.max_v_l] * B, [opt.max_q_l] * B
    assert B * (opt.max_v_l + opt.max_q_l) > 768 * 16
    inp = gi.stage_b_inputs(opt, 43, lens_v[:4], lens_q[:4])
    vid = np.concatenate([inp["src_vid"][b % 4, :lens_v[b]] * (1 + 0.01 * b) for b in range(B)], 0).astype(np.float32)
    txt = np.concatenate([inp["src_txt"][b % 4, :lens_q[b]] * (1 - 0.005 * b) for b in range(B)], 0).astype(np.float32)
    i32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=dev)
    vrow0, trow0 = i32(np.concatenate([[0], np.cumsum(lens_v)[:-1]])), i32(np.concatenate([[0], np.cumsum(lens_q)[:-1]]))
    tok_index = i32(np.concatenate([np.arange(n) for n in lens_q]))

    def run(packed):
        model.set_option("gemm_tall_min_rows", 1)
        model.set_option("tail_packed", packed)
        model.set_option("gemm_tall_packed", packed)
        vproj, tproj = model.project(0, torch.from_numpy(vid).to(dev)), model.project(1, torch.from_numpy(txt).to(dev))
        out = model.forward_packed(vproj, vrow0, i32(lens_v), tproj, trow0, i32(lens_q), opt.max_v_l, opt.max_q_l,
                                   l0=model.layer0_cache(vproj, tproj, opt.max_v_l, tok_index=tok_index), saliency=True)
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}

    lib = _lib.load()
    count = lambda: (lib.cone_test_f32_packed_launches(0), lib.cone_test_f32_packed_launches(1))
    results = []
    for seed in (11, 12):
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(opt, seed).items()})
        c0 = count()
        new = run(1)
        c1 = count()
        old = run(0)
        # the handle's images were attached: both encoder tails ran the packed row kernel, and the tall GEMM its packed form
        assert c1[0] - c0[0] >= opt.enc_layers and c1[1] - c0[1] >= 1, (c0, c1)
        assert count() == c1, "a launch streamed an image with the options off"
        assert len(old) >= 3 and set(old) == set(new)
        for k in old:
            assert torch.equal(old[k], new[k]), (seed, k)
        results.append(new)
    assert not torch.equal(results[0]["pred_spans"], results[1]["pred_spans"])
