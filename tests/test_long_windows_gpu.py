"""Windows of more than 256 tokens (up to 1024) on an MI355X: the streaming attention core of cone_amd/csrc/general.hip
(gen_attn_stream_kernel, selected by kcap > 256 through the existing hook cone_test_gen_attn) and the handle option
"max_window_tokens" that opens the limit behind it.

Tolerances are the project's own: 2e-5 (absolute, inputs ~ N(0, 4)) for the attention core against float64, as
tests/test_general_shape_gpu.py::test_attention_core_matches_float64; 1e-4 on raw stage-B outputs against the oracle / the
reference fixture.  Every test prints the figures it asserts on.
"""
import json
import os

import numpy as np
import pytest
import torch

import inputs as gi
from cone_amd import synth
from cone_amd.config import make_opt
from oracle import cone_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-4
ATTN_TOL = 2e-5
KB = 64             # key block of the streaming core (general.hip: kGenStreamBlock)
SENTINEL = 12345.0


def _gpu():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda", 0)


def maxdiff(a, b):
    return float((torch.as_tensor(a).detach().cpu().double() - torch.as_tensor(b).detach().cpu().double()).abs().max())


def _valid_clips(lens_v, Lv):
    m = np.zeros((len(lens_v), Lv), bool)
    for b, v in enumerate(lens_v):
        m[b, :v] = True
    return m


def _safe_proposals(pred_spans, lens_v, margin=1e-3):
    sp = torch.as_tensor(pred_spans).double()
    dur = torch.as_tensor(np.asarray(lens_v)).double()[:, None]
    x1 = (sp[..., 0] - 0.5 * sp[..., 1]) * dur
    x2 = (sp[..., 0] + 0.5 * sp[..., 1]) * dur
    near = lambda x: (x - x.round()).abs() < margin
    return ~(near(x1) | near(x2))


# ------------------------------------------------------------------------------------------------ attention core
def _attn64(q, k, v, hd):
    s = (q.astype(np.float64) * np.sqrt(1.0 / hd)) @ k.astype(np.float64).T
    s -= s.max(axis=1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=1, keepdims=True)
    return p @ v.astype(np.float64)


def _run_attn(qkv, dq, off, heads, hd, kcap, nq):
    """cone_test_gen_attn on packed rows qkv (M, 3 d) [q | k | v]: the encoder form (nq == 0: both sides packed) or the decoder
    cross form (nq slot queries per window from dq (B nq, 3 d), packed keys).  Output rows start as SENTINEL."""
    from cone_amd import _lib
    lib, dev = _lib.load(), _gpu()
    d = hd * heads
    B = len(off) - 1
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    QKV, OFF = t(qkv), t(np.asarray(off, np.int32))
    p = lambda x: x.data_ptr()
    if nq == 0:
        out = torch.full((qkv.shape[0], d), SENTINEL, device=dev)
        _lib.check(lib.cone_test_gen_attn(p(QKV), 3 * d, p(QKV) + 4 * d, 3 * d, p(QKV) + 8 * d, 3 * d, p(out), d, p(OFF), p(OFF),
                                          B, 0, heads, hd, kcap, _lib.stream()))
    else:
        DQ = t(dq)
        out = torch.full((B * nq, d), SENTINEL, device=dev)
        _lib.check(lib.cone_test_gen_attn(p(DQ), 3 * d, p(QKV) + 4 * d, 3 * d, p(QKV) + 8 * d, 3 * d, p(out), d, None, p(OFF),
                                          B, nq, heads, hd, kcap, _lib.stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _worst(out, qkv, dq, off, heads, hd, nq):
    """Largest absolute difference to float64 over the non-empty windows; an empty window's rows must be untouched."""
    d = hd * heads
    worst = 0.0
    for b in range(len(off) - 1):
        r0, r1 = int(off[b]), int(off[b + 1])
        rows = slice(r0, r1) if nq == 0 else slice(b * nq, (b + 1) * nq)
        if r1 == r0:
            if nq:
                assert (out[rows] == SENTINEL).all()
            continue
        for h in range(heads):
            c = slice(h * hd, (h + 1) * hd)
            q = qkv[r0:r1, c] if nq == 0 else dq[rows, c]
            k, v = qkv[r0:r1, d + h * hd:d + (h + 1) * hd], qkv[r0:r1, 2 * d + h * hd:2 * d + (h + 1) * hd]
            worst = max(worst, float(np.abs(out[rows, c] - _attn64(q, k, v, hd)).max()))
    return worst


LENS = [1, 15, 16, 17, 255, 256, 257, 0, KB - 1, KB, KB + 1, 2 * KB + 3, 1024]


def _random_case(hd, heads, lens, seed):
    d = hd * heads
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rng = np.random.default_rng(seed)
    qkv = (rng.standard_normal((int(off[-1]), 3 * d)) * 2).astype(np.float32)
    dq = (rng.standard_normal((len(lens) * 10, 3 * d)) * 2).astype(np.float32)
    return qkv, dq, off


@pytest.mark.parametrize("hd,heads", [(16, 4), (32, 4), (64, 2)])
def test_streaming_core_matches_float64(hd, heads):
    """kcap = 1024 selects gen_attn_stream_kernel.  One ragged batch with windows of 1, 15, 16, 17, 255, 256, 257, block - 1,
    block, block + 1, 2 block + 3 and 1024 keys and an EMPTY one: the encoder form, the decoder cross form with 5 and with 10
    slot queries (one partly filled 16-query tile); the empty window writes nothing (sentinel fill)."""
    qkv, dq, off = _random_case(hd, heads, LENS, hd * 100 + heads)
    B = len(LENS)
    enc = _run_attn(qkv, None, off, heads, hd, 1024, 0)
    w_enc = _worst(enc, qkv, None, off, heads, hd, 0)
    worst = {"encoder": w_enc}
    for nq in (5, 10):
        oc = _run_attn(qkv, dq[:B * nq], off, heads, hd, 1024, nq)
        worst[f"cross{nq}"] = _worst(oc, qkv, dq[:B * nq], off, heads, hd, nq)
    # a batch of empty windows only: nothing is written at all
    e = _run_attn(qkv[:4], dq[:15], np.zeros(4, np.int32), heads, hd, 1024, 5)
    assert (e == SENTINEL).all()
    print("streaming core vs float64", hd, heads, worst)
    assert max(worst.values()) < ATTN_TOL, worst


@pytest.mark.parametrize("hd,heads", [(16, 4), (32, 4), (64, 2)])
def test_streaming_core_saturated_scores(hd, heads):
    """|score| up to ~60 with every row's maximum in the LAST key block: keys grow along one direction u with the key index
    (score of key j against every query ~ 54 (j + 1) / n, the last key's ~ 60), the first key points the other way (score
    ~ -60), so the running maximum moves in every block and the accumulators are rescaled each time; exp(s - m) spans e^-120 .. 1."""
    d = hd * heads
    lens = [257, KB + 1, 1024, 3 * KB]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rng = np.random.default_rng(7 + hd)
    M = int(off[-1])
    qkv = np.zeros((M, 3 * d), np.float32)
    qkv[:, 2 * d:] = (rng.standard_normal((M, d)) * 2).astype(np.float32)
    a = np.sqrt(60.0 * np.sqrt(hd))
    for h in range(heads):
        u = rng.standard_normal(hd)
        u /= np.linalg.norm(u)
        for b, n in enumerate(lens):
            r0 = int(off[b])
            ramp = 0.9 * (np.arange(n) + 1.0) / n
            ramp[0], ramp[-1] = -1.0, 1.0
            qkv[r0:r0 + n, h * hd:(h + 1) * hd] = a * u + 0.3 * rng.standard_normal((n, hd))
            qkv[r0:r0 + n, d + h * hd:d + (h + 1) * hd] = a * ramp[:, None] * u + 0.3 * rng.standard_normal((n, hd))
    dq = np.tile(qkv[:5], (len(lens), 1)).astype(np.float32)
    # the construction does what it says: scores reach ~ +-60 and the row maxima sit in the last block
    for b, n in enumerate(lens):
        r0 = int(off[b])
        s = (qkv[r0:r0 + n, :hd].astype(np.float64) / np.sqrt(hd)) @ qkv[r0:r0 + n, d:d + hd].astype(np.float64).T
        assert s.max() > 50 and s.min() < -50
        assert (s.argmax(axis=1) >= (n - 1) // KB * KB).all()
    enc = _run_attn(qkv, None, off, heads, hd, 1024, 0)
    assert np.isfinite(enc).all()
    w_enc = _worst(enc, qkv, None, off, heads, hd, 0)
    oc = _run_attn(qkv, dq, off, heads, hd, 1024, 5)
    assert np.isfinite(oc).all()
    w_cross = _worst(oc, qkv, dq, off, heads, hd, 5)
    print("streaming core, saturated scores", hd, heads, w_enc, w_cross)
    assert max(w_enc, w_cross) < ATTN_TOL, (w_enc, w_cross)


def test_streaming_core_is_batch_and_capacity_invariant():
    """The same windows alone, in a small batch at kcap = 512 and between other windows at kcap = 1024: identical bits."""
    hd, heads = 32, 2
    d = hd * heads
    lens = [1, 17, KB, KB + 1, 257, 300, 512]
    qkv, dq, off = _random_case(hd, heads, lens, 5)
    a_enc = _run_attn(qkv, None, off, heads, hd, 512, 0)
    a_cr = _run_attn(qkv, dq[:len(lens) * 5], off, heads, hd, 512, 5)
    rng = np.random.default_rng(6)
    head_rows = (rng.standard_normal((1024, 3 * d)) * 2).astype(np.float32)
    tail_rows = (rng.standard_normal((700, 3 * d)) * 2).astype(np.float32)
    big = np.concatenate([head_rows, qkv, tail_rows])
    big_off = np.concatenate([[0], 1024 + off, [1024 + off[-1] + 700]]).astype(np.int32)
    dq_big = np.concatenate([dq[:5], dq[:len(lens) * 5], dq[5:10]])
    b_enc = _run_attn(big, None, big_off, heads, hd, 1024, 0)
    b_cr = _run_attn(big, dq_big, big_off, heads, hd, 1024, 5)
    assert np.array_equal(a_enc, b_enc[1024:1024 + off[-1]])
    assert np.array_equal(a_cr, b_cr[5:5 + len(lens) * 5])
    for b in (4, 5):        # alone
        r0, r1 = int(off[b]), int(off[b + 1])
        one = _run_attn(qkv[r0:r1], None, np.array([0, r1 - r0], np.int32), heads, hd, 1024, 0)
        assert np.array_equal(one, a_enc[r0:r1])
        one = _run_attn(qkv[r0:r1], dq[5 * b:5 * b + 5], np.array([0, r1 - r0], np.int32), heads, hd, 512, 5)
        assert np.array_equal(one, a_cr[5 * b:5 * b + 5])


@pytest.mark.parametrize("hd,heads", [(16, 4), (32, 4), (64, 2)])
def test_streaming_core_agrees_with_the_resident_kernel(hd, heads):
    """Windows of at most 256 keys through kcap = 300 (streaming) and kcap = 256 (resident): each within the float64 bound,
    their distance within twice that bound (two summation orders, not the same bits)."""
    lens = [1, 17, 101, 0, 256]
    qkv, dq, off = _random_case(hd, heads, lens, 11 + hd)
    B = len(lens)
    for nq in (0, 5):
        s = _run_attn(qkv, dq[:B * 5], off, heads, hd, 300, nq)
        r = _run_attn(qkv, dq[:B * 5], off, heads, hd, 256, nq)
        ws, wr = _worst(s, qkv, dq[:B * 5], off, heads, hd, nq), _worst(r, qkv, dq[:B * 5], off, heads, hd, nq)
        mutual = float(np.abs(s - r).max())
        print("streaming / resident vs float64, mutual", hd, heads, nq, ws, wr, mutual)
        assert ws < ATTN_TOL and wr < ATTN_TOL and mutual <= 2 * ATTN_TOL, (ws, wr, mutual)


# ------------------------------------------------------------------------------------------------ stage B vs the oracle
_MODELS = {}


def get_model(seed, **opt_kw):
    from cone_amd.model import build_model
    key = (seed,) + tuple(sorted(opt_kw.items()))
    if key not in _MODELS:
        opt = make_opt("ego4d", **opt_kw)
        sd = synth.make_state_dict(opt, seed)
        m, _ = build_model(opt)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        _MODELS[key] = (m, opt, O.as_torch_sd(sd), sd)
    return _MODELS[key]


def arena_forward(model, inp, lens_v, lens_q, dev, Lv=None, Lq=None):
    """The eval driver's entry: the windows' valid rows as clip / token arenas, projected once, then forward_packed with a
    (row0, len) list."""
    vid = np.concatenate([inp["src_vid"][b, :lens_v[b]] for b in range(len(lens_v))], 0)
    txt = np.concatenate([inp["src_txt"][b, :lens_q[b]] for b in range(len(lens_q))], 0)
    i32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=dev)
    vrow0 = i32(np.concatenate([[0], np.cumsum(lens_v)[:-1]]))
    trow0 = i32(np.concatenate([[0], np.cumsum(lens_q)[:-1]]))
    vproj = model.project(0, torch.from_numpy(vid).to(dev))
    tproj = model.project(1, torch.from_numpy(txt).to(dev))
    Lv, Lq = Lv or inp["src_vid"].shape[1], Lq or inp["src_txt"].shape[1]
    tok_index = i32(np.concatenate([np.arange(n) for n in lens_q]))
    return model.forward_packed(vproj, vrow0, i32(lens_v), tproj, trow0, i32(lens_q), Lv, Lq,
                                l0=model.layer0_cache(vproj, tproj, Lv, tok_index=tok_index), saliency=True, aux=True)


def padded_forward(model, inp, dev, taps=False):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return model.forward(t(inp["src_txt"]), t(inp["txt_mask"]), t(inp["src_vid"]), t(inp["vid_mask"]), taps=taps)


def _ragged(Lv, Lq):
    return [Lv, 1, Lv // 2 + 3, Lv - 7], [Lq, 3, Lq // 2, Lq - 1]


STAGE_B = [  # (Lv, Lq, hidden_dim, nheads, pre_norm, use_txt_pos)
    (240, 17, 256, 8, False, False),        # 257 tokens: the first length past the old limit
    (300, 20, 256, 8, False, False),
    (480, 32, 256, 8, False, False),
    (992, 32, 256, 8, False, False),        # 1024 tokens: the maximum
    (300, 20, 128, 4, False, False),
    (300, 20, 256, 8, True, False),
    (300, 20, 256, 8, False, True),         # text tokens with their own position rows (txt_position_embed has max_q_l rows)
]


@pytest.mark.parametrize("Lv,Lq,d,h,pre,txt", STAGE_B)
def test_stage_b_matches_oracle(Lv, Lq, d, h, pre, txt):
    """CONE.forward on four ragged windows, the first of full length, against the oracle on the CPU: logits, spans, valid
    saliency, the aux layer, and forward_clip_matching on the proposals away from an integer clip boundary."""
    model, opt, sd, _ = get_model(Lv + d, max_v_l=Lv, max_q_l=Lq, hidden_dim=d, nheads=h, pre_norm=pre, use_txt_pos=txt)
    assert model.long_windows and model.max_window_tokens == Lv + Lq
    lens_v, lens_q = _ragged(Lv, Lq)
    inp = gi.stage_b_inputs(opt, 700 + Lv, lens_v, lens_q)
    t = torch.from_numpy
    with torch.no_grad():
        ref = O.cone_forward(sd, opt, t(inp["src_txt"]), t(inp["txt_mask"]), t(inp["src_vid"]), t(inp["vid_mask"]))
        ref_match = O.clip_matching(sd, opt, t(inp["src_cls_txt"]), t(inp["src_vid"]), t(inp["vid_mask"]), ref["pred_spans"])
    dev = _gpu()
    out = padded_forward(model, inp, dev)
    vm = _valid_clips(lens_v, Lv)
    sal = out["saliency_scores"].cpu().numpy()
    g = lambda a: torch.from_numpy(a).to(dev)
    match = model.forward_clip_matching(g(inp["src_cls_txt"]), g(inp["src_vid"]), g(inp["vid_mask"]),
                                        proposal=ref["pred_spans"].to(dev))
    ok = _safe_proposals(ref["pred_spans"], lens_v).numpy()
    errs = dict(logits=maxdiff(out["pred_logits"], ref["pred_logits"]), spans=maxdiff(out["pred_spans"], ref["pred_spans"]),
                aux_logits=maxdiff(out["aux_outputs"][0]["pred_logits"], ref["aux_outputs"][0]["pred_logits"]),
                aux_spans=maxdiff(out["aux_outputs"][0]["pred_spans"], ref["aux_outputs"][0]["pred_spans"]),
                saliency=float(np.abs(sal - ref["saliency_scores"].numpy())[vm].max()),
                matching=float(np.abs(match.cpu().numpy() - ref_match.numpy())[ok].max()))
    print("stage B vs oracle", (Lv, Lq, d, h, pre, txt), errs)
    assert (sal[~vm] == 0).all()
    assert max(errs.values()) < TOL, errs


def test_stage_b_matches_reference_long_fixture(golden_dir):
    """Raw outputs of the unmodified reference at 300 clips + 20 words (tests/golden/gen_golden_long.py), through both
    entries."""
    fx = np.load(os.path.join(golden_dir, "stageB_long.npz"), allow_pickle=False)
    meta = json.loads(str(fx["meta"]))
    opt = make_opt(meta["preset"], **meta["opt"])
    lens_v, lens_q = [int(x) for x in fx["lens_v"]], [int(x) for x in fx["lens_q"]]
    inp = gi.stage_b_inputs(opt, int(fx["input_seed"]), lens_v, lens_q)
    assert gi.checksum(inp["src_vid"], inp["src_txt"], inp["src_cls_txt"]) == str(fx["input_checksum"])
    sdn = synth.make_state_dict(opt, int(fx["weight_seed"]))
    from cone_amd.model import build_model
    model, _ = build_model(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()})
    dev = _gpu()
    vm = _valid_clips(lens_v, inp["src_vid"].shape[1])
    for entry in ("padded", "arena"):
        out = padded_forward(model, inp, dev, taps=True) if entry == "padded" else arena_forward(model, inp, lens_v, lens_q, dev)
        errs = dict(logits=maxdiff(out["pred_logits"], fx["pred_logits"]), spans=maxdiff(out["pred_spans"], fx["pred_spans"]),
                    aux_logits=maxdiff(out["aux_outputs"][0]["pred_logits"], fx["aux_pred_logits"]),
                    aux_spans=maxdiff(out["aux_outputs"][0]["pred_spans"], fx["aux_pred_spans"]),
                    saliency=float(np.abs(out["saliency_scores"].cpu().numpy() - fx["saliency_scores"])[vm].max()))
        if entry == "padded":
            Lv, st = inp["src_vid"].shape[1], int(fx["mem_stride"])
            mem, ref_mem = out["memory"].cpu().numpy()[..., ::st], fx["memory"]
            errs["memory"] = max(max(np.abs(mem[b, :lens_v[b]] - ref_mem[b, :lens_v[b]]).max(),
                                     np.abs(mem[b, Lv:Lv + lens_q[b]] - ref_mem[b, Lv:Lv + lens_q[b]]).max())
                                 for b in range(len(lens_v)))
            errs["hs"] = maxdiff(out["hs"], fx["hs"])
        print("stage B vs the reference's fixture", entry, errs)
        assert max(errs.values()) < TOL, (entry, errs)
    g = lambda a: torch.from_numpy(a).to(dev)
    match = model.forward_clip_matching(g(inp["src_cls_txt"]), g(inp["src_vid"]), g(inp["vid_mask"]),
                                        proposal=torch.from_numpy(fx["pred_spans"]).to(dev))
    ok = _safe_proposals(fx["pred_spans"], lens_v).numpy()
    assert np.abs(match.cpu().numpy() - fx["matching"])[ok].max() < TOL


# ------------------------------------------------------------------------------------------------ limits
def test_limits_are_named():
    from cone_amd import _lib
    from cone_amd.model import build_model
    model, opt, _, _ = get_model(300 + 256, max_v_l=300, max_q_l=20, hidden_dim=256, nheads=8, pre_norm=False, use_txt_pos=False)
    dev = _gpu()
    inp = gi.stage_b_inputs(opt, 3, [301], [20])                # 321 tokens
    with pytest.raises(_lib.ConeHipError, match="max_window_tokens = 320"):
        padded_forward(model, inp, dev)
    with pytest.raises(_lib.ConeHipError, match="max_window_tokens = 320"):
        arena_forward(model, inp, [301], [20], dev)
    with pytest.raises(_lib.ConeHipError, match="max_window_tokens"):        # a long-window handle is exact fp32 only
        model.set_option("bf16", 1)
    with pytest.raises(_lib.ConeHipError, match="max_window_tokens"):
        model.set_option("split_bf16", 1)
    model.set_option("bf16", 0)
    for bad in (1025, 255):
        with pytest.raises(_lib.ConeHipError, match=r"max_window_tokens %d not in \[256, 1024\]" % bad):
            model.set_option("max_window_tokens", bad)
    out = padded_forward(model, gi.stage_b_inputs(opt, 3, [300], [20]), dev)       # (the refused values changed nothing)
    assert torch.isfinite(out["pred_spans"]).all()
    # a handle left at the default still stops at 256 tokens, and bf16 locks the option
    small, sopt, _, _ = get_model(1, max_v_l=90, max_q_l=20)
    assert not small.long_windows
    with pytest.raises(_lib.ConeHipError, match="exceeds 256 tokens"):
        padded_forward(small, gi.stage_b_inputs(sopt, 3, [237], [20]), dev)
    small.set_option("bf16", 1)
    with pytest.raises(_lib.ConeHipError, match="max_window_tokens"):
        small.set_option("max_window_tokens", 512)
    small.set_option("bf16", 0)
    too_long, _ = build_model(make_opt("ego4d", max_v_l=1000, max_q_l=64))
    with pytest.raises(ValueError, match="max_v_l=1000"):
        too_long.load_state_dict({})


# ------------------------------------------------------------------------------------------------ one path, whatever the entry or the batch
def test_padded_and_arena_entries_are_one_path():
    """On a (300, 20) handle cone_forward_windows and cone_forward_packed give the same bits, and a padded batch whose own
    longest window has 120 tokens gives its windows the bits they get beside a 320-token window (no fall-back to the fused
    path for a short batch)."""
    model, opt, _, _ = get_model(300 + 256, max_v_l=300, max_q_l=20, hidden_dim=256, nheads=8, pre_norm=False, use_txt_pos=False)
    dev = _gpu()
    lens_v, lens_q = [300, 100, 57, 1], [20, 20, 7, 3]
    inp = gi.stage_b_inputs(opt, 41, lens_v, lens_q)
    full = padded_forward(model, inp, dev)
    arena = arena_forward(model, inp, lens_v, lens_q, dev)
    for k in ("pred_logits", "pred_spans", "saliency_scores"):
        assert torch.equal(full[k], arena[k]), k
    assert torch.equal(full["aux_outputs"][0]["pred_spans"], arena["aux_outputs"][0]["pred_spans"])
    short = dict(src_vid=inp["src_vid"][1:, :100], vid_mask=inp["vid_mask"][1:, :100], src_txt=inp["src_txt"][1:], txt_mask=inp["txt_mask"][1:])
    o = padded_forward(model, short, dev)
    a = arena_forward(model, short, lens_v[1:], lens_q[1:], dev)
    for k in ("pred_logits", "pred_spans"):
        assert torch.equal(o[k], full[k][1:]), k
        assert torch.equal(a[k], full[k][1:]), k
    assert torch.equal(o["saliency_scores"], full["saliency_scores"][1:, :100])


# ------------------------------------------------------------------------------------------------ end to end
def _long_split(opt):
    """3 videos of 700 / 1500 / 2300 clips, 6 queries of up to max_q_l tokens."""
    ann, vf, qf = synth.make_dataset(opt, 6, 3, seed=23, ctx_range=(100, 101), lq_range=(5, opt.max_q_l + 1))
    rng = np.random.default_rng(77)
    for cid, n in zip(list(vf), (700, 1500, 2300)):
        vf[cid] = rng.standard_normal((n, opt.v_appear_feat_dim), dtype=np.float32)
    for row in ann:
        row["duration"] = float(vf[row["clip_id"]].shape[0]) * opt.clip_length
    return ann, vf, qf


def test_end_to_end_long_windows_match_oracle():
    """predict_split with max_v_l = 400, max_q_l = 20 against the oracle's pipeline: window rank lists exact, the window rows
    at the project tolerances, fusion + NMS exact on identical candidates; predict_split_async with two splits in flight (one
    of them under hipGraph replay) gives the same lists."""
    from cone_amd import inference as inf
    kw = dict(max_v_l=400, max_q_l=20, nms_thd=0.5, eval_split_name="test", topk_window=5, eval_bsz=4)
    model, _, _, sdn = get_model(9, max_v_l=400, max_q_l=20)
    opt = make_opt("ego4d", **kw)
    ann, vf, qf = _long_split(opt)
    store = inf.FeatureStore(opt, ann, vf, qf)
    (f1, p1, m1), info = inf.predict_split(model, store, opt)
    (fo, po, mo), ranks, mr = O.eval_epoch(sdn, opt, ann, vf, qf)
    for qi, row in enumerate(ann):
        assert [w for w in info["win_idx"][qi].cpu().tolist() if w >= 0] == ranks[row["query_id"]][:opt.topk_window]
    mine, _ = inf.compute_mr_results(model, store, opt, info["win_idx"])
    A = lambda r: np.array(r["pred_relevant_windows"])
    worst = max(np.abs(A(a)[:, 2] - A(b)[:, 2]).max() for a, b in zip(mine, mr))
    worst_sec = max(np.abs(A(a)[:, :2] - A(b)[:, :2]).max() for a, b in zip(mine, mr))
    print("end to end, long windows: worst proposal score / span (s) vs the oracle", worst, worst_sec)
    assert worst <= 2e-4, worst
    assert worst_sec <= 1e-4 * opt.max_v_l * opt.clip_length + 1e-4, worst_sec
    f2, p2, m2 = inf.postprocessing_format_ego4d(mr, opt)          # stage C on the oracle's own rows: bit-exact fusion + NMS
    assert (f2, p2, m2) == (fo, po, mo)
    assert len(f1) == len(fo) == len(ann)
    opt_g = make_opt("ego4d", hip_graph=True, **kw)
    store_g = inf.FeatureStore(opt_g, ann, vf, qf)
    for _ in range(2):                                              # the second round replays the captured graph
        pend = [inf.predict_split_async(model, store, opt), inf.predict_split_async(model, store_g, opt_g)]
        got = [h.result()[0] for h in reversed(pend)]
        assert got[0] == (f1, p1, m1) and got[1] == (f1, p1, m1)


def test_localizer_with_long_windows():
    """CONELocalizator(max_v_l=300) against oracle.localizer_predict."""
    from types import SimpleNamespace
    from cone_amd.localizator import CONELocalizator, LOCALIZER_OPT
    kw = dict(max_v_l=300, topk_window=5)           # (a 1000-clip video has 8 windows of 300 clips)
    opt = SimpleNamespace(**dict(LOCALIZER_OPT, **kw))
    sdn = synth.make_state_dict(opt, 4)
    loc = CONELocalizator(state_dict={k: torch.from_numpy(v) for k, v in sdn.items()}, **kw)
    g = torch.Generator().manual_seed(3)
    vid = torch.randn(1000, 256, generator=g) * 2
    tok, cls = torch.randn(11, 768, generator=g), torch.randn(256, generator=g)
    got = np.array(loc.predict_moment(vid, (tok, cls)))
    ref = np.array(O.localizer_predict(sdn, opt, vid, tok, cls))
    assert got.shape == ref.shape
    assert np.abs(got[:, :2] - ref[:, :2]).max() <= 1e-4 * opt.max_v_l * opt.clip_length + 1e-4
    assert np.abs(got[:, 2] - ref[:, 2]).max() < 2e-3


def test_sharded_drivers_with_long_windows():
    """The window- and query-sharded drivers on a (300, 20) model over a one-rank gloo group reproduce the plain pipeline (the
    multi-rank exchange itself is covered on the CPU by tests/test_parallel_cpu.py; routing is per handle, so a shard runs the
    launches the whole split runs)."""
    import torch.distributed as dist
    from cone_amd import inference as inf
    from cone_amd import parallel as par
    model, _, _, _ = get_model(300 + 256, max_v_l=300, max_q_l=20, hidden_dim=256, nheads=8, pre_norm=False, use_txt_pos=False)
    opt = make_opt("ego4d", max_v_l=300, max_q_l=20, nms_thd=0.5, eval_split_name="test", topk_window=4, eval_bsz=4)
    ann, vf, qf = synth.make_dataset(opt, 7, 2, seed=29, ctx_range=(900, 1400), lq_range=(5, 21))
    store = inf.FeatureStore(opt, ann, vf, qf)
    plain, _ = inf.predict_split(model, store, opt)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29557")
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        for mode in ("window", "query"):
            got, info = par.predict_split_distributed(model, store, opt, mode=mode)
            assert got == plain, mode
            assert info["world"] == 1
            h = par.predict_split_distributed_async(model, store, opt, mode=mode, format_shard=True)
            assert h.result()[0] == plain, mode
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
