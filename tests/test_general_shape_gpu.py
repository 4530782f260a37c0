"""Checkpoints with hidden_dim / nheads other than 256 / 8: the general-shape path (cone_amd/csrc/general.hip) on an MI355X.

Every test here runs a shape that cone_model_create rejected before the general path existed.  Tolerances are those of
tests/test_gpu_parity.py: 1e-4 on raw outputs against the oracle / the reference fixtures, 5e-5 between the general and the
shipped path at 256 / 8 (re-associated sums).
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
AB_TOL = 5e-5
PIPELINE_FLOOR = 0.975
HERE = os.path.dirname(os.path.abspath(__file__))


def _gpu():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda", 0)


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


def arena_forward(model, inp, lens_v, lens_q, dev):
    """The eval driver's entry: the windows' valid rows as clip / token arenas, projected once, then forward_packed."""
    vid = np.concatenate([inp["src_vid"][b, :lens_v[b]] for b in range(len(lens_v))], 0)
    txt = np.concatenate([inp["src_txt"][b, :lens_q[b]] for b in range(len(lens_q))], 0)
    i32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=dev)
    vrow0 = i32(np.concatenate([[0], np.cumsum(lens_v)[:-1]]))
    trow0 = i32(np.concatenate([[0], np.cumsum(lens_q)[:-1]]))
    vproj = model.project(0, torch.from_numpy(vid).to(dev))
    tproj = model.project(1, torch.from_numpy(txt).to(dev))
    Lv, Lq = inp["src_vid"].shape[1], inp["src_txt"].shape[1]
    tok_index = i32(np.concatenate([np.arange(n) for n in lens_q]))
    return model.forward_packed(vproj, vrow0, i32(lens_v), tproj, trow0, i32(lens_q), Lv, Lq,
                                l0=model.layer0_cache(vproj, tproj, Lv, tok_index=tok_index), saliency=True, aux=True)


def forward(entry, model, inp, lens_v, lens_q, dev, taps=False):
    t = lambda a: torch.from_numpy(a).to(dev)
    if entry == "padded":
        return model.forward(t(inp["src_txt"]), t(inp["txt_mask"]), t(inp["src_vid"]), t(inp["vid_mask"]), taps=taps)
    return arena_forward(model, inp, lens_v, lens_q, dev)


def _agree(f1, fo, opt):
    n = 0
    for a, b in zip(f1, fo):
        ra, rb = np.array(a["predicted_times"]), np.array(b["predicted_times"])
        if ra.shape == rb.shape and np.abs(ra - rb).max() <= 1e-4 * opt.max_v_l * opt.clip_length + 2e-4:
            n += 1
    return n


# ------------------------------------------------------------------------------------------------ attention core
def _attn64(q, k, v, hd):
    s = (q.astype(np.float64) * np.sqrt(1.0 / hd)) @ k.astype(np.float64).T
    s -= s.max(axis=1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=1, keepdims=True)
    return p @ v.astype(np.float64)


@pytest.mark.parametrize("hd,heads", [(16, 4), (32, 4), (64, 2), (64, 8)])
def test_attention_core_matches_float64(hd, heads):
    """cone_test_gen_attn against float64: encoder form (queries = keys = the window's packed rows), decoder cross-attention
    form (5 slot queries per window, packed keys) and decoder self-attention form (slots against slots); windows of 1, 17,
    101 and 256 tokens and an EMPTY one, which writes nothing."""
    from cone_amd import _lib
    lib = _lib.load()
    dev = _gpu()
    d = hd * heads
    lens = [1, 17, 0, 101, 256]
    B, nq = len(lens), 5
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    M = int(off[-1])
    rng = np.random.default_rng(hd * 100 + heads)
    qkv = (rng.standard_normal((M, 3 * d)) * 2).astype(np.float32)
    dq = (rng.standard_normal((B * nq, 3 * d)) * 2).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)
    QKV, DQ, OFF = t(qkv), t(dq), t(off)
    p = lambda x: x.data_ptr()
    s = _lib.stream()
    sentinel = 12345.0
    # encoder form
    out = torch.full((M, d), sentinel, device=dev)
    _lib.check(lib.cone_test_gen_attn(p(QKV), 3 * d, p(QKV) + 4 * d, 3 * d, p(QKV) + 8 * d, 3 * d, p(out), d, p(OFF), p(OFF),
                                      B, 0, heads, hd, 256, s))
    # cross form: slot queries, packed keys (the empty window's slots stay untouched)
    oc = torch.full((B * nq, d), sentinel, device=dev)
    _lib.check(lib.cone_test_gen_attn(p(DQ), 3 * d, p(QKV) + 4 * d, 3 * d, p(QKV) + 8 * d, 3 * d, p(oc), d, None, p(OFF),
                                      B, nq, heads, hd, 256, s))
    # self form over the slots
    osf = torch.full((B * nq, d), sentinel, device=dev)
    _lib.check(lib.cone_test_gen_attn(p(DQ), 3 * d, p(DQ) + 4 * d, 3 * d, p(DQ) + 8 * d, 3 * d, p(osf), d, None, None,
                                      B, nq, heads, hd, nq, s))
    torch.cuda.synchronize()
    out, oc, osf = out.cpu().numpy(), oc.cpu().numpy(), osf.cpu().numpy()
    worst = 0.0
    for b in range(B):
        r0, r1 = off[b], off[b + 1]
        for h in range(heads):
            c = slice(h * hd, (h + 1) * hd)
            q, k, v = qkv[r0:r1, c], qkv[r0:r1, d + h * hd:d + (h + 1) * hd], qkv[r0:r1, 2 * d + h * hd:2 * d + (h + 1) * hd]
            sq = dq[b * nq:(b + 1) * nq]
            if r1 > r0:
                worst = max(worst, np.abs(out[r0:r1, c] - _attn64(q, k, v, hd)).max())
                worst = max(worst, np.abs(oc[b * nq:(b + 1) * nq, c] - _attn64(sq[:, c], k, v, hd)).max())
            else:
                assert (oc[b * nq:(b + 1) * nq] == sentinel).all()
            worst = max(worst, np.abs(osf[b * nq:(b + 1) * nq, c] - _attn64(
                sq[:, c], sq[:, d + h * hd:d + (h + 1) * hd], sq[:, 2 * d + h * hd:2 * d + (h + 1) * hd], hd)).max())
    assert worst < 2e-5, worst


# ------------------------------------------------------------------------------------------------ raw outputs vs the oracle
SHAPES = [  # (hidden_dim, nheads, pre_norm, use_txt_pos, num_queries)
    (64, 4, False, False, 1), (128, 4, True, True, 5), (128, 8, False, False, 16), (192, 3, True, False, 5),
    (256, 4, False, True, 5), (256, 16, True, False, 16), (384, 6, False, False, 1), (512, 8, True, True, 5),
    (512, 16, False, False, 5),
]


@pytest.mark.parametrize("entry", ["padded", "arena"])
@pytest.mark.parametrize("d,h,pre,txt,nq", SHAPES)
def test_random_batches_match_oracle(d, h, pre, txt, nq, entry):
    """Ragged batches with a 1-clip window and a 256-token window (230 clips + 26 words) at every listed shape, against the
    oracle: logits, spans, the aux layer, saliency and the proposal matching (adapter hidden width = hidden_dim)."""
    model, opt, sd, _ = get_model(d + h, hidden_dim=d, nheads=h, pre_norm=pre, use_txt_pos=txt, num_queries=nq,
                                  max_v_l=230, max_q_l=26, dim_feedforward=256 if d <= 128 else 512)
    rng = np.random.default_rng(d * 31 + h)
    B = 5
    lens_v = [230, 1] + [int(x) for x in rng.integers(1, 120, B - 2)]
    lens_q = [26, 3] + [int(x) for x in rng.integers(1, 27, B - 2)]
    inp = gi.stage_b_inputs(opt, 500 + d + h, lens_v, lens_q)
    t = torch.from_numpy
    with torch.no_grad():
        ref = O.cone_forward(sd, opt, t(inp["src_txt"]), t(inp["txt_mask"]), t(inp["src_vid"]), t(inp["vid_mask"]))
        ref_match = O.clip_matching(sd, opt, t(inp["src_cls_txt"]), t(inp["src_vid"]), t(inp["vid_mask"]), ref["pred_spans"])
    dev = _gpu()
    out = forward(entry, model, inp, lens_v, lens_q, dev)
    assert tuple(out["pred_logits"].shape) == (B, nq, 2)
    assert maxdiff(out["pred_logits"], ref["pred_logits"]) < TOL
    assert maxdiff(out["pred_spans"], ref["pred_spans"]) < TOL
    assert maxdiff(out["aux_outputs"][0]["pred_logits"], ref["aux_outputs"][0]["pred_logits"]) < TOL
    assert maxdiff(out["aux_outputs"][0]["pred_spans"], ref["aux_outputs"][0]["pred_spans"]) < TOL
    vm = _valid_clips(lens_v, inp["src_vid"].shape[1])
    sal = out["saliency_scores"].cpu().numpy()
    assert np.abs(sal - ref["saliency_scores"].numpy())[vm].max() < TOL
    assert (sal[~vm] == 0).all()
    g = lambda a: torch.from_numpy(a).to(dev)
    match = model.forward_clip_matching(g(inp["src_cls_txt"]), g(inp["src_vid"]), g(inp["vid_mask"]),
                                        proposal=ref["pred_spans"].to(dev))
    ok = _safe_proposals(ref["pred_spans"], lens_v).numpy()
    assert np.abs(match.cpu().numpy() - ref_match.numpy())[ok].max() < TOL


# ------------------------------------------------------------------------------------------------ reference fixtures
@pytest.mark.parametrize("entry", ["padded", "arena"])
@pytest.mark.parametrize("name", ["stageB_shape_128x4_prenorm", "stageB_shape_256x16_prenorm", "stageB_shape_512x8_prenorm"])
def test_stage_b_matches_reference_golden_shapes(golden_dir, name, entry):
    """Raw outputs of the unmodified reference (tests/golden/gen_golden_shapes.py) at three new shapes, through both
    entries: logits, spans, saliency, the aux layer, memory and hs (padded entry's taps), proposal matching."""
    fx = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(fx["meta"]))
    opt = make_opt(meta["preset"], **meta["opt"])
    assert (opt.hidden_dim, opt.nheads) == (int(fx["hidden_dim"]), int(fx["nheads"]))
    lens_v, lens_q = [int(x) for x in fx["lens_v"]], [int(x) for x in fx["lens_q"]]
    inp = gi.stage_b_inputs(opt, int(fx["input_seed"]), lens_v, lens_q)
    assert gi.checksum(inp["src_vid"], inp["src_txt"], inp["src_cls_txt"]) == str(fx["input_checksum"])
    sdn = synth.make_state_dict(opt, int(fx["weight_seed"]))
    from cone_amd.model import build_model
    model, _ = build_model(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()})
    dev = _gpu()
    out = forward(entry, model, inp, lens_v, lens_q, dev, taps=True)
    assert maxdiff(out["pred_logits"], fx["pred_logits"]) < TOL
    assert maxdiff(out["pred_spans"], fx["pred_spans"]) < TOL
    assert maxdiff(out["aux_outputs"][0]["pred_logits"], fx["aux_pred_logits"]) < TOL
    assert maxdiff(out["aux_outputs"][0]["pred_spans"], fx["aux_pred_spans"]) < TOL
    vm = _valid_clips(lens_v, inp["src_vid"].shape[1])
    assert np.abs(out["saliency_scores"].cpu().numpy() - fx["saliency_scores"])[vm].max() < TOL
    if entry == "padded":
        Lv = inp["src_vid"].shape[1]
        st = int(fx["mem_stride"])                  # (the fixture keeps every st-th channel of memory)
        mem, ref_mem = out["memory"].cpu().numpy()[..., ::st], fx["memory"]
        for b in range(len(lens_v)):        # valid rows only (the reference's padded rows are attention garbage)
            assert np.abs(mem[b, :lens_v[b]] - ref_mem[b, :lens_v[b]]).max() < TOL
            assert np.abs(mem[b, Lv:Lv + lens_q[b]] - ref_mem[b, Lv:Lv + lens_q[b]]).max() < TOL
        assert maxdiff(out["hs"], fx["hs"]) < TOL
    g = lambda a: torch.from_numpy(a).to(dev)
    match = model.forward_clip_matching(g(inp["src_cls_txt"]), g(inp["src_vid"]), g(inp["vid_mask"]),
                                        proposal=torch.from_numpy(fx["pred_spans"]).to(dev))
    ok = _safe_proposals(fx["pred_spans"], lens_v).numpy()
    assert np.abs(match.cpu().numpy() - fx["matching"])[ok].max() < TOL


# ------------------------------------------------------------------------------------------------ A/B at 256 / 8
def test_forced_general_path_equals_shipped_path():
    """cone_model_set_option("general_shape", 1) runs a 256 / 8 handle on the general path: raw outputs within the cross-path
    tolerance of the shipped path, kept moments equal except where the shipped path's candidates tie within it.  A handle
    with the option set back to 0 is bit-identical to one that never set it."""
    from cone_amd import inference as inf
    model, opt, sd, _ = get_model(0)
    rng = np.random.default_rng(5)
    B = 32
    lens_v = [int(x) for x in rng.integers(1, opt.max_v_l + 1, B)]
    lens_v[0], lens_v[1] = opt.max_v_l, 1
    lens_q = [int(x) for x in rng.integers(1, opt.max_q_l + 1, B)]
    inp = gi.stage_b_inputs(opt, 321, lens_v, lens_q)
    dev = _gpu()
    keys = ("pred_logits", "pred_spans", "saliency_scores", "memory", "hs")
    base = {k: v.cpu() for k, v in forward("padded", model, inp, lens_v, lens_q, dev, taps=True).items() if k in keys}
    popt = make_opt("ego4d", nms_thd=0.5, eval_split_name="test", topk_window=6, eval_bsz=8)
    ann, vf, qf = synth.make_dataset(popt, 24, 4, seed=41, ctx_range=(150, 400))
    (f0, p0, m0), _ = inf.predict_split(model, inf.FeatureStore(popt, ann, vf, qf), popt)
    try:
        model.set_option("general_shape", 1)
        gen = {k: v.cpu() for k, v in forward("padded", model, inp, lens_v, lens_q, dev, taps=True).items() if k in keys}
        arena = arena_forward(model, inp, lens_v, lens_q, dev)
        (f1, _, _), _ = inf.predict_split(model, inf.FeatureStore(popt, ann, vf, qf), popt)
    finally:
        model.set_option("general_shape", 0)
    for k in keys:
        assert maxdiff(gen[k], base[k]) < AB_TOL, k
    for k in ("pred_logits", "pred_spans", "saliency_scores"):
        assert torch.equal(arena[k].cpu(), gen[k]), k           # the two entries are one path
    agree = _agree(f1, f0, popt)
    assert agree >= PIPELINE_FLOOR * len(f0), agree
    again = {k: v.cpu() for k, v in forward("padded", model, inp, lens_v, lens_q, dev, taps=True).items() if k in keys}
    for k in keys:
        assert torch.equal(again[k], base[k]), k
    (f2, p2, m2), _ = inf.predict_split(model, inf.FeatureStore(popt, ann, vf, qf), popt)
    assert (f2, p2, m2) == (f0, p0, m0)


# ------------------------------------------------------------------------------------------------ invariance
def test_window_outputs_do_not_depend_on_the_batch():
    """At (128, 4): a window's outputs are bit-identical alone, inside a batch, and padded to a longer batch shape."""
    model, opt, _, _ = get_model(3, hidden_dim=128, nheads=4)
    rng = np.random.default_rng(2)
    B = 9
    lens_v = [int(x) for x in rng.integers(1, opt.max_v_l + 1, B)]
    lens_q = [int(x) for x in rng.integers(1, opt.max_q_l + 1, B)]
    inp = gi.stage_b_inputs(opt, 99, lens_v, lens_q)
    dev = _gpu()
    full = forward("padded", model, inp, lens_v, lens_q, dev)
    arena = arena_forward(model, inp, lens_v, lens_q, dev)
    for b in (0, 4, 8):
        one = dict(src_vid=inp["src_vid"][b:b + 1, :lens_v[b]], vid_mask=inp["vid_mask"][b:b + 1, :lens_v[b]],
                   src_txt=inp["src_txt"][b:b + 1, :lens_q[b]], txt_mask=inp["txt_mask"][b:b + 1, :lens_q[b]])
        o = forward("padded", model, one, [lens_v[b]], [lens_q[b]], dev)
        for k in ("pred_logits", "pred_spans"):
            assert torch.equal(o[k][0].cpu(), full[k][b].cpu()), (b, k)
            assert torch.equal(arena[k][b].cpu(), full[k][b].cpu()), (b, k)
        assert torch.equal(o["saliency_scores"][0].cpu(), full["saliency_scores"][b, :lens_v[b]].cpu())


# ------------------------------------------------------------------------------------------------ pipeline, CLI, localizer
def _ckpt(tmp_path, opt, seed):
    sdn = synth.make_state_dict(opt, seed)
    d = tmp_path / "run"
    d.mkdir()
    torch.save({"model": {k: torch.from_numpy(v) for k, v in sdn.items()}, "epoch": 1}, d / "model_best.ckpt")
    with open(d / "opt.json", "w") as f:
        json.dump({k: v for k, v in vars(opt).items() if isinstance(v, (int, float, str, bool, type(None)))}, f)
    return d, sdn


def test_pipeline_and_cli_at_128x4(tmp_path):
    """predict_split at (128, 4) against the oracle's eval_epoch (rank lists exact, kept moments within the span tolerance),
    and the inference CLI on a checkpoint whose opt.json says 128 / 4 (the command line's --hidden_dim 256 loses) writes
    what predict_split returns."""
    from cone_amd import inference as inf
    from cone_amd.model import build_model
    opt = make_opt("ego4d", nms_thd=0.5, eval_split_name="test", topk_window=5, eval_bsz=8, hidden_dim=128, nheads=4)
    ckpt_dir, sdn = _ckpt(tmp_path, opt, 8)
    model, _ = build_model(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()})
    ann, vf, qf = synth.make_dataset(opt, 17, 3, seed=19, ctx_range=(130, 400))
    store = inf.FeatureStore(opt, ann, vf, qf)
    (f1, p1, m1), info = inf.predict_split(model, store, opt)
    (fo, _, _), ranks, _ = O.eval_epoch(sdn, opt, ann, vf, qf)
    for qi, row in enumerate(ann):
        assert [w for w in info["win_idx"][qi].cpu().tolist() if w >= 0] == ranks[row["query_id"]][:5]
    agree = _agree(f1, fo, opt)
    assert agree >= PIPELINE_FLOOR * len(f1), agree
    # the CLI: annotations + features from a packed store, opt.json beside the checkpoint
    eval_path = tmp_path / "test.jsonl"
    eval_path.write_text("\n".join(json.dumps(r) for r in ann))
    packed = inf.FeatureStore(opt, ann, vf, qf, device=torch.device("cpu")).save_packed(str(tmp_path / "test.conefs"))
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    argv = ["--resume", str(ckpt_dir / "model_best.ckpt"), "--eval_split_name", "test", "--eval_path", str(eval_path),
            "--eval_id", "g", "--eval_results_dir", str(out_dir), "--packed_features", packed, "--nms_thd", "0.5",
            "--topk_window", "5", "--hidden_dim", "256", "--nheads", "8"]
    inf.start_inference(argv)
    sub = json.loads((out_dir / "inference_ego4d_test_g_preds.json").read_text())
    assert sub["results"] == json.loads(json.dumps(f1))


def test_end_to_end_matches_reference_golden_128x4(golden_dir):
    """The reference's eval_epoch at (128, 4) on a small Ego4D split (tests/golden/e2e_shape_128x4.json): rank lists exact,
    kept moments within the span tolerance of the existing end-to-end tests."""
    from cone_amd import inference as inf
    from cone_amd.model import build_model
    with open(os.path.join(golden_dir, "e2e_shape_128x4.json")) as f:
        fx = json.load(f)
    opt = make_opt(fx["preset"], nms_thd=0.5, eval_split_name="test", **fx["opt"])
    assert (opt.hidden_dim, opt.nheads) == (128, 4)
    ref_fusion = json.loads(fx["files"]["inference_ego4d_test_golden_preds.json"])["results"]
    sdn = synth.make_state_dict(opt, fx["weight_seed"])
    model, _ = build_model(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()})
    ann, vf, qf = synth.make_dataset(opt, fx["n_queries"], fx["n_videos"], seed=fx["data_seed"], ctx_range=tuple(fx["ctx_range"]))
    (fusion, _, _), info = inf.predict_split(model, inf.FeatureStore(opt, ann, vf, qf), opt)
    for qi, row in enumerate(ann):
        assert [w for w in info["win_idx"][qi].cpu().tolist() if w >= 0] == fx["ranks"][row["query_id"]][:opt.topk_window]
    key = lambda r: (r["annotation_uid"], r["query_idx"])
    fusion = sorted(json.loads(json.dumps(fusion)), key=key)
    ref_fusion = sorted(ref_fusion, key=key)
    assert [key(r) for r in fusion] == [key(r) for r in ref_fusion]
    agree = _agree(fusion, ref_fusion, opt)
    assert agree >= PIPELINE_FLOOR * len(fusion), agree


def test_localizer_at_a_new_shape():
    """CONELocalizator(hidden_dim=192, nheads=3) against oracle.localizer_predict; the hip-graph replay equals eager."""
    from cone_amd.localizator import CONELocalizator, LOCALIZER_OPT
    from types import SimpleNamespace
    kw = dict(hidden_dim=192, nheads=3)
    opt = SimpleNamespace(**dict(LOCALIZER_OPT, **kw))
    sdn = synth.make_state_dict(opt, 4)
    sd = {k: torch.from_numpy(v) for k, v in sdn.items()}
    eager, graph = CONELocalizator(state_dict=sd, **kw), CONELocalizator(state_dict=sd, hip_graph=True, **kw)
    g = torch.Generator().manual_seed(3)
    for ctx_l, lq in [(900, 9), (900, 9), (1100, 20)]:
        vid = torch.randn(ctx_l, 256, generator=g) * 2
        tok, cls = torch.randn(lq, 768, generator=g), torch.randn(256, generator=g)
        got = eager.predict_moment(vid, (tok, cls))
        assert graph.predict_moment(vid, (tok, cls)) == got
        ref = np.array(O.localizer_predict(sdn, opt, vid, tok, cls))
        got = np.array(got)
        assert got.shape == ref.shape
        assert np.abs(got[:, :2] - ref[:, :2]).max() <= 1e-4 * opt.max_v_l * opt.clip_length + 1e-4
        assert np.abs(got[:, 2] - ref[:, 2]).max() < 2e-3


def test_split_bf16_is_refused_at_a_new_shape():
    from cone_amd import _lib
    model, _, _, _ = get_model(3, hidden_dim=128, nheads=4)
    with pytest.raises(_lib.ConeHipError, match="split_bf16 needs hidden_dim 256 with 8 heads"):
        model.set_option("split_bf16", 1)
    model.set_option("split_bf16", 0)


def test_distributed_driver_single_rank_at_a_new_shape():
    """The 1-rank RCCL group's window- and query-sharded drivers reproduce the plain pipeline at (256, 16)."""
    import torch.distributed as dist
    from cone_amd import inference as inf
    from cone_amd import parallel as par
    model, _, _, _ = get_model(6, hidden_dim=256, nheads=16)
    opt = make_opt("ego4d", nms_thd=0.5, eval_split_name="test", topk_window=5, eval_bsz=4, hidden_dim=256, nheads=16)
    ann, vf, qf = synth.make_dataset(opt, 9, 3, seed=27, ctx_range=(100, 300))
    store = inf.FeatureStore(opt, ann, vf, qf)
    plain, _ = inf.predict_split(model, store, opt)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29541")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=_gpu())
    try:
        for mode in ("window", "query"):
            got, info = par.predict_split_distributed(model, store, opt, mode=mode)
            assert got == plain, mode
        dist.barrier()
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
