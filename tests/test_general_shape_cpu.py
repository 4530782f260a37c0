"""hidden_dim / nheads other than 256 / 8 without a GPU: the oracle against the reference's fixtures at the new shapes
(tests/golden/gen_golden_shapes.py), the state-dict layout at the new widths, and the shape check on the host and in
cone_model_create.  CPU only."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import inputs as gi
from cone_amd import synth
from cone_amd.config import SUPPORTED_SHAPES, check_model_shape, make_opt
from oracle import cone_oracle as O

TOL = 1e-4

SUPPORTED = [(64, 4), (64, 1), (128, 4), (128, 8), (192, 3), (256, 4), (256, 8), (256, 16), (384, 6), (512, 8), (512, 16),
             (512, 32), (320, 5)]
UNSUPPORTED = [(128, 1), (512, 4), (256, 32), (100, 4), (576, 9), (32, 2), (192, 4), (256, 0), (640, 10)]


@pytest.mark.parametrize("name", ["stageB_shape_128x4_prenorm", "stageB_shape_256x16_prenorm", "stageB_shape_512x8_prenorm"])
def test_oracle_reproduces_shape_fixtures(golden_dir, name):
    fx = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(fx["meta"]))
    opt = make_opt(meta["preset"], **meta["opt"])
    assert (opt.hidden_dim, opt.nheads) == (int(fx["hidden_dim"]), int(fx["nheads"]))
    sdn = synth.make_state_dict(opt, int(fx["weight_seed"]))
    assert synth.state_dict_checksum(sdn) == str(fx["weight_checksum"])
    sd = O.as_torch_sd(sdn)
    lens_v, lens_q = fx["lens_v"].tolist(), fx["lens_q"].tolist()
    inp = gi.stage_b_inputs(opt, int(fx["input_seed"]), lens_v, lens_q)
    assert gi.checksum(inp["src_vid"], inp["src_txt"], inp["src_cls_txt"]) == str(fx["input_checksum"])
    t = torch.from_numpy
    with torch.no_grad():
        out = O.cone_forward(sd, opt, t(inp["src_txt"]), t(inp["txt_mask"]), t(inp["src_vid"]), t(inp["vid_mask"]),
                             return_intermediates=True)
        match = O.clip_matching(sd, opt, t(inp["src_cls_txt"]), t(inp["src_vid"]), t(inp["vid_mask"]), out["pred_spans"])
    d = lambda a, b: float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
    assert d(out["pred_logits"], fx["pred_logits"]) < TOL
    assert d(out["pred_spans"], fx["pred_spans"]) < TOL
    assert d(out["aux_outputs"][0]["pred_logits"], fx["aux_pred_logits"]) < TOL
    assert d(out["aux_outputs"][0]["pred_spans"], fx["aux_pred_spans"]) < TOL
    Lv = inp["src_vid"].shape[1]
    for b, v in enumerate(lens_v):
        assert d(out["saliency_scores"][b, :v], fx["saliency_scores"][b, :v]) < TOL
    assert d(match, fx["matching"]) < TOL
    assert d(out["hs"], fx["hs"]) < TOL
    st = int(fx["mem_stride"])
    mem = out["memory"].numpy()[..., ::st]
    for b, (v, q) in enumerate(zip(lens_v, lens_q)):
        assert d(mem[b, :v], fx["memory"][b, :v]) < TOL
        assert d(mem[b, Lv:Lv + q], fx["memory"][b, Lv:Lv + q]) < TOL


def test_oracle_reproduces_shape_end_to_end_fixture(golden_dir):
    with open(os.path.join(golden_dir, "e2e_shape_128x4.json")) as f:
        fx = json.load(f)
    opt = make_opt(fx["preset"], nms_thd=0.5, eval_split_name="test", save_all=True, **fx["opt"])
    assert (opt.hidden_dim, opt.nheads) == (128, 4)
    sd = synth.make_state_dict(opt, fx["weight_seed"])
    assert synth.state_dict_checksum(sd) == fx["weight_checksum"]
    ann, vf, qf = synth.make_dataset(opt, fx["n_queries"], fx["n_videos"], seed=fx["data_seed"], ctx_range=tuple(fx["ctx_range"]))
    _, ranks, mr = O.eval_epoch(sd, opt, ann, vf, qf)
    assert dict(ranks) == fx["ranks"]
    assert len(mr) == len(fx["mr_res"])
    worst = 0.0
    for a, b in zip(mr, fx["mr_res"]):
        assert a["query_id"] == b["query_id"] and a["clip_id"] == b["clip_id"]
        worst = max(worst, np.abs(np.array(a["pred_relevant_windows"]) - np.array(b["pred_relevant_windows"])).max())
    assert worst <= 1.01e-4, worst


@pytest.mark.parametrize("d,h", [(64, 4), (128, 4), (192, 3), (512, 16)])
def test_state_dict_spec_at_new_widths(d, h):
    opt = make_opt("ego4d", hidden_dim=d, nheads=h, dim_feedforward=512, use_txt_pos=True, pre_norm=True)
    spec = synth.state_dict_spec(opt)
    assert spec["transformer.encoder.layers.0.self_attn.in_proj_weight"] == (3 * d, d)
    assert spec["transformer.encoder.layers.1.linear1.weight"] == (512, d)
    assert spec["transformer.decoder.layers.1.multihead_attn.out_proj.weight"] == (d, d)
    assert spec["query_embed.weight"] == (opt.num_queries, d)
    assert spec["input_vid_proj.0.net.1.weight"] == (d, opt.v_motion_feat_dim)
    assert spec["input_txt_proj.1.net.1.weight"] == (d, d)
    assert spec["adapter_layer.layers.0.weight"] == (d, opt.v_appear_feat_dim)
    assert spec["span_embed.layers.2.weight"] == (2, d)
    assert spec["transformer.encoder.norm.weight"] == (d,)
    assert spec["txt_position_embed.position_embeddings.weight"] == (opt.max_q_l, d)
    sd = synth.make_state_dict(opt, 0)
    assert all(tuple(sd[k].shape) == tuple(v) for k, v in spec.items())


@pytest.mark.parametrize("d,h", SUPPORTED)
def test_host_shape_check_accepts_the_supported_set(d, h):
    check_model_shape(d, h)
    from cone_amd.model import build_model
    model, _ = build_model(make_opt("ego4d", hidden_dim=d, nheads=h))       # no GPU work until load_state_dict
    assert model.hidden_dim == d


@pytest.mark.parametrize("d,h", UNSUPPORTED)
def test_host_shape_check_rejects_other_shapes(d, h):
    with pytest.raises(ValueError, match="supported are hidden_dim a multiple of 64") as ei:
        check_model_shape(d, h)
    assert SUPPORTED_SHAPES in str(ei.value) and f"hidden_dim={d} nheads={h}" in str(ei.value)
    from cone_amd.model import build_model
    with pytest.raises(ValueError, match="unsupported model shape"):
        build_model(make_opt("ego4d", hidden_dim=d, nheads=h))


def _create(lib, _lib, d, h):
    w = _lib.Weights()          # every weight pointer NULL
    w.hidden_dim, w.nheads, w.dim_ff, w.enc_layers, w.dec_layers, w.num_queries = d, h, 1024, 2, 2, 5
    w.n_input_proj, w.t_dim, w.v_dim, w.v_motion_dim, w.has_adapter = 2, 768, 256, 256, 1
    handle = C.c_void_p()
    rc = lib.cone_model_create(C.byref(w), C.byref(handle))
    return rc, lib.cone_last_error().decode(), handle


@pytest.mark.parametrize("d,h", SUPPORTED[:6] + UNSUPPORTED[:5])
def test_model_create_checks_the_shape_before_any_hip_call(d, h):
    """cone_model_create with null weight pointers: a supported shape gets as far as the weight check ("a required weight
    pointer is null"), any other shape stops at the shape check with a message that names the supported set.  Both answers
    come before the first HIP call of the function (its first is the arena's hipMalloc: on a machine without a GPU that
    would answer CONE_E_HIP instead)."""
    from cone_amd import _lib
    lib = _lib.load()
    rc, msg, handle = _create(lib, _lib, d, h)
    assert rc == -1 and not handle.value
    ok = (64 <= d <= 512 and d % 64 == 0 and h > 0 and d % h == 0 and d // h in (16, 32, 64))
    if ok:
        assert "a required weight pointer is null" in msg, msg
    else:
        assert f"unsupported model shape hidden_dim={d} nheads={h}" in msg, msg
        assert "hidden_dim a multiple of 64 in [64, 512] with head_dim = hidden_dim / nheads in {16, 32, 64}" in msg, msg
