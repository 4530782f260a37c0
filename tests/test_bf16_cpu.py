"""Option ``bf16`` (plain-bf16 layer tails), the parts that need no GPU: the fixtures made by
tests/golden/gen_golden_bf16.py, the command line, the header."""
import json
import os

import numpy as np
import pytest
import torch

import inputs as gi
from cone_amd import synth
from cone_amd.config import build_parser, make_opt, parse_test_options
from oracle import cone_oracle as O

TOL = 1e-4
FIXTURES = ["bf16_ego4d", "bf16_ego4d_prenorm", "bf16_mad"]
TENSORS = ("pred_logits", "pred_spans", "saliency_scores", "hs", "memory", "matching")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", FIXTURES)
def test_bf16_fixture_is_reproducible_and_matches_the_oracle(golden_dir, name):
    """Weights and inputs regenerate from the stored seeds (checksums), the oracle reproduces the reference's fp32 tensors
    within 1e-4, and every tensor carries a positive autocast yardstick."""
    fx = np.load(os.path.join(golden_dir, name + ".npz"))
    opt = make_opt(str(fx["preset"]), pre_norm="pre_norm" in fx.files)
    sd = synth.make_state_dict(opt, int(fx["weight_seed"]))
    assert synth.state_dict_checksum(sd) == str(fx["weight_checksum"])
    sd = O.as_torch_sd(sd)
    lens_v, lens_q = fx["lens_v"].tolist(), fx["lens_q"].tolist()
    assert len(lens_v) >= 16
    inp = gi.stage_b_inputs(opt, int(fx["input_seed"]), lens_v, lens_q)
    assert gi.checksum(inp["src_vid"], inp["src_txt"], inp["src_cls_txt"]) == str(fx["input_checksum"])
    t = torch.from_numpy
    with torch.no_grad():
        out = O.cone_forward(sd, opt, t(inp["src_txt"]), t(inp["txt_mask"]), t(inp["src_vid"]), t(inp["vid_mask"]),
                             return_intermediates=True)
        match = O.clip_matching(sd, opt, t(inp["src_cls_txt"]), t(inp["src_vid"]), t(inp["vid_mask"]), out["pred_spans"])
    st = int(fx["mem_stride"])
    got = dict(pred_logits=out["pred_logits"], pred_spans=out["pred_spans"], saliency_scores=out["saliency_scores"],
               hs=out["hs"], memory=out["memory"][..., ::st], matching=match)
    for k in TENSORS:
        assert np.abs(got[k].numpy() - fx[k]).max() < TOL, k
        e = float(fx["ref_autocast_err_" + k])
        assert 1e-4 < e < 2.0, (k, e)       # a bf16 run of this model: far above fp32 noise, far below the values' scale


def test_bf16_flag_parses_and_opt_json_cannot_set_it(tmp_path):
    p = build_parser()
    assert p.parse_args([]).bf16 is False
    assert p.parse_args(["--bf16"]).bf16 is True
    with open(tmp_path / "opt.json", "w") as f:
        json.dump(dict(bf16=True, split_bf16=True, hidden_dim=256), f)
    ck = str(tmp_path / "model.ckpt")
    opt = parse_test_options(["--resume", ck])
    assert opt.bf16 is False and opt.split_bf16 is False
    assert parse_test_options(["--resume", ck, "--bf16"]).bf16 is True


def test_bf16_with_split_bf16_is_rejected_by_setup_model(monkeypatch, tmp_path):
    """``--bf16 --split_bf16``: setup_model hands both to the handle and the library's refusal (which names both options)
    ends the run before any evaluation.  Here the handle is a stand-in that applies the library's rule."""
    from cone_amd import inference as inf

    class Handle:
        def __init__(self):
            self.o = {}

        def load_state_dict(self, sd):
            pass

        def set_option(self, name, value):
            other = {"bf16": "split_bf16", "split_bf16": "bf16"}[name]
            if value and self.o.get(other):
                raise RuntimeError(f"set_option: {name} = 1 while {other} = 1: the two modes exclude each other")
            self.o[name] = value

    monkeypatch.setattr(inf, "build_model", lambda opt: (Handle(), None))
    monkeypatch.setattr(inf.torch, "load", lambda *a, **k: {"model": {}})
    opt = build_parser().parse_args(["--bf16", "--split_bf16", "--resume", "x.ckpt"])
    with pytest.raises(RuntimeError, match="bf16 = 1 while split_bf16 = 1"):
        inf.setup_model(opt)
    opt = build_parser().parse_args(["--bf16", "--resume", "x.ckpt"])
    model = inf.setup_model(opt)[0]
    assert model.o == {"bf16": 1}


def test_header_documents_bf16():
    with open(os.path.join(ROOT, "include", "cone_hip.h")) as f:
        h = f.read()
    assert '"bf16" (default 0, OPT-IN' in h
    assert "CONE_HIP_ABI_VERSION 8" in h.replace("  ", " ")
