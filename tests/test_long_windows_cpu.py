"""Windows of more than 256 tokens without a GPU: the header's new limit and option, the host's argument handling, and the
oracle against the reference's own outputs at 300 clips + 20 words (tests/golden/gen_golden_long.py -> stageB_long.npz;
every other fixture is at most 256 tokens).  CPU only."""
import json
import os
import re

import numpy as np
import pytest
import torch

import inputs as gi
from cone_amd import synth
from cone_amd.config import MAX_LONG_WINDOW_TOKENS, MAX_WINDOW_TOKENS, make_opt, window_token_limit
from oracle import cone_oracle as O

TOL = 2e-5      # tests/test_oracle_golden.py: same torch build on both sides, differences are only op-fusion order
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "cone_hip.h")) as f:
        return f.read()


def test_header_defines_the_long_window_limit():
    h = _header()
    assert re.search(r"^#define\s+CONE_MAX_LONG_WINDOW_TOKENS\s+1024\b", h, re.M)
    assert re.search(r"^#define\s+CONE_MAX_WINDOW_TOKENS\s+256\b", h, re.M)         # (unchanged)
    assert (MAX_WINDOW_TOKENS, MAX_LONG_WINDOW_TOKENS) == (256, 1024)


def test_option_is_in_the_documented_option_list():
    """The comment block ahead of cone_model_set_option lists every option as ``"name" (default ...)``."""
    h = _header()
    doc = h[:h.index("int cone_model_set_option(")]
    doc = doc[doc.rindex("/*"):]
    names = re.findall(r'^ \* "(\w+)" \(default', doc, re.M)
    assert "dec_fold" in names and "bf16" in names          # (the pattern really finds the list)
    assert "max_window_tokens" in names
    assert "CONE_MAX_LONG_WINDOW_TOKENS" in doc


@pytest.mark.parametrize("v,q,want", [(90, 20, 256), (125, 25, 256), (230, 26, 256), (240, 17, 257), (300, 20, 320), (992, 32, 1024),
                                      (1000, 24, 1024), (0, 0, 256)])
def test_window_token_limit(v, q, want):
    assert window_token_limit(v, q) == want


@pytest.mark.parametrize("v,q", [(1000, 64), (993, 32), (1025, 0), (2000, 20)])
def test_window_token_limit_refuses_more_than_1024(v, q):
    with pytest.raises(ValueError) as ei:
        window_token_limit(v, q)
    assert f"max_v_l={v}" in str(ei.value) and f"max_q_l={q}" in str(ei.value) and "1024" in str(ei.value)


def test_build_model_takes_long_window_args_and_refuses_too_long_ones_before_gpu_work():
    from cone_amd.model import build_model
    model, _ = build_model(make_opt("ego4d", max_v_l=400, max_q_l=20))      # no GPU work until load_state_dict
    assert not model.long_windows                                           # (nothing loaded yet: the default)
    opt = make_opt("ego4d", max_v_l=1000, max_q_l=64)
    model, _ = build_model(opt)
    with pytest.raises(ValueError, match="max_v_l=1000") as ei:             # ahead of the library load and of the GPU check
        model.load_state_dict({})
    assert "max_q_l=64" in str(ei.value)


def test_oracle_reproduces_the_long_window_fixture(golden_dir):
    fx = np.load(os.path.join(golden_dir, "stageB_long.npz"), allow_pickle=False)
    meta = json.loads(str(fx["meta"]))
    opt = make_opt(meta["preset"], **meta["opt"])
    assert (opt.max_v_l, opt.max_q_l) == (300, 20) and opt.max_v_l + opt.max_q_l > 256
    sdn = synth.make_state_dict(opt, int(fx["weight_seed"]))
    assert synth.state_dict_checksum(sdn) == str(fx["weight_checksum"])
    sd = O.as_torch_sd(sdn)
    lens_v, lens_q = fx["lens_v"].tolist(), fx["lens_q"].tolist()
    assert lens_v[0] == 300 and lens_q[0] == 20 and len(lens_v) == 3
    inp = gi.stage_b_inputs(opt, int(fx["input_seed"]), lens_v, lens_q)
    assert gi.checksum(inp["src_vid"], inp["src_txt"], inp["src_cls_txt"]) == str(fx["input_checksum"])
    t = torch.from_numpy
    with torch.no_grad():
        out = O.cone_forward(sd, opt, t(inp["src_txt"]), t(inp["txt_mask"]), t(inp["src_vid"]), t(inp["vid_mask"]),
                             return_intermediates=True)
        match = O.clip_matching(sd, opt, t(inp["src_cls_txt"]), t(inp["src_vid"]), t(inp["vid_mask"]), out["pred_spans"])
    d = lambda a, b: float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
    errs = dict(pred_logits=d(out["pred_logits"], fx["pred_logits"]), pred_spans=d(out["pred_spans"], fx["pred_spans"]),
                aux_logits=d(out["aux_outputs"][0]["pred_logits"], fx["aux_pred_logits"]),
                aux_spans=d(out["aux_outputs"][0]["pred_spans"], fx["aux_pred_spans"]),
                matching=d(match, fx["matching"]), hs=d(out["hs"], fx["hs"]))
    Lv = inp["src_vid"].shape[1]
    st = int(fx["mem_stride"])
    mem = out["memory"].numpy()[..., ::st]
    for b, (v, q) in enumerate(zip(lens_v, lens_q)):
        errs[f"saliency_{b}"] = d(out["saliency_scores"][b, :v], fx["saliency_scores"][b, :v])
        errs[f"memory_{b}"] = max(d(mem[b, :v], fx["memory"][b, :v]), d(mem[b, Lv:Lv + q], fx["memory"][b, Lv:Lv + q]))
    print(errs)
    assert max(errs.values()) < TOL, errs
