"""Option ``general_bf16`` without a GPU: the CLI flag and its forwarding, the new fixtures' input checksums, the header."""
import json
import os
import re

import numpy as np
import pytest

import inputs as gi
from cone_amd import config
from cone_amd.config import make_opt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_exists_and_is_forwarded_from_the_command_line():
    p = config.build_parser()
    assert p.parse_args([]).general_bf16 is False
    assert p.parse_args(["--general_bf16"]).general_bf16 is True
    assert "general_bf16" in config.CLI_WINS            # the command line's value wins over the checkpoint's opt.json
    help_text = " ".join(p.format_help().split())
    assert "NOT fp32-accurate" in help_text[help_text.rindex("--general_bf16"):help_text.rindex("--gpus")]


def test_flag_survives_the_opt_json_round_trip(tmp_path):
    with open(tmp_path / "opt.json", "w") as f:
        json.dump(dict(hidden_dim=128, nheads=4, general_bf16=False), f)
    opt = config.parse_test_options(["--resume", str(tmp_path / "model.ckpt"), "--general_bf16"])
    assert opt.general_bf16 is True and opt.hidden_dim == 128


@pytest.mark.parametrize("name", ["bf16_shape_128x4", "bf16_long"])
def test_new_fixtures_inputs_regenerate_from_their_seeds(golden_dir, name):
    fx = np.load(os.path.join(golden_dir, name + ".npz"))
    meta = json.loads(str(fx["meta"]))
    opt = make_opt(meta["preset"], **meta["opt"])
    inp = gi.stage_b_inputs(opt, int(fx["input_seed"]), fx["lens_v"].tolist(), fx["lens_q"].tolist())
    assert gi.checksum(inp["src_vid"], inp["src_txt"], inp["src_cls_txt"]) == str(fx["input_checksum"])
    for k in ("pred_logits", "pred_spans", "saliency_scores", "hs", "memory", "matching"):
        assert k in fx.files and float(fx["ref_autocast_err_" + k]) > 0
    assert os.path.getsize(os.path.join(golden_dir, name + ".npz")) < 1 << 20
    if name == "bf16_long":
        assert int(fx["lens_v"][0]) + int(fx["lens_q"][0]) == opt.max_v_l + opt.max_q_l == 320


def test_header_declares_the_new_symbols_and_the_option():
    with open(os.path.join(ROOT, "include", "cone_hip.h")) as f:
        h = f.read()
    assert re.search(r"\bint\s+cone_test_gemm_bf16\s*\(", h)
    assert re.search(r"\bsize_t\s+cone_test_gemm_bf16_image_bytes\s*\(\s*int\s+N\s*,\s*int\s+K\s*\)", h)
    assert '"general_bf16"' in h and "NOT fp32-accurate" in h
    from cone_amd import _lib
    assert {"cone_test_gemm_bf16", "cone_test_gemm_bf16_image_bytes"} <= set(_lib.EXPORTS)
