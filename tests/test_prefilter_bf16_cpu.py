"""The opt-in bf16 pre-filter (``--prefilter_bf16``), the parts that need no GPU: the float64 restatement of its contract,
the planted inputs of the pipeline test, the command line, the header."""
import json
import os
import re

import numpy as np
import pytest
import torch

import prefilter_bf16_ref as R
from cone_amd import synth
from cone_amd.config import build_parser, make_opt, parse_test_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cone_rows_to_bf16", "cone_adapter_norm_bf16", "cone_prefilter_scores_bf16_workspace",
               "cone_prefilter_scores_bf16", "cone_prefilter_batched_bf16")


def _bf16_by_hand(x: float) -> float:
    """fp32 -> bf16, round to nearest even, on the bit pattern (no torch.bfloat16)."""
    b = int(np.float32(x).view(np.uint32))
    b = (b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000
    return float(np.uint32(b).view(np.float32))


@pytest.mark.parametrize("W", [4, 5])
def test_restatement_agrees_with_a_direct_float64_evaluation(W):
    """A tiny case written out with Python floats: operands rounded on their bit patterns, products and sums in float64,
    the window max over the frame range itself -- and the header's half-window form gives the same windows."""
    g = torch.Generator().manual_seed(W)
    ctx, cls = torch.randn(7, 32, generator=g), torch.randn(2, 32, generator=g)
    win, ab = R.window_scores(ctx, cls, W)
    S = W // 2
    nw = -(-7 // S) + 1
    assert win.shape == (2, nw) == (2, R.num_windows(7, W))
    for q in range(2):
        b = [_bf16_by_hand(v) for v in cls[q].tolist()]
        fs = [sum(_bf16_by_hand(v) * w for v, w in zip(ctx[f].tolist(), b)) for f in range(7)]
        for i in range(nw):
            lo, hi = max((i - 1) * S, 0), min((i - 1) * S + W, 7)
            assert abs(float(win[q, i]) - max(fs[lo:hi])) <= 1e-14, (q, i)
    fs, _ = R.frame_scores(ctx, cls)
    assert torch.equal(R.window_scores_by_halves(fs, W), win)
    assert bool((ab >= win.abs()).all())
    # the rounding is visible: the unrounded scores are another set of numbers
    assert not torch.equal(R.window_scores(ctx, cls, W, rounded=False)[0], win)


def test_half_window_form_equals_the_frame_range_form_on_the_shapes_of_the_gpu_test():
    g = torch.Generator().manual_seed(1)
    for ctx_l, W in ((1, 90), (44, 90), (45, 90), (46, 90), (91, 90), (1000, 125), (1000, 2)):
        fs = torch.randn(3, ctx_l, generator=g, dtype=torch.float64)
        assert torch.equal(R.window_scores_by_halves(fs, W), R.window_reduce(fs, W)), (ctx_l, W)


def planted_split(nq=12, nv=3):
    """The inputs of the GPU pipeline test: tests/test_bf16_gpu.py:_split's synthetic split with planted clips."""
    opt = make_opt("ego4d", nms_thd=0.5, eval_split_name="test", topk_window=4, eval_bsz=4)
    ann, vf, qf = synth.make_dataset(opt, nq, nv, seed=3, ctx_range=(150, 400))
    return opt, ann, R.plant(opt, ann, vf, qf), qf


def test_planted_inputs_make_the_rank_rule_non_vacuous():
    """By the restatement alone (float64 adapter + normalisation on the synthetic weights of the GPU test's model): for at
    least half of the queries the top-1 window clears the (K+1)-th by more than 2 eps, so rule 1 of the pipeline test binds."""
    opt, ann, vf, qf = planted_split()
    sd = synth.make_state_dict(opt, 0)
    covered = 0
    for row in ann:
        ctx = torch.from_numpy(R.adapted_rows_f64(sd, vf[row["clip_id"]]))
        cls = qf[row["query_id"]]["cls_features"].astype(np.float64)
        cls = torch.from_numpy(cls / (np.linalg.norm(cls) + 1e-5))[None, :]
        win, _ = R.window_scores(ctx, cls, opt.max_v_l, rounded=False)
        covered += R.covered_top1(win[0], opt.topk_window)
    print(f"[prefilter_bf16] planted split: rule 1 covers the top-1 window of {covered} / {len(ann)} queries")
    assert covered * 2 >= len(ann), (covered, len(ann))


def test_eps_is_the_issue_s_figure():
    assert R.EPS_UNIT == 2.0 ** -8 * (1 + 2.0 ** -9) + 256 * 2.0 ** -23


def test_prefilter_bf16_flag_parses_and_opt_json_cannot_set_it(tmp_path):
    p = build_parser()
    assert p.parse_args([]).prefilter_bf16 is False
    assert p.parse_args(["--prefilter_bf16"]).prefilter_bf16 is True
    assert p.parse_args(["--prefilter_bf16"]).bf16 is False          # a switch of its own
    with open(tmp_path / "opt.json", "w") as f:
        json.dump(dict(prefilter_bf16=True, hidden_dim=256), f)
    ck = str(tmp_path / "model.ckpt")
    assert parse_test_options(["--resume", ck]).prefilter_bf16 is False
    assert parse_test_options(["--resume", ck, "--prefilter_bf16"]).prefilter_bf16 is True


def test_graph_key_and_ctx_sharded_refusal_name_the_option():
    from types import SimpleNamespace
    from cone_amd import inference as inf
    from cone_amd import parallel as par
    opt = make_opt("ego4d", topk_window=4, nms_thd=0.5)
    model = SimpleNamespace()
    k0 = inf._graph_key(model, opt)
    opt.prefilter_bf16 = True
    assert inf._graph_key(model, opt) != k0
    with pytest.raises(ValueError, match="prefilter_bf16"):
        par.prefilter_ctx_sharded(torch.zeros(4, 32), 4, torch.zeros(1, 32), 90, 2, prefilter_bf16=True)
    with pytest.raises(ValueError, match="prefilter_bf16"):
        par.prefilter_one_video_ctx_sharded(SimpleNamespace(q_vid=[0]), opt, hooks=None)


def test_header_declares_the_new_entries_and_stays_abi_8():
    from cone_amd import _lib
    with open(os.path.join(ROOT, "include", "cone_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"#define\s+CONE_HIP_ABI_VERSION\s+8\b", hdr)
    declared = set(re.findall(r"\b(cone_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS, name
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    assert "NOT fp32-accurate" in hdr
