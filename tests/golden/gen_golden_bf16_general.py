#!/usr/bin/env python3
"""Golden fixtures of option ``general_bf16`` (the general path's bf16 GEMMs) on the two grounds the fused path's ``bf16``
fixtures do not cover: another model shape and a long window.

Runs ONLY where the reference checkout is available, next to gen_golden_bf16.py, whose ``gen`` it calls unchanged (the
reference in fp32 and under ``torch.autocast("cpu", dtype=torch.bfloat16)`` on one ragged padded batch; keys as in
``bf16_ego4d.npz``: the fp32 tensors, ``ref_autocast_err_<tensor>``, input checksum, seeds; the model options in ``meta``):

    PYTHONPATH=<reference checkout>:. PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_bf16_general.py

(from the repository root).  Writes

    bf16_shape_128x4.npz   hidden_dim 128 / 4 heads, post-norm, the batch of stageB_shape_128x4_prenorm;
    bf16_long.npz          256 / 8 at max_v_l 300 + max_q_l 20 (320 tokens: the streaming attention core), four ragged windows,
                           the first of full length; narrow feature widths and every 8th channel of memory keep it small.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden_bf16 as gb  # noqa: E402  (gen_golden's stubs + the reference modules)


def main():
    torch.manual_seed(0)
    gb.gen("bf16_shape_128x4", "ego4d", 24, [90, 45, 17, 1, 63], [12, 5, 20, 7, 17], 2, hidden_dim=128, nheads=4)
    gb.gen("bf16_long", "ego4d", 25, [300, 157, 1, 222], [20, 7, 13, 3], 8, max_v_l=300, max_q_l=20,
           v_motion_feat_dim=64, v_appear_feat_dim=64, t_feat_dim=64)


if __name__ == "__main__":
    main()
