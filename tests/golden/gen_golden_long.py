#!/usr/bin/env python3
"""Golden fixture of a window longer than 256 tokens, made by the REFERENCE itself.

Every other stage-B fixture is at most 256 tokens (clips + words) per window; this one pins the reference at
``max_v_l = 300``, ``max_q_l = 20`` (320 tokens: the general path with the streaming attention core).  Runs ONLY where the
reference checkout is available, next to gen_golden.py / gen_golden_shapes.py, whose helpers it imports unchanged:

    PYTHONPATH=<reference checkout>:. PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_long.py

(from the repository root).  Writes ``stageB_long.npz`` in the layout of gen_golden_shapes.gen_stage_b_shape: seeds and a
checksum for the inputs, the reference's own output tensors.  Narrow feature widths (64 / 64) and every 8th channel of
memory keep the file small.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden_shapes as gs  # noqa: E402  (gen_golden's stubs + the reference modules)


def main():
    torch.manual_seed(0)
    gs.gen_stage_b_shape("stageB_long", "ego4d", 21, [300, 157, 1], [20, 7, 13], 8, max_v_l=300, max_q_l=20,
                         v_motion_feat_dim=64, v_appear_feat_dim=64, t_feat_dim=64)


if __name__ == "__main__":
    main()
