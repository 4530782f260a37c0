#!/usr/bin/env python3
"""Golden fixtures of the general-shape path (hidden_dim / nheads other than 256 / 8), made by the REFERENCE itself.

Runs ONLY where the reference checkout is available, next to gen_golden.py, whose helpers it imports (``ref_opt``, ``ref_model``, the
in-memory datasets, ``gen_e2e``); gen_golden.py itself is unchanged:

    PYTHONPATH=<reference checkout>:. PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_shapes.py

(from the repository root).

gen_stage_b does not record the model shape, so the stage-B fixtures here are written by their own function: the same
outputs plus ``hidden_dim`` / ``nheads`` and a ``meta`` JSON string with the preset and the reference options.  memory is
stored on every ``mem_stride``-th channel (valid rows compared only), to keep each file under ~600 KB.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as gg  # noqa: E402  (stubs + the reference modules)
import inputs as gi  # noqa: E402


def gen_stage_b_shape(name, preset, seed, lens_v, lens_q, mem_stride, **opt_kw):
    """CONE.forward + forward_clip_matching of the unmodified reference on one ragged padded batch at a model shape."""
    opt = gg.ref_opt(preset, **opt_kw)
    model, cks = gg.ref_model(opt, seed)
    inp = gi.stage_b_inputs(opt, 1000 + seed, lens_v, lens_q)
    vid, txt, vmask, tmask, cls = (inp[k] for k in ("src_vid", "src_txt", "vid_mask", "txt_mask", "src_cls_txt"))
    cap = {}
    model.transformer.encoder.register_forward_hook(lambda m, i, o: cap.__setitem__("memory", o))
    model.transformer.decoder.register_forward_hook(lambda m, i, o: cap.__setitem__("hs", o))
    with torch.no_grad():
        t = lambda a: torch.from_numpy(a)
        out = model(t(txt), t(tmask), t(vid), t(vmask))
        match = model.forward_clip_matching(t(cls), t(vid), t(vmask), proposal=out["pred_spans"])
    np.savez_compressed(
        os.path.join(HERE, name + ".npz"),
        meta=json.dumps(dict(preset=preset, opt=opt_kw)), hidden_dim=opt.hidden_dim, nheads=opt.nheads,
        weight_seed=seed, weight_checksum=cks, input_seed=1000 + seed,
        lens_v=np.array(lens_v), lens_q=np.array(lens_q), input_checksum=gi.checksum(vid, txt, cls),
        pred_logits=out["pred_logits"].numpy(), pred_spans=out["pred_spans"].numpy(),
        saliency_scores=out["saliency_scores"].numpy(), matching=match.numpy(),
        aux_pred_logits=out["aux_outputs"][0]["pred_logits"].numpy(),
        aux_pred_spans=out["aux_outputs"][0]["pred_spans"].numpy(),
        mem_stride=mem_stride, memory=np.ascontiguousarray(cap["memory"].transpose(0, 1).numpy()[..., ::mem_stride]),
        hs=cap["hs"].permute(0, 2, 1, 3).numpy(),                  # (layers, B, Nq, d)
    )
    print("wrote", name, os.path.getsize(os.path.join(HERE, name + ".npz")))


def main():
    torch.manual_seed(0)
    gen_stage_b_shape("stageB_shape_128x4_prenorm", "ego4d", 11, [90, 45, 17, 1, 63], [12, 5, 20, 7, 17], 2,
                      hidden_dim=128, nheads=4, pre_norm=True)
    gen_stage_b_shape("stageB_shape_256x16_prenorm", "ego4d", 12, [60, 33, 1, 48], [12, 5, 9, 17], 4,
                      hidden_dim=256, nheads=16, pre_norm=True)
    gen_stage_b_shape("stageB_shape_512x8_prenorm", "ego4d", 13, [40, 21, 1, 33], [9, 5, 3, 11], 8,
                      hidden_dim=512, nheads=8, pre_norm=True, dim_feedforward=1024)
    gg.gen_e2e("e2e_shape_128x4", "ego4d", 14, 10, 3, (100, 330), hidden_dim=128, nheads=4, eval_bsz=4, topk_window=4)


if __name__ == "__main__":
    main()
