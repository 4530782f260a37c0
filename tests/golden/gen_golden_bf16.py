#!/usr/bin/env python3
"""Golden fixtures of option ``bf16``: the REFERENCE's fp32 outputs and the reference's OWN bf16-autocast error.

Runs ONLY where the reference checkout is available, next to gen_golden.py, whose helpers it imports (``ref_opt``,
``ref_model``); gen_golden.py itself is unchanged:

    PYTHONPATH=<reference checkout>:. PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_bf16.py

(from the repository root).

Per configuration the unmodified reference model runs twice on one ragged padded batch of 16 windows: in fp32, and under
``torch.autocast("cpu", dtype=torch.bfloat16)``.  Stored: seeds and checksums of weights and inputs, the fp32 outputs
(``pred_logits``, ``pred_spans``, ``saliency_scores``, ``hs``, ``memory`` on every ``mem_stride``-th channel, ``matching``)
and, per tensor, ``ref_autocast_err_<tensor>`` = max |autocast - fp32| over the valid entries: the yardstick the mode's
own error is held against (tests/test_bf16_gpu.py).
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

TENSORS = ("pred_logits", "pred_spans", "saliency_scores", "hs", "memory", "matching")


def run_ref(model, inp, autocast):
    cap = {}
    h1 = model.transformer.encoder.register_forward_hook(lambda m, i, o: cap.__setitem__("memory", o))
    h2 = model.transformer.decoder.register_forward_hook(lambda m, i, o: cap.__setitem__("hs", o))
    t = lambda a: torch.from_numpy(a)
    vid, txt, vmask, tmask, cls = (inp[k] for k in ("src_vid", "src_txt", "vid_mask", "txt_mask", "src_cls_txt"))
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        out = model(t(txt), t(tmask), t(vid), t(vmask))
        match = model.forward_clip_matching(t(cls), t(vid), t(vmask), proposal=out["pred_spans"].float())
    h1.remove(); h2.remove()
    f = lambda x: x.detach().float().numpy()
    return dict(pred_logits=f(out["pred_logits"]), pred_spans=f(out["pred_spans"]), saliency_scores=f(out["saliency_scores"]),
                matching=f(match), memory=f(cap["memory"].transpose(0, 1)), hs=f(cap["hs"].permute(0, 2, 1, 3)))


def gen(name, preset, seed, lens_v, lens_q, mem_stride, **opt_kw):
    opt = gg.ref_opt(preset, **opt_kw)
    model, cks = gg.ref_model(opt, seed)
    inp = gi.stage_b_inputs(opt, 1000 + seed, lens_v, lens_q)
    ref, ac = run_ref(model, inp, False), run_ref(model, inp, True)
    B, Lv, Lq = len(lens_v), max(lens_v), max(lens_q)
    vmask = np.zeros((B, Lv + Lq), bool)
    for b in range(B):
        vmask[b, :lens_v[b]] = True
        vmask[b, Lv:Lv + lens_q[b]] = True
    valid = dict(memory=vmask, saliency_scores=vmask[:, :Lv])
    errs = {}
    for k in TENSORS:
        d = np.abs(ac[k] - ref[k])
        errs[k] = float(d[valid[k]].max() if k in valid else d.max())
    ref["memory"] = np.ascontiguousarray(ref["memory"][..., ::mem_stride])
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(
        path, meta=json.dumps(dict(preset=preset, opt=opt_kw)), preset=preset, weight_seed=seed, weight_checksum=cks,
        input_seed=1000 + seed, **({"pre_norm": 1} if opt_kw.get("pre_norm") else {}),
        lens_v=np.array(lens_v), lens_q=np.array(lens_q),
        input_checksum=gi.checksum(inp["src_vid"], inp["src_txt"], inp["src_cls_txt"]), mem_stride=mem_stride,
        **ref, **{"ref_autocast_err_" + k: np.float64(v) for k, v in errs.items()})
    print("wrote", name, os.path.getsize(path), {k: round(v, 5) for k, v in errs.items()})


def main():
    torch.manual_seed(0)
    lv = [90, 45, 17, 1, 63, 88, 30, 72, 5, 90, 54, 12, 81, 66, 23, 39]
    lq = [12, 5, 20, 7, 17, 9, 3, 14, 20, 1, 8, 11, 6, 16, 10, 13]
    gen("bf16_ego4d", "ego4d", 21, lv, lq, 4)
    gen("bf16_ego4d_prenorm", "ego4d", 22, lv, lq, 4, pre_norm=True)
    lvm = [125, 60, 17, 1, 99, 120, 30, 72, 5, 125, 54, 12, 81, 110, 23, 39]
    lqm = [12, 5, 25, 7, 17, 9, 3, 14, 20, 1, 8, 11, 6, 16, 10, 13]
    gen("bf16_mad", "mad", 23, lvm, lqm, 4)


if __name__ == "__main__":
    main()
