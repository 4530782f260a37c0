#!/usr/bin/env python
"""Digest of cone_forward_packed over the matrix of layer-tail forms: run it on two builds, diff the outputs.

For each cell -- {post-norm, pre-norm} x numeric mode {fp32, split_bf16, bf16} x ffn_fused {2, 1, 0} x ffn_spread {1, 0} x
qkv_fused {0, 1, 2} x batch size x {layer-0 caches, none} x general_shape {0, 1} -- one seeded batch goes through
cone_forward_packed with every tap; the line printed is a SHA-256 of pred_logits | pred_spans | saliency | memory | hs |
aux_logits | aux_spans and of the sequence of (kind, a, b, c) of the launch records (cone_prof_*; times dropped).  A cell
the library refuses prints the refusal text instead.  Only the C ABI is used, so the same file runs on any commit:

    python tools/forward_digest.py > profiles/forward_digest_<commit>.txt       # once per build, then diff the two files

The batch sizes land in the four forms of the exact-fp32 tail (thresholds of ffn.hip / ffn_wide.hip at 256 CUs): 4 windows
(440 token rows: spread), 40 (4 400: wide), 128 (14 080: 64-row tiles, 2 * tiles128 <= n_cu), 300 (33 000: one full round of
128-row tiles + a wide remainder).  --launches prints the launch sequences in full.
"""
import argparse
import ctypes as C
import hashlib
import itertools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cone_amd import _lib, synth                         # noqa: E402
from cone_amd.config import make_opt                     # noqa: E402
from cone_amd.model import build_model                   # noqa: E402

LV, LQ = 90, 20
SIZES = (4, 40, 128, 300)
MODES = ("fp32", "split_bf16", "bf16")


def batch(B, d, dev):
    """B windows over a clip arena and a token arena of projected rows (a query's windows share its tokens)."""
    g = torch.Generator().manual_seed(1000 + B)
    vlen = torch.randint(LV // 2, LV + 1, (B,), generator=g, dtype=torch.int32)
    vrow0 = (torch.cumsum(vlen, 0) - vlen).to(torch.int32)
    n_q = (B + 3) // 4
    q_len = torch.randint(3, LQ + 1, (n_q,), generator=g, dtype=torch.int32)
    q_row0 = (torch.cumsum(q_len, 0) - q_len).to(torch.int32)
    qi = torch.arange(B) // 4
    vproj = torch.randn(int(vlen.sum()), d, generator=g)
    tproj = torch.randn(int(q_len.sum()), d, generator=g)
    return [t.to(dev) for t in (vproj, vrow0, vlen, tproj, q_row0[qi].contiguous(), q_len[qi].contiguous())]


def forward(model, b, caches):
    lib, h = _lib.load(), model._h()
    vproj, vrow0, vlen, tproj, trow0, qlen = b
    B, dev, d = vrow0.shape[0], vproj.device, model.hidden_dim
    nq, nd = model.num_queries, model.args.dec_layers
    keep = []
    l0p = None
    if caches:
        keep = [model.layer0_rows(vproj), model.layer0_rows(tproj)]
        l0s = _lib.Layer0(keep[0].data_ptr(), keep[1].data_ptr(), None, None, LV, None, None, 0)
        l0p = C.byref(l0s)
    out = dict(pred_logits=torch.zeros(B, nq, 2, device=dev), pred_spans=torch.zeros(B, nq, 2, device=dev),
               saliency=torch.zeros(B, LV, device=dev), memory=torch.zeros(B, LV + LQ, d, device=dev),
               hs=torch.zeros(nd, B, nq, d, device=dev), aux_logits=torch.zeros(max(nd - 1, 1), B, nq, 2, device=dev),
               aux_spans=torch.zeros(max(nd - 1, 1), B, nq, 2, device=dev))
    t = _lib.Taps()
    t.memory, t.hs = out["memory"].data_ptr(), out["hs"].data_ptr()
    t.aux_logits, t.aux_spans = out["aux_logits"].data_ptr(), out["aux_spans"].data_ptr()
    ws = model._ws.get(lib.cone_forward_packed_workspace(h, B, LV, LQ, l0p), dev)
    i32 = torch.int32
    torch.cuda.synchronize()
    lib.cone_prof_enable(1)
    try:
        _lib.check(lib.cone_forward_packed(h, _lib.ptr(vproj), _lib.ptr(vrow0, i32), _lib.ptr(vlen, i32), _lib.ptr(tproj),
                                           _lib.ptr(trow0, i32), _lib.ptr(qlen, i32), B, LV, LQ, _lib.ptr(out["pred_logits"]),
                                           _lib.ptr(out["pred_spans"]), _lib.ptr(out["saliency"]), C.byref(t), l0p, _lib.ptr(ws),
                                           ws.numel(), _lib.stream()))
        torch.cuda.synchronize()
        rec = np.zeros((4096, 5), dtype=np.float64)
        n = lib.cone_prof_collect(rec.ctypes.data, 4096)
    finally:
        lib.cone_prof_enable(0)
    sha = hashlib.sha256()
    for k in ("pred_logits", "pred_spans", "saliency", "memory", "hs", "aux_logits", "aux_spans"):
        sha.update(out[k].cpu().numpy().tobytes())
    return sha.hexdigest(), [tuple(int(x) for x in r[:4]) for r in rec[:n]]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", action="store_true", help="print every cell's launch sequence, not only its hash")
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    batches = {B: batch(B, 256, dev) for B in a.sizes}
    for pre in (False, True):
        opt = make_opt("ego4d", **({"pre_norm": True} if pre else {}))
        model, _ = build_model(opt)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(opt, 7).items()})
        model.to(dev)
        for mode, ff, spread, qkv, B, caches, gen in itertools.product(MODES, (2, 1, 0), (1, 0), (0, 1, 2), a.sizes, (1, 0), (0, 1)):
            cell = (f"{'pre' if pre else 'post'}-norm {mode:10s} ffn_fused={ff} ffn_spread={spread} qkv_fused={qkv} B={B:<3d} "
                    f"caches={caches} general_shape={gen}")
            try:
                model.set_option("split_bf16", 0).set_option("bf16", 0)
                if mode != "fp32":
                    model.set_option(mode, 1)
                model.set_option("ffn_fused", ff).set_option("ffn_spread", spread).set_option("qkv_fused", qkv)
                model.set_option("general_shape", gen)
                digest, launches = forward(model, batches[B], caches)
            except _lib.ConeHipError as e:
                print(f"{cell}  REFUSED: {e}")
                continue
            lsha = hashlib.sha256(repr(launches).encode()).hexdigest()[:16]
            print(f"{cell}  out={digest[:32]}  launches={len(launches)}:{lsha}")
            if a.launches:
                print("    " + " ".join("%d(%d,%d,%d)" % r for r in launches))


if __name__ == "__main__":
    main()
