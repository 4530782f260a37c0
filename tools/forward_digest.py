#!/usr/bin/env python
"""Digest of the forward entries over the matrix of layer-tail forms and of forward-level paths: run it on two builds, diff
the outputs.

Two sections (--sections tail forward):

tail -- {post-norm, pre-norm} x numeric mode {fp32, split_bf16, bf16} x ffn_fused {2, 1, 0} x ffn_spread {1, 0} x
qkv_fused {0, 1, 2} x batch size x {layer-0 caches, none} x general_shape {0, 1}, cone_forward_packed with every tap.

forward -- the tail options at their defaults; models {post-norm, pre-norm, --use_txt_pos}; what the cone_layer0 brings
{row caches, nothing; for --use_txt_pos also caches + txt_pos rows, txt_pos rows only}:
  * 4 windows: the full cross dec_fold 0 .. 5 x pos_tables x l0_gather x res_gather x dec0_const x rows_chain;
  * 1 and 300 windows (one window: no shared first-layer cross-attention operand; 300: the heads chain engages): each of
    those options moved alone from its default;
  * taps {all, none} x saliency {wanted, not} x dec_fold 0 .. 5 at 1, 4 and 300 windows;
  * a length bound beyond 192 tokens on paths that must refuse it;
  * the second entry, cone_forward_windows on a padded batch of the same window lengths: the full cross at 4 windows, each
    option moved alone at 1 and 300, taps x saliency at all three.

Every line carries the byte count the workspace-size entry returned, a SHA-256 of pred_logits | pred_spans | saliency |
memory | hs | aux_logits | aux_spans (buffers a cell does not ask for stay zero) and of the sequence of (kind, a, b, c) of
the launch records (cone_prof_*; times dropped).  A cell the library refuses prints the refusal text instead.  Only the C
ABI is used, so the same file runs on any commit:

    python tools/forward_digest.py > forward_digest_<commit>.txt        # once per build, then diff the two files

--summary prints one line per group of cells instead (section, model, numeric mode or entry, batch size, cone_layer0
form): the number of cells, how many were refused, and a SHA-256 over the group's full lines -- two builds agree in every
cell exactly when the summaries are equal, and the summary is what is small enough to keep under profiles/.  A group that
differs is then looked into with the full output.

The tail section's batch sizes land in the four forms of the exact-fp32 tail (thresholds of ffn.hip / ffn_wide.hip at 256
CUs): 4 windows (440 token rows: spread), 40 (4 400: wide), 128 (14 080: 64-row tiles, 2 * tiles128 <= n_cu), 300 (33 000: one
full round of 128-row tiles + a wide remainder).  --launches prints the launch sequences in full.
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


FWD_OPTS = ("dec_fold", "pos_tables", "l0_gather", "res_gather", "dec0_const", "rows_chain")
FWD_DEFAULT = dict(dec_fold=2, pos_tables=1, l0_gather=1, res_gather=1, dec0_const=1, rows_chain=1)
FWD_RANGE = dict(dec_fold=range(6), pos_tables=(1, 0), l0_gather=(1, 0), res_gather=(1, 0), dec0_const=(1, 0), rows_chain=(1, 0))


def batch(B, d, dev, opt=None):
    """B windows over a clip arena and a token arena of projected rows (a query's windows share its tokens); with opt also
    the padded raw batch of the same window lengths for cone_forward_windows."""
    g = torch.Generator().manual_seed(1000 + B)
    vlen = torch.randint(LV // 2, LV + 1, (B,), generator=g, dtype=torch.int32)
    vrow0 = (torch.cumsum(vlen, 0) - vlen).to(torch.int32)
    n_q = (B + 3) // 4
    q_len = torch.randint(3, LQ + 1, (n_q,), generator=g, dtype=torch.int32)
    q_row0 = (torch.cumsum(q_len, 0) - q_len).to(torch.int32)
    qi = torch.arange(B) // 4
    vproj = torch.randn(int(vlen.sum()), d, generator=g)
    tproj = torch.randn(int(q_len.sum()), d, generator=g)
    b = [t.to(dev) for t in (vproj, vrow0, vlen, tproj, q_row0[qi].contiguous(), q_len[qi].contiguous())]
    if opt is None:
        return b
    tok_index = torch.cat([torch.arange(int(n), dtype=torch.int32) for n in q_len])
    qlen = q_len[qi]
    vid = torch.randn(B, LV, opt.v_motion_feat_dim, generator=g) * (torch.arange(LV)[None, :] < vlen[:, None])[..., None]
    txt = torch.randn(B, LQ, opt.t_feat_dim, generator=g) * (torch.arange(LQ)[None, :] < qlen[:, None])[..., None]
    return b + [tok_index.to(dev), vid.contiguous().to(dev), txt.contiguous().to(dev)]


def forward(model, b, l0form="caches", taps=True, sal=True, entry="packed", lv=LV, lq=LQ):
    """l0form: "none", or "+"-joined of caches (row caches) and txt (the tokens' own position rows, --use_txt_pos)."""
    lib, h = _lib.load(), model._h()
    vproj, vrow0, vlen, tproj, trow0, qlen = b[:6]
    B, dev, d = vrow0.shape[0], vproj.device, model.hidden_dim
    nq, nd = model.num_queries, model.args.dec_layers
    keep = []
    l0p = None
    if entry == "packed" and l0form != "none":
        l0s = _lib.Layer0(None, None, None, None, LV, None, None, 0)
        if "caches" in l0form:
            keep += [model.layer0_rows(vproj), model.layer0_rows(tproj)]
            l0s.qkv_vid, l0s.qkv_txt = keep[0].data_ptr(), keep[1].data_ptr()
        if "txt" in l0form:
            keep += list(model.text_positions(tproj, b[6]))
            l0s.txt_pos, l0s.txt_pos_qk, l0s.n_txt = keep[-2].data_ptr(), keep[-1].data_ptr(), int(tproj.shape[0])
        l0p = C.byref(l0s)
    out = dict(pred_logits=torch.zeros(B, nq, 2, device=dev), pred_spans=torch.zeros(B, nq, 2, device=dev),
               saliency=torch.zeros(B, lv, device=dev), memory=torch.zeros(B, lv + lq, d, device=dev),
               hs=torch.zeros(nd, B, nq, d, device=dev), aux_logits=torch.zeros(max(nd - 1, 1), B, nq, 2, device=dev),
               aux_spans=torch.zeros(max(nd - 1, 1), B, nq, 2, device=dev))
    t = _lib.Taps()
    if taps:
        t.memory, t.hs = out["memory"].data_ptr(), out["hs"].data_ptr()
        t.aux_logits, t.aux_spans = out["aux_logits"].data_ptr(), out["aux_spans"].data_ptr()
    salp = _lib.ptr(out["saliency"]) if sal else None
    i32 = torch.int32
    if entry == "packed":
        nbytes = lib.cone_forward_packed_workspace(h, B, lv, lq, l0p)
    else:
        nbytes = lib.cone_forward_workspace(h, B, lv, lq)
    ws = model._ws.get(nbytes, dev)
    torch.cuda.synchronize()
    lib.cone_prof_enable(1)
    try:
        if entry == "packed":
            rc = lib.cone_forward_packed(h, _lib.ptr(vproj), _lib.ptr(vrow0, i32), _lib.ptr(vlen, i32), _lib.ptr(tproj),
                                         _lib.ptr(trow0, i32), _lib.ptr(qlen, i32), B, lv, lq, _lib.ptr(out["pred_logits"]),
                                         _lib.ptr(out["pred_spans"]), salp, C.byref(t), l0p, _lib.ptr(ws), ws.numel(),
                                         _lib.stream())
        else:
            rc = lib.cone_forward_windows(h, _lib.ptr(b[7]), _lib.ptr(vlen, i32), _lib.ptr(b[8]), _lib.ptr(qlen, i32), B, lv, lq,
                                          _lib.ptr(out["pred_logits"]), _lib.ptr(out["pred_spans"]), salp, C.byref(t),
                                          _lib.ptr(ws), ws.numel(), _lib.stream())
        _lib.check(rc)
        torch.cuda.synchronize()
        rec = np.zeros((4096, 5), dtype=np.float64)
        n = lib.cone_prof_collect(rec.ctypes.data, 4096)
    finally:
        lib.cone_prof_enable(0)
    sha = hashlib.sha256()
    for k in ("pred_logits", "pred_spans", "saliency", "memory", "hs", "aux_logits", "aux_spans"):
        sha.update(out[k].cpu().numpy().tobytes())
    return sha.hexdigest(), [tuple(int(x) for x in r[:4]) for r in rec[:n]], int(nbytes)


def make_model(dev, **kw):
    opt = make_opt("ego4d", **kw)
    model, _ = build_model(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(opt, 7).items()})
    return model.to(dev), opt


GROUPS = {}      # --summary: group -> [cells, refused, running SHA-256 of the cells' lines]


def emit(a, group, line, refused=False):
    if not a.summary:
        print(line)
        return
    g = GROUPS.setdefault(group, [0, 0, hashlib.sha256()])
    g[0] += 1
    g[1] += int(refused)
    g[2].update((line + "\n").encode())


def run_cell(a, group, cell, model, opts, *args, **kw):
    """Set the options, run one forward, print the cell's line (--summary: add it to its group)."""
    try:
        for k, v in opts:
            model.set_option(k, v)
        digest, launches, nbytes = forward(model, *args, **kw)
    except _lib.ConeHipError as e:
        emit(a, group, f"{cell}  REFUSED: {e}", True)
        return
    lsha = hashlib.sha256(repr(launches).encode()).hexdigest()[:16]
    emit(a, group, f"{cell}  ws={nbytes}  out={digest[:32]}  launches={len(launches)}:{lsha}")
    if a.launches:
        emit(a, group, "    " + " ".join("%d(%d,%d,%d)" % r for r in launches))


def tail_section(a, dev):
    batches = {B: batch(B, 256, dev) for B in a.sizes}
    for pre in (False, True):
        model, _ = make_model(dev, **({"pre_norm": True} if pre else {}))
        for mode, ff, spread, qkv, B, caches, gen in itertools.product(MODES, (2, 1, 0), (1, 0), (0, 1, 2), a.sizes, (1, 0), (0, 1)):
            cell = (f"{'pre' if pre else 'post'}-norm {mode:10s} ffn_fused={ff} ffn_spread={spread} qkv_fused={qkv} B={B:<3d} "
                    f"caches={caches} general_shape={gen}")
            opts = [("split_bf16", 0), ("bf16", 0)] + ([(mode, 1)] if mode != "fp32" else [])
            opts += [("ffn_fused", ff), ("ffn_spread", spread), ("qkv_fused", qkv), ("general_shape", gen)]
            group = f"tail    {'pre' if pre else 'post'}-norm {mode:10s} B={B:<3d}"
            run_cell(a, group, cell, model, opts, batches[B], "caches" if caches else "none")


def one_moved():
    """The defaults, then every forward option moved alone through its other values."""
    yield dict(FWD_DEFAULT)
    for k in FWD_OPTS:
        for v in FWD_RANGE[k]:
            if v != FWD_DEFAULT[k]:
                yield dict(FWD_DEFAULT, **{k: v})


def forward_section(a, dev):
    models = (("post-norm", {}, ("caches", "none")), ("pre-norm", {"pre_norm": True}, ("caches", "none")),
              ("txt-pos", {"use_txt_pos": True}, ("caches+txt", "txt", "caches", "none")))
    for name, kw, l0forms in models:
        model, opt = make_model(dev, **kw)
        batches = {B: batch(B, 256, dev, opt) for B in (1, 4, 300)}

        def cell(entry, B, l0form, o, taps=True, sal=True, lv=LV, lq=LQ):
            text = (f"{name:9s} {entry:7s} B={B:<3d} l0={l0form:10s} " + " ".join(f"{k}={o[k]}" for k in FWD_OPTS) +
                    f" taps={int(taps)} saliency={int(sal)}" + (f" Lv_max={lv}" if lv != LV else ""))
            group = f"forward {name:9s} {entry:7s} B={B:<3d} l0={l0form}"
            run_cell(a, group, text, model, list(o.items()), batches[B], l0form, taps, sal, entry, lv, lq)

        for l0form in l0forms:
            for vals in itertools.product(*(FWD_RANGE[k] for k in FWD_OPTS)):
                cell("packed", 4, l0form, dict(zip(FWD_OPTS, vals)))
            for B in (1, 300):
                for o in one_moved():
                    cell("packed", B, l0form, o)
        for B, fold, taps, sal in itertools.product((1, 4, 300), range(6), (True, False), (True, False)):
            if not (taps and sal):
                cell("packed", B, l0forms[0], dict(FWD_DEFAULT, dec_fold=fold), taps, sal)
        for fold, tables in ((2, 0), (1, 1), (0, 1)):       # 200 > 192 tokens off the default path: refused ahead of any launch
            cell("packed", 4, l0forms[0], dict(FWD_DEFAULT, dec_fold=fold, pos_tables=tables), lv=180)
        for vals in itertools.product(*(FWD_RANGE[k] for k in FWD_OPTS)):
            cell("windows", 4, "own", dict(zip(FWD_OPTS, vals)))
        for B in (1, 300):
            for o in one_moved():
                cell("windows", B, "own", o)
        for B in (1, 4, 300):
            for taps, sal in ((True, False), (False, True), (False, False)):
                cell("windows", B, "own", dict(FWD_DEFAULT), taps, sal)
        for k, v in FWD_DEFAULT.items():
            model.set_option(k, v)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", action="store_true", help="print every cell's launch sequence, not only its hash")
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES), help="batch sizes of the tail section")
    ap.add_argument("--sections", nargs="*", default=["tail", "forward"], choices=["tail", "forward"])
    ap.add_argument("--summary", action="store_true", help="one line per group of cells: count, refusals, SHA-256 of its lines")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if "tail" in a.sections:
        tail_section(a, dev)
    if "forward" in a.sections:
        forward_section(a, dev)
    for group, (n, refused, sha) in GROUPS.items():
        print(f"{group:44s} cells={n:<4d} refused={refused:<2d} sha256={sha.hexdigest()}")


if __name__ == "__main__":
    main()
