"""Option ``bf16`` on the GPU (through the C ABI): the layer-tail GEMMs with operands rounded ONCE to bf16, one MFMA per
operand pair, fp32 accumulation (ffn_bf16.hip).  Accuracy is held against the reference model's OWN bf16-autocast error
(fixtures of tests/golden/gen_golden_bf16.py); the arithmetic contract against a float64 computation on bf16-rounded
operands.  Needs an MI355X: ``pytest -m gpu``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import inputs as gi
import test_dist_inference_gpu as D
import test_gpu_parity as P
from cone_amd import synth
from cone_amd.config import make_opt

pytestmark = pytest.mark.gpu

FIXTURES = ["bf16_ego4d", "bf16_ego4d_prenorm", "bf16_mad"]
U = 2.0 ** -24      # unit roundoff of fp32


@pytest.fixture
def bf16_off():
    """Every cached model back on the default path afterwards."""
    yield
    for m, _, _ in P._MODELS.values():
        m.set_option("bf16", 0)


@pytest.mark.parametrize("entry", ["padded", "arena"])
@pytest.mark.parametrize("name", FIXTURES)
def test_bf16_error_within_the_references_autocast_error(golden_dir, name, entry, bf16_off):
    """bf16 = 1 against the reference's fp32 tensors: per tensor max |ours - fp32| <= ref_autocast_err, the reference's own
    error under torch.autocast(bfloat16) on the same batch -- no margin (the mode rounds strictly fewer quantities)."""
    fx = np.load(os.path.join(golden_dir, name + ".npz"))
    kw = {"pre_norm": True} if "pre_norm" in fx.files else {}
    model, opt, _ = P.get_model(str(fx["preset"]), int(fx["weight_seed"]), **kw)
    model.set_option("bf16", 1)
    lens_v, lens_q = fx["lens_v"].tolist(), fx["lens_q"].tolist()
    inp = gi.stage_b_inputs(opt, int(fx["input_seed"]), lens_v, lens_q)
    assert gi.checksum(inp["src_vid"], inp["src_txt"], inp["src_cls_txt"]) == str(fx["input_checksum"])
    dev = P._gpu()
    t = lambda a: torch.from_numpy(a).to(dev)
    out = P.stage_b_forward(entry, model, opt, inp, lens_v, lens_q, dev, taps=True)
    Lv, Lq = inp["src_vid"].shape[1], inp["src_txt"].shape[1]
    vm = P._valid_token_mask(lens_v, lens_q, Lv, Lq)
    errs = {}
    if entry == "padded":
        errs["hs"] = P.maxdiff(out["hs"], fx["hs"])
        errs["memory"] = float(np.abs(out["memory"].cpu().numpy()[..., ::int(fx["mem_stride"])] - fx["memory"])[vm].max())
    errs["pred_logits"] = P.maxdiff(out["pred_logits"], fx["pred_logits"])
    errs["pred_spans"] = P.maxdiff(out["pred_spans"], fx["pred_spans"])
    errs["saliency_scores"] = float(np.abs(out["saliency_scores"].cpu().numpy() - fx["saliency_scores"])[vm[:, :Lv]].max())
    # matching runs no layer tail: on its own proposals it follows the mode's spans (as the reference's autocast run does)
    match = model.forward_clip_matching(t(inp["src_cls_txt"]), t(inp["src_vid"]), t(inp["vid_mask"]), proposal=out["pred_spans"])
    errs["matching"] = float(np.abs(match.cpu().numpy() - fx["matching"]).max())
    yard = {k: float(fx["ref_autocast_err_" + k]) for k in errs}
    P.record_measured(f"bf16_golden[{name},{entry}]", **{k: [errs[k], yard[k]] for k in errs})
    for k in errs:
        assert errs[k] <= yard[k], (k, errs[k], yard[k])
    # ... and the mode is really on (pre-norm handles included): bf16 operands leave the fp32 path's 1e-4 by far
    assert errs["pred_logits"] > 1e-3, errs["pred_logits"]


def _bf(x):
    """fp32 -> bf16 (round to nearest even) -> float64: the one rounding of the contract."""
    return x.float().bfloat16().double()


def _flip(v64, e):
    """Where the kernel's fp32 value (within e of v64) may round to the OTHER bf16 neighbour than v64 does: the distance
    that rounding can then add (one bf16 spacing at |v64|), else 0."""
    v = v64.float()
    lo = v.bfloat16().double()
    ulp = torch.clamp(v64.abs(), min=2.0 ** -126).log2().floor().exp2() * 2.0 ** -7
    # distance of v64 to the nearer rounding boundary (midpoint between bf16 neighbours) = ulp / 2 - |v64 - rn(v64)|
    to_mid = ulp / 2 - (v64 - lo).abs()
    return torch.where(to_mid <= e, ulp, torch.zeros_like(ulp))


def _ln_bound(z, d, g, b):
    """|LayerNorm_fp32(z + error <= d) - LayerNorm_float64(z)| elementwise: first-order propagation of the input error through
    mean (dm), centring and the 1-Lipschitz standard deviation (ds), plus the fp32 evaluation itself (a 256-term sum: 256 U
    relative on mean and variance, a few U on each element)."""
    mu = z.mean(-1, keepdim=True)
    c = z - mu
    sig = (c.pow(2).mean(-1, keepdim=True) + 1e-5).sqrt()
    d = d + 4 * U * z.abs()
    dm = d.mean(-1, keepdim=True) + 256 * U * z.abs().mean(-1, keepdim=True)
    dc = d + dm
    ds = dc.pow(2).mean(-1, keepdim=True).sqrt() + 260 * U * sig
    out = c / sig * g + b
    return g.abs() * (dc / (sig - ds) + c.abs() * ds / (sig * (sig - ds))) + 8 * U * (out.abs() + b.abs())


def _ffn_ref(x64, ex, xb, W1, b1, W2, b2, lg, lb):
    """float64 feed-forward block on bf16-rounded operands + the worst-case bound of the kernel's fp32 accumulation.
    x64 / ex: the fp32 block input (residual) and its error bound; xb: its bf16 image as the kernel may hold it (the
    possible other-neighbour roundings are inside ``fx``)."""
    ff = W1.shape[0]
    W1b, W2b = _bf(W1), _bf(W2)
    fx = _flip(x64, ex)
    pre = xb @ W1b.t() + b1.double()
    e1 = 256 * U * (xb.abs() @ W1b.abs().t()) + fx @ W1b.abs().t() + 2 * U * pre.abs()
    h = pre.clamp(min=0)
    hb = _bf(h)
    fh = _flip(h, e1)
    y = hb @ W2b.t()
    e2 = ff * U * (hb.abs() @ W2b.abs().t()) + fh @ W2b.abs().t()
    z = x64 + y + b2.double()
    d = ex + e2 + 4 * U * (x64.abs() + y.abs() + b2.double().abs())
    ref = torch.nn.functional.layer_norm(z, (256,), lg.double(), lb.double(), 1e-5)
    return ref, _ln_bound(z, d, lg.double(), lb.double())


@pytest.mark.parametrize("M,ff", [(1, 1024), (16, 64), (127, 1024), (129, 1024), (1000, 2048), (300, 96), (40000, 1024)])
def test_bf16_tail_is_one_rounding_fp32_accumulate(M, ff):
    """One FFN block, and one attention-projection + FFN tail, against float64 on operands rounded to bf16 exactly as the
    contract says.  Products of bf16 pairs are exact in fp32, so only the accumulation differs: every output element
    within K * 2^-24 * sum |a b| of its GEMM (K = 256 resp. ff terms), carried through the second GEMM and the LayerNorm
    (where an intermediate lies within its own WORST-CASE bound of a bf16 rounding boundary, one bf16 spacing is allowed for
    it).  How sharp that is depends on ff: at ff = 64 / 96 hardly any hidden unit is granted a spacing and a twice-rounded or
    unrounded operand, a residual taken from the rounded input or a dropped piece leaves the bound by a factor 4 - 60; at
    ff >= 1024 about one hidden unit in twenty is granted one and the bound (~1e-2) only catches coarse faults such as
    truncated weights.  ff is a run-time value of ONE kernel, so the small-ff cases pin the arithmetic and the large ones
    the ring, the tile loop and the row tails at the shipped width.  max_err is recorded per case."""
    from cone_amd import _lib
    dev = P._gpu()
    g = torch.Generator().manual_seed(M * 31 + ff + 1)
    X = torch.randn(M, 256, generator=g) * 1.5
    W1 = torch.randn(ff, 256, generator=g) / 16
    b1 = torch.randn(ff, generator=g) * 0.2
    W2 = torch.randn(256, ff, generator=g) / ff ** 0.5
    b2 = torch.randn(256, generator=g) * 0.2
    lg, lb = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g)
    d = lambda t: t.to(dev).contiguous()
    Xd, W1d, b1d, W2d, b2d, lgd, lbd = map(d, (X, W1, b1, W2, b2, lg, lb))
    lib = _lib.load()
    img = torch.empty(lib.cone_test_ffn_split_image_bytes(ff), dtype=torch.uint8, device=dev)
    out = torch.full((M + 3, 256), float("nan"), device=dev)
    _lib.check(lib.cone_test_ffn_split(_lib.ptr(Xd), _lib.ptr(W1d), _lib.ptr(b1d), _lib.ptr(W2d), _lib.ptr(b2d),
                                       _lib.ptr(lgd), _lib.ptr(lbd), _lib.ptr(out), M, ff, _lib.ptr(img), 3, _lib.stream()))
    torch.cuda.synchronize()
    ref, bound = _ffn_ref(X.double(), torch.zeros(M, 256, dtype=torch.float64), _bf(X), W1, b1, W2, b2, lg, lb)
    err = (out[:M].cpu().double() - ref).abs()
    P.record_measured(f"bf16_ffn_exact[{M},{ff}]", max_err=float(err.max()), max_err_over_bound=float((err / bound).max()),
                      fp32_kernel_scale=float(ref.abs().max()))
    assert bool((err <= bound).all()), float((err / bound).max())
    assert bool(torch.isnan(out[M:]).all())
    # this IS bf16 arithmetic, not the fp32-accurate split: the unrounded float64 block is far outside the bound
    h = (X.double() @ W1.double().t() + b1.double()).clamp(min=0)
    full = torch.nn.functional.layer_norm(X.double() + h @ W2.double().t() + b2.double(), (256,), lg.double(), lb.double(), 1e-5)
    assert float((out[:M].cpu().double() - full).abs().max()) > 1e-4
    # with the attention output projection + residual + LayerNorm in the kernel as well, in place over R
    A = torch.randn(M, 256, generator=g)
    Wo = torch.randn(256, 256, generator=g) / 16
    bo = torch.randn(256, generator=g) * 0.2
    pg, pb = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g) * 0.3
    Ab, Wob = _bf(A), _bf(Wo)
    proj = Ab @ Wob.t()
    z0 = X.double() + proj + bo.double()
    d0 = 256 * U * (Ab.abs() @ Wob.abs().t()) + 4 * U * (X.double().abs() + proj.abs() + bo.double().abs())
    x1 = torch.nn.functional.layer_norm(z0, (256,), pg.double(), pb.double(), 1e-5)
    ex1 = _ln_bound(z0, d0, pg.double(), pb.double())
    ref, bound = _ffn_ref(x1, ex1, _bf(x1), W1, b1, W2, b2, lg, lb)
    Ad, Wod, bod, pgd, pbd = map(d, (A, Wo, bo, pg, pb))
    R = torch.full((M + 3, 256), float("nan"), device=dev)
    R[:M] = Xd
    wo_img = torch.empty(lib.cone_test_proj_split_image_bytes(), dtype=torch.uint8, device=dev)
    _lib.check(lib.cone_test_proj_ffn_split(_lib.ptr(Ad), _lib.ptr(Wod), _lib.ptr(bod), _lib.ptr(R), _lib.ptr(pgd),
                                            _lib.ptr(pbd), _lib.ptr(W1d), _lib.ptr(b1d), _lib.ptr(W2d), _lib.ptr(b2d),
                                            _lib.ptr(lgd), _lib.ptr(lbd), _lib.ptr(R), M, ff, _lib.ptr(img), _lib.ptr(wo_img),
                                            3, _lib.stream()))
    torch.cuda.synchronize()
    err = (R[:M].cpu().double() - ref).abs()
    P.record_measured(f"bf16_proj_ffn_exact[{M},{ff}]", max_err=float(err.max()), max_err_over_bound=float((err / bound).max()))
    assert bool((err <= bound).all()), float((err / bound).max())
    assert bool(torch.isnan(R[M:]).all())


@pytest.mark.parametrize("M,N", [(1, 32), (127, 768), (1000, 768), (40000, 768), (300, 256), (513, 64)])
def test_bf16_row_gemm_is_one_rounding_fp32_accumulate(M, N):
    from cone_amd import _lib
    dev = P._gpu()
    g = torch.Generator().manual_seed(M + 7 * N + 1)
    X = torch.randn(M, 256, generator=g) * 1.5
    W = torch.randn(N, 256, generator=g) / 16
    b = torch.randn(N, generator=g) * 0.2
    Xb, Wb = _bf(X), _bf(W)
    ref = Xb @ Wb.t() + b.double()
    bound = 256 * U * (Xb.abs() @ Wb.abs().t()) + 2 * U * ref.abs()
    lib = _lib.load()
    img = torch.empty(lib.cone_test_rows_split_image_bytes(N), dtype=torch.uint8, device=dev)
    C = torch.full((M + 2, N), float("nan"), device=dev)
    Xd, Wd, bd = X.to(dev), W.to(dev), b.to(dev)
    _lib.check(lib.cone_test_rows_split(_lib.ptr(Xd), _lib.ptr(Wd), _lib.ptr(bd), _lib.ptr(C), M, N, _lib.ptr(img), 3,
                                        _lib.stream()))
    torch.cuda.synchronize()
    err = (C[:M].cpu().double() - ref).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    assert bool(torch.isnan(C[M:]).all())


def _split(preset="ego4d", nq=12, nv=3, **kw):
    from cone_amd import inference as inf
    model, opt, _ = P.get_model(preset, 0)
    opt = make_opt(preset, nms_thd=0.5, eval_split_name="test", topk_window=4, eval_bsz=4, **kw)
    ann, vf, qf = synth.make_dataset(opt, nq, nv, seed=3, ctx_range=(150, 400))
    return inf, model, opt, inf.FeatureStore(opt, ann, vf, qf)


def _run(inf, model, store, opt):
    lists, info = inf.predict_split(model, store, opt)
    wt = inf.window_table(store, opt, info["win_idx"])
    raw = inf.run_windows(model, store, opt, wt)
    torch.cuda.synchronize()
    return lists, info["win_idx"].clone(), {k: v.clone() for k, v in wt.items() if torch.is_tensor(v)}, \
        {k: v.clone() for k, v in raw.items() if torch.is_tensor(v)}


def test_bf16_leaves_stage_a_untouched_and_switches_back_bit_for_bit(bf16_off):
    """Stage A does not change: the window rank lists and the window tables of bf16 = 1 are array_equal to the default's.
    bf16 = 1, then bf16 = 0 on the same handle: the default path's outputs bit for bit -- while the mode's own differ."""
    inf, model, opt, store = _split()
    l0, w0, t0, r0 = _run(inf, model, store, opt)
    model.set_option("bf16", 1)
    l1, w1, t1, r1 = _run(inf, model, store, opt)
    l1b, _, _, r1b = _run(inf, model, store, opt)
    model.set_option("bf16", 0)
    l2, w2, t2, r2 = _run(inf, model, store, opt)
    assert np.array_equal(w0.cpu().numpy(), w1.cpu().numpy())
    for k in t0:
        assert np.array_equal(t0[k].cpu().numpy(), t1[k].cpu().numpy()), k
    assert not torch.equal(r0["pred_logits"], r1["pred_logits"])
    for k in r0:
        assert torch.equal(r0[k], r2[k]), k
        assert torch.equal(r1[k], r1b[k]), k        # run-to-run determinism of the mode
    assert l0 == l2 and l1 == l1b


def test_bf16_flip_is_not_replayed_from_a_stale_graph(bf16_off):
    """hipGraph replay: a capture taken in one mode is not replayed in the other on the same handle and store, and
    bf16 = 1 -> 0 with replays in between restores the default's outputs bit for bit (torch.equal on the kept-row tensors
    the graph returns, and on the window outputs of an eager run_windows afterwards)."""
    inf, model, opt, store = _split(hip_graph=True)

    def graph_run():
        lists, info = inf.predict_split(model, store, opt)
        torch.cuda.synchronize()
        return lists, {k: v.clone() for k, v in info.items() if torch.is_tensor(v)}

    a0, i0 = graph_run()
    a0b, i0b = graph_run()                               # a replay
    _, _, _, r0 = _run(inf, model, store, make_opt("ego4d", nms_thd=0.5, eval_split_name="test", topk_window=4, eval_bsz=4))
    model.set_option("bf16", 1)
    a1, i1 = graph_run()
    a1b, i1b = graph_run()
    model.set_option("bf16", 0)
    a2, i2 = graph_run()
    eager_opt = make_opt("ego4d", nms_thd=0.5, eval_split_name="test", topk_window=4, eval_bsz=4)
    _, _, _, r2 = _run(inf, model, store, eager_opt)
    model.set_option("bf16", 1)
    e1, _ = inf.predict_split(model, store, eager_opt)
    assert a0 == a0b == a2
    assert a1 == a1b == e1
    assert a1 != a0
    assert set(i0) == set(i2) and len(i0) > 0
    for k in i0:
        assert torch.equal(i0[k], i0b[k]) and torch.equal(i0[k], i2[k]), k
        assert torch.equal(i1[k], i1b[k]), k
    assert any(not torch.equal(i0[k], i1[k]) for k in i0)
    for k in r0:
        assert torch.equal(r0[k], r2[k]), k


def test_bf16_padding_independence_batch_invariance_determinism(bf16_off):
    """test_padding_independence_and_determinism's demands, in the mode."""
    model, opt, _ = P.get_model("ego4d", 0)
    model.set_option("bf16", 1)
    dev = P._gpu()
    inp = gi.stage_b_inputs(opt, 5, [90, 33, 61], [7, 12, 3])
    g = lambda a: torch.from_numpy(a).to(dev)
    a = model.forward(g(inp["src_txt"]), g(inp["txt_mask"]), g(inp["src_vid"]), g(inp["vid_mask"]))
    a2 = model.forward(g(inp["src_txt"]), g(inp["txt_mask"]), g(inp["src_vid"]), g(inp["vid_mask"]))
    pad_t = np.zeros((3, 20, inp["src_txt"].shape[2]), np.float32)
    pad_t[:, :12] = inp["src_txt"]
    pad_m = np.zeros((3, 20), np.float32)
    pad_m[:, :12] = inp["txt_mask"]
    b = model.forward(g(pad_t), g(pad_m), g(inp["src_vid"]), g(inp["vid_mask"]))
    c = model.forward(g(inp["src_txt"][1:2, :12]), g(inp["txt_mask"][1:2, :12]), g(inp["src_vid"][1:2]), g(inp["vid_mask"][1:2]))
    for k in ("pred_logits", "pred_spans"):
        assert torch.equal(a[k], a2[k])
        assert torch.equal(a[k], b[k])
        assert torch.equal(a[k][1:2], c[k])


def test_bf16_refusals_name_the_option(bf16_off):
    model, _, _ = P.get_model("ego4d", 0)
    model.set_option("bf16", 0)
    model.set_option("split_bf16", 1)
    try:
        with pytest.raises(Exception, match=r"bf16 = 1 while split_bf16 = 1"):
            model.set_option("bf16", 1)
    finally:
        model.set_option("split_bf16", 0)
    model.set_option("bf16", 1)
    try:
        with pytest.raises(Exception, match=r"split_bf16 = 1 while bf16 = 1"):
            model.set_option("split_bf16", 1)
    finally:
        model.set_option("bf16", 0)
    general, _, _ = P.get_model("ego4d", 0, hidden_dim=128, nheads=4)
    general.set_option("bf16", 0)
    with pytest.raises(Exception, match=r"set_option: bf16 needs hidden_dim 256"):
        general.set_option("bf16", 1)


# ------------------------------------------------------------------------------- the CLI
def _iou(a, b):
    inter = max(0.0, min(a[1], b[1]) - max(a[0], b[0]))
    union = max(a[1], b[1]) - min(a[0], b[0])
    return inter / union if union > 0 else 0.0


def _rows(path, preset):
    with open(path) as fh:
        return [json.loads(l) for l in fh.read().split("\n") if l] if preset == "mad" else json.load(fh)["results"]


@pytest.mark.parametrize("name", ["e2e_ego4d", "e2e_mad"])
def test_cli_bf16_end_to_end_writes_well_formed_files(golden_dir, tmp_path, name):
    """``python -m cone_amd.inference ... --bf16`` on the inputs of the reference's end-to-end fixtures: the same files with
    the same query ids and counts as the default run, every query's moments ordered by score and inside the video.  The
    kept moments are COMPARED with the default run's, not asserted equal: the share of queries whose top-1 moment has
    temporal IoU >= 0.7 with the default's top-1 is recorded (a measurement; README / DESIGN.md quote it)."""
    with open(os.path.join(golden_dir, name + ".json")) as f:
        fx = json.load(f)
    preset = fx["preset"]
    saved = make_opt(preset, nms_thd=0.5, **fx["opt"])
    resume = D._checkpoint(tmp_path, saved, fx["weight_seed"])
    ann, vf, qf = synth.make_dataset(saved, fx["n_queries"], fx["n_videos"], seed=fx["data_seed"], ctx_range=tuple(fx["ctx_range"]))
    eval_path, packed = D._packed(tmp_path, saved, ann, vf, qf, "test")
    argv = ["--resume", resume, "--eval_split_name", "test", "--eval_path", eval_path, "--eval_id", "golden",
            "--packed_features", packed, "--nms_thd", "0.5", "--topk_window", str(saved.topk_window), "--eval_bsz",
            str(saved.eval_bsz), "--save_all"]
    case = dict(dir=tmp_path, argv=argv)
    ref, _ = D._cli(case, "default", [])
    got, _ = D._cli(case, "bf16", ["--bf16"])
    assert sorted(os.listdir(got)) == sorted(os.listdir(ref))
    dur = {r["query_id"]: float(r["duration"]) for r in ann}
    n_top1 = n_q = n_out = n_out_default = 0
    # "inside the video": the span head predicts (centre, width) in [0, 1] of its WINDOW and nothing clamps the composed
    # seconds, so a moment can overhang its window -- hence the video -- by up to half a window length; the unmodified
    # reference's own rows in these fixtures do (-11.7 s, duration + 8.4 s).  Asserted: inside the video up to that overhang;
    # recorded: how many moments leave [0, duration] at all, in this run and in the default run
    half = 0.5 * saved.max_v_l * saved.clip_length
    ext = "jsonl" if preset == "mad" else "json"
    for tag, col in (("", 4), ("proposal_", 2), ("matching_", 3)):    # rows [st, ed, proposal, matching, fused]: each file's own key
        fn = f"inference_{preset}_test_golden_{tag}preds.{ext}"
        a, b = _rows(got / fn, preset), _rows(ref / fn, preset)
        assert len(a) == len(b) == len(ann)
        for ga, rb, row in zip(a, b, ann):
            assert {k: v for k, v in ga.items() if k != "predicted_times"} == {k: v for k, v in rb.items() if k != "predicted_times"}
            pa, pb = ga["predicted_times"], rb["predicted_times"]
            assert len(pa) == len(pb) and len(pa) > 0
            sc = [m[col] for m in pa]
            assert sc == sorted(sc, reverse=True), (tag, row["query_id"])
            for m, md in zip(pa, pb):
                assert all(np.isfinite(m)) and m[0] <= m[1]
                assert -half <= m[0] and m[1] <= dur[row["query_id"]] + half, (m, dur[row["query_id"]])
                n_out += not (0.0 <= m[0] and m[1] <= dur[row["query_id"]])
                n_out_default += not (0.0 <= md[0] and md[1] <= dur[row["query_id"]])
            if tag == "":
                n_q += 1
                n_top1 += _iou(pa[0][:2], pb[0][:2]) >= 0.7
    P.record_measured(f"bf16_cli_e2e[{name}]", queries=n_q, top1_tiou_ge_0p7_with_default=int(n_top1), share=n_top1 / n_q,
                      moments_outside_0_duration=int(n_out), same_in_default_run=int(n_out_default))


def test_cli_bf16_two_ranks_write_the_single_process_files(ego4d_case):
    """``--gpus 2 --bf16``: byte-identical to the single-process ``--bf16`` run (every rank sets the option on its handle),
    and not the default run's files."""
    ref, _ = D._plain(ego4d_case, "bf16", ["--bf16"])
    got, _ = D._cli(ego4d_case, "two_bf16", ["--bf16"], n_gpus=2)
    D._same_files(got, ref, D.EGO4D_FILES)
    dflt, _ = D._plain(ego4d_case, "default", [])
    assert (dflt / D.EGO4D_FILES[0]).read_bytes() != (ref / D.EGO4D_FILES[0]).read_bytes()


def test_cli_bf16_with_split_bf16_exits_with_the_librarys_message(ego4d_case):
    out = ego4d_case["dir"] / "out_both"
    out.mkdir()
    cmd = [sys.executable, "-m", "cone_amd.inference"] + ego4d_case["argv"] + ["--eval_results_dir", str(out), "--bf16", "--split_bf16"]
    r = subprocess.run(cmd, cwd=str(ego4d_case["dir"]), env=D._env(), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "bf16 = 1 while split_bf16 = 1" in r.stderr + r.stdout
    assert os.listdir(out) == []        # before any evaluation


ego4d_case = D.ego4d_case      # the sharded tests' module fixture (checkpoint + packed Ego4D val split), built once here too
