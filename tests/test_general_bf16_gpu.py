"""Option ``general_bf16`` on the GPU: the general path's layer GEMMs (another model shape than 256 / 8, windows of more
than 256 tokens, or ``general_shape = 1``) with operands rounded ONCE to bf16 on the bf16 matrix cores, fp32 accumulation
(gemm_bf16.hip).  The arithmetic contract is held against float64 on operands rounded exactly as the contract says, with
the worst-case fp32 accumulation bound of tests/test_bf16_gpu.py; the model's accuracy against the reference's OWN
bf16-autocast error (fixtures of tests/golden/gen_golden_bf16.py and gen_golden_bf16_general.py), without a margin.
Needs an MI355X: ``pytest -m gpu``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import inputs as gi
import test_bf16_gpu as B16
import test_dist_inference_gpu as D
import test_gpu_parity as P
from cone_amd import synth
from cone_amd.config import make_opt

pytestmark = pytest.mark.gpu

U = 2.0 ** -24      # unit roundoff of fp32
RELU, RESIDUAL, LN = 1, 2, 4


def _bf(x):
    """fp32 -> bf16 (round to nearest even) -> float64: the one rounding of the contract."""
    return x.float().bfloat16().double()


def _gemm_bf16(A, W, bias=None, A2=None, a2_mod=0, R=None, r_mod=0, flags=0, ldc=0, M_dev=None, M=None, guard_rows=2, **bad):
    """cone_test_gemm_bf16 on CPU tensors; C (M + guard_rows, ldc or N) starts as NaN.  Returns C on the CPU."""
    from cone_amd import _lib
    lib, dev = _lib.load(), P._gpu()
    M = A.shape[0] if M is None else M
    N, K = W.shape
    d = lambda t: None if t is None else t.to(dev).contiguous()
    Ad, Wd, bd, A2d, Rd = d(A), d(W), d(bias), d(A2), d(R)
    img = torch.empty(lib.cone_test_gemm_bf16_image_bytes(N, K), dtype=torch.uint8, device=dev)
    C = torch.full((M + guard_rows, ldc or N), float("nan"), device=dev)
    md = None if M_dev is None else torch.tensor([M_dev], dtype=torch.int32, device=dev)
    p = _lib.ptr
    _lib.check(lib.cone_test_gemm_bf16(p(Ad), p(A2d), a2_mod, p(Wd), p(bd), p(Rd), p(d(bad.get("ln_g"))), p(d(bad.get("ln_b"))),
                                       p(C), p(d(bad.get("C2"))), p(d(bad.get("ADD"))), M, N, K, flags, p(img), ldc, r_mod, p(md),
                                       _lib.stream()))
    torch.cuda.synchronize()
    return C.cpu()


# (M, N, K, what): every M of {1, 15, 16, 17, 127, 129, 300} and 257 (two full tiles of 128 rows and one row), every (N, K) of
# {(64, 64), (192, 128), (96, 512), (1536, 512), (128, 96), (256, 2048)}, and each epilogue / operand form at least once
CASES = [
    (1, 64, 64, dict(bias=True)),
    (15, 192, 128, dict(bias=True, a2="full")),
    (16, 96, 512, dict(bias=True, relu=True)),
    (17, 128, 96, dict(bias=True, res="full", ldc=160)),
    (127, 1536, 512, dict(bias=True, a2="mod")),
    (129, 256, 2048, dict(bias=True, relu=True, res="mod")),
    (300, 192, 128, dict(res="mod", ldc=576, a2="full")),          # no bias: the decoder's in-projection form
    (257, 64, 64, dict(bias=True, m_dev=131)),
    (300, 96, 512, dict(bias=True, relu=True, res="full", m_dev=129, ldc=100)),
    (129, 128, 96, dict(bias=True, a2="mod", relu=True, res="mod", ldc=132)),
]


@pytest.mark.parametrize("M,N,K,what", CASES, ids=[f"{m}x{n}x{k}" for m, n, k, _ in CASES])
def test_gemm_bf16_is_one_rounding_fp32_accumulate(M, N, K, what):
    """C = bf16(A (+ A2, summed in fp32)) bf16(W)^T (fp32 accumulation) + bias, ReLU, + R (never rounded) against float64 on
    the same rounded operands.  Products of bf16 pairs are exact in fp32, so only the accumulation differs: every element
    within K 2^-24 (|A_b| |W_b|^T) + 2 2^-24 |ref| (the bound of test_bf16_row_gemm_is_one_rounding_fp32_accumulate), plus one
    term of the same form, 2 2^-24 |result|, for the fp32 residual add.  Rows past M / *M_dev and columns past N stay NaN.
    The float64 product of the UNROUNDED operands lies outside the bound: the mode is really bf16."""
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K + 1)
    A = torch.randn(M, K, generator=g) * 1.5
    W = torch.randn(N, K, generator=g) / K ** 0.5
    bias = torch.randn(N, generator=g) * 0.2 if what.get("bias") else None
    a2_mod = 5 if what.get("a2") == "mod" else 0
    A2 = torch.randn(a2_mod or M, K, generator=g) if what.get("a2") else None
    r_mod = 5 if what.get("res") == "mod" else 0
    R = torch.randn(r_mod or M, N, generator=g) if what.get("res") else None
    flags = (RELU if what.get("relu") else 0) | (RESIDUAL if R is not None else 0)
    rows = torch.arange(M)
    a_sum = A if A2 is None else A + A2[rows % a2_mod if a2_mod else rows]          # the fp32 sum, then ONE rounding
    Ab, Wb = _bf(a_sum), _bf(W)
    pre = Ab @ Wb.t() + (bias.double() if bias is not None else 0.0)
    bound = K * U * (Ab.abs() @ Wb.abs().t()) + 2 * U * pre.abs()
    ref = pre.clamp(min=0) if what.get("relu") else pre
    full = a_sum.double() @ W.double().t() + (bias.double() if bias is not None else 0.0)
    full = full.clamp(min=0) if what.get("relu") else full
    if R is not None:
        r = R[rows % r_mod if r_mod else rows].double()
        ref, full = ref + r, full + r
        bound = bound + 2 * U * ref.abs()
    m_dev, ldc = what.get("m_dev"), what.get("ldc", 0)
    C = _gemm_bf16(A, W, bias, A2, a2_mod, R, r_mod, flags, ldc, m_dev).double()
    live = m_dev if m_dev is not None else M
    err = (C[:live, :N] - ref[:live]).abs()
    outside = (C[:live, :N] - full[:live]).abs() > bound[:live]
    P.record_measured(f"general_bf16_gemm[{M},{N},{K}]", max_err=float(err.max()), max_err_over_bound=float((err / bound[:live]).max()),
                      unrounded_outside_share=float(outside.float().mean()))
    assert bool((err <= bound[:live]).all()), float((err / bound[:live]).max())
    assert bool(torch.isnan(C[live:]).all())                # the guard rows, and the rows past *M_dev
    assert bool(torch.isnan(C[:, N:]).all())                # the guard columns
    assert bool(outside.any())


def test_gemm_bf16_rows_do_not_depend_on_the_batch():
    """Rows 100 .. 110 computed alone are torch.equal to the same rows inside a 300-row launch (one tile form)."""
    g = torch.Generator().manual_seed(11)
    A, A2 = torch.randn(300, 512, generator=g), torch.randn(300, 512, generator=g)
    W, bias = torch.randn(192, 512, generator=g) / 16, torch.randn(192, generator=g)
    R = torch.randn(300, 192, generator=g)
    whole = _gemm_bf16(A, W, bias, A2, 0, R, 0, RELU | RESIDUAL)
    alone = _gemm_bf16(A[100:111], W, bias, A2[100:111], 0, R[100:111], 0, RELU | RESIDUAL)
    assert not torch.isnan(whole[:300]).any()
    assert torch.equal(whole[100:111], alone[:11])


def test_gemm_bf16_refuses_what_it_does_not_compute():
    from cone_amd import _lib
    g = torch.Generator().manual_seed(3)
    A, W, v = torch.randn(16, 64, generator=g), torch.randn(64, 64, generator=g), torch.randn(64, generator=g)
    with pytest.raises(_lib.ConeHipError, match="EPI_LN"):
        _gemm_bf16(A, W, flags=LN, ln_g=v, ln_b=v)
    with pytest.raises(_lib.ConeHipError, match="C2 / ADD"):
        _gemm_bf16(A, W, C2=torch.zeros(16, 64), ADD=torch.zeros(16, 64))
    with pytest.raises(_lib.ConeHipError, match="K=48"):
        _gemm_bf16(torch.randn(16, 48, generator=g), torch.randn(64, 48, generator=g))
    assert _lib.load().cone_test_gemm_bf16_image_bytes(40, 64) == 0        # N % 16
    assert _lib.load().cone_test_gemm_bf16_image_bytes(64, 4096) == 0      # K > 2048


# ------------------------------------------------------------------------------------------------ the model
@pytest.fixture
def options_off():
    """Every cached model back on its default path afterwards."""
    yield
    for m, _, _ in P._MODELS.values():
        m.set_option("general_bf16", 0)
        m.set_option("general_shape", 0)


FIXTURES = ["bf16_ego4d", "bf16_ego4d_prenorm", "bf16_mad", "bf16_shape_128x4", "bf16_long"]


@pytest.mark.parametrize("entry", ["padded", "arena"])
@pytest.mark.parametrize("name", FIXTURES)
def test_general_bf16_error_within_the_references_autocast_error(golden_dir, name, entry, options_off):
    """general_bf16 = 1 against the reference's fp32 tensors: per tensor max |ours - fp32| <= ref_autocast_err, the
    reference's own error under torch.autocast(bfloat16) on the same batch -- no margin (the mode rounds a strict subset of
    what autocast rounds and keeps every output in fp32).  The three 256 / 8 fixtures of option bf16 run on a handle with
    general_shape = 1; the 128 / 4 and the 320-token fixture are general-path handles by themselves."""
    fx = np.load(os.path.join(golden_dir, name + ".npz"))
    kw = json.loads(str(fx["meta"]))["opt"]
    model, opt, _ = P.get_model(str(fx["preset"]), int(fx["weight_seed"]), **kw)
    if opt.hidden_dim == 256 and opt.nheads == 8 and not model.long_windows:
        model.set_option("general_shape", 1)
    model.set_option("general_bf16", 1)
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
    # matching runs none of the mode's GEMMs: on its own proposals it follows the mode's spans (as the reference's autocast run)
    match = model.forward_clip_matching(t(inp["src_cls_txt"]), t(inp["src_vid"]), t(inp["vid_mask"]), proposal=out["pred_spans"])
    errs["matching"] = float(np.abs(match.cpu().numpy() - fx["matching"]).max())
    yard = {k: float(fx["ref_autocast_err_" + k]) for k in errs}
    P.record_measured(f"general_bf16_golden[{name},{entry}]", **{k: [errs[k], yard[k]] for k in errs})
    for k in errs:
        assert errs[k] <= yard[k], (k, errs[k], yard[k])
    assert errs["pred_logits"] > 1e-3, errs["pred_logits"]      # ... and the mode is really on


def _general_256(preset="ego4d"):
    model, opt, _ = P.get_model(preset, 0)
    model.set_option("general_shape", 1)
    return model, opt


def _forward(model, inp, dev):
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return model.forward(g(inp["src_txt"]), g(inp["txt_mask"]), g(inp["src_vid"]), g(inp["vid_mask"]))


def test_general_bf16_switches_back_bit_for_bit_and_is_deterministic(options_off):
    """general_bf16 = 1 -> 0 on the same handle restores the exact-fp32 general path bit for bit; two runs in the mode are
    equal, and differ from the fp32 path's."""
    model, opt = _general_256()
    dev = P._gpu()
    inp = gi.stage_b_inputs(opt, 9, [90, 33, 61, 1], [7, 12, 3, 20])
    keys = ("pred_logits", "pred_spans", "saliency_scores")
    r0 = _forward(model, inp, dev)
    model.set_option("general_bf16", 1)
    r1, r1b = _forward(model, inp, dev), _forward(model, inp, dev)
    model.set_option("general_bf16", 0)
    r2 = _forward(model, inp, dev)
    for k in keys:
        assert torch.equal(r0[k], r2[k]), k
        assert torch.equal(r1[k], r1b[k]), k
    assert not torch.equal(r0["pred_logits"], r1["pred_logits"])


def test_general_bf16_padding_independence_batch_invariance_determinism(options_off):
    """test_bf16_padding_independence_batch_invariance_determinism's demands, in this mode."""
    model, opt = _general_256()
    model.set_option("general_bf16", 1)
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


def test_general_bf16_flip_is_not_replayed_from_a_stale_graph(options_off):
    """hipGraph replay on a general-path handle: a capture taken in one mode is not replayed in the other, and 1 -> 0 with
    replays in between restores the fp32 general path's outputs bit for bit."""
    from cone_amd import inference as inf
    model, _ = _general_256()
    kw = dict(nms_thd=0.5, eval_split_name="test", topk_window=4, eval_bsz=4)
    opt = make_opt("ego4d", hip_graph=True, **kw)
    ann, vf, qf = synth.make_dataset(opt, 12, 3, seed=3, ctx_range=(150, 400))
    store = inf.FeatureStore(opt, ann, vf, qf)

    def graph_run():
        lists, info = inf.predict_split(model, store, opt)
        torch.cuda.synchronize()
        return lists, {k: v.clone() for k, v in info.items() if torch.is_tensor(v)}

    a0, i0 = graph_run()
    a0b, i0b = graph_run()                               # a replay
    model.set_option("general_bf16", 1)
    a1, i1 = graph_run()
    a1b, i1b = graph_run()
    e1, _ = inf.predict_split(model, store, make_opt("ego4d", **kw))        # eager, in the mode
    model.set_option("general_bf16", 0)
    a2, i2 = graph_run()
    assert a0 == a0b == a2
    assert a1 == a1b == e1
    assert a1 != a0
    assert set(i0) == set(i2) and len(i0) > 0
    for k in i0:
        assert torch.equal(i0[k], i0b[k]) and torch.equal(i0[k], i2[k]), k
        assert torch.equal(i1[k], i1b[k]), k
    assert any(not torch.equal(i0[k], i1[k]) for k in i0)


def test_general_bf16_is_refused_on_the_fused_path_and_independent_of_other_options(options_off):
    """A default 256 / 8 handle refuses the option, naming bf16; 0 is always accepted; general_shape = 0 afterwards leaves it
    set and inert (the fused path's bits); on a long-window handle it can be set before and after unrelated options, and
    bf16's own refusals stay what they were."""
    from cone_amd import _lib
    model, opt, _ = P.get_model("ego4d", 0)
    model.set_option("general_shape", 0)
    model.set_option("general_bf16", 0)
    with pytest.raises(_lib.ConeHipError, match=r"general_bf16 applies to the general path only.*use bf16"):
        model.set_option("general_bf16", 1)
    dev = P._gpu()
    inp = gi.stage_b_inputs(opt, 2, [90, 12], [20, 4])
    fused = _forward(model, inp, dev)
    model.set_option("general_shape", 1)
    model.set_option("general_bf16", 1)
    model.set_option("bf16", 1)                 # independent of bf16, in both set orders
    model.set_option("bf16", 0)
    model.set_option("general_shape", 0)        # inert now: the fused path never reads it
    again = _forward(model, inp, dev)
    for k in ("pred_logits", "pred_spans", "saliency_scores"):
        assert torch.equal(fused[k], again[k]), k
    long_model, lopt, _ = P.get_model("ego4d", 1, max_v_l=300, max_q_l=20, v_motion_feat_dim=64, v_appear_feat_dim=64, t_feat_dim=64)
    assert long_model.long_windows
    long_model.set_option("general_bf16", 1)
    long_model.set_option("rows_chain", 0)
    long_model.set_option("general_bf16", 0)
    long_model.set_option("rows_chain", 1)
    long_model.set_option("general_bf16", 1)
    with pytest.raises(_lib.ConeHipError, match=r"windows beyond 256 tokens run the general path"):
        long_model.set_option("bf16", 1)
    linp = gi.stage_b_inputs(lopt, 4, [300, 40], [20, 3])
    on = _forward(long_model, linp, dev)
    long_model.set_option("general_bf16", 0)
    off = _forward(long_model, linp, dev)
    assert not torch.equal(on["pred_logits"], off["pred_logits"])


# ------------------------------------------------------------------------------------------------ the CLI
def _case(golden_dir, tmp_path, name):
    with open(os.path.join(golden_dir, name + ".json")) as f:
        fx = json.load(f)
    saved = make_opt(fx["preset"], nms_thd=0.5, **fx["opt"])
    resume = D._checkpoint(tmp_path, saved, fx["weight_seed"])
    ann, vf, qf = synth.make_dataset(saved, fx["n_queries"], fx["n_videos"], seed=fx["data_seed"], ctx_range=tuple(fx["ctx_range"]))
    eval_path, packed = D._packed(tmp_path, saved, ann, vf, qf, "test")
    argv = ["--resume", resume, "--eval_split_name", "test", "--eval_path", eval_path, "--eval_id", "golden",
            "--packed_features", packed, "--nms_thd", "0.5", "--topk_window", str(saved.topk_window), "--eval_bsz",
            str(saved.eval_bsz), "--save_all"]
    return dict(dir=tmp_path, argv=argv), saved, ann


def test_cli_general_bf16_end_to_end_writes_well_formed_files(golden_dir, tmp_path):
    """``python -m cone_amd.inference ... --general_bf16`` on the inputs of e2e_shape_128x4: the same files with the same query
    ids and counts as the default run, every query's moments ordered by score and finite.  The share of queries whose top-1
    moment has temporal IoU >= 0.7 with the default run's top-1 is RECORDED, not asserted (nobody has measured a floor)."""
    case, saved, ann = _case(golden_dir, tmp_path, "e2e_shape_128x4")
    ref, _ = D._cli(case, "default", [])
    got, _ = D._cli(case, "general_bf16", ["--general_bf16"])
    assert sorted(os.listdir(got)) == sorted(os.listdir(ref))
    n_top1 = n_q = 0
    differs = False
    for tag, col in (("", 4), ("proposal_", 2), ("matching_", 3)):
        fn = f"inference_ego4d_test_golden_{tag}preds.json"
        a, b = B16._rows(got / fn, "ego4d"), B16._rows(ref / fn, "ego4d")
        assert len(a) == len(b) == len(ann)
        differs |= a != b
        for ga, rb in zip(a, b):
            assert {k: v for k, v in ga.items() if k != "predicted_times"} == {k: v for k, v in rb.items() if k != "predicted_times"}
            pa, pb = ga["predicted_times"], rb["predicted_times"]
            assert len(pa) == len(pb) and len(pa) > 0
            sc = [m[col] for m in pa]
            assert sc == sorted(sc, reverse=True), tag
            assert all(np.isfinite(m).all() and m[0] <= m[1] for m in pa)
            if tag == "":
                n_q += 1
                n_top1 += B16._iou(pa[0][:2], pb[0][:2]) >= 0.7
    assert differs                                       # the flag reached the handle
    P.record_measured("general_bf16_cli_e2e[e2e_shape_128x4]", queries=n_q, top1_tiou_ge_0p7_with_default=int(n_top1),
                      share=n_top1 / n_q)


def test_cli_general_bf16_on_a_fused_path_checkpoint_exits_with_the_librarys_message(golden_dir, tmp_path):
    case, _, _ = _case(golden_dir, tmp_path, "e2e_ego4d")
    out = tmp_path / "out_refused"
    out.mkdir()
    cmd = [sys.executable, "-m", "cone_amd.inference"] + case["argv"] + ["--eval_results_dir", str(out), "--general_bf16"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=D._env(), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "general_bf16 applies to the general path only" in r.stderr + r.stdout
    assert os.listdir(out) == []        # before any evaluation
