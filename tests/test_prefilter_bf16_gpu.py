"""The opt-in bf16 pre-filter on the GPU: producers of the bf16 arena, the scoring kernels against the float64 restatement
of the contract (tests/prefilter_bf16_ref.py), batch invariance, the grouped entry, the pipeline switch, the refusals."""
import json
import os

import numpy as np
import pytest
import torch

import prefilter_bf16_ref as R
import test_bf16_gpu as B
import test_dist_inference_gpu as D
import test_gpu_parity as P
from cone_amd import synth
from cone_amd.config import make_opt
from test_prefilter_bf16_cpu import planted_split

pytestmark = pytest.mark.gpu

BASE = (1000, 90, 256, 5)           # (ctx_l, W, dv, nq): every axis is taken to its extremes around this point
MQ_MIN = 5                          # CONE_PF16_MQ_MIN: the nq list below has both sides of it (4 | 5)


def _unit_rows(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g)
    return x / x.norm(dim=1, keepdim=True)


_CASES = {}


def _case(ctx_l, dv, seed=0, scale=0):
    """L2-normalised rows and 65 query vectors of one (ctx_l, dv), made once; scale: ctx * 2^scale, cls * 2^-scale."""
    key = (ctx_l, dv, seed, scale)
    if key not in _CASES:
        ctx, cls = _unit_rows(ctx_l, dv, 11 + seed), _unit_rows(65, dv, 12 + seed)
        _CASES[key] = (ctx * 2.0 ** scale, cls * 2.0 ** -scale)
    return _CASES[key]


def _check_scores(ctx, cls, W, got, tag):
    dv = ctx.shape[1]
    win, ab = R.window_scores(ctx, cls, W)
    bound = R.accumulation_bound(win, ab, dv)
    err = (got.cpu().double() - win).abs()
    raw = R.window_scores(ctx, cls, W, rounded=False)[0]
    P.record_measured(f"prefilter_bf16_scores[{tag}]", max_err_over_bound=float((err / bound).max()),
                      unrounded_over_bound=float(((raw - got.cpu().double()).abs() / bound).max()))
    assert got.shape == win.shape
    assert bool((err <= bound).all()), (tag, float((err / bound).max()))
    # the mode is on: the unrounded fp32 score is not what was computed
    assert bool(((raw - got.cpu().double()).abs() > bound).any()), tag


def _axis_cases():
    c, w, d, q = BASE
    out = [(x, w, d, q) for x in (1, 44, 45, 46, 91, 1000, 70001)]
    out += [(c, x, d, q) for x in (125, 2)]
    out += [(c, w, x, q) for x in (32, 96, 512, 1024)]
    out += [(c, w, d, x) for x in (1, 2, 3, 4, 7, 16, 17, 64, 65)]
    return out


@pytest.mark.parametrize("ctx_l,W,dv,nq", _axis_cases())
def test_window_scores_are_the_contract_within_fp32_accumulation(ctx_l, W, dv, nq):
    """Every window score within dv U max_f sum|a b| + 2 U |score| of the float64 contract value, and the unrounded fp32
    score further than that for at least one window.  Each (ctx_l, W, dv) case also runs the streaming form (its first 3
    queries) next to the form nq selects."""
    from cone_amd import ops
    dev = P._gpu()
    ctx, cls = _case(ctx_l, dv)
    arena = ops.rows_to_bf16(ctx.to(dev))
    assert arena.dtype == torch.bfloat16 and torch.equal(arena.cpu(), ctx.bfloat16())
    for n in sorted({nq, 3} if nq == BASE[3] else {nq}):
        fs, got = ops.prefilter_scores(arena, cls[:n].to(dev).contiguous(), W, frame_scores=False)
        torch.cuda.synchronize()
        assert fs is None
        _check_scores(ctx, cls[:n], W, got, f"{ctx_l},{W},{dv},{n}")


@pytest.mark.parametrize("nq", [3, 5])
def test_window_scores_have_no_hidden_range_assumption(nq):
    """Rows scaled by 2^20, queries by 2^-20: the same bound (scaling by a power of two commutes with every rounding)."""
    from cone_amd import ops
    dev = P._gpu()
    ctx_l, W, dv, _ = BASE
    ctx, cls = _case(ctx_l, dv, scale=20)
    _, got = ops.prefilter_scores(ops.rows_to_bf16(ctx.to(dev)), cls[:nq].to(dev).contiguous(), W, frame_scores=False)
    torch.cuda.synchronize()
    _check_scores(ctx, cls[:nq], W, got, f"scaled,{nq}")


def test_a_query_s_bits_do_not_depend_on_the_launch_it_shares():
    """Streaming form: alone == 2nd of 3 == 4th of 4 (torch.equal).  Streaming vs matrix-core form: within twice the bound."""
    from cone_amd import ops
    dev = P._gpu()
    ctx_l, W, dv, _ = BASE
    ctx, cls = _case(ctx_l, dv)
    arena = ops.rows_to_bf16(ctx.to(dev))
    run = lambda rows: ops.prefilter_scores(arena, rows.to(dev).contiguous(), W, frame_scores=False)[1]
    q = cls[7:8]
    alone = run(q)
    assert torch.equal(alone[0], run(torch.cat([cls[0:1], q, cls[1:2]]))[1])
    assert torch.equal(alone[0], run(torch.cat([cls[0:3], q]))[3])
    mq = run(torch.cat([cls[0:MQ_MIN - 1], q]))[MQ_MIN - 1]            # MQ_MIN queries: the matrix-core form
    win, ab = R.window_scores(ctx, q, W)
    bound = R.accumulation_bound(win, ab, dv)[0]
    assert bool(((mq.cpu().double() - alone[0].cpu().double()).abs() <= 2 * bound).all())


def _producer_model(dim, adapter):
    kw = dict(v_appear_feat_dim=dim, v_motion_feat_dim=dim, adapter_module=adapter)
    return P.get_model("ego4d", 0, **kw)[0]


@pytest.mark.parametrize("adapter", ["linear", "none"])
@pytest.mark.parametrize("dim", [32, 256, 512])
def test_producers_store_the_fp32_value_rounded_once(dim, adapter):
    """cone_rows_to_bf16 and cone_adapter_norm_bf16 (renorm 0 / 1; an ``adapter_module none`` handle passes through) are
    bit-equal to the fp32 entry followed by torch's .bfloat16(); rows past the end of a NaN-filled output stay untouched."""
    from cone_amd import _lib
    dev = P._gpu()
    lib = _lib.load()
    model = _producer_model(dim, adapter)
    h = model._h()
    nan16 = torch.tensor(float("nan")).bfloat16().view(torch.int16).item()
    for n in (1, 63, 64, 1000):
        g = torch.Generator().manual_seed(100 * dim + n)
        x = (torch.randn(n, dim, generator=g) * torch.rand(n, 1, generator=g) * 3).to(dev)
        out = torch.full((n + 2, dim), float("nan"), dtype=torch.bfloat16, device=dev)
        _lib.check(lib.cone_rows_to_bf16(_lib.ptr(x), n, dim, _lib.ptr(out), _lib.stream()))
        assert torch.equal(out[:n].view(torch.int16), x.bfloat16().view(torch.int16)), ("rows_to_bf16", n)
        assert bool((out[n:].view(torch.int16) == nan16).all())
        for renorm in (0, 1):
            want = model.adapter_norm(x, renorm=bool(renorm)).bfloat16()
            out = torch.full((n + 2, dim), float("nan"), dtype=torch.bfloat16, device=dev)
            nbytes = lib.cone_adapter_norm_workspace(h, n)
            ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
            _lib.check(lib.cone_adapter_norm_bf16(h, _lib.ptr(x), n, _lib.ptr(out), renorm, _lib.ptr(ws), ws.numel(),
                                                  _lib.stream()))
            torch.cuda.synchronize()
            assert torch.equal(out[:n].view(torch.int16), want.view(torch.int16)), ("adapter_norm_bf16", n, renorm)
            assert bool((out[n:].view(torch.int16) == nan16).all())
            assert torch.equal(model.adapter_norm(x, renorm=bool(renorm), out_dtype=torch.bfloat16), want)
    if adapter == "linear":          # the L2 norm's bf16 store against cone_l2_normalize_rows + .bfloat16(), through renorm = 1 above
        assert not torch.equal(want.float(), x)


def test_grouped_entry_equals_the_single_video_streaming_form():
    """A ragged three-video split (ctx_l 1, 137, 2 300; 11 queries, one video with 6): window scores torch.equal to the
    single-video entry's streaming form on the same rows; top-k rows = the stable descending sort, -1 padded."""
    from cone_amd import ops
    dev = P._gpu()
    W, S, dv, k = 90, 45, 256, 6
    lens, per_video = [1, 137, 2300], [2, 6, 3]
    rows = _unit_rows(sum(lens), dv, 5)
    cls = _unit_rows(11, dv, 6)
    arena = ops.rows_to_bf16(rows.to(dev))
    cls_d = cls.to(dev)
    off = np.concatenate([[0], np.cumsum(lens)])
    g_row0, g_ctx_l, g_q, q_ctx = [], [], [], []
    # queries spread unevenly: video order 1, 0, 1, 2, 1, ... by hand
    q_vid = [1, 0, 1, 2, 1, 1, 2, 0, 1, 2, 1]
    assert [q_vid.count(v) for v in range(3)] == per_video
    for v in range(3):
        qs = [i for i, x in enumerate(q_vid) if x == v]
        for c0 in range(0, len(qs), 4):
            grp = qs[c0:c0 + 4]
            g_row0.append(int(off[v])); g_ctx_l.append(lens[v]); g_q.append(grp + [-1] * (4 - len(grp)))
    q_ctx = np.array([lens[v] for v in q_vid], dtype=np.int64)
    q_nw = (q_ctx + S - 1) // S + 1
    t = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt, device=dev)
    woff = np.concatenate([[0], np.cumsum(q_nw)[:-1]])
    plan = dict(g_row0=t(g_row0, torch.int64), g_ctx_l=t(g_ctx_l, torch.int32), g_q=t(g_q, torch.int32).contiguous(),
                ng=len(g_row0), max_ctx_l=max(lens), q_win_off=t(woff, torch.int64), q_ctx_l=t(q_ctx, torch.int32),
                win_total=int(q_nw.sum()))
    idx, fs, ws = ops.prefilter_batched(arena, cls_d, plan, W, k)
    torch.cuda.synchronize()
    assert fs is None
    for q, v in enumerate(q_vid):
        one = ops.prefilter_scores(arena[off[v]:off[v + 1]], cls_d[q:q + 1].contiguous(), W, frame_scores=False)[1][0]
        mine = ws[woff[q]:woff[q] + q_nw[q]]
        assert torch.equal(mine, one), (q, v)
        assert idx[q].tolist() == R.stable_topk(mine.cpu(), k), (q, v)


def _planted_store():
    from cone_amd import inference as inf
    model = P.get_model("ego4d", 0)[0]
    opt, ann, vf, qf = planted_split()
    return inf, model, opt, ann, inf.FeatureStore(opt, ann, vf, qf)


def _fp32_window_scores(inf, model, store, opt):
    from cone_amd import ops
    plan = store.prefilter_plan()
    r0, r1 = plan["band"]
    ctx = model.adapter_norm(ops.l2_normalize(store.vid_raw[r0:r1], 1e-5))
    cls = store.cls_raw if store.cls_normalized else ops.l2_normalize(store.cls_raw, 1e-5)
    _, _, ws = ops.prefilter_batched(ctx, cls, plan, opt.max_v_l, opt.topk_window)
    off = plan["q_win_off"].tolist() + [plan["win_total"]]
    return [ws[off[q]:off[q + 1]].cpu().double() for q in range(len(off) - 1)]


def test_predict_split_rank_lists_obey_the_derived_rule_and_the_flag_switches_back():
    """opt.prefilter_bf16 against the default on the planted synthetic split: every fp32 top-K window that clears the fp32
    (K+1)-th by more than 2 eps is in the bf16 top-K, no bf16 top-K window scores below the fp32 K-th minus 2 eps (eps =
    2^-8 (1 + 2^-9) + 256 2^-23, unit-norm rows); rule 1 covers the top-1 of at least half of the queries (recorded).
    Downstream is well formed, and switching the flag off restores the default's outputs torch.equal."""
    inf, model, opt, ann, store = _planted_store()
    K = opt.topk_window
    l0, w0, t0, r0 = B._run(inf, model, store, opt)
    opt.prefilter_bf16 = True
    l1, w1, t1, r1 = B._run(inf, model, store, opt)
    opt.prefilter_bf16 = False
    l2, w2, t2, r2 = B._run(inf, model, store, opt)
    assert torch.equal(w0, w2) and l0 == l2
    for k in r0:
        assert torch.equal(r0[k], r2[k]), k
    wins = _fp32_window_scores(inf, model, store, opt)
    covered = 0
    for q, row in enumerate(wins):
        assert w0[q].tolist() == R.stable_topk(row.float(), K)             # the default run ranks these very scores
        missing, intruders = R.check_rank_rule(row, w1[q].tolist(), K)
        assert not missing and not intruders, (q, missing, intruders)
        covered += R.covered_top1(row, K)
    P.record_measured("prefilter_bf16_predict_split", queries=len(wins), top1_covered_by_rule_1=covered,
                      same_topk_set=sum(set(a) == set(b) for a, b in zip(w0.tolist(), w1.tolist())))
    assert covered * 2 >= len(wins)
    # downstream of the ranking: one list per query, moments ordered by score, finite
    assert len(l1[0]) == len(l0[0]) == len(ann)
    for a, b in zip(l1[0], l0[0]):
        assert {k: v for k, v in a.items() if k != "predicted_times"} == {k: v for k, v in b.items() if k != "predicted_times"}
        pa = a["predicted_times"]
        assert len(pa) > 0 and all(np.isfinite(m).all() and m[0] <= m[1] for m in pa)
        sc = [m[-1] for m in pa]                                           # the fused list's own score column
        assert sc == sorted(sc, reverse=True)
    for k in t1:
        assert t1[k].shape == t0[k].shape, k


def test_a_graph_captured_in_one_mode_is_not_replayed_in_the_other():
    inf, model, opt, ann, store = _planted_store()
    opt.hip_graph = True

    def run():
        lists, info = inf.predict_split(model, store, opt)
        torch.cuda.synchronize()
        return lists, info["win_idx"].clone()

    la, wa = run()
    la2, wa2 = run()                                    # replay
    opt.prefilter_bf16 = True
    lb, wb = run()
    opt.hip_graph = False
    le, we = run()                                      # the mode, eager
    opt.prefilter_bf16, opt.hip_graph = False, True
    lc, wc = run()
    assert torch.equal(wa, wa2) and torch.equal(wa, wc) and la == la2 == lc
    assert torch.equal(wb, we) and lb == le
    assert len(store.__dict__["_graphs"]) == 2


def test_cli_prefilter_bf16_end_to_end(golden_dir, tmp_path):
    """``python -m cone_amd.inference ... --prefilter_bf16`` on the e2e_ego4d inputs: the same files, ids and counts as the
    default run.  Recorded, not asserted: the share of queries whose top-K window set (hence every file) equals the default's
    is not visible in the files, so the share of equal prediction lists and of top-1 moments with tIoU >= 0.7 are."""
    name = "e2e_ego4d"
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
    got, _ = D._cli(case, "prefilter_bf16", ["--prefilter_bf16"])
    assert sorted(os.listdir(got)) == sorted(os.listdir(ref))
    n_q = n_top1 = n_same = 0
    for tag in ("", "proposal_", "matching_"):
        fn = f"inference_{preset}_test_golden_{tag}preds.json"
        a, b = B._rows(got / fn, preset), B._rows(ref / fn, preset)
        assert len(a) == len(b) == len(ann)
        for ga, rb in zip(a, b):
            assert {k: v for k, v in ga.items() if k != "predicted_times"} == {k: v for k, v in rb.items() if k != "predicted_times"}
            pa, pb = ga["predicted_times"], rb["predicted_times"]
            assert len(pa) == len(pb) and len(pa) > 0
            if tag == "":
                n_q += 1
                n_top1 += B._iou(pa[0][:2], pb[0][:2]) >= 0.7
                n_same += pa == pb              # the same windows went into stage B: the same moments come out
    P.record_measured(f"prefilter_bf16_cli_e2e[{name}]", queries=n_q, same_window_set_share=n_same / n_q,
                      top1_tiou_ge_0p7_with_default_share=n_top1 / n_q)


def test_localizer_returns_moments_and_graph_equals_eager():
    from cone_amd.localizator import CONELocalizator, LOCALIZER_OPT
    from types import SimpleNamespace
    dev = P._gpu()
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(SimpleNamespace(**LOCALIZER_OPT), 0).items()}
    g = torch.Generator().manual_seed(9)
    vid, tok, cls = torch.randn(400, 256, generator=g), torch.randn(9, 768, generator=g), torch.randn(256, generator=g)
    vid[130:133] = cls
    eager = CONELocalizator(state_dict=sd, prefilter_bf16=True)
    graph = CONELocalizator(state_dict=sd, prefilter_bf16=True, hip_graph=True)
    a = eager.predict_moment(vid, (tok, cls))
    b = graph.predict_moment(vid, (tok, cls))
    c = graph.predict_moment(vid, (tok, cls))           # the replay
    assert len(a) > 0 and all(np.isfinite(m).all() and m[0] <= m[1] for m in a)
    assert a == b == c
    assert all(key[2] is True for key in graph._consts)         # the capture cache is keyed by the mode


def test_refusals_name_what_they_refuse():
    from cone_amd import _lib, ops
    dev = P._gpu()
    ctx, cls = _case(91, 256)
    arena = ops.rows_to_bf16(ctx.to(dev))
    cls_d = cls[:2].to(dev).contiguous()
    with pytest.raises(ValueError, match="frame_scores"):
        ops.prefilter_scores(arena, cls_d, 90, frame_scores=True)
    with pytest.raises(ValueError, match="split_bf16"):
        ops.prefilter_scores(arena, cls_d, 90, frame_scores=False, split_bf16=True)
    buf = torch.zeros(91 * 256 + 8, dtype=torch.bfloat16, device=dev)
    shifted = buf[4:4 + 91 * 256].view(91, 256)                 # 8 B past a 16-B boundary
    assert shifted.data_ptr() % 16 == 8
    with pytest.raises(_lib.ConeHipError, match="16-B aligned"):
        ops.prefilter_scores(shifted, cls_d, 90, frame_scores=False)
    with pytest.raises(_lib.ConeHipError, match="multiple of 32"):
        ops.prefilter_scores(ops.rows_to_bf16(_unit_rows(8, 48, 1).to(dev)), _unit_rows(1, 48, 2).to(dev), 90, frame_scores=False)
    from cone_amd import parallel as par
    with pytest.raises(ValueError, match="prefilter_bf16"):
        par.prefilter_ctx_sharded(arena, 91, cls_d, 90, 2, prefilter_bf16=True)
