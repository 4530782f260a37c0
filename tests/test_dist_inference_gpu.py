"""The inference CLI sharded over N ranks on the GPU: `python -m cone_amd.inference ... --gpus N` writes the same bytes as the
plain single-process run.  A one-GPU box cannot host two RCCL ranks, so the N > 1 runs put every rank on the one GPU
(CONE_DIST_ONE_DEVICE=1) over gloo; the 1-rank run under torch.distributed.run uses RCCL.  Every run is a subprocess under a
time limit, at most three GPU processes at once."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cone_amd import synth
from cone_amd.config import make_opt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCH_VARS = ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "GROUP_RANK", "MASTER_ADDR", "MASTER_PORT",
               "TORCHELASTIC_RUN_ID")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in LAUNCH_VARS}
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    env.update(kw)
    return env


def _run(cmd, cwd, env, timeout=600):
    r = subprocess.run(cmd, cwd=str(cwd), env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (cmd, r.stdout[-2000:], r.stderr[-4000:])
    return r


def _cli(case, tag, extra, n_gpus=None, torchrun=False):
    """One CLI run of `case` into its own results directory; returns (directory, stdout)."""
    out = case["dir"] / f"out_{tag}"
    out.mkdir()
    args = case["argv"] + ["--eval_results_dir", str(out)] + extra
    env = _env()
    if torchrun:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
               "--nproc-per-node", "1", "-m", "cone_amd.inference"] + args + ["--gpus", "1"]
    else:
        cmd = [sys.executable, "-m", "cone_amd.inference"] + args
        if n_gpus:
            cmd += ["--gpus", str(n_gpus), "--dist_backend", "gloo"]
            env["CONE_DIST_ONE_DEVICE"] = "1"
    return out, _run(cmd, case["dir"], env).stdout


def _same_files(a, b, names):
    got = sorted(os.listdir(a))
    assert got == sorted(os.listdir(b)) and set(names) <= set(got), (got, names)
    for f in got:
        assert (a / f).read_bytes() == (b / f).read_bytes(), f


def _checkpoint(d, saved, seed):
    sdn = synth.make_state_dict(saved, seed)
    ckpt = d / "run"
    ckpt.mkdir()
    torch.save({"model": {k: torch.from_numpy(v) for k, v in sdn.items()}, "epoch": 2}, ckpt / "model_best.ckpt")
    with open(ckpt / "opt.json", "w") as f:
        json.dump({k: v for k, v in vars(saved).items() if isinstance(v, (int, float, str, bool, type(None)))}, f)
    return str(ckpt / "model_best.ckpt")


def _packed(d, opt, ann, vf, qf, name):
    from cone_amd import inference as inf
    eval_path = d / f"{name}.jsonl"
    eval_path.write_text("\n".join(json.dumps(r) for r in ann))
    store = inf.FeatureStore(opt, ann, vf, qf, device=torch.device("cpu"))
    return str(eval_path), store.save_packed(str(d / f"{name}.conefs"))


def _ego4d_ground_truth(ann):
    gt = {"videos": [{"clips": []}]}
    for r in ann:
        uid, qidx = r["query_id"].split("_")
        c = next((c for c in gt["videos"][0]["clips"] if c["clip_uid"] == r["clip_id"]), None)
        if c is None:
            c = {"clip_uid": r["clip_id"], "annotations": []}
            gt["videos"][0]["clips"].append(c)
        a = next((a for a in c["annotations"] if a["annotation_uid"] == uid), None)
        if a is None:
            a = {"annotation_uid": uid, "language_queries": {}}
            c["annotations"].append(a)
        a["language_queries"][int(qidx)] = {"clip_start_sec": r["timestamps"][0], "clip_end_sec": r["timestamps"][1]}
    for c in gt["videos"][0]["clips"]:
        for a in c["annotations"]:
            m = max(a["language_queries"])
            a["language_queries"] = [a["language_queries"].get(i, {"clip_start_sec": 0.0, "clip_end_sec": 1.0})
                                     for i in range(m + 1)]
    return gt


@pytest.fixture(scope="module")
def ego4d_case(tmp_path_factory):
    """Checkpoint + opt.json, a packed Ego4D val split of 13 queries over 2 videos, and the ground truth at the path the
    reference hard-codes (relative to the working directory of the runs)."""
    d = tmp_path_factory.mktemp("ego4d")
    saved = make_opt("ego4d", nms_thd=0.5, topk_window=4, eval_bsz=8, max_after_nms=7)
    resume = _checkpoint(d, saved, 3)
    ann, vf, qf = synth.make_dataset(saved, 13, 2, seed=6, ctx_range=(150, 400))
    rng = np.random.default_rng(1)
    for r in ann:
        a = float(rng.uniform(0, 0.7 * r["duration"]))
        r["timestamps"] = [round(a, 3), round(a + 12.5, 3)]
    (d / "data" / "ego4d_ori_data").mkdir(parents=True)
    (d / "data" / "ego4d_ori_data" / "nlq_val.json").write_text(json.dumps(_ego4d_ground_truth(ann)))
    eval_path, packed = _packed(d, saved, ann, vf, qf, "val")
    argv = ["--resume", resume, "--eval_split_name", "val", "--eval_path", eval_path, "--eval_id", "t1",
            "--packed_features", packed, "--nms_thd", "0.5", "--topk_window", "5", "--max_after_nms", "7", "--eval_bsz", "8",
            "--save_all"]
    return dict(dir=d, argv=argv, plain={})


EGO4D_FILES = ["inference_ego4d_val_t1_preds.json", "inference_ego4d_val_t1_proposal_preds.json",
               "inference_ego4d_val_t1_matching_preds.json", "inference_ego4d_val_t1_preds.txt"]


def _plain(case, tag, extra):
    if tag not in case["plain"]:
        case["plain"][tag] = _cli(case, "plain_" + tag, extra)
    return case["plain"][tag]


@pytest.mark.parametrize("tag,extra", [("default", []), ("debug", ["--debug"]), ("split_bf16", ["--split_bf16"])])
def test_cli_two_ranks_write_the_single_gpu_files(ego4d_case, tag, extra):
    """Ego4D val (several videos: the replicated plan), `--gpus 2`: prediction files and metric .txt byte-identical to the plain
    run of the same command line; each table printed once (rank 0 alone prints)."""
    ref, ref_out = _plain(ego4d_case, tag, extra)
    got, out = _cli(ego4d_case, "two_" + tag, extra, n_gpus=2)
    _same_files(got, ref, EGO4D_FILES)
    for title in ("Window Pre-filtering Epoch", "Fusion Epoch", "Proposal Epoch", "Matching Epoch", "total model running time"):
        assert out.count(title) == 1 == ref_out.count(title), title
    if tag == "debug":
        sub = json.loads((got / EGO4D_FILES[0]).read_text())
        assert len(sub["results"]) == 8             # the first batch of eval_bsz queries only


def test_cli_one_rccl_rank_under_torchrun(ego4d_case):
    """`torch.distributed.run --nproc-per-node 1 -m cone_amd.inference ... --gpus 1`: one RCCL rank, the preflight passes,
    and the distributed code path (plan "plain") writes the plain run's bytes."""
    ref, _ = _plain(ego4d_case, "default", [])
    got, out = _cli(ego4d_case, "torchrun1", [], torchrun=True)
    _same_files(got, ref, EGO4D_FILES)
    assert out.count("Fusion Epoch") == 1


def _mad_case(d, nq, seed):
    """ONE long MAD video and nq queries; the clip rows are drawn from a small pool of coarse rows, so that many windows tie
    EXACTLY (identical rows score identically) and others nearly."""
    saved = make_opt("mad", nms_thd=0.5, topk_window=6, eval_bsz=4, max_after_nms=5)
    resume = _checkpoint(d, saved, 4)
    ann, vf, qf = synth.make_dataset(saved, nq, 1, seed=seed, ctx_range=(2600, 2601))
    g = np.random.default_rng(seed)
    for k in vf:
        pool = np.round(g.standard_normal((24, vf[k].shape[1])) * 4) / 4
        vf[k] = pool[g.integers(0, len(pool), vf[k].shape[0])].astype(np.float32)
    for k in qf:
        key = "cls_features" if "cls_features" in qf[k] else "eot_features"
        qf[k][key] = (np.round(g.standard_normal(np.asarray(qf[k][key]).shape) * 2) / 2).astype(np.float32)
    for r in ann:
        a = float(g.uniform(0, 0.8 * r["duration"]))
        r["timestamps"] = [round(a, 3), round(a + 9.5, 3)]
    eval_path, packed = _packed(d, saved, ann, vf, qf, "mad_val")
    argv = ["--resume", resume, "--eval_split_name", "val", "--eval_path", eval_path, "--eval_id", "m",
            "--packed_features", packed, "--nms_thd", "0.5", "--topk_window", "6", "--eval_bsz", "4", "--save_all"]
    return dict(dir=d, argv=argv, plain={}), (saved, ann, vf, qf)


MAD_FILES = ["inference_mad_val_m_preds.jsonl", "inference_mad_val_m_proposal_preds.jsonl",
             "inference_mad_val_m_matching_preds.jsonl", "inference_mad_val_m_preds.txt"]


@pytest.mark.parametrize("nq", [3, 6, 16])
def test_cli_one_long_video_ctx_plan_writes_the_single_gpu_files(tmp_path, nq):
    """MAD val, ONE video (the ctx plan: pre-filter sharded along the video, then the window-sharded model), 2 and 3 ranks, query
    counts on both sides of the pre-filter's kernel switch (CONE_PF_MQ_MIN = 5) and at 16: the same bytes as the plain run."""
    case, _ = _mad_case(tmp_path, nq, seed=nq)
    ref, ref_out = _cli(case, "plain", [])
    for world in (2, 3):
        got, out = _cli(case, f"n{world}", [], n_gpus=world)
        _same_files(got, ref, MAD_FILES)
        assert out.count("Fusion Epoch") == 1 == ref_out.count("Fusion Epoch")


def test_ctx_sharded_prefilter_equals_single_gpu_prefilter(tmp_path):
    """In process: the HIP hooks' ctx-sharded pre-filter of one video == inference.prefilter, element for element -- through the
    driver (a 1-rank group) and rank by rank for worlds 2, 3 and 8 (each rank's local stable top-k, merged as the all_gather
    would), for query counts on both sides of the prefilter_scores kernel switch."""
    import torch.distributed as dist
    from cone_amd import inference as inf
    from cone_amd import ops
    from cone_amd import parallel as par
    from cone_amd.model import build_model
    for nq in (3, 6, 16):
        d = tmp_path / f"q{nq}"
        d.mkdir()
        _, (opt, ann, vf, qf) = _mad_case(d, nq, seed=nq)
        model, _ = build_model(opt)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(opt, 4).items()})
        store = inf.FeatureStore(opt, ann, vf, qf)
        want = inf.prefilter(model, store, opt)
        hooks = par.HipHooks(model)
        ctx_l, k = int(store.ctx_l[0]), opt.topk_window
        for world in (2, 3, 8):
            vals, idxs = [], []
            for r in range(world):
                shard = par.ctx_shard(ctx_l, opt.max_v_l, r, world)
                local = hooks.ctx_rows(store, shard[2], shard[3])
                v, i = par.local_window_topk(local, shard, hooks.cls_norm(store), opt.max_v_l, k, hooks.window_scores_fn,
                                             ops.topk_windows)
                vals.append(v)
                idxs.append(i)
            gi, _ = par.merge_topk(torch.cat(vals, 1), torch.cat(idxs, 1), k, ops.topk_windows)
            assert torch.equal(gi, want), (nq, world)
        if nq == 6:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29547")
            dist.init_process_group("gloo", rank=0, world_size=1)
            try:
                assert torch.equal(par.prefilter_one_video_ctx_sharded(store, opt, hooks), want)
            finally:
                dist.destroy_process_group()
