"""The inference CLI / eval_epoch sharded over N ranks, on the CPU: eval_epoch(..., group=...) over gloo worlds 2 and 3 with
the oracle as the per-rank compute (CheckerHooks of tests/test_parallel_cpu.py), the shard-plan rule, and the launcher of
``python -m cone_amd.inference --gpus N`` (CONE_DIST_LAUNCH_CHECK=1: rendezvous + preflight, no GPU)."""
import json
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from cone_amd import parallel as par
from cone_amd import synth
from cone_amd.config import make_opt
from oracle import cone_oracle as O
from test_parallel_cpu import CheckerHooks, _cpu_window_scores, _free_port, _long_video_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(name):
    """(opt, ann, vf, qf, one_video): the splits of the distributed eval_epoch cases."""
    if name == "ego4d_test":        # several videos: the replicated plan
        opt = make_opt("ego4d", nms_thd=0.5, topk_window=3, eval_bsz=4, max_after_nms=5, eval_split_name="test",
                       save_all=True)
        ann, vf, qf = synth.make_dataset(opt, 10, 3, seed=9, ctx_range=(20, 120))
        return opt, ann, vf, qf, False
    if name == "ego4d_debug":       # --debug: the first eval_bsz queries only
        opt = make_opt("ego4d", nms_thd=0.5, topk_window=3, eval_bsz=4, max_after_nms=5, eval_split_name="test",
                       debug=True)
        ann, vf, qf = synth.make_dataset(opt, 11, 3, seed=4, ctx_range=(30, 200))
        return opt, ann, vf, qf, False
    if name == "mad_one_video":     # MAD JSONL, an unscored split, ONE video: the ctx plan
        opt = make_opt("mad", nms_thd=0.5, topk_window=4, eval_bsz=3, max_after_nms=5, eval_split_name="train",
                       save_all=True)
        ann, vf, qf = _long_video_case(opt, 7, 900, 3)
        return opt, ann, vf, qf, True
    if name == "tiny":              # 1 query x 2 windows: at world 3 one rank owns no window (and no clip row)
        opt = make_opt("ego4d", nms_thd=0.5, topk_window=3, eval_bsz=4, max_after_nms=5, eval_split_name="test")
        ann, vf, qf = _long_video_case(opt, 1, 30, 7)
        return opt, ann, vf, qf, True
    raise KeyError(name)


CASES = ("ego4d_test", "ego4d_debug", "mad_one_video", "tiny")


def _expected(opt, sd, ann, vf, qf, store, one_video):
    """The single-process answer: the oracle's three submission lists (and the rank lists the hooks serve)."""
    if not one_video:
        (fo, po, mo), ranks, _ = O.eval_epoch(sd, opt, ann, vf, qf)
    else:       # the ctx plan scores the store's raw rows (exactly representable: see _long_video_case)
        full = _cpu_window_scores(store.vid_raw, store.cls_raw, opt.max_v_l)
        ranks = {r["query_id"]: O.rank_windows(full[i]) for i, r in enumerate(ann)}
        with torch.no_grad():
            fo, po, mo = O.postprocess(O.compute_mr_results(sd, opt, ann, vf, qf, ranks), opt)
    if opt.debug:
        fo, po, mo = fo[:opt.eval_bsz], po[:opt.eval_bsz], mo[:opt.eval_bsz]
    return (fo, po, mo), ranks


def _worker(rank, world, port, out, root):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cone_amd import inference as inf
        for name in CASES:
            opt, ann, vf, qf, one_video = _case(name)
            opt.results_dir = os.path.join(root, name, f"rank{rank}")
            os.makedirs(opt.results_dir)
            sd = synth.make_state_dict(opt, 0)
            store = inf.FeatureStore(opt, ann, vf, qf, device=torch.device("cpu"), cls_normalized=one_video)
            assert par.shard_plan(store, world) == ("ctx" if one_video else "replicated")
            lists, ranks = _expected(opt, sd, ann, vf, qf, store, one_video)
            hooks = CheckerHooks(opt, sd, ann, vf, qf, store, ranks=ranks)
            ext = "jsonl" if opt.dset_name == "mad" else "json"
            fn = f"inference_{opt.dset_name}_{opt.eval_split_name}_t_preds.{ext}"
            got = inf.eval_epoch(None, store, opt, fn, group=dist.group.WORLD, hooks=hooks)
            if rank == 0:       # the single-process files, written from the oracle's lists
                ref = os.path.join(root, name, "expected")
                os.makedirs(ref)
                inf.write_submissions(SimpleNamespace(**dict(vars(opt), results_dir=ref)), *lists, fn)
            dist.barrier()
            # every rank returns rank 0's tuple
            objs = [None] * world
            dist.all_gather_object(objs, got)
            assert all(o == objs[0] for o in objs), name
            assert got[0] is None and got[1] is None and got[2] == [] and len(got[3]) == (3 if opt.save_all else 1)
            assert all(p.startswith(os.path.join(root, name, "rank0")) for p in got[3])
            if rank == 0:
                mine, ref_files = sorted(os.listdir(opt.results_dir)), sorted(os.listdir(ref))
                assert mine == ref_files and len(mine) == len(got[3]), (name, mine, ref_files)
                for f in mine:
                    with open(os.path.join(opt.results_dir, f), "rb") as a, open(os.path.join(ref, f), "rb") as b:
                        assert a.read() == b.read(), (name, f)
            else:
                assert os.listdir(opt.results_dir) == [], name          # only rank 0 writes
            if name == "tiny" and world == 3:
                assert par.ctx_shard(int(store.ctx_l[0]), opt.max_v_l, 2, 3)[:2] == (2, 2)   # rank 2 owned no window
        if rank == 0:
            out.put("ok")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_eval_epoch_sharded_writes_the_single_process_files(world, tmp_path):
    """eval_epoch(..., group=...) on every rank: the replicated plan (Ego4D JSON, also with --debug), the ctx plan (a MAD JSONL
    split of ONE video), a rank without windows; rank 0 alone writes, byte for byte the files of the oracle's lists, and
    every rank returns the same tuple."""
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, out, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert out.get(timeout=5) == "ok"


def _err_worker(rank, world, port, out, root):
    """Rank 0 fails after the sharded step (here: the Ego4D ground truth of a val split is missing): every rank raises,
    none is left waiting in a collective."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cone_amd import inference as inf
        opt, ann, vf, qf, _ = _case("ego4d_test")
        opt.eval_split_name = "val"
        opt.ego4d_gt_path = os.path.join(root, "no_such_dir", "nlq_val.json")
        opt.results_dir = os.path.join(root, f"rank{rank}")
        os.makedirs(opt.results_dir)
        sd = synth.make_state_dict(opt, 0)
        store = inf.FeatureStore(opt, ann, vf, qf, device=torch.device("cpu"))
        hooks = CheckerHooks(opt, sd, ann, vf, qf, store)
        with pytest.raises(FileNotFoundError if rank == 0 else RuntimeError) as e:
            inf.eval_epoch(None, store, opt, "inference_ego4d_val_t_preds.json", group=dist.group.WORLD, hooks=hooks)
        assert rank == 0 or "rank 0 of the evaluation failed: FileNotFoundError" in str(e.value), e.value
        dist.barrier()
        if rank == 0:
            out.put([sorted(os.listdir(os.path.join(root, f"rank{r}"))) for r in range(world)])
    finally:
        dist.destroy_process_group()


def test_gloo_eval_epoch_rank0_failure_reaches_every_rank(tmp_path):
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_err_worker, args=(r, 2, port, out, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    written, other = out.get(timeout=5)
    assert "inference_ego4d_val_t_preds.json" in written and other == []      # rank 0 wrote before the scoring failed


def test_shard_plan_rule():
    from cone_amd import inference as inf
    opt = make_opt("ego4d", topk_window=3, eval_bsz=4)
    ann, vf, qf = synth.make_dataset(opt, 9, 3, seed=2, ctx_range=(30, 120))
    many = inf.FeatureStore(opt, ann, vf, qf, device=torch.device("cpu"))
    ann1, vf1, qf1 = synth.make_dataset(opt, 5, 1, seed=3, ctx_range=(300, 301))
    one = inf.FeatureStore(opt, ann1, vf1, qf1, device=torch.device("cpu"))
    assert [par.shard_plan(one, w) for w in (1, 2, 3, 8)] == ["plain", "ctx", "ctx", "ctx"]
    assert [par.shard_plan(many, w) for w in (1, 2, 3, 8)] == ["plain", "replicated", "replicated", "replicated"]
    # the rule reads the queries' videos: a view whose queries all refer to one video of a bigger arena is a ctx split
    q_vid = many.q_vid.tolist()
    a = q_vid.index(q_vid[0])
    b = a + q_vid.count(q_vid[0])
    assert par.shard_plan(many.view(a, b), 2) == "ctx" and par.shard_plan(many.view(a, b + 1), 2) == "replicated"


# ---------------------------------------------------------------------------------------------- the launcher
def _plain_env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
                                                            "LOCAL_WORLD_SIZE", "GROUP_RANK", "TORCHELASTIC_RUN_ID")}
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    env.update(kw)
    return env


def _cli(args, env, cwd, timeout=600):
    return subprocess.run([sys.executable, "-m", "cone_amd.inference"] + args, env=env, cwd=cwd, capture_output=True,
                          text=True, timeout=timeout)


def test_cli_gpus_2_starts_its_own_ranks(tmp_path):
    """`python -m cone_amd.inference --gpus 2` from a plain shell: the process starts torch.distributed.run as a child, the two
    ranks rendezvous and pass the collective preflight (gloo, CPU tensors: CONE_DIST_LAUNCH_CHECK=1 stops there), rank 0's ONE
    JSON line and the exit status are relayed."""
    args = ["--gpus", "2", "--dist_backend", "gloo", "--eval_bsz", "8", "--topk_window", "5"]
    r = _cli(args, _plain_env(CONE_DIST_LAUNCH_CHECK="1"), str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["launch_check"] and res["n_gpus"] == 2 and res["ranks_seen"] == 2
    pf = res["collective_preflight"]
    assert pf["ok"] and pf["world"] == 2 and pf["backend"] == "gloo" and pf["bytes_per_rank"] == 8 * 5 * 5 * 4 * 4


def test_cli_launch_check_failure_and_world_mismatch_exit_nonzero(tmp_path):
    r = _cli(["--gpus", "2"], _plain_env(CONE_DIST_LAUNCH_CHECK="1", CONE_DIST_LAUNCH_CHECK_FAIL_RANK="1"), str(tmp_path))
    assert r.returncode != 0
    assert "collective preflight failed on rank" in r.stderr and "of 2 (gloo)" in r.stderr, r.stderr[-3000:]
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    env = _plain_env(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    r = _cli(["--gpus", "2"], env, str(tmp_path), timeout=300)
    assert r.returncode == 2 and "--gpus 2 but the launcher started WORLD_SIZE=1" in r.stderr, r.stderr[-2000:]


def test_nothing_in_the_package_replaces_its_process():
    pat = re.compile(r"\bos\.exec\w*|\bexecv\w*")
    pkg = os.path.join(ROOT, "cone_amd")
    hits = []
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                with open(os.path.join(dirpath, f)) as fh:
                    hits += [(f, i) for i, ln in enumerate(fh, 1) if pat.search(ln)]
    assert hits == []


def test_opt_json_never_overrides_the_launch_options(tmp_path):
    from cone_amd.config import build_parser, parse_test_options
    a = build_parser().parse_args([])
    assert a.gpus == 1 and a.dist_backend == "nccl"
    (tmp_path / "opt.json").write_text(json.dumps(dict(vars(make_opt("ego4d")), gpus=4, dist_backend="gloo")))
    opt = parse_test_options(["--resume", str(tmp_path / "model_best.ckpt")])
    assert opt.gpus == 1 and opt.dist_backend == "nccl"
    opt = parse_test_options(["--resume", str(tmp_path / "model_best.ckpt"), "--gpus", "3", "--dist_backend", "gloo"])
    assert opt.gpus == 3 and opt.dist_backend == "gloo"
