"""Multi-GPU launch of the inference CLI: ``python -m cone_amd.inference ... --gpus N``.

A plain process (no ``RANK`` in the environment) with N > 1 becomes a launcher before it loads libcone_hip.so or makes any
GPU call: it starts ``python -m torch.distributed.run --standalone ... -m cone_amd.inference <same arguments>`` as a CHILD
process (never an exec), relays the child's stdout (stderr is inherited) and returns its exit status -- bench.py's
``self_launch``.  A process started by ``torch.distributed.run`` (ours or the user's own torchrun) is a rank: it binds
``cuda:LOCAL_RANK``, joins the default process group and runs a collective preflight before the evaluation.

Test-only environment switches (never set by the launcher):
  * ``CONE_DIST_ONE_DEVICE=1``  -- every rank on the ``--device`` GPU, so that a one-GPU box runs N = 2 or 3 over
    ``--dist_backend gloo`` (RCCL refuses two ranks on one device);
  * ``CONE_DIST_LAUNCH_CHECK=1`` -- launcher + rendezvous + preflight only, over gloo on CPU tensors: rank 0 prints one JSON
    line and the ranks exit (no GPU needed);
  * ``CONE_DIST_LAUNCH_CHECK_FAIL_RANK=r`` -- with the launch check: rank r sends a wrong value, so the preflight fails.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
import time

import torch

PROG = "cone_amd.inference"


def launched_as_rank() -> bool:
    return "RANK" in os.environ


def rank_env():
    """(rank, world, local_rank) as torch.distributed.run sets them."""
    return (int(os.environ["RANK"]), int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("LOCAL_RANK", "0")))


def self_launch(n_gpus: int, argv, module: str = PROG) -> int:
    """Start ``n_gpus`` ranks of ``python -m module argv`` through torch.distributed.run as a child process, relay its
    stdout and return its exit status.  The child runs in the caller's working directory (relative paths of the command
    line, and the reference's hard-coded ground-truth path, keep their meaning) and imports this same package."""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC: RCCL across processes needs it
    env.setdefault("OMP_NUM_THREADS", "1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = root + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    py = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    # --standalone: the launcher's own c10d rendezvous picks a free port itself
    cmd = py + ["-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
                "--nproc-per-node", str(n_gpus), "-m", module] + list(argv)
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    for line in proc.stdout:
        sys.stdout.write(line)
        sys.stdout.flush()
    return proc.wait()


def fail(msg: str, code: int = 2, hard: bool = False):
    """One line on stderr, then exit (no stack of frames in the middle of N ranks' output).  ``hard``: after a failed
    collective -- leave at once, without tearing down a communicator that may be in a broken state."""
    sys.stderr.write(f"{PROG}: {msg}\n")
    sys.stderr.flush()
    if hard:
        sys.stdout.flush()
        os._exit(code)
    sys.exit(code)


def rank_device(local_rank: int, device: int) -> torch.device:
    """cuda:LOCAL_RANK, or the --device GPU for every rank under CONE_DIST_ONE_DEVICE=1 (test-only)."""
    idx = device if os.environ.get("CONE_DIST_ONE_DEVICE") == "1" else local_rank
    return torch.device("cuda", idx)


def init_group(backend: str, device: torch.device):
    """The default process group of the ranks; RCCL gets its device eagerly (one communicator, created here)."""
    import torch.distributed as dist
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=device)
    else:
        dist.init_process_group(backend)
    return dist.group.WORLD


def preflight(shape, backend: str, device="cuda"):
    """ONE all_gather_into_tensor of the step's message shape (the window-sharded step gathers (rows, num_queries, 4) fp32
    per rank) on the default group, checked for rank order and values.  A failure becomes one line naming rank, world and
    backend on stderr and exit status 3 instead of a hang or a stack of C++ frames later in the run."""
    import torch.distributed as dist
    rank, world = dist.get_rank(), dist.get_world_size()
    try:
        t0 = time.perf_counter()
        val = float(rank)
        if os.environ.get("CONE_DIST_LAUNCH_CHECK_FAIL_RANK") == str(rank):
            val = -1.0                                      # test-only: this rank sends a wrong value
        send = torch.full(tuple(shape), val, dtype=torch.float32, device=device)
        recv = torch.empty((world * shape[0],) + tuple(shape[1:]), dtype=torch.float32, device=device)
        dist.all_gather_into_tensor(recv, send)
        want = torch.arange(world, dtype=torch.float32, device=device).repeat_interleave(shape[0])
        if not bool((recv.reshape(world * shape[0], -1) == want[:, None]).all()):
            raise RuntimeError("gathered shards are not in rank order / not the values the ranks sent")
        return {"ok": True, "backend": backend, "world": world, "bytes_per_rank": int(send.numel() * 4),
                "first_collective_ms": round((time.perf_counter() - t0) * 1e3, 2)}
    except Exception as e:          # noqa: BLE001
        fail(f"collective preflight failed on rank {rank} of {world} ({backend}): "
             f"{type(e).__name__}: {str(e).splitlines()[0] if str(e) else ''}", 3, hard=True)


def launch_check(shape):
    """CONE_DIST_LAUNCH_CHECK=1: the ranks rendezvous over gloo on CPU tensors and run the preflight; rank 0 prints one
    JSON line."""
    import torch.distributed as dist
    dist.init_process_group("gloo")
    try:
        pf = preflight(shape, "gloo", device="cpu")
        if dist.get_rank() == 0:
            print(json.dumps({"launch_check": True, "n_gpus": dist.get_world_size(), "ranks_seen": dist.get_world_size(),
                              "collective_preflight": pf}), flush=True)
    finally:
        dist.destroy_process_group()
