"""What the GPU test modules, the rank workers (tests/tools/*_dist_worker.py) and the timing tools (tests/tools/time_*.py)
share: the synthetic scene model, one run of the `mesh_nerf` exporter, the launcher of N ranks under torch.distributed.run,
the 1-rank-against-N comparison, and the timers.  A plain module (`from tests import gpu_support`), not a conftest: it
imports without a GPU and without the built library -- every import of HIP code is inside the function that needs it."""
import contextlib
import io
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RENDEZVOUS = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")


# ---- the scene and the exporter -------------------------------------------------------------------------------------------

def scene_model(device, chunksize=None, weights=None, **hparams):
    """NeRFModel on the synthetic scene: make_scene_weights() in the coarse and in the fine network, eval mode, on `device`.
    `hparams` go to synthetic.hparams(); one with a dot in its name ("experiment.chamfer_loss") sets that entry of the flat
    configuration.  `weights`: another network's arrays for both, those the model has no entry for left out."""
    from nerfmeshes_amd import models, synthetic as S
    if chunksize is not None:
        hparams["chunksize"] = chunksize
    hp = S.hparams(**{k: v for k, v in hparams.items() if "." not in k})
    hp.update({k: v for k, v in hparams.items() if "." in k})
    torch.manual_seed(0)                                     # identical replicas on every rank
    model = models.NeRFModel(hp)
    sd = model.state_dict()
    for prefix in ("model_coarse.", "model_fine."):
        for k, v in (S.make_scene_weights() if weights is None else weights).items():
            if prefix + k in sd:
                sd[prefix + k] = torch.from_numpy(np.ascontiguousarray(v))
    model.load_state_dict(sd)
    return model.eval().to(device)


def export_args(save_dir, *argv):
    """the `mesh_nerf` namespace every exporter test starts from; `argv` comes last, so it wins"""
    from nerfmeshes_amd import mesh_nerf
    return mesh_nerf.build_parser().parse_args(["--save-dir", str(save_dir), "--view-disparity-max-bound", "1.0", "--iso-level", "32",
                                                "--batch-size", "4096", *argv])


def export_mesh(model, save_dir, *argv, device="cuda"):
    """`mesh_nerf.export_marching_cubes` with export_args(save_dir, *argv) -> what it returns"""
    from nerfmeshes_amd import mesh_nerf
    args = export_args(save_dir, *argv)
    with torch.no_grad():
        return mesh_nerf.export_marching_cubes(model, args, model.cfg, device)


def gpu_ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X")
    from nerfmeshes_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def ops():
    return gpu_ops()


@pytest.fixture(scope="module")
def scene():
    return scene_model("cuda", chunksize=3000)


def to_device(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def to_numpy(t):
    return None if t is None else t.cpu().numpy()


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


# ---- ranks ----------------------------------------------------------------------------------------------------------------

def single_rank(fn, gather="all_gather_rows"):
    """`fn` as a process outside any group runs it (nd.world() -> (0, 1)): the 1-rank result, computed on this rank.  `gather`
    names the collective of nerfmeshes_amd.dist that `fn` reaches (mesh_surface_ray: all_gather_ragged)."""
    from nerfmeshes_amd import dist as nd
    real = nd.world, getattr(nd, gather)
    nd.world = lambda: (0, 1)
    setattr(nd, gather, lambda local, *counts: local)
    try:
        return fn()
    finally:
        nd.world = real[0]
        setattr(nd, gather, real[1])


def rank_dir(stage, rank, *parts):
    """a fresh directory for one export of one rank"""
    return tempfile.mkdtemp(prefix="_".join(("nm", stage, str(rank), *map(str, parts))) + "_")


def same_export(got, want, what, rank):
    """`got` and `want` are export_marching_cubes' four results and the save directory behind them: the mesh, the normals, the
    colours and, on rank 0, the OBJ of `got` must be those of the 1-rank run `want`, bit for bit."""
    for name, a, b in zip(("vertices", "triangles", "normals"), got[:3], want[:3]):
        assert a.shape == b.shape and torch.equal(a, b), f"{what}: {name} differ from the 1-rank mesh"
    assert got[3].shape == want[3].shape and (got[3] == want[3]).all(), f"{what}: colours differ"
    if rank == 0:
        a = open(os.path.join(got[4], "mesh.obj"), "rb").read()
        assert a == open(os.path.join(want[4], "mesh.obj"), "rb").read(), f"{what}: OBJ differs"


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def clean_env(**extra):
    """os.environ without an enclosing launcher's rendezvous, with HSA's IPC mode that ranks sharing one GPU need, and `extra`"""
    env = dict(os.environ)
    for k in RENDEZVOUS:
        env.pop(k, None)
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    env.update(extra)
    return env


def launch_ranks(worker, world, *args, env=None, timeout=600, ranks_per_gpu=True):
    """`worker` (a script, relative to the repository root) on `world` ranks under torch.distributed.run, rendezvous on
    127.0.0.1, the whole launch under `timeout -k 10`: it ends the group before subprocess.run's own limit is reached.
    `ranks_per_gpu`: the ranks share one GPU over gloo.  -> the CompletedProcess; where it failed, the first worker's own
    traceback stands in front of its stderr."""
    extra = dict(env or {})
    if ranks_per_gpu:
        extra["NERFMESHES_RANKS_PER_GPU"] = str(world)
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={world}", "--master-addr", "127.0.0.1", "--master-port", str(free_port()), worker, *args]
    r = subprocess.run(cmd, cwd=ROOT, env=clean_env(**extra), capture_output=True, text=True, timeout=timeout + 30)
    if r.returncode != 0:      # the launcher's summary hides the workers' own tracebacks: put the first one in front
        lines = r.stderr.splitlines()
        first = next((i for i, ln in enumerate(lines) if ln.startswith("Traceback")), None)
        if first is not None:
            r.stderr = "\n".join(lines[first:first + 40]) + "\n...\n" + r.stderr
            r.stdout = ""
    return r


def assert_ranks_ok(result, marker):
    errors = result.stderr[:6000] if result.stderr.startswith("Traceback") else result.stderr[-6000:]
    assert result.returncode == 0, result.stdout[-3000:] + errors
    assert marker in result.stdout, result.stdout[-2000:]


# ---- timing ---------------------------------------------------------------------------------------------------------------

def gpu_times(fn, reps, warm=2, calls=1):
    """`reps` windows of `calls` back-to-back fn() on the current stream, each under a pair of HIP events, after `warm` windows
    that are not timed -> the time per call of every window, sorted"""
    for _ in range(warm * calls):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / calls)
    return sorted(times)


def gpu_ms(fn, reps, warm=2, calls=1):
    """the median of gpu_times"""
    return gpu_times(fn, reps, warm, calls)[reps // 2]


def wall_ms(fn, reps):
    """median wall-clock time of fn(), synchronised, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return sorted(times)[len(times) // 2]


def write_json(obj, path):
    """`obj` into `path`, its directory made first; no path, no file"""
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(json.dumps(obj, indent=1) + "\n")


def time_export(model, argv, runs, stages, device, rest_key=None, warm=True):
    """The whole export `mesh_nerf <argv>` `runs` times (one more in front that is not counted, unless `warm` is off), wall
    clock, synchronised.  `stages`: report key -> name of a `mesh_nerf` function, which is timed the same way inside the run;
    `rest_key` names the difference between the whole and the stages.  -> ({"median": the run with the median whole_ms,
    "whole_ms_all_runs": sorted}, the last run's result)"""
    from nerfmeshes_amd import mesh_nerf
    spent = {}

    def timed(key, fn):
        def wrapper(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn(*a, **kw)
            torch.cuda.synchronize()
            spent[key] = spent.get(key, 0.0) + 1e3 * (time.perf_counter() - t0)
            return r
        return wrapper

    args = mesh_nerf.build_parser().parse_args(list(argv))
    real = {name: getattr(mesh_nerf, name) for name in stages.values()}
    for key, name in stages.items():
        setattr(mesh_nerf, name, timed(key, real[name]))
    try:
        rows = []
        for i in range(runs + bool(warm)):
            spent.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with quiet(), torch.no_grad():
                result = mesh_nerf.export_marching_cubes(model, args, model.cfg, device)
            torch.cuda.synchronize()
            whole = 1e3 * (time.perf_counter() - t0)
            if i or not warm:
                rows.append(dict(spent, whole_ms=whole))
                if rest_key:
                    rows[-1][rest_key] = whole - sum(spent.values())
    finally:
        for name, fn in real.items():
            setattr(mesh_nerf, name, fn)
    rows.sort(key=lambda r: r["whole_ms"])
    return {"median": rows[len(rows) // 2], "whole_ms_all_runs": [r["whole_ms"] for r in rows]}, result
