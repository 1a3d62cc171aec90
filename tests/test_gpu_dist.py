"""GPU: the RCCL path on real hardware.  One process per GPU under torch.distributed.run (rendezvous on 127.0.0.1):
world size 1 always (the collective entry points run on a one-rank RCCL communicator), world size 2 when the box has
two GPUs (N-rank pixels / grid / mesh == 1-rank, bit for bit).  Also bench.py's launcher behaviour: `--gpus N` beyond
the visible GPUs must exit non-zero instead of mislabelling a 1-GPU run, and the RCCL leg of the bench must report
what the all-gather delivered."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests.gpu_support import assert_ranks_ok, clean_env, launch_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("world", [1, 2])
def test_rccl_sharded_render_grid_mesh(world):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X")
    if torch.cuda.device_count() < world:
        pytest.skip(f"needs {world} GPUs, this box has {torch.cuda.device_count()}")
    r = launch_ranks(os.path.join("tests", "tools", "dist_worker.py"), world, ranks_per_gpu=False)
    assert_ranks_ok(r, f"DIST_OK world={world} backend=nccl")


@pytest.mark.parametrize("world", [2, 3, 8])
def test_ranks_sharing_one_gpu_over_gloo(world):
    """N > 1 with the REAL kernels on a one-GPU box: `world` processes on cuda:0 over gloo (RCCL refuses duplicate
    devices).  Sharded pixels, slab-sharded grid -> marching cubes, vertex-sharded appearance re-query + OBJ, ragged
    eval-loss gather, gradient all-reduce of a real training step, and the 480-plane / 5-plane per-slab marching-cubes
    rehearsal (ragged and empty triangle shards, ranks without a cube layer) -- each equal to the 1-rank result bit for
    bit.  world = 8 is the node size the driver's scaling run uses: every 8-rank code path has run before it does."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X")
    r = launch_ranks(os.path.join("tests", "tools", "dist_worker.py"), world, timeout=1500, env={"NM_EXPECT_BACKEND": "gloo"})
    assert_ranks_ok(r, f"DIST_OK world={world} backend=gloo device=cuda:0")


def test_bench_refuses_more_gpus_than_visible():
    n = torch.cuda.device_count() + 1
    r = subprocess.run([sys.executable, "bench.py", "--gpus", str(n), "--steps", "1", "--warmup", "0", "--headline-only"],
                       cwd=ROOT, env=clean_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "visible" in (r.stderr + r.stdout)
    assert '"n_gpus"' not in r.stdout, "no bench line may be printed for a run that could not happen"


def test_bench_plain_run_is_the_headline_and_dumps_its_last_step(tmp_path):
    """A plain `bench.py` run measures the headline alone (everything else takes `--full`), `--steps` is the number of timed
    steps, `ms_per_step` the time of one, and `--dump-outputs` writes the pixels the last timed step rendered."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "0", "--dump-outputs", str(tmp_path)],
                       cwd=ROOT, env=clean_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    printed = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(printed) == 1, printed
    line = json.loads(printed[0])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "rays/s" and line["dtype"] == "f32"
    assert abs(line["value"] - 640000 / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    for name in ("cpu_baseline", "parity", "mesh", "buff", "eval", "tiny", "train", "bf16x3"):
        assert name not in line, name
    import numpy as np
    rgb = np.load(tmp_path / "rgb_map.npy")
    assert rgb.shape == (640000, 3) and rgb.dtype == np.float32 and np.isfinite(rgb).all()
    assert rgb.min() >= 0.0 and rgb.max() <= 1.0 + 1e-5 and rgb.std() > 0


def test_bench_rccl_leg_on_one_rank():
    """bench.py under a launcher environment of ONE rank: RCCL is initialised, the pixels go through the all-gather,
    and the line says how many ranks the collective saw."""
    r = launch_ranks("bench.py", 1, "--gpus", "1", "--steps", "1", "--warmup", "1", "--headline-only", ranks_per_gpu=False)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    printed = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(printed) == 1, f"stdout must carry the ONE JSON line only (RCCL prints its banner there): {printed}"
    line = json.loads(printed[0])
    assert line["n_gpus"] == 1 and line["rccl"]["backend"] == "nccl" and line["rccl"]["ranks_in_all_gather"] == 1
    assert line["rccl"]["slots_match_rank_checksums"] is True
    assert line["value"] > 1e5 and 0.5 < line["roofline"]["frac"] < 1.0


@pytest.mark.parametrize("mode", ["weak", "strong"])
def test_bench_two_ranks_on_one_gpu_carries_the_sharded_objects(mode):
    """`python bench.py --gpus 1 --ranks-per-gpu 2 --full` (self-launching, gloo): the N > 1 legs of BASELINE configs 3 / 4 / 5
    -- views dealt to the ranks or one view's rays split over them, the slab-sharded density grid + all-gather +
    marching cubes (bitwise vs the C oracle in-run), the ray-sharded BuFF view -- all present on the line, with
    per-rank roofline fractions, and labelled as a functional (not a scaling) run."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--ranks-per-gpu", "2", "--steps", "1", "--warmup", "1",
                        "--mode", mode, "--mesh-res", "120", "--no-cpu-baseline", "--full"],
                       cwd=ROOT, env=clean_env(), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    printed = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(printed) == 1, printed
    line = json.loads(printed[0])
    assert len(printed[0]) <= 4096, "the printed line is the compact one (benchlib/line.py)"
    assert line["n_gpus"] == 1 and line["ranks_per_gpu"] == 2 and line["scaling"] == mode and "FUNCTIONAL" in line["note"]
    assert line["rccl"]["backend"] == "gloo" and line["rccl"]["ranks_in_all_gather"] == 2
    assert line["rccl"]["slots_match_rank_checksums"] is True and len(line["rccl"]["roofline_frac_per_rank"]) == 2
    assert line["config"]["rays_per_step_per_rank"] == (320000 if mode == "strong" else 640000)
    # what a SCALE record needs to be read on its own, on the line itself
    sd = line["scaling_detail"]
    assert sd["mode"] == mode and sd["collectives_per_step"] == 1 and sd["gathered_bytes_per_step"] == line["rccl"]["gathered_bytes_per_step"]
    assert abs(sd["value_per_gpu"] - line["value"]) < 1e-3 * line["value"] and sd["efficiency_vs_n1_frac"] > 0 and sd["n1_value_source"].startswith("profiles/")
    assert line["mesh"]["sharded"]["meshes_equal_single_grid"] is True and line["mesh"]["marching_cubes"]["bitwise"] is True
    assert line["mesh"]["sharded"]["grid_ms"] > 0 and line["mesh"]["sharded"]["triangles_ms"] > 0 and 0 < line["buff"]["frac"] <= 1
    # ... and every object as measured in the file the line names
    line = json.load(open(os.path.join(ROOT, line["full"])))
    mesh, buff = line["mesh"], line["buff"]
    assert mesh["grid_query"]["planes_per_rank"] == [60, 60] and len(mesh["grid_query"]["roofline"]["frac_per_rank"]) == 2
    sh = mesh["sharded"]
    assert sh["all_gather_of_the_grid"]["ms"] > 0 and sh["all_gather_of_the_grid"]["bytes_total"] == 120 ** 3 * 4
    assert sh["default"] == "triangles" and sh["all_gather_of_the_triangles"]["bytes_total"] < 120 ** 3 * 4
    for strategy in ("grid", "triangles"):      # both end-to-end variants reproduce the single-grid mesh
        assert sh["strategies"][strategy]["faces_and_normals_equal_single_grid_mesh"] is True and sh["strategies"][strategy]["ms_end_to_end"] > 0
    assert mesh["marching_cubes"]["bitwise_identical_to_oracle"] is True and mesh["marching_cubes"]["iso_equals_numpy_fp32"] is True
    assert buff["rays_per_rank"] == [95256, 95256] and len(buff["roofline"]["frac_per_rank"]) == 2 and buff["value"] > 1e4
    assert "cpu_baseline" not in line and "train" not in line            # N = 1 only


@pytest.mark.parametrize("inject,expect", [("mesh:1", "asymmetric"), ("buff:all", "symmetric")])
def test_bench_line_survives_a_failing_secondary_object_at_two_ranks(inject, expect):
    """The first real N-GPU run must not be able to lose its headline to a secondary object.
    `NM_BENCH_INJECT_FAILURE` raises inside an object: on rank 1 only -- rank 0 is then inside the object's first collective,
    which rank 1 never joins; rank 1 gives up waiting for the others' verdicts, leaves, the launcher terminates rank 0 and
    its emergency writer still emits the ONE line (headline + an error for the object) -- or on every rank, where all
    ranks agree through the rendezvous store, skip the object together and the REST of the line is complete."""
    env = clean_env(NM_BENCH_INJECT_FAILURE=inject)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--ranks-per-gpu", "2", "--steps", "1", "--warmup", "1",
                        "--mesh-res", "60", "--no-cpu-baseline", "--full"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    printed = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(printed) == 1, (printed, r.stderr[-3000:])
    line = json.loads(printed[0])
    assert line["value"] > 1e5 and line["n_gpus"] == 1 and line["rccl"]["ranks_in_all_gather"] == 2, "the headline must be intact"
    if expect == "asymmetric":
        assert "error" in line["mesh"] and "errors" in line and r.returncode != 0
    else:
        assert r.returncode == 0, r.stderr[-3000:]
        assert "injected failure" in line["buff"]["error"] and line["buff"]["failed_ranks"] == [0, 1]
        assert line["mesh"]["marching_cubes"]["bitwise"] is True, "the other objects still ran"


def test_bench_eight_ranks_on_one_gpu():
    """`python bench.py --gpus 1 --ranks-per-gpu 8 --mesh-res 120 --full`: the exact launch shape of the driver's 8-GPU scaling run
    (8 ranks, views dealt to the ranks, 8-way slab split of the mesh grid, ray-sharded BuFF view) rehearsed on one GPU over
    gloo -- a functional run: its rates say nothing about scaling, its objects must all be there and consistent."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--ranks-per-gpu", "8", "--steps", "1", "--warmup", "1",
                        "--mesh-res", "120", "--no-cpu-baseline", "--full"],
                       cwd=ROOT, env=clean_env(), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    printed = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(printed) == 1, printed
    line = json.loads(printed[0])
    assert line["n_gpus"] == 1 and line["ranks_per_gpu"] == 8 and line["scaling"] == "weak" and "FUNCTIONAL" in line["note"]
    assert line["rccl"]["ranks_in_all_gather"] == 8 and line["rccl"]["slots_match_rank_checksums"] is True
    assert line["rccl"]["gathered_bytes_per_step"] == 8 * 640000 * 3 * 4 and len(line["rccl"]["roofline_frac_per_rank"]) == 8
    assert line["scaling_detail"]["gathered_bytes_per_step"] == 8 * 640000 * 3 * 4 and len(printed[0]) <= 4096
    line = json.load(open(os.path.join(ROOT, line["full"])))
    mesh = line["mesh"]
    assert mesh["grid_query"]["planes_per_rank"] == [15] * 8
    for strategy in ("grid", "triangles"):
        assert mesh["sharded"]["strategies"][strategy]["faces_and_normals_equal_single_grid_mesh"] is True
    assert mesh["marching_cubes"]["bitwise_identical_to_oracle"] is True
    assert len(line["buff"]["rays_per_rank"]) == 8 and sum(line["buff"]["rays_per_rank"]) == 504 * 378


def test_bench_self_launches_two_ranks():
    """`python bench.py --gpus 2` with no launcher must start two ranks by itself and print n_gpus: 2."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "1", "--warmup", "1", "--headline-only"],
                       cwd=ROOT, env=clean_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["rccl"]["ranks_in_all_gather"] == 2 and line["rccl"]["slots_match_rank_checksums"]
