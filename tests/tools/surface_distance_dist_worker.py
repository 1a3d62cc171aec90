"""Launched by tests/test_gpu_surface_distance.py under `python -m torch.distributed.run --nproc-per-node N` with
`NERFMESHES_RANKS_PER_GPU=N` (N ranks sharing one GPU over gloo).  `hip_ops.mesh_surface_distance` of two spheres with 5 001
samples each -- ragged slices of the queries on every rank, one all-gather per array -- must return the single-rank numbers
and arrays byte for byte on EVERY rank; `mesh_nerf.export_marching_cubes --res 24 --target-mesh ... --target-surface exact
--target-fscore ...` on the synthetic scene must write the 1-rank <stem>.chamfer.json in both `--gather` modes.  Prints
SURFACE_DISTANCE_DIST_OK on rank 0."""
import contextlib
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from nerfmeshes_amd import dist as nd  # noqa: E402
from tests import gpu_support as gs  # noqa: E402
from tests import mesh_metrics as MM  # noqa: E402


def write_obj(path, verts, faces):
    with open(path, "w") as fh:
        for v in verts:
            fh.write("v " + " ".join(repr(float(c)) for c in v) + "\n")
        for f in faces:
            fh.write("f " + " ".join(str(int(i) + 1) for i in f) + "\n")


def main():
    rank, world, dev = nd.init_from_env()
    from nerfmeshes_amd import hip_ops
    verts, faces = MM.uv_sphere(32, 16)
    va, fa = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)
    vb = va * 1.0625 + 0.03125

    def measure():
        gen = torch.Generator(device=dev)
        gen.manual_seed(9)
        return hip_ops.mesh_surface_distance(va, fa, vb, fa, 5001, generator=gen, thresholds=(0.05, 0.2))

    got, want = measure(), gs.single_rank(measure)
    assert set(got) == set(want)
    for k, v in want.items():
        if isinstance(v, torch.Tensor):
            a, b = got[k].cpu().numpy(), v.cpu().numpy()
            assert a.shape == (5001,) and a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"rank {rank}: {k} differs from one rank's"
        elif isinstance(v, float):
            assert np.float64(got[k]).tobytes() == np.float64(v).tobytes(), (rank, k, got[k], v)
        else:
            assert got[k] == v, (rank, k, got[k], v)
    assert 0.0 < want["fscore"][0]["fscore"] < 1.0 and want["fscore"][1]["fscore"] == 1.0

    model = gs.scene_model(dev, chunksize=3000)
    target = os.path.join(gs.rank_dir("sdist", rank, "target"), "target.obj")
    write_obj(target, verts * np.float32(0.5), faces)
    files = {}
    for tag, gather in (("triangles", "triangles"), ("grid", "grid"), ("one", "triangles")):
        d = gs.rank_dir("sdist", rank, tag)
        with contextlib.redirect_stdout(io.StringIO()):
            run = lambda: gs.export_mesh(model, d, "--res", "24", "--gather", gather, "--target-mesh", target,   # noqa: E731
                                         "--chamfer-samples", "3001", "--target-surface", "exact", "--target-fscore", "0.05,0.5",
                                         device=dev)
            gs.single_rank(run) if tag == "one" else run()
        if rank == 0 or tag == "one":
            files[tag] = open(os.path.join(d, "mesh.chamfer.json"), "rb").read()
    torch.cuda.synchronize()
    if rank == 0:
        for tag in ("triangles", "grid"):
            assert files[tag] == files["one"], f"--gather {tag}: the report of N ranks differs from the 1-rank report"
        assert b'"surface": "exact"' in files["one"] and b'"fscore"' in files["one"]
    flag = torch.ones(1, device=dev)
    nd.all_reduce(flag)
    if rank == 0:
        assert int(flag.item()) == world
        print(f"SURFACE_DISTANCE_DIST_OK world={world} accuracy={got['accuracy']}", flush=True)
    nd.shutdown()


if __name__ == "__main__":
    main()
