"""Launched by tests/test_gpu_mesh_simplify_adaptive.py under `python -m torch.distributed.run --nproc-per-node N` with
`NERFMESHES_RANKS_PER_GPU=N` (N ranks sharing one GPU over gloo): `mesh_nerf.export_marching_cubes` with `--simplify-cell 2
--simplify-placement quadric --simplify-levels 2` on the synthetic scene, with both `--gather` modes.  Every rank simplifies
the gathered mesh redundantly, and every level's sums and maxima are exact: mesh, normals, colours and the OBJ must be the
1-rank run's bit for bit, and have fewer faces than the uniform clustering's.  Prints SIMPLIFY_ADAPTIVE_DIST_OK on rank 0."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from nerfmeshes_amd import dist as nd  # noqa: E402
from tests import gpu_support as gs  # noqa: E402


def main():
    rank, world, dev = nd.init_from_env()
    model = gs.scene_model(dev, chunksize=3000)
    out = {}
    options = {"adaptive": ["--simplify-levels", "2", "--simplify-error", "0.25"], "uniform": []}
    for tag, gather, kind in (("triangles", "triangles", "adaptive"), ("grid", "grid", "adaptive"), ("one", "triangles", "adaptive"),
                              ("uniform", "triangles", "uniform")):
        d = gs.rank_dir("simplify_adaptive", rank, tag)
        with gs.quiet():
            run = lambda: gs.export_mesh(model, d, "--res", "64", "--gather", gather, "--simplify-cell", "2",   # noqa: E731
                                         "--simplify-placement", "quadric", *options[kind], device=dev)
            out[tag] = (gs.single_rank(run) if tag in ("one", "uniform") else run()) + (d,)
    for multi in ("triangles", "grid"):
        gs.same_export(out[multi], out["one"], f"--gather {multi}", rank)
    assert 0 < out["one"][1].shape[0] < out["uniform"][1].shape[0], "the levels leave fewer faces"
    torch.cuda.synchronize()
    if rank == 0:
        print(f"SIMPLIFY_ADAPTIVE_DIST_OK world={world} vertices={int(out['one'][0].shape[0])}", flush=True)
    nd.shutdown()


if __name__ == "__main__":
    main()
