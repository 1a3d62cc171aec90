"""Launched by tests/test_gpu_mesh_simplify_quadric.py under `python -m torch.distributed.run --nproc-per-node N` with
`NERFMESHES_RANKS_PER_GPU=N` (N ranks sharing one GPU over gloo): `mesh_nerf.export_marching_cubes` with `--simplify-cell 4
--simplify-placement quadric` on the synthetic scene, with both `--gather` modes.  Every rank simplifies the gathered mesh
redundantly, and the quadrics are exact integer sums: mesh, normals, colours and the OBJ must be the 1-rank run's bit for bit,
and differ from mean placement's.  Prints SIMPLIFY_QUADRIC_DIST_OK on rank 0."""
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
    options = {"quadric": ["--simplify-placement", "quadric"], "mean": []}
    for tag, gather, placement in (("triangles", "triangles", "quadric"), ("grid", "grid", "quadric"), ("one", "triangles", "quadric"),
                                   ("mean", "triangles", "mean")):
        d = gs.rank_dir("simplify_quadric", rank, tag)
        with gs.quiet():
            run = lambda: gs.export_mesh(model, d, "--res", "64", "--gather", gather, "--simplify-cell", "4",   # noqa: E731
                                         *options[placement], device=dev)
            out[tag] = (gs.single_rank(run) if tag in ("one", "mean") else run()) + (d,)
    for multi in ("triangles", "grid"):
        gs.same_export(out[multi], out["one"], f"--gather {multi}", rank)
    assert torch.equal(out["one"][1], out["mean"][1]) and not torch.equal(out["one"][0], out["mean"][0]), "only positions move"
    torch.cuda.synchronize()
    if rank == 0:
        print(f"SIMPLIFY_QUADRIC_DIST_OK world={world} vertices={int(out['one'][0].shape[0])}", flush=True)
    nd.shutdown()


if __name__ == "__main__":
    main()
