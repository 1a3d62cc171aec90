"""Launched by tests/test_gpu_super_sampling.py under `python -m torch.distributed.run --nproc-per-node N` with
`NERFMESHES_RANKS_PER_GPU=N` (N ranks sharing one GPU over gloo): `mesh_nerf.export_marching_cubes --super-sampling` on
the synthetic scene with both `--gather` modes -- refinement after the redundant marching cubes (grid), or of every slab's
own vertices before the triangle all-gather (triangles) -- must give the 1-rank mesh, colours and OBJ bit for bit.
Prints SS_DIST_OK on rank 0."""
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
    for res in ("44", "100"):
        for tag, gather in (("triangles", "triangles"), ("grid", "grid"), ("one", "triangles")):
            d = gs.rank_dir("ss", rank, res, tag)
            with gs.quiet():
                run = lambda: gs.export_mesh(model, d, "--res", res, "--gather", gather, "--super-sampling", "2", device=dev)   # noqa: E731
                out[res, tag] = (gs.single_rank(run) if tag == "one" else run()) + (d,)
        for multi in ("triangles", "grid"):
            gs.same_export(out[res, multi], out[res, "one"], f"res {res}, --gather {multi}", rank)
    torch.cuda.synchronize()
    if rank == 0:
        print(f"SS_DIST_OK world={world} vertices={int(out['100', 'one'][0].shape[0])}", flush=True)
    nd.shutdown()


if __name__ == "__main__":
    main()
