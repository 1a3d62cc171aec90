"""Launched by tests/test_gpu_network_normals.py under `python -m torch.distributed.run --nproc-per-node N` with
`NERFMESHES_RANKS_PER_GPU=N` (N ranks sharing one GPU over gloo): `mesh_nerf.export_marching_cubes --normals network` on the
synthetic scene, plain and with `--super-sampling 2`, with both `--gather` modes -- every rank computes the network normals of
its own vertex range, one ragged all-gather assembles them -- must give the 1-rank mesh, normals, colours and OBJ bit for bit.
Prints NN_DIST_OK on rank 0."""
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
    for res, ss in (("44", "0"), ("100", "2")):
        for tag, gather in (("triangles", "triangles"), ("grid", "grid"), ("one", "triangles")):
            d = gs.rank_dir("nn", rank, res, tag)
            with gs.quiet():
                run = lambda: gs.export_mesh(model, d, "--res", res, "--gather", gather, "--super-sampling", ss,   # noqa: E731
                                             "--normals", "network", device=dev)
                out[res, tag] = (gs.single_rank(run) if tag == "one" else run()) + (d,)
        for multi in ("triangles", "grid"):
            gs.same_export(out[res, multi], out[res, "one"], f"res {res}, --gather {multi}", rank)
    torch.cuda.synchronize()
    if rank == 0:
        print(f"NN_DIST_OK world={world} vertices={int(out['100', 'one'][0].shape[0])}", flush=True)
    nd.shutdown()


if __name__ == "__main__":
    main()
