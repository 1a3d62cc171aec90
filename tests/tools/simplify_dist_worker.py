"""Launched by tests/test_gpu_mesh_simplify.py under `python -m torch.distributed.run --nproc-per-node N` with
`NERFMESHES_RANKS_PER_GPU=N` (N ranks sharing one GPU over gloo): `mesh_nerf.export_marching_cubes` with `--simplify-cell 2` on
the synthetic scene -- plain, with `--normals network`, and with `--super-sampling 2` behind the component filter, with both
`--gather` modes.  Every rank simplifies the gathered mesh redundantly, so the vertex ranges and the colour all-gather see the
simplified vertex count on every rank: mesh, normals, colours and the OBJ must be the 1-rank run's bit for bit.  Prints
SIMPLIFY_DIST_OK on rank 0."""
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
    cases = {"plain": ["--res", "64"], "network": ["--res", "44", "--normals", "network"],
             "ss2_filtered": ["--res", "64", "--super-sampling", "2", "--min-component-faces", "60", "--keep-largest", "2"]}
    for case, extra in cases.items():
        for tag, gather in (("triangles", "triangles"), ("grid", "grid"), ("one", "triangles"), ("dense", "triangles")):
            d = gs.rank_dir("simplify", rank, case, tag)
            option = [] if tag == "dense" else ["--simplify-cell", "2"]
            with gs.quiet():
                run = lambda: gs.export_mesh(model, d, "--gather", gather, *extra, *option, device=dev)   # noqa: E731
                out[case, tag] = (gs.single_rank(run) if tag in ("one", "dense") else run()) + (d,)
        assert 0 < out[case, "one"][1].shape[0] < out[case, "dense"][1].shape[0], f"{case}: fewer triangles, not none"
        assert 0 < out[case, "one"][0].shape[0] < out[case, "dense"][0].shape[0], f"{case}: fewer vertices, not none"
        for multi in ("triangles", "grid"):
            gs.same_export(out[case, multi], out[case, "one"], f"{case}, --gather {multi}", rank)
    torch.cuda.synchronize()
    if rank == 0:
        print(f"SIMPLIFY_DIST_OK world={world} faces={int(out['plain', 'one'][1].shape[0])} of {int(out['plain', 'dense'][1].shape[0])}",
              flush=True)
    nd.shutdown()


if __name__ == "__main__":
    main()
