"""Launched by tests/test_gpu_mesh_smooth.py under `python -m torch.distributed.run --nproc-per-node N` with
`NERFMESHES_RANKS_PER_GPU=N` (N ranks sharing one GPU over gloo): `mesh_nerf.export_marching_cubes` with `--smooth-iters 3` on
the synthetic scene -- plain, with `--normals network`, and with `--super-sampling 2` behind the component filter and in front
of `--simplify-cell 2`, with both `--gather` modes.  Every rank smooths the gathered mesh redundantly: mesh, normals, colours
and the OBJ must be the 1-rank run's bit for bit.  Prints SMOOTH_DIST_OK on rank 0."""
import contextlib
import io
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
             "ss2_filtered_simplified": ["--res", "64", "--super-sampling", "2", "--min-component-faces", "60", "--keep-largest", "2",
                                         "--simplify-cell", "2"]}
    for case, extra in cases.items():
        for tag, gather in (("triangles", "triangles"), ("grid", "grid"), ("one", "triangles"), ("rough", "triangles")):
            d = gs.rank_dir("smooth", rank, case, tag)
            option = [] if tag == "rough" else ["--smooth-iters", "3"]
            text = io.StringIO()
            with contextlib.redirect_stdout(text):
                run = lambda: gs.export_mesh(model, d, "--gather", gather, *extra, *option, device=dev)   # noqa: E731
                out[case, tag] = (gs.single_rank(run) if tag in ("one", "rough") else run()) + (d,)
            assert ("Smooth: 3 iterations" in text.getvalue()) == (tag != "rough"), f"{case}, {tag}: the Smooth line"
        smoothed, rough = out[case, "one"][0], out[case, "rough"][0]
        assert smoothed.shape != rough.shape or not torch.equal(smoothed, rough), f"{case}: smoothing moved nothing"
        for multi in ("triangles", "grid"):
            gs.same_export(out[case, multi], out[case, "one"], f"{case}, --gather {multi}", rank)
    torch.cuda.synchronize()
    if rank == 0:
        print(f"SMOOTH_DIST_OK world={world} vertices={int(out['plain', 'one'][0].shape[0])}", flush=True)
    nd.shutdown()


if __name__ == "__main__":
    main()
