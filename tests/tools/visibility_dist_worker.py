"""Launched by tests/test_gpu_mesh_visibility.py under `python -m torch.distributed.run --nproc-per-node N` with
`NERFMESHES_RANKS_PER_GPU=N` (N ranks sharing one GPU over gloo): `mesh_nerf.export_marching_cubes` with `--cull-hidden-views 6
--cull-size 96` on the synthetic scene.  Every rank culls the gathered mesh redundantly: the OBJ and the visibility report must
be the 1-rank run's byte for byte.  Prints VISIBILITY_DIST_OK on rank 0."""
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
    files = {}
    for tag in ("many", "one"):
        d = gs.rank_dir("visibility", rank, tag)
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            run = lambda: gs.export_mesh(model, d, "--res", "48", "--cull-hidden-views", "6", "--cull-size", "96", device=dev)   # noqa: E731
            gs.single_rank(run) if tag == "one" else run()
        assert "Hidden-face filter: kept" in text.getvalue(), f"{tag}: the report line"
        if rank == 0 or tag == "one":
            files[tag] = [open(os.path.join(d, name), "rb").read() for name in ("mesh.obj", "mesh.visibility.json")]
    torch.cuda.synchronize()
    if rank == 0:
        assert files["many"][0] == files["one"][0], "the OBJ of N ranks differs from the 1-rank OBJ"
        assert files["many"][1] == files["one"][1], "the visibility report of N ranks differs from the 1-rank report"
        print(f"VISIBILITY_DIST_OK world={world} bytes={len(files['one'][0])}", flush=True)
    nd.shutdown()


if __name__ == "__main__":
    main()
