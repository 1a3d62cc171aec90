"""Launched by tests/test_gpu_mesh_raster.py under `python -m torch.distributed.run --nproc-per-node N` with
`NERFMESHES_RANKS_PER_GPU=N` (N ranks sharing one GPU over gloo): `mesh_nerf.export_marching_cubes` with `--render-views 3
--render-size 64` on the synthetic scene.  The views are dealt round-robin to the ranks and the rows gathered: the report
file must be the 1-rank run's byte for byte.  Prints RASTER_DIST_OK on rank 0."""
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
    reports = {}
    for tag in ("many", "one"):
        d = gs.rank_dir("raster", rank, tag)
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            run = lambda: gs.export_mesh(model, d, "--res", "48", "--render-views", "3", "--render-size", "64", device=dev)   # noqa: E731
            gs.single_rank(run) if tag == "one" else run()
        assert "Mesh render: 3 views" in text.getvalue(), f"{tag}: the report lines"
        path = os.path.join(d, "mesh.render.json")
        reports[tag] = open(path, "rb").read() if (rank == 0 or tag == "one") else None
    torch.cuda.synchronize()
    if rank == 0:
        assert reports["many"] == reports["one"], "the report of N ranks differs from the 1-rank report"
        print(f"RASTER_DIST_OK world={world} bytes={len(reports['one'])}", flush=True)
    nd.shutdown()


if __name__ == "__main__":
    main()
