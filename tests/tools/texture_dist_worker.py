"""Launched by tests/test_gpu_mesh_texture.py under `python -m torch.distributed.run --nproc-per-node N` with
`NERFMESHES_RANKS_PER_GPU=N` (N ranks sharing one GPU over gloo): `mesh_nerf.export_marching_cubes` with `--simplify-cell 2
--texture-res 4 --render-views 3 --render-size 64` on the synthetic scene.  Every rank bakes a contiguous range of faces and one
all-gather assembles the colours: the OBJ, the MTL, the PNG and the report must be the 1-rank run's byte for byte.  Prints
TEXTURE_DIST_OK on rank 0."""
import contextlib
import io
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from nerfmeshes_amd import dist as nd  # noqa: E402
from tests import gpu_support as gs  # noqa: E402

FILES = ("mesh.obj", "mesh.mtl", "mesh.png", "mesh.render.json")


def main():
    rank, world, dev = nd.init_from_env()
    model = gs.scene_model(dev, chunksize=3000)
    written = {}
    for tag in ("many", "one"):
        d = gs.rank_dir("texture", rank, tag)
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            run = lambda: gs.export_mesh(model, d, "--res", "48", "--simplify-cell", "2", "--texture-res", "4",   # noqa: E731
                                         "--render-views", "3", "--render-size", "64", device=dev)
            gs.single_rank(run) if tag == "one" else run()
        assert "Texture atlas:" in text.getvalue() and "Mesh render: 3 views" in text.getvalue(), f"{tag}: the printed lines"
        if rank == 0 or tag == "one":
            written[tag] = {name: open(os.path.join(d, name), "rb").read() for name in FILES}
    torch.cuda.synchronize()
    if rank == 0:
        for name in FILES:
            assert written["many"][name] == written["one"][name], f"{name} of N ranks differs from the 1-rank file"
        print(f"TEXTURE_DIST_OK world={world} bytes={sum(len(b) for b in written['one'].values())}", flush=True)
    nd.shutdown()


if __name__ == "__main__":
    main()
