"""Launched by tests/test_gpu_mesh_texture.py under `python -m torch.distributed.run --nproc-per-node N` with
`NERFMESHES_RANKS_PER_GPU=N` (N ranks sharing one GPU over gloo): `mesh_nerf.export_marching_cubes` with `--simplify-cell 2
--texture-res 4 --render-views 3 --render-size 64` on the synthetic scene.  Every rank bakes a contiguous range of faces and one
all-gather assembles the colours: the OBJ, the MTL, the PNG and the report must be the 1-rank run's byte for byte.  Prints
TEXTURE_DIST_OK on rank 0."""
import contextlib
import io
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from nerfmeshes_amd import dist as nd, synthetic as S  # noqa: E402

FILES = ("mesh.obj", "mesh.mtl", "mesh.png", "mesh.render.json")


def single_rank(fn):
    """`fn` as a process outside any group runs it (nd.world() -> (0, 1)), on this rank."""
    real = nd.world, nd.all_gather_rows
    nd.world, nd.all_gather_rows = (lambda: (0, 1)), (lambda local, counts: local)
    try:
        return fn()
    finally:
        nd.world, nd.all_gather_rows = real


def main():
    rank, world, dev = nd.init_from_env()
    from nerfmeshes_amd import mesh_nerf, models
    hp = S.hparams(chunksize=3000)
    torch.manual_seed(0)
    model = models.NeRFModel(hp)
    sd = model.state_dict()
    for prefix in ("model_coarse.", "model_fine."):
        for k, v in S.make_scene_weights().items():
            sd[prefix + k] = torch.from_numpy(v)
    model.load_state_dict(sd)
    model = model.eval().to(dev)
    written = {}
    for tag in ("many", "one"):
        d = tempfile.mkdtemp(prefix=f"nm_texture_{rank}_{tag}_")
        args = mesh_nerf.build_parser().parse_args(["--save-dir", d, "--view-disparity-max-bound", "1.0", "--iso-level", "32",
                                                    "--batch-size", "4096", "--res", "48", "--simplify-cell", "2", "--texture-res", "4",
                                                    "--render-views", "3", "--render-size", "64"])
        text = io.StringIO()
        with torch.no_grad(), contextlib.redirect_stdout(text):
            run = lambda: mesh_nerf.export_marching_cubes(model, args, model.cfg, dev)   # noqa: E731
            single_rank(run) if tag == "one" else run()
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
