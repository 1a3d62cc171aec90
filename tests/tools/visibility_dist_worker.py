"""Launched by tests/test_gpu_mesh_visibility.py under `python -m torch.distributed.run --nproc-per-node N` with
`NERFMESHES_RANKS_PER_GPU=N` (N ranks sharing one GPU over gloo): `mesh_nerf.export_marching_cubes` with `--cull-hidden-views 6
--cull-size 96` on the synthetic scene.  Every rank culls the gathered mesh redundantly: the OBJ and the visibility report must
be the 1-rank run's byte for byte.  Prints VISIBILITY_DIST_OK on rank 0."""
import contextlib
import io
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from nerfmeshes_amd import dist as nd, synthetic as S  # noqa: E402


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
    files = {}
    for tag in ("many", "one"):
        d = tempfile.mkdtemp(prefix=f"nm_visibility_{rank}_{tag}_")
        args = mesh_nerf.build_parser().parse_args(["--save-dir", d, "--view-disparity-max-bound", "1.0", "--iso-level", "32",
                                                    "--batch-size", "4096", "--res", "48", "--cull-hidden-views", "6",
                                                    "--cull-size", "96"])
        text = io.StringIO()
        with torch.no_grad(), contextlib.redirect_stdout(text):
            run = lambda: mesh_nerf.export_marching_cubes(model, args, model.cfg, dev)   # noqa: E731
            single_rank(run) if tag == "one" else run()
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
