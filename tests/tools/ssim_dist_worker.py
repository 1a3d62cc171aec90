"""Launched by tests/test_gpu_image_ssim.py under `python -m torch.distributed.run --nproc-per-node N` with
`NERFMESHES_RANKS_PER_GPU=N` (N ranks sharing one GPU over gloo): `mesh_render.main --ssim --compare-nerf --views 3 --img-size 64
--out R.json` on a coloured sphere and the synthetic scene (the checkpoint loading replaced by the scene in memory).  The views
are dealt round-robin to the ranks and the rows -- the SSIM columns among them -- gathered: the report file must be the 1-rank
run's byte for byte.  Prints SSIM_DIST_OK on rank 0."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from nerfmeshes_amd import dist as nd  # noqa: E402
from tests import gpu_support as gs, mesh_metrics as MM  # noqa: E402


def main():
    rank, world, dev = nd.init_from_env()
    from nerfmeshes_amd import mesh_render, models
    from nerfmeshes_amd.nerf.nerf_helpers import export_obj
    model = gs.scene_model(dev, chunksize=3000)

    class Parser:
        checkpoint_path = "memory"

        def parse(self, *a):
            return model.cfg, None

    mesh_render.PathParser = Parser
    getattr(models, model.cfg.experiment.model).load_from_checkpoint = classmethod(lambda cls, path: model)
    real_init, real_shutdown = nd.init_from_env, nd.shutdown
    nd.init_from_env, nd.shutdown = (lambda: (*nd.world(), dev)), (lambda: None)       # main() inside one group, twice
    verts, faces = MM.uv_sphere(24, 12)
    colors = np.random.default_rng(7).random((len(verts), 3), dtype=np.float32)
    reports = {}
    d = gs.rank_dir("ssim", rank)
    obj = os.path.join(d, "sphere.obj")                        # one file for both runs: the report names it
    with gs.quiet():
        export_obj(verts, faces, colors, verts, obj)
    for tag in ("many", "one"):
        out = os.path.join(d, f"R_{tag}.json")
        argv = ["--mesh", obj, "--log-checkpoint", "memory", "--views", "3", "--img-size", "64", "--compare-nerf", "--ssim",
                "--out", out, "--save-dir", d]
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            run = lambda: mesh_render.main(argv)   # noqa: E731
            gs.single_rank(run) if tag == "one" else run()
        assert "Mesh render: 3 views" in text.getvalue() and "SSIM to the network" in text.getvalue(), f"{tag}: the report lines"
        reports[tag] = open(out, "rb").read() if (rank == 0 or tag == "one") else None
    nd.init_from_env, nd.shutdown = real_init, real_shutdown
    torch.cuda.synchronize()
    if rank == 0:
        rows = json.loads(reports["one"])["views"]
        assert len(rows) == 3 and all(r["ssim_nerf"] is not None and -1.0 <= r["ssim_nerf"] <= 1.0 for r in rows)
        assert len({r["ssim_nerf"] for r in rows}) == 3, "three views, three numbers"
        assert reports["many"] == reports["one"], f"the report of N ranks differs from the 1-rank report:\n{reports['many']}\n{reports['one']}"
        print(f"SSIM_DIST_OK world={world} bytes={len(reports['one'])}", flush=True)
    nd.shutdown()


if __name__ == "__main__":
    main()
