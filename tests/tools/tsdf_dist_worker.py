"""Launched by tests/test_gpu_tsdf_fuse.py under `python -m torch.distributed.run --nproc-per-node N` with
`NERFMESHES_RANKS_PER_GPU=N` (N ranks sharing one GPU over gloo): `mesh_nerf.export_marching_cubes` with `--geometry tsdf --res 24
--tsdf-views 6 --tsdf-size 48` on the synthetic scene, for both `--gather` modes.  The views are rendered by the ranks in turn,
the field is fused per slab: the OBJ must be the 1-rank run's byte for byte, and so must the report up to its last entry, the
seconds.  Prints TSDF_DIST_OK on rank 0."""
import contextlib
import io
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from nerfmeshes_amd import dist as nd  # noqa: E402
from tests import gpu_support as gs  # noqa: E402


def stable(report):
    """the report without the seconds, which come last"""
    head, mark, _ = report.partition(b'\n "seconds": {')
    assert mark and head.count(b"\n") >= 10, "the seconds are the report's last entry"
    return head


def main():
    rank, world, dev = nd.init_from_env()
    model = gs.scene_model(dev, chunksize=3000)
    files = {}
    for tag, gather in (("triangles", "triangles"), ("grid", "grid"), ("one", "triangles")):
        d = gs.rank_dir("tsdf", rank, tag)
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            run = lambda: gs.export_mesh(model, d, "--geometry", "tsdf", "--res", "24", "--tsdf-views", "6",   # noqa: E731
                                         "--tsdf-size", "48", "--gather", gather, device=dev)
            gs.single_rank(run) if tag == "one" else run()
        assert "TSDF: 6 views of 48² fused into 24 x 24 x 24 voxels" in text.getvalue(), f"{tag}: the report line"
        if rank == 0 or tag == "one":
            files[tag] = [open(os.path.join(d, name), "rb").read() for name in ("mesh.obj", "mesh.tsdf.json")]
    torch.cuda.synchronize()
    if rank == 0:
        for tag in ("triangles", "grid"):
            assert files[tag][0] == files["one"][0], f"--gather {tag}: the OBJ of N ranks differs from the 1-rank OBJ"
            assert stable(files[tag][1]) == stable(files["one"][1]), f"--gather {tag}: the report of N ranks differs from the 1-rank report"
        print(f"TSDF_DIST_OK world={world} bytes={len(files['one'][0])}", flush=True)
    nd.shutdown()


if __name__ == "__main__":
    main()
