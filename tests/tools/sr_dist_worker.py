"""Launched by tests/test_gpu_surface_ray.py under `python -m torch.distributed.run --nproc-per-node N` with
`NERFMESHES_RANKS_PER_GPU=N` (N ranks sharing one GPU over gloo): `mesh_surface_ray.export_ray_trace` over 5 views -- a
ragged split, or more ranks than views -- must return the 1-rank arrays and write the 1-rank PLY byte for byte, in both
formats and under both depth rules.  Prints SR_DIST_OK on rank 0."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from nerfmeshes_amd import dist as nd  # noqa: E402
from tests import gpu_support as gs  # noqa: E402


def main():
    rank, world, dev = nd.init_from_env()
    from nerfmeshes_amd import mesh_surface_ray as msr
    model = gs.scene_model(dev, chunksize=3000)
    points = 0
    for extra in ((), ("--ply-format", "binary", "--min-opacity", "0.99")):
        out = {}
        for tag in ("multi", "one"):
            d = gs.rank_dir("sr", rank, tag)
            args = msr.build_parser().parse_args(["--save-dir", d, "--views-y", "5", "--views-x", "1", "--img-size", "72", "--focal",
                                                  str(1111.1111 * 72 / 800), *extra])
            with torch.no_grad(), gs.quiet():
                run = lambda: msr.export_ray_trace(model, args, model.cfg, dev)   # noqa: E731
                out[tag] = (gs.single_rank(run, gather="all_gather_ragged") if tag == "one" else run()) + (d,)
        got, want = out["multi"], out["one"]
        for name, a, b in zip(("vertices", "normals", "colours", "uchar colours"), got[:4], want[:4]):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{extra}: {name} differ from the 1-rank result"
        assert len(want[0]) > 100, "the views see the object"
        points = len(want[0])
        if rank == 0:
            a = open(os.path.join(got[4], "lego-sampling.ply"), "rb").read()
            assert a == open(os.path.join(want[4], "lego-sampling.ply"), "rb").read(), f"{extra}: the PLY differs"
        else:
            assert not os.path.exists(os.path.join(got[4], "lego-sampling.ply")), "only rank 0 writes"
    torch.cuda.synchronize()
    if rank == 0:
        print(f"SR_DIST_OK world={world} points={points}", flush=True)
    nd.shutdown()


if __name__ == "__main__":
    main()
