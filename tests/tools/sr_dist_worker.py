"""Launched by tests/test_gpu_surface_ray.py under `python -m torch.distributed.run --nproc-per-node N` with
`NERFMESHES_RANKS_PER_GPU=N` (N ranks sharing one GPU over gloo): `mesh_surface_ray.export_ray_trace` over 5 views -- a
ragged split, or more ranks than views -- must return the 1-rank arrays and write the 1-rank PLY byte for byte, in both
formats and under both depth rules.  Prints SR_DIST_OK on rank 0."""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from nerfmeshes_amd import dist as nd, synthetic as S  # noqa: E402


def single_rank(fn):
    """`fn` as a process outside any group runs it (nd.world() -> (0, 1)), on this rank."""
    real = nd.world, nd.all_gather_ragged
    nd.world, nd.all_gather_ragged = (lambda: (0, 1)), (lambda local: local)
    try:
        return fn()
    finally:
        nd.world, nd.all_gather_ragged = real


def main():
    rank, world, dev = nd.init_from_env()
    from nerfmeshes_amd import mesh_surface_ray as msr, models
    hp = S.hparams(chunksize=3000)
    torch.manual_seed(0)
    model = models.NeRFModel(hp)
    sd = model.state_dict()
    for prefix in ("model_coarse.", "model_fine."):
        for k, v in S.make_scene_weights().items():
            sd[prefix + k] = torch.from_numpy(v)
    model.load_state_dict(sd)
    model = model.eval().to(dev)
    quiet = contextlib.redirect_stdout(io.StringIO())
    points = 0
    for extra in ((), ("--ply-format", "binary", "--min-opacity", "0.99")):
        out = {}
        for tag in ("multi", "one"):
            d = tempfile.mkdtemp(prefix=f"nm_sr_{rank}_{tag}_")
            args = msr.build_parser().parse_args(["--save-dir", d, "--views-y", "5", "--views-x", "1", "--img-size", "72", "--focal",
                                                  str(1111.1111 * 72 / 800), *extra])
            with torch.no_grad(), quiet:
                run = lambda: msr.export_ray_trace(model, args, model.cfg, dev)   # noqa: E731
                out[tag] = (single_rank(run) if tag == "one" else run()) + (d,)
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
