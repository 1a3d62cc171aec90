"""Launched by tests/test_gpu_network_normals.py under `python -m torch.distributed.run --nproc-per-node N` with
`NERFMESHES_RANKS_PER_GPU=N` (N ranks sharing one GPU over gloo): `mesh_nerf.export_marching_cubes --normals network` on the
synthetic scene, plain and with `--super-sampling 2`, with both `--gather` modes -- every rank computes the network normals of
its own vertex range, one ragged all-gather assembles them -- must give the 1-rank mesh, normals, colours and OBJ bit for bit.
Prints NN_DIST_OK on rank 0."""
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
    quiet = contextlib.redirect_stdout(io.StringIO())
    out = {}
    for res, ss in (("44", "0"), ("100", "2")):
        for tag, gather in (("triangles", "triangles"), ("grid", "grid"), ("one", "triangles")):
            d = tempfile.mkdtemp(prefix=f"nm_nn_{rank}_{res}_{tag}_")
            args = mesh_nerf.build_parser().parse_args(["--res", res, "--save-dir", d, "--view-disparity-max-bound", "1.0",
                                                        "--iso-level", "32", "--batch-size", "4096", "--gather", gather,
                                                        "--super-sampling", ss, "--normals", "network"])
            with torch.no_grad(), quiet:
                run = lambda: mesh_nerf.export_marching_cubes(model, args, model.cfg, dev)   # noqa: E731
                out[res, tag] = (single_rank(run) if tag == "one" else run()) + (d,)
        for multi in ("triangles", "grid"):
            got, want = out[res, multi], out[res, "one"]
            for name, a, b in zip(("vertices", "triangles", "normals"), got[:3], want[:3]):
                assert a.shape == b.shape and torch.equal(a, b), f"res {res}, --gather {multi}: {name} differ from the 1-rank mesh"
            assert got[3].shape == want[3].shape and (got[3] == want[3]).all(), f"res {res}, --gather {multi}: colours differ"
            if rank == 0:
                a = open(os.path.join(got[4], "mesh.obj"), "rb").read()
                assert a == open(os.path.join(want[4], "mesh.obj"), "rb").read(), f"res {res}, --gather {multi}: OBJ differs"
    torch.cuda.synchronize()
    if rank == 0:
        print(f"NN_DIST_OK world={world} vertices={int(out['100', 'one'][0].shape[0])}", flush=True)
    nd.shutdown()


if __name__ == "__main__":
    main()
