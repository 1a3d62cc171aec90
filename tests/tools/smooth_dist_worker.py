"""Launched by tests/test_gpu_mesh_smooth.py under `python -m torch.distributed.run --nproc-per-node N` with
`NERFMESHES_RANKS_PER_GPU=N` (N ranks sharing one GPU over gloo): `mesh_nerf.export_marching_cubes` with `--smooth-iters 3` on
the synthetic scene -- plain, with `--normals network`, and with `--super-sampling 2` behind the component filter and in front
of `--simplify-cell 2`, with both `--gather` modes.  Every rank smooths the gathered mesh redundantly: mesh, normals, colours
and the OBJ must be the 1-rank run's bit for bit.  Prints SMOOTH_DIST_OK on rank 0."""
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
    out = {}
    cases = {"plain": ["--res", "64"], "network": ["--res", "44", "--normals", "network"],
             "ss2_filtered_simplified": ["--res", "64", "--super-sampling", "2", "--min-component-faces", "60", "--keep-largest", "2",
                                         "--simplify-cell", "2"]}
    for case, extra in cases.items():
        for tag, gather in (("triangles", "triangles"), ("grid", "grid"), ("one", "triangles"), ("rough", "triangles")):
            d = tempfile.mkdtemp(prefix=f"nm_smooth_{rank}_{case}_{tag}_")
            option = [] if tag == "rough" else ["--smooth-iters", "3"]
            args = mesh_nerf.build_parser().parse_args(["--save-dir", d, "--view-disparity-max-bound", "1.0", "--iso-level", "32",
                                                        "--batch-size", "4096", "--gather", gather, *extra, *option])
            text = io.StringIO()
            with torch.no_grad(), contextlib.redirect_stdout(text):
                run = lambda: mesh_nerf.export_marching_cubes(model, args, model.cfg, dev)   # noqa: E731
                out[case, tag] = (single_rank(run) if tag in ("one", "rough") else run()) + (d,)
            assert ("Smooth: 3 iterations" in text.getvalue()) == (tag != "rough"), f"{case}, {tag}: the Smooth line"
        smoothed, rough = out[case, "one"][0], out[case, "rough"][0]
        assert smoothed.shape != rough.shape or not torch.equal(smoothed, rough), f"{case}: smoothing moved nothing"
        for multi in ("triangles", "grid"):
            got, want = out[case, multi], out[case, "one"]
            for name, a, b in zip(("vertices", "triangles", "normals"), got[:3], want[:3]):
                assert a.shape == b.shape and torch.equal(a, b), f"{case}, --gather {multi}: {name} differ from the 1-rank mesh"
            assert got[3].shape == want[3].shape and (got[3] == want[3]).all(), f"{case}, --gather {multi}: colours differ"
            if rank == 0:
                a = open(os.path.join(got[4], "mesh.obj"), "rb").read()
                assert a == open(os.path.join(want[4], "mesh.obj"), "rb").read(), f"{case}, --gather {multi}: OBJ differs"
    torch.cuda.synchronize()
    if rank == 0:
        print(f"SMOOTH_DIST_OK world={world} vertices={int(out['plain', 'one'][0].shape[0])}", flush=True)
    nd.shutdown()


if __name__ == "__main__":
    main()
