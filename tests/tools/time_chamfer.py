"""The chamfer measure (mesh_chamfer, mesh_nerf --target-mesh) on the --res 480 --iso-level 32 --limit 1.2 mesh of the synthetic
scene, under HIP events after warm-up (median of --reps):

* `points_nearest` at N = M = 10^5 and 10^6 -- points sampled on the mesh against points sampled on the same mesh jittered --
  as pairs/s and as a fraction of the packed-fp32 VALU roof (8 flops per pair against 157.3 TFLOP/s);
* the same search as chunked `torch.cdist(...).min(1)` on the device (each block at most 4 GB), results compared up to
  cdist's different rounding, and the ratio of the two times;
* sampling 10^6 points: weights + scan + sample;
* the whole `mesh_nerf` export with and without `--target-mesh` (wall clock), i.e. the stage's share of the export.

    python tests/tools/time_chamfer.py [--res 480] [--reps 21] [--cdist-reps 3] [--runs 3] [--out profiles/r10_chamfer.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nerfmeshes_amd import hip_ops, mesh_nerf  # noqa: E402
from nerfmeshes_amd.nerf.nerf_helpers import export_obj  # noqa: E402
from tests import gpu_support as gs  # noqa: E402

ROOF_FLOPS = 157.3e12          # packed fp32 vector peak of the MI355X
FLOPS_PER_PAIR = 8             # three subtractions, three products, two additions


def cdist_nearest(x, y, block_bytes=4 << 30):
    """the torch formulation: row blocks of the N x M distance matrix, each at most `block_bytes`"""
    rows = max(1, block_bytes // (4 * max(1, y.shape[0])))
    d2 = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    idx = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    for lo in range(0, x.shape[0], rows):
        d, i = torch.cdist(x[lo:lo + rows], y).min(1)
        d2[lo:lo + rows] = d * d
        idx[lo:lo + rows] = i
    return d2, idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=480)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--cdist-reps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    model = gs.scene_model(dev)
    common = ["--res", str(opt.res), "--iso-level", "32", "--limit", "1.2"]
    out = {"res": opt.res, "scene": "synthetic.make_scene_weights (8x256)", "iso_level": 32, "limit": 1.2, "reps": opt.reps,
           "device": torch.cuda.get_device_name(0), "roof_flops": ROOF_FLOPS, "flops_per_pair": FLOPS_PER_PAIR}

    def save():
        print(json.dumps(out), flush=True)
        gs.write_json(out, opt.out)

    with torch.no_grad():
        args = mesh_nerf.build_parser().parse_args(common)
        with gs.quiet():
            v, f, n, _ = mesh_nerf.extract_geometry(model, dev, args)
        f = f.to(torch.int32)
        out.update(vertices=int(v.shape[0]), faces=int(f.shape[0]))
        gen = torch.Generator(device=dev)
        gen.manual_seed(0)
        jittered = v + 0.002 * torch.randn(v.shape, device=dev, generator=gen)
        out["nearest"] = {}
        for size in opt.sizes:
            x = hip_ops.mesh_sample_points(v, f, n=size, generator=gen)[0]
            y = hip_ops.mesh_sample_points(jittered, f, n=size, generator=gen)[0]
            ms = gs.gpu_ms(lambda: hip_ops.points_nearest(x, y), opt.reps)
            pairs = float(size) * float(size) / (ms * 1e-3)
            row = {"n": size, "m": size, "ms": ms, "pairs_per_s": pairs, "fraction_of_valu_roof": pairs * FLOPS_PER_PAIR / ROOF_FLOPS}
            out["nearest"][str(size)] = row
            save()
            d2, idx = hip_ops.points_nearest(x, y)
            cd2, cidx = cdist_nearest(x, y)
            row["cdist_index_agreement"] = float((cidx == idx.long()).float().mean())
            row["cdist_max_abs_dist2_difference"] = float((cd2 - d2).abs().max())
            row["cdist_ms"] = gs.gpu_ms(lambda: cdist_nearest(x, y), opt.cdist_reps, warm=1)
            row["cdist_over_kernel"] = row["cdist_ms"] / ms
            save()
        u = torch.rand(1_000_000, 3, device=dev, generator=gen)
        out["sample_1e6_ms"] = gs.gpu_ms(lambda: hip_ops.mesh_sample_points(v, f, u=u), opt.reps)
        out["face_weights_ms"] = gs.gpu_ms(lambda: hip_ops.mesh_face_weights(v, f), opt.reps)
        save()
        # the whole export with and without the stage; the target is the plain mesh itself, written once
        tdir = tempfile.mkdtemp(prefix="nm_chamfer_target_")
        target = os.path.join(tdir, "target.obj")
        with gs.quiet():
            export_obj(v.cpu(), f.cpu(), torch.zeros(0, 3), n.cpu(), target)
        for tag, extra in (("export_default", []), ("export_target_mesh", ["--target-mesh", target])):
            d = tempfile.mkdtemp(prefix="nm_chamfer_time_")
            a = mesh_nerf.build_parser().parse_args(common + ["--save-dir", d, *extra])

            def run():
                with gs.quiet():
                    mesh_nerf.export_marching_cubes(model, a, model.cfg, dev)

            out[tag] = {"wall_ms": gs.wall_ms(run, opt.runs)}
            save()
        t0 = time.perf_counter()
        from nerfmeshes_amd.nerf.nerf_helpers import load_obj
        load_obj(target)
        out["load_obj_target_ms"] = 1e3 * (time.perf_counter() - t0)
        args_t = mesh_nerf.build_parser().parse_args(common + ["--save-dir", tdir, "--target-mesh", target])
        tv, tf = load_obj(target)

        def stage():
            from nerfmeshes_amd import mesh_chamfer
            mesh_chamfer.compare_meshes(v, f, tv, tf, samples=args_t.chamfer_samples, seed=0, device=dev)

        out["chamfer_stage_without_reading_ms"] = gs.wall_ms(stage, opt.runs)
        out["stage_share_of_export"] = 1.0 - out["export_default"]["wall_ms"] / out["export_target_mesh"]["wall_ms"]
        save()


if __name__ == "__main__":
    main()
