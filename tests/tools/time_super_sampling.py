"""Super-sampled meshing (mesh_nerf --super-sampling) at --res 480 on the synthetic scene: vertices, fine points, per-stage
milliseconds (grid, iso, mc, keys, points, density, refine), the density stage's fraction of the fp32 MFMA peak, and the
whole extract_geometry* time for ss = 0 and every ss.

    python tests/tools/time_super_sampling.py [--res 480] [--ss 1 2 4] [--reps 5] [--out FILE.json]
"""
import argparse
import functools
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchlib.common import FP32_MFMA_PEAK_TFLOPS  # noqa: E402
from nerfmeshes_amd import _lib, hip_ops, mesh_nerf  # noqa: E402
from nerfmeshes_amd.hip_ops import _ptr, _stream, check  # noqa: E402
from tests import gpu_support as gs  # noqa: E402


gpu_ms = functools.partial(gs.gpu_ms, warm=1)                     # one warm-up call, as these figures were taken


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=480)
    ap.add_argument("--ss", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    model = gs.scene_model(dev)
    net = model.get_model().hip("f32")
    lib = _lib.load()
    res = opt.res
    nums = (res, res, res)
    args = mesh_nerf.build_parser().parse_args(["--res", str(res), "--iso-level", "32"])
    ax = mesh_nerf._axes(args, nums, dev)
    out = {"res": res, "scene": "synthetic.make_scene_weights (8x256)", "reps": opt.reps, "peak_tflops": FP32_MFMA_PEAK_TFLOPS,
           "device": torch.cuda.get_device_name(0), "stages_ms": {}, "per_ss": []}
    with torch.no_grad():
        density = net.grid_query(*ax, density_only=True).view(*nums)
        out["stages_ms"]["grid"] = gpu_ms(lambda: net.grid_query(*ax, density_only=True), opt.reps)
        with gs.quiet():
            iso = mesh_nerf.extract_iso_level(density, args)
            out["stages_ms"]["iso"] = gs.wall_ms(lambda: mesh_nerf.extract_iso_level(density, args), opt.reps)
        out["iso"] = float(iso)
        out["stages_ms"]["mc"] = gs.wall_ms(lambda: hip_ops.marching_cubes(density, iso), opt.reps)
        # the key export alone: count + emit as hip_ops.marching_cubes does, then nm_mc_vertex_edges under events
        ws = torch.empty(int(lib.nm_mc_workspace_bytes(res, res, res)), dtype=torch.uint8, device=dev)
        nv, nf = C.c_int64(), C.c_int64()
        check(lib.nm_mc_count(_ptr(density), res, res, res, iso, _ptr(ws), C.byref(nv), C.byref(nf), _stream()), "nm_mc_count")
        buf, ptrs, views = hip_ops._mc_outputs(nv.value, nf.value, dev)
        scratch = torch.empty(int(lib.nm_mc_vertex_scratch_bytes(nv.value, nf.value)) + 256, dtype=torch.uint8, device=dev)
        check(lib.nm_mc_emit(_ptr(density), res, res, res, iso, _ptr(ws), _ptr(scratch), nv.value, nf.value, *ptrs, _stream()), "nm_mc_emit")
        keys = torch.empty(nv.value, dtype=torch.int64, device=dev)
        out["vertices"] = V = nv.value
        out["faces"] = nf.value
        out["stages_ms"]["keys"] = gpu_ms(lambda: check(lib.nm_mc_vertex_edges(_ptr(scratch), V, 0, res, res, res, 0, _ptr(keys), _stream()),
                                                        "nm_mc_vertex_edges"), opt.reps)
        verts = views()[0]
        out["centre_vertices"] = int(((keys & 3) == 3).sum())
        with gs.quiet():
            out["extract_geometry_ms_ss0"] = gs.wall_ms(lambda: mesh_nerf.extract_geometry(model, dev, args), opt.reps)
        flops = net.flops_per_sample(density_only=True)
        for ss in opt.ss:
            fine = [hip_ops.fine_axis(args.limit, n, ss) for n in nums]
            pts = hip_ops.mc_edge_points(keys, nums, ss, ax, fine)
            n_pts = pts.numel() // 3
            sigma = net.sample_density(pts.view(-1, 3))
            row = {"ss": ss, "fine_points": n_pts, "stages_ms": {}}
            row["stages_ms"]["points"] = gpu_ms(lambda: hip_ops.mc_edge_points(keys, nums, ss, ax, fine), opt.reps)
            t_density = gpu_ms(lambda: net.sample_density(pts.view(-1, 3)), opt.reps)
            row["stages_ms"]["density"] = t_density
            row["stages_ms"]["refine"] = gpu_ms(lambda: hip_ops.mc_refine_vertices(density, 0, iso, keys, ss, sigma.view(-1, ss),
                                                                                 verts.clone()), opt.reps)
            row["density_tflops"] = n_pts * flops / (t_density * 1e-3) / 1e12
            row["density_frac_of_peak"] = row["density_tflops"] / FP32_MFMA_PEAK_TFLOPS
            ss_args = mesh_nerf.build_parser().parse_args(["--res", str(res), "--iso-level", "32", "--super-sampling", str(ss)])
            with gs.quiet():
                row["extract_geometry_ms"] = gs.wall_ms(lambda: mesh_nerf.extract_geometry_with_super_sampling(model, dev, ss_args), opt.reps)
            row["extra_over_ss0"] = row["extract_geometry_ms"] / out["extract_geometry_ms_ss0"] - 1.0
            # what the dense grids of the reference's sketch would cost at the measured grid rate
            dense_points = sum((n - 1) * (ss + 1) + 1 for n in nums) * res * res
            row["dense_grids_points"] = dense_points
            row["dense_grids_est_ms"] = out["stages_ms"]["grid"] * dense_points / (res ** 3)
            out["per_ss"].append(row)
            print(json.dumps(row), flush=True)
    text = json.dumps(out, indent=1)
    print(text)
    gs.write_json(out, opt.out)


if __name__ == "__main__":
    main()
