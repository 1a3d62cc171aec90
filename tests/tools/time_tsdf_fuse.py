"""TSDF fusion (mesh_nerf --geometry tsdf) at --res 480 with 32 views of 800^2 on the synthetic scene: the render of the views
(wall clock, synchronised), nm_tsdf_integrate alone under HIP events (warm-up, median), the same rule written with torch device
ops beside it -- compared for equal bytes --, and the whole `--geometry tsdf` export beside the `--geometry density` export, each
with `--render-views 8 --render-ssim`: seconds, vertex and face counts, PSNR / SSIM / depth difference / IoU against the
network's own renders.  A projection is counted as one voxel in one view; the field's bytes as what the call must move once.

    python tests/tools/time_tsdf_fuse.py [--res 480] [--views 32] [--size 800] [--reps 11] [--out profiles/r17_tsdf_fuse.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nerfmeshes_amd import hip_ops, mesh_nerf  # noqa: E402
from tests import gpu_support as gs  # noqa: E402


def torch_integrate(views, depth, opacity, axes, trunc, near, min_opacity):
    """the rule of include/nerfmeshes_hip.h ("TSDF fusion") with torch ops: every operation a kernel of its own, so none is
    fused -> (field, observations, counts)"""
    n0, n1, n2 = (a.numel() for a in axes)
    shape = (n0, n1, n2)
    px = axes[0].double()[:, None, None].expand(shape).reshape(-1)
    py = axes[1].double()[None, :, None].expand(shape).reshape(-1)
    pz = axes[2].double()[None, None, :].expand(shape).reshape(-1)
    total = torch.zeros_like(px)
    n = torch.zeros(px.shape, dtype=torch.int32, device=px.device)
    occluded = torch.zeros(px.shape, dtype=torch.bool, device=px.device)
    for v, view in enumerate(views):
        m = [[float(view.c2w[4 * a + k]) for k in range(4)] for a in range(3)]
        height, width, focal = int(view.height), int(view.width), float(view.focal)
        dx, dy, dz = px - m[0][3], py - m[1][3], pz - m[2][3]
        cx, cy, cz = ((m[0][k] * dx + m[1][k] * dy) + m[2][k] * dz for k in range(3))
        z = -cz
        inside = z >= near
        col = torch.round((cx / z) * focal + 0.5 * width)
        row = torch.round(0.5 * height - (cy / z) * focal)
        inside &= (col >= 0) & (col <= width - 1) & (row >= 0) & (row <= height - 1)
        at = torch.where(inside, row * width + col, torch.zeros_like(row)).long()
        d = depth[v].reshape(-1)[at]
        hit = torch.isfinite(d) & (d > 0)
        if opacity is not None:
            hit &= opacity[v].reshape(-1)[at].double() >= min_opacity
        s = z - d.double()
        hidden = inside & hit & (s > trunc)
        t = torch.where(hit, torch.clamp_min(s / trunc, -1.0), torch.full_like(s, -1.0))
        seen = inside & ~hidden
        total = torch.where(seen, total + t, total)
        n += seen
        occluded |= hidden
    field = torch.where(n > 0, (total / n.clamp_min(1).double()).float(),
                        torch.where(occluded, torch.ones_like(total, dtype=torch.float32), -torch.ones_like(total, dtype=torch.float32)))
    counts = torch.stack(((n > 0).sum(), ((n == 0) & occluded).sum(), ((n == 0) & ~occluded).sum()))
    return field, n, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=480)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--render-views", type=int, default=8)
    ap.add_argument("--skip-export", action="store_true", help="only the render and the fusion, not the whole exports")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    model = gs.scene_model(dev)
    cfg = model.cfg
    limit = 1.2
    common = ["--res", str(opt.res), "--iso-level", "32", "--limit", str(limit), "--view-disparity-max-bound", "1e0"]
    tsdf = ["--geometry", "tsdf", "--tsdf-views", str(opt.views), "--tsdf-size", str(opt.size)]
    out = {"res": opt.res, "scene": "synthetic.make_scene_weights (8x256)", "limit": limit, "views": opt.views, "size": opt.size,
           "reps": opt.reps, "device": torch.cuda.get_device_name(0)}

    with torch.no_grad():
        args = mesh_nerf.build_parser().parse_args(common + tsdf)
        with gs.quiet():                                              # the first view warms the render kernels up
            mesh_nerf.tsdf_render_views(model, mesh_nerf.build_parser().parse_args(common + tsdf[:2] + ["--tsdf-views", "1", "--tsdf-size",
                                                                                                       str(opt.size)]), cfg, dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        views, depth, opacity = mesh_nerf.tsdf_render_views(model, args, cfg, dev)
        torch.cuda.synchronize()
        out["render_s"] = time.perf_counter() - t0
        out["render_s_per_view"] = out["render_s"] / opt.views
        nums = (opt.res,) * 3
        axes = mesh_nerf._axes(args, nums, dev)
        trunc = float(args.tsdf_trunc) * 2.0 * limit / (opt.res - 1)
        near, min_opacity = float(cfg.dataset.near), float(args.tsdf_min_opacity)
        run = lambda: hip_ops.tsdf_integrate(views, depth, opacity, axes, trunc, near, min_opacity=min_opacity)   # noqa: E731
        got = run()
        voxels = opt.res ** 3
        ms = gs.gpu_ms(run, opt.reps)
        out["integrate"] = {"ms": ms, "projections": voxels * opt.views, "projections_per_s": voxels * opt.views / (ms * 1e-3),
                            "field_gb_per_s": 4 * voxels / (ms * 1e-3) / 1e9,
                            "counts": dict(zip(hip_ops.TSDF_COUNTS, (int(x) for x in got["counts"].tolist()))),
                            "hit_pixels": int(((opacity >= min_opacity) & torch.isfinite(depth) & (depth > 0)).sum()),
                            "pixels": int(depth.numel())}
        print(json.dumps({"render_s": out["render_s"], "integrate": out["integrate"]}), flush=True)
        gs.write_json(out, opt.out)
        want = torch_integrate(views, depth, opacity, axes, trunc, near, min_opacity)
        out["torch_ops"] = {"field_bytes_equal": bool(torch.equal(want[0].view(torch.int32), got["field"].view(torch.int32))),
                            "counts_equal": want[2].tolist() == got["counts"].tolist(),
                            "fields_differing": int((want[0].view(torch.int32) != got["field"].view(torch.int32)).sum())}
        del want
        out["torch_ops"]["ms"] = gs.gpu_ms(lambda: torch_integrate(views, depth, opacity, axes, trunc, near, min_opacity), 3)
        print(json.dumps({"torch_ops": out["torch_ops"]}), flush=True)
        gs.write_json(out, opt.out)
        del got, depth, opacity
        if not opt.skip_export:
            out["export"] = {}
            scoring = ["--render-views", str(opt.render_views), "--render-ssim"]
            for name, extra in (("density", []), ("tsdf", tsdf)):
                d = tempfile.mkdtemp(prefix=f"nm_tsdf_time_{name}_")
                a = mesh_nerf.build_parser().parse_args(common + extra + scoring + ["--save-dir", d])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with gs.quiet():
                    v, f, _, _ = mesh_nerf.export_marching_cubes(model, a, cfg, dev)
                torch.cuda.synchronize()
                row = {"whole_s": time.perf_counter() - t0, "vertices": int(v.shape[0]), "faces": int(f.shape[0]),
                       "obj_bytes": os.path.getsize(os.path.join(d, "mesh.obj")),
                       "render_mean": json.load(open(os.path.join(d, "mesh.render.json")))["mean"]}
                if name == "tsdf":
                    row["report"] = json.load(open(os.path.join(d, "mesh.tsdf.json")))
                out["export"][name] = row
                print(json.dumps({f"export {name}": row}), flush=True)
                gs.write_json(out, opt.out)
    gs.write_json(out, opt.out)


if __name__ == "__main__":
    main()
