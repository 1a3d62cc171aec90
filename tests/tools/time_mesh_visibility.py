"""The hidden-face filter (mesh_nerf --cull-hidden-views N) at --res 480 --iso-level 32 --limit 1.2 on the synthetic scene:
nm_mesh_visibility_views for N = 32, 64, 128 at the automatic --cull-size under HIP events (warm-up, median) with the
per-view time, the new_faces curve and what is kept; nm_mesh_visibility_select and _compact beside it; then the whole export
and the export with --simplify-cell 4 --texture-res 8, each with and without the option (the run without it is the former code path: the
comparison basis), and the culled mesh against the unculled one in image space -- both OBJs drawn from the 8 --render-views
poses, the PSNR between the two images of every pose (inf: no pixel differs) and each mesh's PSNR to the network's own render.

    python tests/tools/time_mesh_visibility.py [--res 480] [--reps 11] [--runs 2] [--out profiles/r15_mesh_visibility.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nerfmeshes_amd import _lib, hip_ops, mesh_nerf, mesh_render, synthetic as S  # noqa: E402
from nerfmeshes_amd.nerf.nerf_helpers import load_obj_attributes  # noqa: E402
from tests import gpu_support as gs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=480)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--views", type=int, nargs="*", default=[32, 64, 128])
    ap.add_argument("--export-views", type=int, default=64, help="--cull-hidden-views of the whole exports")
    ap.add_argument("--skip-export", action="store_true", help="only the stage, not the whole exports")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    model = gs.scene_model(dev)
    limit, radius, rings = 1.2, 3.0, 1
    size = mesh_nerf.cull_size(opt.res)
    common = ["--res", str(opt.res), "--iso-level", "32", "--limit", str(limit), "--view-disparity-max-bound", "1e0"]
    out = {"res": opt.res, "scene": "synthetic.make_scene_weights (8x256)", "iso_level": 32, "limit": limit, "reps": opt.reps,
           "runs": opt.runs, "device": torch.cuda.get_device_name(0), "cull_size": size, "cull_radius": radius, "cull_rings": rings,
           "stage": {}, "export": {}}
    with torch.no_grad():
        args = mesh_nerf.build_parser().parse_args(common)
        with gs.quiet():
            v, f, n, _ = mesh_nerf.extract_geometry(model, dev, args)
        v, f, n = v.contiguous(), f.to(torch.int32).contiguous(), n.contiguous()
        nv, nf = int(v.shape[0]), int(f.shape[0])
        centre, distance, focal, near = mesh_render.frame_views(v, radius, size)
        ws = torch.empty(int(lib.nm_mesh_visibility_workspace_bytes(nv, nf, size, size)), dtype=torch.uint8, device=dev)
        ptr, stream = hip_ops._ptr, hip_ops._stream
        out.update(vertices=nv, faces=nf, workspace_bytes=int(ws.numel()), focal=focal, near=near,
                   pixels_per_voxel=0.95 * size * (2.0 * limit / opt.res) / (2.0 * distance / radius))
        kept = [C.c_int64() for _ in range(4)]

        def select():
            hip_ops.check(lib.nm_mesh_visibility_select(ptr(f), nf, nv, rings, ptr(ws), *(C.byref(k) for k in kept), stream()),
                          "nm_mesh_visibility_select")

        for count in opt.views:
            views = [hip_ops.make_view(p, h, w, fl) for p, h, w, fl, _ in mesh_render.sphere_views(count, centre, distance, size, focal)]
            array = (_lib.View * count)(*views)
            new = torch.empty(count, dtype=torch.int64, device=dev)
            counts = torch.empty(count, len(hip_ops.RASTER_COUNTS), dtype=torch.int64, device=dev)

            def run():
                hip_ops.check(lib.nm_mesh_visibility_views(array, count, ptr(v), nv, ptr(f), nf, near, hip_ops.RASTER_LARGE_THRESHOLD, 1,
                                                           ptr(ws), ptr(new), ptr(counts), stream()), "nm_mesh_visibility_views")

            row = {"views_ms": gs.gpu_ms(run, opt.reps)}
            row["ms_per_view"] = row["views_ms"] / count
            row["select_ms"] = gs.gpu_ms(select, opt.reps)                # includes its one host synchronisation
            kv, kf = kept[0].value, kept[1].value
            ov, on = torch.empty(kv, 3, device=dev), torch.empty(kv, 3, device=dev)
            of, oi = torch.empty(kf, 3, dtype=torch.int32, device=dev), torch.empty(kf, dtype=torch.int32, device=dev)
            row["compact_ms"] = gs.gpu_ms(lambda: hip_ops.check(lib.nm_mesh_visibility_compact(
                ptr(ws), ptr(f), nf, nv, ptr(v), ptr(n), kv, kf, ptr(ov), ptr(of), ptr(on), ptr(oi), stream()),
                "nm_mesh_visibility_compact"), opt.reps)
            totals = counts.sum(0).tolist()
            row.update(vertices_kept=kv, faces_kept=kf, faces_seen=kept[2].value, bad_faces=kept[3].value, new_faces=new.tolist(),
                       raster_counts=dict(zip(hip_ops.RASTER_COUNTS, totals)))
            out["stage"][f"views={count}"] = row
            print(json.dumps({f"views={count}": {k: row[k] for k in row if k not in ("new_faces", "raster_counts")}}), flush=True)
        if not opt.skip_export:
            textured = ["--simplify-cell", "4", "--texture-res", "8"]     # the texture row of the README: 45 samples per face
            stages = {name + "_ms": name for name in ("extract_geometry", "cull_hidden", "bake_texture", "render_report")}
            for tag, extra in (("plain", []), ("culled", ["--cull-hidden-views", str(opt.export_views)]),
                               ("plain_textured", textured),
                               ("culled_textured", textured + ["--cull-hidden-views", str(opt.export_views)]),
                               ("plain_render8", ["--render-views", "8"]),
                               ("culled_render8", ["--render-views", "8", "--cull-hidden-views", str(opt.export_views)])):
                d = tempfile.mkdtemp(prefix="nm_visibility_time_")
                once = "render8" in tag                                # the render runs are there for their report, once, cold
                row, _ = gs.time_export(model, common + ["--save-dir", d] + extra, 1 if once else opt.runs, stages, dev, warm=not once)
                row.update(obj_bytes=os.path.getsize(os.path.join(d, "mesh.obj")), dir=d)
                for name in ("visibility", "render"):
                    path = os.path.join(d, f"mesh.{name}.json")
                    if os.path.exists(path):
                        report = json.load(open(path))
                        row[name] = report["mean"] if name == "render" else {k: report[k] for k in report if k != "new_faces"}
                out["export"][tag] = row
                print(json.dumps({f"export {tag}": {k: row[k] for k in row if k != "dir"}}), flush=True)
            # the two OBJs in image space: the 8 --render-views poses, vertex colours, the same rasteriser
            cfg = model.cfg
            background = (1.0,) * 3 if cfg.dataset.white_background else (0.0,) * 3
            meshes = {tag: load_obj_attributes(os.path.join(out["export"][tag]["dir"], "mesh.obj")) for tag in ("plain", "culled")}
            rows = []
            for pose, h, w, fl, _ in mesh_render.orbit_views(8, 800, 800, S.LEGO_FOCAL_800):
                images = {tag: mesh_render.render_mesh(m[0], m[1], m[2], pose, h, w, fl, cfg.dataset.near / 4, background)
                          for tag, m in meshes.items()}
                mse = float(torch.nn.functional.mse_loss(images["culled"]["rgb"], images["plain"]["rgb"]))
                rows.append({"psnr_culled_to_unculled": mesh_render.psnr(mse) if mse else None,      # None: no pixel differs
                             "pixels_that_differ": int((images["culled"]["rgb"] != images["plain"]["rgb"]).any(-1).sum()),
                             "covered_unculled": images["plain"]["counts"]["covered"],
                             "covered_culled": images["culled"]["counts"]["covered"]})
            out["image_space"] = rows
            print(json.dumps({"image_space": rows}), flush=True)
            for row in out["export"].values():
                del row["dir"]
    gs.write_json(out, opt.out)


if __name__ == "__main__":
    main()
