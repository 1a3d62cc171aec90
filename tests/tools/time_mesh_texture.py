"""The texture atlas (mesh_nerf --texture-res N) at --res 480 --iso-level 32 --limit 1.2 --simplify-cell 4 on the synthetic
scene: the three kernels that carry data -- samples, fill, and the lookup at an 800 x 800 view -- under HIP events (warm-up,
median) with the bytes each must move, the interpolation of per-vertex colours at the same view beside the lookup, and the
whole export with and without the texture on the same commit, per stage (geometry, simplify, the bake, the files), so that
what the texture costs stands next to what it is added to.

    python tests/tools/time_mesh_texture.py [--res 480] [--texture-res 8] [--reps 21] [--runs 3] [--out profiles/r14_mesh_texture.json]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nerfmeshes_amd import hip_ops, mesh_nerf, synthetic as S  # noqa: E402
from tests import gpu_support as gs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=480)
    ap.add_argument("--simplify-cell", type=float, default=4.0)
    ap.add_argument("--texture-res", type=int, default=8)
    ap.add_argument("--img-size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--skip-export", action="store_true", help="only the stages, not the whole exports")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    model = gs.scene_model(dev)
    limit, n = 1.2, opt.texture_res
    common = ["--res", str(opt.res), "--iso-level", "32", "--limit", str(limit), "--view-disparity-max-bound", "1e0",
              "--simplify-cell", str(opt.simplify_cell)]
    out = {"res": opt.res, "scene": "synthetic.make_scene_weights (8x256)", "iso_level": 32, "limit": limit, "reps": opt.reps,
           "runs": opt.runs, "simplify_cell": opt.simplify_cell, "texture_res": n, "device": torch.cuda.get_device_name(0),
           "stage": {}, "export": {}}
    with torch.no_grad():
        args = mesh_nerf.build_parser().parse_args(common)
        with gs.quiet():
            v, f, normals, _ = mesh_nerf.extract_geometry(model, dev, args)
            v, f, normals = mesh_nerf.simplify_mesh(v, f.to(torch.int32), normals, opt.simplify_cell, args)
        nv, nf = int(v.shape[0]), int(f.shape[0])
        layout = hip_ops.mesh_texture_layout(nf, n)
        per_face = layout["samples_per_face"]
        samples, texels = nf * per_face, layout["width"] * layout["height"]
        out.update(vertices=nv, faces=nf, layout=layout, samples=samples)
        stage = out["stage"]
        # bytes that must move: the faces and their corners' positions and normals once, 24 bytes out per sample
        moved = 12 * nf + 24 * nv + 24 * samples
        ms = gs.gpu_ms(lambda: hip_ops.mesh_texture_samples(v, f, normals, n, flip=mesh_nerf.SMOOTH_FLIP), opt.reps)
        stage["samples"] = {"ms": ms, "bytes": moved, "gb_per_s": moved / ms / 1e6, "includes": "two allocations and the count read-back"}
        colours = torch.rand(samples, 3, device=dev)
        moved = 12 * samples + 3 * texels                           # every colour in once, every texel out once
        ms = gs.gpu_ms(lambda: hip_ops.mesh_texture_fill(colours, nf, n), opt.reps)
        stage["fill"] = {"ms": ms, "bytes": moved, "gb_per_s": moved / ms / 1e6}
        atlas, uv = hip_ops.mesh_texture_fill(colours, nf, n), hip_ops.mesh_texture_uv(nf, n)
        stage["uv"] = {"ms": gs.gpu_ms(lambda: hip_ops.mesh_texture_uv(nf, n), opt.reps), "bytes": 24 * nf}
        size = opt.img_size
        view = hip_ops.make_view(list(S.orbit_poses(4))[1], size, size, S.LEGO_FOCAL_800 * size / 800.0)
        raster = hip_ops.mesh_rasterize(v, f, view, 0.5)
        covered = raster[3]["covered"]
        moved = 16 * size * size + covered * (24 + 12) + 12 * size * size   # id + barycentrics, uv rows + 4 texels, rgb out
        ms = gs.gpu_ms(lambda: hip_ops.mesh_texture_lookup(raster, uv, atlas, (1.0, 1.0, 1.0)), opt.reps)
        stage["lookup"] = {"ms": ms, "bytes": moved, "gb_per_s": moved / ms / 1e6, "pixels": size * size, "covered": covered}
        vertex_colours = torch.rand(nv, 3, device=dev)
        stage["interpolate_vertex_colours"] = {"ms": gs.gpu_ms(lambda: hip_ops.mesh_interpolate(raster, f, vertex_colours, (1.0, 1.0, 1.0)),
                                                            opt.reps)}
        stage["rasterize"] = {"ms": gs.gpu_ms(lambda: hip_ops.mesh_rasterize(v, f, view, 0.5), opt.reps)}
        print(json.dumps({"stage": stage}), flush=True)
        if not opt.skip_export:
            stages = {name + "_ms": name for name in ("extract_geometry", "simplify_mesh", "bake_texture", "export_obj",
                                                      "export_obj_textured")}
            for tag, extra in (("vertex_colours", []), ("texture", ["--texture-res", str(n)]),
                               ("texture_no_view_dependence", ["--texture-res", str(n), "--no-view-dependence"]),
                               ("vertex_colours_no_view_dependence", ["--no-view-dependence"])):
                d = tempfile.mkdtemp(prefix="nm_texture_time_")
                row, _ = gs.time_export(model, common + ["--save-dir", d] + extra, opt.runs, stages, dev,
                                        rest_key="vertex_appearance_and_rest_ms")
                out["export"][tag] = dict(row, bytes={name: os.path.getsize(os.path.join(d, name)) for name in sorted(os.listdir(d))})
                print(json.dumps({f"export {tag}": out["export"][tag]}), flush=True)
    gs.write_json(out, opt.out)


if __name__ == "__main__":
    main()
