"""Surface point cloud (mesh_surface_ray) per 800 x 800 view on the synthetic 8x256 scene -> profiles/r08_surface_ray.json:
the render (NeRFModel.query_view); the new stage (nm_surface_filter + nm_surface_gather) under HIP events, warm, many calls per
timed window; the same stage done the reference's way with torch device ops (25 clamped gathers, compare / reduce chains,
boolean-mask indexing: what a user has without the kernels -- it lives here, not in the package); the bytes the stage has to
move over its time against the HBM roof; the full 32-view run and the PLY write in both formats; and the figures of the
oracle comparison (tests/test_gpu_surface_ray.py::test_against_the_cpu_oracle_under_min_opacity).

    python tests/tools/time_surface_ray.py [--size 800] [--reps 5] [--skip-full] [--skip-parity] [--out FILE.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchlib.common import HBM_PEAK_GBS  # noqa: E402
from nerfmeshes_amd import hip_ops, mesh_surface_ray as msr, synthetic as S  # noqa: E402
from tests import gpu_support as gs  # noqa: E402


def spread(fn, reps, calls=1):
    """{median, min, max} over `reps` windows of `calls` back-to-back fn(), per call (one warm-up window first)"""
    times = gs.gpu_times(fn, reps, warm=1, calls=calls)
    return {"median": times[len(times) // 2], "min": times[0], "max": times[-1]}


def torch_stage(origin, dirs, depth, rgb, size, step, dist_threshold, prob_threshold):
    """the reference's post-processing with torch device ops, in its order of operations"""
    surface = (origin + dirs * depth[..., None]).view(size, size, 3)
    rows, cols = torch.meshgrid(torch.arange(size, device=dirs.device), torch.arange(size, device=dirs.device), indexing="ij")
    near = []
    for a in range(-step, step + 1):
        for b in range(-step, step + 1):
            shifted = surface[(rows + a).clamp(0, size - 1), (cols + b).clamp(0, size - 1)]
            near.append(((shifted - surface) ** 2).sum(-1) < dist_threshold)
    votes = torch.stack(near, -1).sum(-1)
    keep = ((votes > ((2 * step + 1) ** 2 - 1) * prob_threshold) & (depth.view(size, size) > 0)).view(-1)
    d, z, c = dirs[keep], depth[keep], rgb[keep]                      # boolean-mask indexing: one host sync each
    return origin + d * z[..., None], -d, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-full", action="store_true")
    ap.add_argument("--skip-parity", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_surface_ray.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    model = gs.scene_model(dev, chunksize=3000)
    size = a.size
    tmp = tempfile.mkdtemp(prefix="nm_sr_time_")
    args = msr.build_parser().parse_args(["--save-dir", tmp, "--img-size", str(size), "--focal", str(1111.1111 * size / 800)])
    pose = S.pose_spherical(30.0, -30.0, 4.0)
    res = {"scene": "synthetic smooth scene, 8x256 coarse + fine, 64 + 128 samples", "view": f"{size} x {size}, pose_spherical(30, -30, 4)",
           "device": torch.cuda.get_device_name(0), "reps": a.reps}
    with torch.no_grad():
        bounds = torch.tensor([2.0, 6.0])
        render = lambda: model.query_view(torch.from_numpy(pose), size, size, args.focal, bounds)   # noqa: E731
        res["render_ms"] = spread(render, max(3, a.reps // 2))
        out = render()
        o, d = hip_ops.view_rays(hip_ops.make_view(pose, size, size, args.focal))
        o = o[:1].contiguous()
        mv = hip_ops.surface_min_votes(args.step_size, args.prob_threshold)
        flt = hip_ops.surface_filter(o, d, out.depth_map, size, size, args.step_size, args.dist_threshold, mv)
        kept = int(flt["count"].item())
        rows = hip_ops.surface_gather(flt, out.rgb_map, count=kept)

        def hip_stage():
            f = hip_ops.surface_filter(o, d, out.depth_map, size, size, args.step_size, args.dist_threshold, mv)
            return hip_ops.surface_gather(f, out.rgb_map, count=kept)

        def hip_filter():
            return hip_ops.surface_filter(o, d, out.depth_map, size, size, args.step_size, args.dist_threshold, mv)

        res["kept_pixels"] = kept
        res["hip_stage_ms"] = spread(hip_stage, a.reps, calls=50)
        res["hip_filter_only_ms"] = spread(hip_filter, a.reps, calls=50)
        t0 = time.perf_counter()
        for _ in range(20):
            f = hip_ops.surface_filter(o, d, out.depth_map, size, size, args.step_size, args.dist_threshold, mv)
            hip_ops.surface_gather(f, out.rgb_map)                       # with the count's D2H copy, as export_ray_trace runs it
        torch.cuda.synchronize()
        res["hip_stage_with_count_readback_wall_ms"] = 1e3 * (time.perf_counter() - t0) / 20
        ref = lambda: torch_stage(o, d, out.depth_map, out.rgb_map, size, args.step_size, args.dist_threshold, args.prob_threshold)   # noqa: E731
        res["torch_stage_ms"] = spread(ref, a.reps, calls=5)
        tp, tn, tc = ref()
        res["torch_stage_equals_hip"] = bool(torch.equal(tp, rows[0]) and torch.equal(tn, rows[1]) and torch.equal(tc, rows[2]))
        res["speedup_over_torch_stage"] = res["torch_stage_ms"]["median"] / res["hip_stage_ms"]["median"]
        # what the stage has to move: filter reads directions + depth (16 B / pixel, shared origin), writes votes + mask (5 B) and
        # one 8-byte word + 4-byte prefix per 64 pixels; gather re-reads directions, depth, colours of the kept pixels (28 B) and
        # writes 39 B per kept pixel
        n = size * size
        moved = n * (16 + 5) + (n // 64) * 12 + kept * (28 + 39)
        res["stage_bytes"] = moved
        res["stage_gb_per_s"] = moved / (res["hip_stage_ms"]["median"] * 1e-3) / 1e9
        res["stage_share_of_hbm_roof"] = res["stage_gb_per_s"] / HBM_PEAK_GBS
        res["hbm_roof_gb_per_s"] = HBM_PEAK_GBS
        res["stage_share_of_view"] = res["hip_stage_ms"]["median"] / (res["render_ms"]["median"] + res["hip_stage_ms"]["median"])

        if not a.skip_full:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with gs.quiet():
                v, nrm, c, cu = msr.export_ray_trace(model, args, model.cfg, dev)
            res["full_run"] = {"views": 32, "points": int(len(v)), "wall_s": time.perf_counter() - t0}
            for fmt in ("ascii", "binary"):
                path = os.path.join(tmp, f"cloud_{fmt}.ply")
                times = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    hip_ops.export_ply(v, nrm, cu, path, binary=fmt == "binary")
                    times.append(time.perf_counter() - t0)
                res["full_run"][f"ply_{fmt}"] = {"write_s": sorted(times)[1], "bytes": os.path.getsize(path)}

    if not a.skip_parity:
        fig = os.path.join(tmp, "figures.json")
        r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider",
                            "tests/test_gpu_surface_ray.py::test_against_the_cpu_oracle_under_min_opacity"], cwd=ROOT,
                           env=dict(os.environ, NERFMESHES_SURFACE_RAY_FIGURES=fig), capture_output=True, text=True)
        res["oracle_comparison"] = json.load(open(fig)) if os.path.exists(fig) else {"error": r.stdout[-2000:]}
        res["oracle_comparison"]["test_passed"] = r.returncode == 0
    gs.write_json(res, a.out)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
