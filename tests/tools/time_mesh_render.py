"""The mesh rasteriser on a turntable of the synthetic scene's mesh at --res 480 --iso-level 32 --limit 1.2, 800 x 800, 64 orbit
views: the full-resolution mesh (triangles of a pixel or two: the one-lane path) and its --simplify-cell 4 version (larger
triangles), each at several large_threshold values.  Per mesh and threshold: nm_mesh_rasterize and nm_mesh_interpolate per
view under HIP events (two warm-up views, then every view timed, median and spread), the faces per path, the fragments -- the
(face, pixel) pairs that pass coverage: the most atomics the frame can issue -- against the pixels covered, and the bytes the
frame must move once (12 V + 12 F in, 8 H W written and read) held against the time.  The network's own render of a view
(query_view) stands beside it.  With --kernels the tool starts itself once more under rocprofv3's kernel trace, in a process
of its own, and adds the per-kernel times (mr_vertices, mr_faces, mr_large, mr_resolve, mr_interpolate) from its statistics.

    python tests/tools/time_mesh_render.py [--res 480] [--views 64] [--size 800] [--kernels] [--out profiles/r13_mesh_render.json]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nerfmeshes_amd import hip_ops, mesh_nerf, synthetic as S  # noqa: E402
from tests import gpu_support as gs  # noqa: E402

KERNELS = ("mr_vertices", "mr_faces", "mr_large", "mr_resolve", "mr_interpolate")


def stats(times):
    times = sorted(times)
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1]}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def turntable(verts, faces, colors, poses, size, focal, near, threshold):
    raster_ms, interp_ms, counts = [], [], None
    for nr in [0, 1] + list(range(len(poses))):                          # the first two views again: warm-up
        view = hip_ops.make_view(poses[nr], size, size, focal)
        ms, raster = timed(lambda: hip_ops.mesh_rasterize(verts, faces, view, near, large_threshold=threshold))
        ms2, _ = timed(lambda: hip_ops.mesh_interpolate(raster, faces, colors, (1.0, 1.0, 1.0)))
        raster_ms.append(ms)
        interp_ms.append(ms2)
        counts = raster[3] if counts is None else {k: counts[k] + v for k, v in raster[3].items()}
    return raster_ms[2:], interp_ms[2:], counts


def kernel_trace(opt):
    """this tool again under rocprofv3, in a process of its own -> {kernel: average microseconds per launch}"""
    d = tempfile.mkdtemp(prefix="nm_mesh_render_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "t", "--output-format", "csv", "--", sys.executable,
           os.path.abspath(__file__), "--res", str(opt.res), "--views", str(min(opt.views, 8)), "--size", str(opt.size)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=900)
    out = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            for k in KERNELS:
                if f"nm::{k}(" in row["Name"]:
                    out[k] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3,
                              "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=480)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--thresholds", type=int, nargs="*", default=[16, hip_ops.RASTER_LARGE_THRESHOLD, 1024, 2 ** 31 - 1])
    ap.add_argument("--kernels", action="store_true", help="add per-kernel times from a rocprofv3 run of this tool")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    model = gs.scene_model(dev)
    limit, size = 1.2, opt.size
    focal = S.LEGO_FOCAL_800 * size / 800.0
    near = model.cfg.dataset.near / 4
    poses = S.orbit_poses(opt.views)
    out = {"res": opt.res, "scene": "synthetic.make_scene_weights (8x256)", "iso_level": 32, "limit": limit, "views": opt.views,
           "size": size, "focal": focal, "near": near, "device": torch.cuda.get_device_name(0), "meshes": {}}
    with torch.no_grad():
        args = mesh_nerf.build_parser().parse_args(["--res", str(opt.res), "--iso-level", "32", "--limit", str(limit)])
        with gs.quiet():
            v, f, n, _ = mesh_nerf.extract_geometry(model, dev, args)
            sv, sf, _ = mesh_nerf.simplify_mesh(v, f, n, 4.0, args)
        for name, (mv, mf) in (("full", (v, f)), ("simplify_cell_4", (sv, sf))):
            mv, mf = mv.contiguous(), mf.to(torch.int32).contiguous()
            colors = (mv - mv.min()) / (mv.max() - mv.min())
            nv, nf = int(mv.shape[0]), int(mf.shape[0])
            must_move = 12 * nv + 12 * nf + 2 * 8 * size * size
            entry = {"vertices": nv, "faces": nf, "bytes_that_must_move": must_move, "thresholds": {}}
            for threshold in opt.thresholds:
                raster_ms, interp_ms, counts = turntable(mv, mf, colors, poses, size, focal, near, threshold)
                row = {"rasterize": stats(raster_ms), "interpolate": stats(interp_ms),
                       "per_view": {k: c / (opt.views + 2) for k, c in counts.items()}}
                row["fragments_per_covered_pixel"] = counts["fragments"] / max(counts["covered"], 1)
                row["gb_per_s_of_bytes_that_must_move"] = must_move / (row["rasterize"]["median_ms"] * 1e-3) / 1e9
                entry["thresholds"][str(threshold)] = row
                print(json.dumps({name: {str(threshold): row}}), flush=True)
            out["meshes"][name] = entry
        bounds = torch.tensor([model.cfg.dataset.near, model.cfg.dataset.far], dtype=torch.float32)
        chunk = 160000                                                   # rays per call, as a renderer of whole views would use

        def network_view(pose):
            for first in range(0, size * size, chunk):
                model.query_view(pose, size, size, focal, bounds, first=first, count=min(chunk, size * size - first))

        network = [timed(lambda: network_view(poses[nr % opt.views]))[0] for nr in range(5)]
        out["network_view"] = stats(network[2:])
        print(json.dumps({"network_view": out["network_view"]}), flush=True)
    if opt.kernels:
        out["kernels_full_and_simplified_all_thresholds"] = kernel_trace(opt)
        print(json.dumps(out["kernels_full_and_simplified_all_thresholds"]), flush=True)
    gs.write_json(out, opt.out)


if __name__ == "__main__":
    main()
