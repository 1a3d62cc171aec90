"""Taubin smoothing (mesh_nerf --smooth-iters N) at --res 480 --iso-level 32 --limit 1.2 on the synthetic scene, for
N = 1, 5, 10, 20: nm_mesh_smooth_build (edge table, boundary bits, adjacency) and nm_mesh_smooth_run (the 2 N half-steps)
separately under HIP events (warm-up, median), the vertex normals of the result, the same filter written with torch device ops
(index_add in fp64: close to, not bit for bit, the kernels' exact means) beside it, and the whole export per stage -- geometry,
smooth, appearance, OBJ -- with chamfer(smoothed, unsmoothed) at mesh_chamfer's default sample count.  A half-step's bytes are
counted as what it must move once -- per vertex its row in and out, its degree and its offset, per list entry the index and the
neighbour's row -- so that bytes / time can be held against the HBM rate.  N = 0 is the export as it was.

    python tests/tools/time_mesh_smooth.py [--res 480] [--reps 21] [--runs 3] [--out profiles/r12_mesh_smooth.json]
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

from nerfmeshes_amd import _lib, hip_ops, mesh_chamfer, mesh_nerf  # noqa: E402
from tests import gpu_support as gs  # noqa: E402


def torch_adjacency(v, f):
    """unique undirected edges with torch device ops -> (src, dst: both directions; degree (V,) fp64; movable (V,) bool)"""
    e = torch.cat((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]])).long()
    e = e[e[:, 0] != e[:, 1]]
    key, count = torch.unique((e.min(dim=1).values << 32) | e.max(dim=1).values, return_counts=True)
    a, b = key >> 32, key & 0xFFFFFFFF
    src, dst = torch.cat((a, b)), torch.cat((b, a))
    degree = torch.zeros(v.shape[0], dtype=torch.float64, device=v.device).index_add(0, src, torch.ones_like(src, dtype=torch.float64))
    pinned = torch.zeros(v.shape[0], dtype=torch.bool, device=v.device)
    pinned[a[count == 1]] = True
    pinned[b[count == 1]] = True
    return src, dst, degree, (degree > 0) & ~pinned


def torch_run(v, adjacency, iterations, lam, mu):
    src, dst, degree, movable = adjacency
    x = v
    for _ in range(iterations):
        for factor in (lam, mu):
            mean = torch.zeros(v.shape[0], 3, dtype=torch.float64, device=v.device).index_add(0, src, x[dst].double()) / degree[:, None]
            x = torch.where(movable[:, None], (x.double() + factor * (mean - x.double())).float(), x)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=480)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iterations", type=int, nargs="*", default=[1, 5, 10, 20])
    ap.add_argument("--skip-export", action="store_true", help="only the stage, not the whole exports")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    model = gs.scene_model(dev)
    limit, lam, mu = 1.2, 0.5, -0.53
    common = ["--res", str(opt.res), "--iso-level", "32", "--limit", str(limit), "--view-disparity-max-bound", "1e0"]
    out = {"res": opt.res, "scene": "synthetic.make_scene_weights (8x256)", "iso_level": 32, "limit": limit, "reps": opt.reps,
           "runs": opt.runs, "device": torch.cuda.get_device_name(0), "lambda": lam, "mu": mu, "stage": {}, "export": {}}
    with torch.no_grad():
        args = mesh_nerf.build_parser().parse_args(common)
        with gs.quiet():
            v, f, n, _ = mesh_nerf.extract_geometry(model, dev, args)
        v, f, n = v.contiguous(), f.to(torch.int32).contiguous(), n.contiguous()
        nv, nf = int(v.shape[0]), int(f.shape[0])
        ws = torch.empty(int(lib.nm_mesh_smooth_workspace_bytes(nv, nf)), dtype=torch.uint8, device=dev)
        counts = (C.c_int64 * 9)()
        ptr, stream = hip_ops._ptr, hip_ops._stream
        sv, sn = torch.empty_like(v), torch.empty_like(n)

        def build():
            hip_ops.check(lib.nm_mesh_smooth_build(ptr(v), nv, ptr(f), nf, ptr(ws), counts, stream()), "nm_mesh_smooth_build")

        def run(iterations):
            hip_ops.check(lib.nm_mesh_smooth_run(ptr(ws), ptr(v), nv, iterations, lam, mu, 0, ptr(sv), stream()), "nm_mesh_smooth_run")

        def normals():
            hip_ops.check(lib.nm_mesh_vertex_normals(ptr(sv), nv, ptr(f), nf, ptr(n), mesh_nerf.SMOOTH_FLIP, ptr(ws), ptr(sn), stream()),
                          "nm_mesh_vertex_normals")

        build()
        edges = int(counts[0])
        step_bytes = nv * (12 + 12 + 4 + 8) + 2 * edges * (4 + 12)
        out.update(vertices=nv, faces=nf, edges=edges, boundary_vertices=int(counts[3]), workspace_bytes=int(ws.numel()),
                   half_step_bytes=step_bytes, build_ms=gs.gpu_ms(build, opt.reps))
        adjacency = torch_adjacency(v, f)
        out["torch_ops_build_ms"] = gs.gpu_ms(lambda: torch_adjacency(v, f), max(3, opt.reps // 4))
        print(json.dumps({key: out[key] for key in ("vertices", "faces", "edges", "build_ms", "torch_ops_build_ms")}), flush=True)
        for k in opt.iterations:
            row = {"run_ms": gs.gpu_ms(lambda: run(k), opt.reps)}
            row["half_step_us"] = 1e3 * row["run_ms"] / (2 * k)
            row["half_step_gb_per_s"] = step_bytes / (row["half_step_us"] * 1e-6) / 1e9
            run(k)
            row["normals_ms"] = gs.gpu_ms(normals, opt.reps)
            tv = torch_run(v, adjacency, k, lam, mu)
            row["torch_max_abs_position_difference"] = float((tv - sv).abs().max())
            row["torch_ops_run_ms"] = gs.gpu_ms(lambda: torch_run(v, adjacency, k, lam, mu), max(3, opt.reps // 4))
            row["largest_displacement_voxels"] = float(torch.linalg.vector_norm(sv - v, dim=1).max()) / (2.0 * limit / opt.res)
            report = mesh_chamfer.compare_meshes(sv, f, v, f, device=dev)
            row["chamfer_to_unsmoothed"] = {key: report[key] for key in report if not isinstance(report[key], dict)}
            out["stage"][f"N={k}"] = row
            print(json.dumps({f"N={k}": row}), flush=True)
        if not opt.skip_export:
            stages = {"geometry_ms": "extract_geometry", "smooth_ms": "smooth_mesh", "obj_ms": "export_obj"}
            for k in [0] + list(opt.iterations):
                d = tempfile.mkdtemp(prefix="nm_smooth_time_")
                row, _ = gs.time_export(model, common + ["--save-dir", d, "--smooth-iters", str(k)], opt.runs, stages, dev,
                                        rest_key="appearance_and_rest_ms")
                out["export"][f"N={k}"] = dict(row, obj_bytes=os.path.getsize(os.path.join(d, "mesh.obj")))
                print(json.dumps({f"export N={k}": out["export"][f"N={k}"]}), flush=True)
    gs.write_json(out, opt.out)


if __name__ == "__main__":
    main()
