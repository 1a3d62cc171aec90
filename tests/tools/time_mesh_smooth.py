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
import contextlib
import ctypes as C
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nerfmeshes_amd import _lib, hip_ops, mesh_chamfer, mesh_nerf, models, synthetic as S  # noqa: E402


def gpu_ms(fn, reps):
    """median of `reps` HIP-event timings of fn() on the current stream (two warm-up calls first)"""
    fn()
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


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
    model = models.NeRFModel(S.hparams())
    sd = model.state_dict()
    for prefix in ("model_coarse.", "model_fine."):
        for k, v in S.make_scene_weights().items():
            sd[prefix + k] = torch.from_numpy(v)
    model.load_state_dict(sd)
    model = model.eval().to(dev)
    quiet = lambda: contextlib.redirect_stdout(io.StringIO())      # noqa: E731
    limit, lam, mu = 1.2, 0.5, -0.53
    common = ["--res", str(opt.res), "--iso-level", "32", "--limit", str(limit), "--view-disparity-max-bound", "1e0"]
    out = {"res": opt.res, "scene": "synthetic.make_scene_weights (8x256)", "iso_level": 32, "limit": limit, "reps": opt.reps,
           "runs": opt.runs, "device": torch.cuda.get_device_name(0), "lambda": lam, "mu": mu, "stage": {}, "export": {}}
    with torch.no_grad():
        args = mesh_nerf.build_parser().parse_args(common)
        with quiet():
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
                   half_step_bytes=step_bytes, build_ms=gpu_ms(build, opt.reps))
        adjacency = torch_adjacency(v, f)
        out["torch_ops_build_ms"] = gpu_ms(lambda: torch_adjacency(v, f), max(3, opt.reps // 4))
        print(json.dumps({key: out[key] for key in ("vertices", "faces", "edges", "build_ms", "torch_ops_build_ms")}), flush=True)
        for k in opt.iterations:
            row = {"run_ms": gpu_ms(lambda: run(k), opt.reps)}
            row["half_step_us"] = 1e3 * row["run_ms"] / (2 * k)
            row["half_step_gb_per_s"] = step_bytes / (row["half_step_us"] * 1e-6) / 1e9
            run(k)
            row["normals_ms"] = gpu_ms(normals, opt.reps)
            tv = torch_run(v, adjacency, k, lam, mu)
            row["torch_max_abs_position_difference"] = float((tv - sv).abs().max())
            row["torch_ops_run_ms"] = gpu_ms(lambda: torch_run(v, adjacency, k, lam, mu), max(3, opt.reps // 4))
            row["largest_displacement_voxels"] = float(torch.linalg.vector_norm(sv - v, dim=1).max()) / (2.0 * limit / opt.res)
            report = mesh_chamfer.compare_meshes(sv, f, v, f, device=dev)
            row["chamfer_to_unsmoothed"] = {key: report[key] for key in report if not isinstance(report[key], dict)}
            out["stage"][f"N={k}"] = row
            print(json.dumps({f"N={k}": row}), flush=True)
        if not opt.skip_export:
            stages = {}

            def timed(name, fn):
                def wrapper(*a, **kw):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    r = fn(*a, **kw)
                    torch.cuda.synchronize()
                    stages[name] = stages.get(name, 0.0) + 1e3 * (time.perf_counter() - t0)
                    return r
                return wrapper

            real = mesh_nerf.extract_geometry, mesh_nerf.smooth_mesh, mesh_nerf.export_obj
            mesh_nerf.extract_geometry = timed("geometry_ms", real[0])
            mesh_nerf.smooth_mesh = timed("smooth_ms", real[1])
            mesh_nerf.export_obj = timed("obj_ms", real[2])
            try:
                for k in [0] + list(opt.iterations):
                    d = tempfile.mkdtemp(prefix="nm_smooth_time_")
                    a = mesh_nerf.build_parser().parse_args(common + ["--save-dir", d, "--smooth-iters", str(k)])
                    runs = []
                    for i in range(opt.runs + 1):                  # the first run warms up
                        stages.clear()
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        with quiet():
                            mesh_nerf.export_marching_cubes(model, a, model.cfg, dev)
                        torch.cuda.synchronize()
                        whole = 1e3 * (time.perf_counter() - t0)
                        if i:
                            runs.append(dict(stages, whole_ms=whole, appearance_and_rest_ms=whole - sum(stages.values())))
                    runs.sort(key=lambda r: r["whole_ms"])
                    out["export"][f"N={k}"] = {"median": runs[len(runs) // 2], "whole_ms_all_runs": [r["whole_ms"] for r in runs],
                                               "obj_bytes": os.path.getsize(os.path.join(d, "mesh.obj"))}
                    print(json.dumps({f"export N={k}": out["export"][f"N={k}"]}), flush=True)
            finally:
                mesh_nerf.extract_geometry, mesh_nerf.smooth_mesh, mesh_nerf.export_obj = real
    text = json.dumps(out, indent=1)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
