"""Adaptive levels (mesh_nerf --simplify-cell K --simplify-placement quadric --simplify-levels L --simplify-error E) at --res 480
--iso-level 32 --limit 1.2 on the synthetic scene, K = 2, L = 1, 2, 3: the stage (hip_ops.mesh_simplify) under HIP events
against the uniform quadric stage (levels = 0) and against each other in alternating rounds, so that they share whatever else
the machine does; every level's call (nm_mesh_simplify_adaptive_level) alone, then the faces and the emit call; the info dict;
and the exact surface report (mesh_chamfer.compare_meshes, surface="exact": accuracy, completeness, F-score at half a voxel and
at one) of the adaptive outputs and of uniform K = 2, 4 and 8 against the dense mesh.  `--parent-lib PATH` names a
libnerfmeshes_hip.so built from the parent commit: the uniform quadric stage through the C entries is then timed parent | this |
parent in the same rounds, to show that levels = 0 did not move.  Per-kernel times are a profiler's: run this tool with
--reps 3 under `rocprofv3 --kernel-trace --stats` and read the msa_* / ms_* rows.

    python tests/tools/time_mesh_simplify_adaptive.py [--res 480] [--reps 21] [--error 0.25] [--parent-lib PATH] [--out profiles/r20_simplify_adaptive.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nerfmeshes_amd import _lib, hip_ops, mesh_chamfer, mesh_nerf  # noqa: E402
from tests import gpu_support as gs  # noqa: E402
from tests.tools.time_mesh_simplify_quadric import alternating  # noqa: E402

ENTRIES = ("nm_mesh_simplify_workspace_bytes", "nm_mesh_simplify_cluster", "nm_mesh_simplify_quadric_workspace_bytes",
           "nm_mesh_simplify_quadric_faces", "nm_mesh_simplify_emit_quadric")


def bind(path):
    """the uniform quadric stage's entries of the library at `path`"""
    lib = C.CDLL(path)
    for name in ENTRIES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def quadric_stage(lib, v, f, n, cell, origin):
    """hip_ops.mesh_simplify(placement="quadric") as calls of `lib` -> the closure that runs it"""
    nv, nf = v.shape[0], f.shape[0]
    ws = torch.empty(int(lib.nm_mesh_simplify_workspace_bytes(nv, nf)), dtype=torch.uint8, device=v.device)
    qws = torch.empty(int(lib.nm_mesh_simplify_quadric_workspace_bytes(nv, nf)), dtype=torch.uint8, device=v.device)
    counts, tally = (C.c_int64 * 7)(), (C.c_int64 * 5)()
    ptr, stream = hip_ops._ptr, hip_ops._stream
    flags = 1 if hip_ops.SIMPLIFY_AGGREGATE else 0
    face_flags = 1 if hip_ops.SIMPLIFY_QUADRIC_AGGREGATE else 0

    def run():
        assert lib.nm_mesh_simplify_cluster(ptr(v), nv, ptr(f), nf, ptr(n), *origin, cell, flags, ptr(ws), counts, stream()) == 0
        kv, kf = int(counts[1]), int(counts[2])
        ov, of, on = torch.empty(kv, 3, device=v.device), torch.empty(kf, 3, dtype=torch.int32, device=v.device), torch.empty(kv, 3, device=v.device)
        assert lib.nm_mesh_simplify_quadric_faces(ptr(ws), ptr(v), nv, ptr(f), nf, *origin, cell, face_flags, ptr(qws), stream()) == 0
        assert lib.nm_mesh_simplify_emit_quadric(ptr(ws), ptr(qws), ptr(v), nv, ptr(f), nf, ptr(n), *origin, cell, kv, kf, ptr(ov),
                                                 ptr(of), ptr(on), tally, stream()) == 0
        return ov, of, on
    return run


def level_calls(lib, v, f, n, cell, origin, levels, error):
    """-> {name: closure}: every level's call alone, in the order a run makes them, then the faces and the emit call"""
    nv, nf = v.shape[0], f.shape[0]
    ws = torch.empty(int(lib.nm_mesh_simplify_workspace_bytes(nv, nf)), dtype=torch.uint8, device=v.device)
    qws = torch.empty(int(lib.nm_mesh_simplify_quadric_workspace_bytes(nv, nf)), dtype=torch.uint8, device=v.device)
    aws = torch.empty(int(lib.nm_mesh_simplify_adaptive_workspace_bytes(nv, nf)), dtype=torch.uint8, device=v.device)
    counts, tally = (C.c_int64 * 79)(), (C.c_int64 * 14)()
    ptr, stream = hip_ops._ptr, hip_ops._stream
    flags = (1 if hip_ops.SIMPLIFY_AGGREGATE else 0) | (2 if hip_ops.SIMPLIFY_QUADRIC_AGGREGATE else 0)
    out = {}
    for level in range(levels, -1, -1):
        out[f"level_{level}"] = lambda level=level: lib.nm_mesh_simplify_adaptive_level(
            ptr(v), nv, ptr(f), nf, ptr(n), *origin, cell, level, levels, error, flags, ptr(ws), ptr(qws), ptr(aws), stream())
    out["faces"] = lambda: lib.nm_mesh_simplify_adaptive_faces(ptr(f), nf, nv, levels, ptr(ws), ptr(aws), counts, stream())

    def emit():
        kv, kf = int(counts[1]), int(counts[2])
        ov, of, on = torch.empty(kv, 3, device=v.device), torch.empty(kf, 3, dtype=torch.int32, device=v.device), torch.empty(kv, 3, device=v.device)
        return lib.nm_mesh_simplify_adaptive_emit(ptr(ws), ptr(aws), ptr(f), nf, nv, levels, 1, kv, kf, ptr(ov), ptr(of), ptr(on), tally,
                                                  stream())
    out["emit"] = emit
    return out


def surface_report(sv, sf, v, f, voxel, dev):
    report = mesh_chamfer.compare_meshes(sv, sf, v, f, device=dev, surface="exact", fscore=(0.5 * voxel, voxel))
    keep = {key: report[key] for key in ("accuracy", "completeness", "hausdorff", "normal_consistency") if key in report}
    keep["accuracy_voxels"], keep["completeness_voxels"] = report["accuracy"] / voxel, report["completeness"] / voxel
    keep["fscore_half_voxel"], keep["fscore_one_voxel"] = (row["fscore"] for row in report["fscore"])
    return keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=480)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--cell", type=float, default=2.0)
    ap.add_argument("--levels", type=int, nargs="*", default=[1, 2, 3])
    ap.add_argument("--error", type=float, default=mesh_nerf.SIMPLIFY_ERROR_DEFAULT, help="voxels")
    ap.add_argument("--parent-lib", default=None, help="a libnerfmeshes_hip.so built from the parent commit")
    ap.add_argument("--no-surface", action="store_true", help="skip the surface reports")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    model = gs.scene_model(dev)
    limit = 1.2
    voxel = 2.0 * limit / opt.res
    common = ["--res", str(opt.res), "--iso-level", "32", "--limit", str(limit), "--view-disparity-max-bound", "1e0"]
    out = {"res": opt.res, "scene": "synthetic.make_scene_weights (8x256)", "iso_level": 32, "limit": limit, "reps": opt.reps,
           "device": torch.cuda.get_device_name(0), "cell_voxels": opt.cell, "error_voxels": opt.error,
           "timing": "HIP events around one call, 2 warm-up rounds, variants alternating within every round", "levels": {}}
    lib = _lib.load()
    with torch.no_grad():
        args = mesh_nerf.build_parser().parse_args(common)
        with gs.quiet():
            v, f, n, _ = mesh_nerf.extract_geometry(model, dev, args)
        f = f.to(torch.int32).contiguous()
        out.update(vertices=int(v.shape[0]), faces=int(f.shape[0]))
        origin = (-limit,) * 3
        cell, error = float(opt.cell * voxel), float(opt.error * voxel)
        stage = {"uniform": lambda: hip_ops.mesh_simplify(v, f, n, cell=cell, origin=origin, placement="quadric")}
        for L in opt.levels:
            stage[f"L={L}"] = lambda L=L: hip_ops.mesh_simplify(v, f, n, cell=cell, origin=origin, placement="quadric", levels=L,
                                                                max_error=error)
        out["stage_ms"] = alternating(stage, opt.reps)
        base = out["stage_ms"]["uniform"]["median_ms"]
        out["stage_ratio_to_uniform"] = {name: row["median_ms"] / base for name, row in out["stage_ms"].items()}
        if opt.parent_lib:
            parent = bind(opt.parent_lib)
            three = {"parent_first": quadric_stage(parent, v, f, n, cell, origin), "this_commit": quadric_stage(lib, v, f, n, cell, origin),
                     "parent_again": quadric_stage(parent, v, f, n, cell, origin)}
            a, b = three["this_commit"](), three["parent_first"]()
            assert all(torch.equal(x, y) for x, y in zip(a, b)), "the uniform path's bytes moved"
            out["uniform_stage_c_entries_ms"] = alternating(three, opt.reps)
        for L in opt.levels:
            row = {"calls_ms": alternating(level_calls(lib, v, f, n, cell, origin, L, error), opt.reps)}
            sv, sf, _, info = hip_ops.mesh_simplify(v, f, n, cell=cell, origin=origin, placement="quadric", levels=L, max_error=error)
            row["info"] = info
            row["largest_error_voxels"] = info["largest_error"] / voxel
            if not opt.no_surface:
                row["surface_to_dense"] = surface_report(sv, sf, v, f, voxel, dev)
            out["levels"][f"L={L}"] = row
            print(json.dumps({f"L={L}": row}), flush=True)
        out["uniform"] = {}
        for k in (opt.cell, 2 * opt.cell, 4 * opt.cell):
            sv, sf, _, info = hip_ops.mesh_simplify(v, f, n, cell=float(k * voxel), origin=origin, placement="quadric")
            row = {"info": info}
            if not opt.no_surface:
                row["surface_to_dense"] = surface_report(sv, sf, v, f, voxel, dev)
            out["uniform"][f"K={k:g}"] = row
            print(json.dumps({f"K={k:g}": row}), flush=True)
    print(json.dumps({key: out[key] for key in ("stage_ms", "stage_ratio_to_uniform", "uniform_stage_c_entries_ms") if key in out}), flush=True)
    gs.write_json(out, opt.out)


if __name__ == "__main__":
    main()
