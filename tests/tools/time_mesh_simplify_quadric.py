"""Quadric placement (mesh_nerf --simplify-cell K --simplify-placement quadric) at --res 480 --iso-level 32 --limit 1.2 on the
synthetic scene, for K = 2 and 4: the stage (hip_ops.mesh_simplify) under HIP events with both placements and both insertion
variants, measured in alternating rounds so that they share whatever else the machine does; the face pass alone and the
zeroing of its array alone; the five counts; and chamfer(simplified, dense) under both placements at mesh_chamfer's default
sample count.  `--parent-lib PATH` names a libnerfmeshes_hip.so built from the parent commit: the mean stage through the C
entries (cluster + emit, the wrapper's calls) is then timed against this commit's library in the same rounds, to show that
the default path did not move.

    python tests/tools/time_mesh_simplify_quadric.py [--res 480] [--reps 21] [--parent-lib PATH] [--out profiles/r18_simplify_quadric.json]
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

ENTRIES = ("nm_mesh_simplify_workspace_bytes", "nm_mesh_simplify_cluster", "nm_mesh_simplify_emit")


def bind(path):
    """the three mean-placement entries of the library at `path`"""
    lib = C.CDLL(path)
    for name in ENTRIES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def mean_stage(lib, v, f, n, cell, origin):
    """hip_ops.mesh_simplify's mean path as calls of `lib`: cluster (with its read-back), then emit -> the closure that runs it"""
    nv, nf = v.shape[0], f.shape[0]
    ws = torch.empty(int(lib.nm_mesh_simplify_workspace_bytes(nv, nf)), dtype=torch.uint8, device=v.device)
    counts = (C.c_int64 * 7)()
    ptr, stream = hip_ops._ptr, hip_ops._stream

    def run():
        assert lib.nm_mesh_simplify_cluster(ptr(v), nv, ptr(f), nf, ptr(n), *origin, cell, 0, ptr(ws), counts, stream()) == 0
        kv, kf = int(counts[1]), int(counts[2])
        ov, of, on = torch.empty(kv, 3, device=v.device), torch.empty(kf, 3, dtype=torch.int32, device=v.device), torch.empty(kv, 3, device=v.device)
        assert lib.nm_mesh_simplify_emit(ptr(ws), ptr(v), nv, ptr(f), nf, ptr(n), *origin, cell, kv, kf, ptr(ov), ptr(of), ptr(on),
                                         stream()) == 0
        return ov, of, on
    return run


def alternating(fns, reps, warm=2):
    """every fn of the dict once per round, `reps` timed rounds after `warm`, each call under its own pair of HIP events
    -> {name: {"median_ms", "min_ms", "max_ms"}}"""
    times = {name: [] for name in fns}
    for i in range(warm + reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= warm:
                times[name].append(a.elapsed_time(b))
    return {name: {"median_ms": sorted(t)[len(t) // 2], "min_ms": min(t), "max_ms": max(t)} for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=480)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--cells", type=float, nargs="*", default=[2.0, 4.0])
    ap.add_argument("--parent-lib", default=None, help="a libnerfmeshes_hip.so built from the parent commit")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    model = gs.scene_model(dev)
    limit = 1.2
    common = ["--res", str(opt.res), "--iso-level", "32", "--limit", str(limit), "--view-disparity-max-bound", "1e0"]
    out = {"res": opt.res, "scene": "synthetic.make_scene_weights (8x256)", "iso_level": 32, "limit": limit, "reps": opt.reps,
           "device": torch.cuda.get_device_name(0), "default_aggregate": hip_ops.SIMPLIFY_AGGREGATE,
           "default_quadric_aggregate": hip_ops.SIMPLIFY_QUADRIC_AGGREGATE, "timing": "HIP events around one call, 2 warm-up rounds, variants alternating within every round", "cells": {}}
    lib = _lib.load()
    parent = bind(opt.parent_lib) if opt.parent_lib else None
    with torch.no_grad():
        args = mesh_nerf.build_parser().parse_args(common)
        with gs.quiet():
            v, f, n, _ = mesh_nerf.extract_geometry(model, dev, args)
        f = f.to(torch.int32).contiguous()
        nv, nf = int(v.shape[0]), int(f.shape[0])
        out.update(vertices=nv, faces=nf)
        origin = (-limit,) * 3
        for k in opt.cells:
            cell = float(k * (2.0 * limit / opt.res))
            row = {"cell_world": cell}
            stage = {f"{placement}_{name}": (lambda p=placement, a=aggregate: hip_ops.mesh_simplify(v, f, n, cell=cell, origin=origin,
                                                                                                    aggregate=a, placement=p))
                     for placement in hip_ops.SIMPLIFY_PLACEMENTS for name, aggregate in (("lane_atomics", False), ("wave_aggregated", True))}
            # hip_ops' defaults: SIMPLIFY_AGGREGATE for the vertex pass, SIMPLIFY_QUADRIC_AGGREGATE for the face pass
            stage["quadric_default"] = lambda: hip_ops.mesh_simplify(v, f, n, cell=cell, origin=origin, placement="quadric")
            row["stage_ms"] = alternating(stage, opt.reps)
            # the face pass alone (its array zeroed first, as in every call) and the zeroing alone (no faces), after one cluster call
            ptr, stream = hip_ops._ptr, hip_ops._stream
            ws = torch.empty(int(lib.nm_mesh_simplify_workspace_bytes(nv, nf)), dtype=torch.uint8, device=dev)
            qws = torch.empty(int(lib.nm_mesh_simplify_quadric_workspace_bytes(nv, nf)), dtype=torch.uint8, device=dev)
            counts = (C.c_int64 * 7)()
            assert lib.nm_mesh_simplify_cluster(ptr(v), nv, ptr(f), nf, ptr(n), *origin, cell, 0, ptr(ws), counts, stream()) == 0
            passes = {name: (lambda faces=faces, flags=flags: lib.nm_mesh_simplify_quadric_faces(ptr(ws), ptr(v), nv, ptr(f), faces,
                                                                                                 *origin, cell, flags, ptr(qws), stream()))
                      for name, faces, flags in (("zeroing_only", 0, 0), ("lane_atomics", nf, 0), ("wave_aggregated", nf, 1))}
            row["face_pass_ms"] = alternating(passes, opt.reps)
            row["quadric_workspace_bytes"] = int(qws.numel())
            if parent is not None:
                both = {"this_commit": mean_stage(lib, v, f, n, cell, origin), "parent_commit": mean_stage(parent, v, f, n, cell, origin)}
                a, b = both["this_commit"](), both["parent_commit"]()
                assert all(torch.equal(x, y) for x, y in zip(a, b)), "the default path's bytes moved"
                row["mean_stage_c_entries_ms"] = alternating(both, opt.reps)
            mv, mf, _, _ = hip_ops.mesh_simplify(v, f, n, cell=cell, origin=origin)
            qv, qf, _, info = hip_ops.mesh_simplify(v, f, n, cell=cell, origin=origin, placement="quadric")
            assert torch.equal(mf, qf)
            row["info"] = info
            row["largest_move_in_cells"] = float((qv - mv).abs().max()) / cell
            for name, sv in (("mean", mv), ("quadric", qv)):
                report = mesh_chamfer.compare_meshes(sv, mf, v, f, device=dev)
                row[f"chamfer_to_dense_{name}"] = {key: report[key] for key in report if not isinstance(report[key], dict)}
            out["cells"][f"K={k:g}"] = row
            print(json.dumps({f"K={k:g}": row}), flush=True)
    gs.write_json(out, opt.out)


if __name__ == "__main__":
    main()
