"""Mesh simplification (mesh_nerf --simplify-cell K) at --res 480 --iso-level 32 --limit 1.2 on the synthetic scene, for
K = 1.5, 2, 3, 4: the cluster + emit stage under HIP events (warm-up, median), with lane atomics and with wave aggregation, the
same result computed with torch device ops (unique / sort / scatter_add) beside it, and the whole export per stage -- geometry,
simplify, appearance, OBJ -- with the OBJ's bytes and chamfer(simplified, unsimplified) at mesh_chamfer's default sample count,
so that the accuracy cost stands next to the time saved.  K = 0 is the export as it was: its runs give the run-to-run noise.

    python tests/tools/time_mesh_simplify.py [--res 480] [--reps 21] [--runs 3] [--out profiles/r11_mesh_simplify.json]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nerfmeshes_amd import hip_ops, mesh_chamfer, mesh_nerf  # noqa: E402
from tests import gpu_support as gs  # noqa: E402


def torch_simplify(v, f, cell, origin):
    """the stage with torch device ops: cells, unique, scatter_add means (fp64: close to, not bit for bit, the kernels' exact
    means), degenerate and duplicate faces by a second unique, compaction -> (verts, faces)"""
    c = torch.floor((v - origin) / cell).to(torch.int64)
    key = c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)
    uniq, cluster = torch.unique(key, return_inverse=True)
    nc = uniq.shape[0]
    index = torch.arange(v.shape[0], device=v.device)
    rep = torch.full((nc,), v.shape[0], dtype=torch.int64, device=v.device).scatter_reduce(0, cluster, index, "amin")
    count = torch.zeros(nc, dtype=torch.float64, device=v.device).scatter_add(0, cluster, torch.ones_like(cluster, dtype=torch.float64))
    mean = torch.zeros(nc, 3, dtype=torch.float64, device=v.device).index_add(0, cluster, v.double()) / count[:, None]
    tri = rep[cluster[f.long()]]
    live = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    alive = torch.nonzero(live)[:, 0]
    t = tri[alive]
    k = torch.argmin(t, dim=1, keepdim=True)
    canon = torch.gather(t, 1, (k + torch.arange(3, device=v.device)) % 3)
    _, inverse = torch.unique(canon, dim=0, return_inverse=True)
    first = torch.full((int(inverse.max()) + 1 if inverse.numel() else 0,), f.shape[0], dtype=torch.int64,
                       device=v.device).scatter_reduce(0, inverse, alive, "amin")
    kept = torch.sort(first).values
    used = torch.zeros(v.shape[0], dtype=torch.bool, device=v.device)
    used[tri[kept].reshape(-1)] = True
    new = torch.cumsum(used, 0) - 1
    reps = torch.nonzero(used)[:, 0]
    return mean[cluster[reps]].float(), new[tri[kept]].to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=480)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cells", type=float, nargs="*", default=[1.5, 2.0, 3.0, 4.0])
    ap.add_argument("--skip-export", action="store_true", help="only the stage, not the whole exports")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    model = gs.scene_model(dev)
    limit = 1.2
    common = ["--res", str(opt.res), "--iso-level", "32", "--limit", str(limit), "--view-disparity-max-bound", "1e0"]
    out = {"res": opt.res, "scene": "synthetic.make_scene_weights (8x256)", "iso_level": 32, "limit": limit, "reps": opt.reps,
           "runs": opt.runs, "device": torch.cuda.get_device_name(0), "default_aggregate": hip_ops.SIMPLIFY_AGGREGATE,
           "stage": {}, "export": {}}
    with torch.no_grad():
        args = mesh_nerf.build_parser().parse_args(common)
        with gs.quiet():
            v, f, n, _ = mesh_nerf.extract_geometry(model, dev, args)
        out.update(vertices=int(v.shape[0]), faces=int(f.shape[0]))
        origin = (-limit,) * 3
        origin_t = torch.tensor(origin, device=dev)
        for k in opt.cells:
            cell = k * (2.0 * limit / opt.res)
            row = {"cell_world": cell}
            for name, aggregate in (("lane_atomics_ms", False), ("wave_aggregated_ms", True)):
                row[name] = gs.gpu_ms(lambda: hip_ops.mesh_simplify(v, f, n, cell=cell, origin=origin, aggregate=aggregate), opt.reps)
            sv, sf, _, info = hip_ops.mesh_simplify(v, f, n, cell=cell, origin=origin)
            row["info"] = info
            tv, tf = torch_simplify(v, f, cell, origin_t)
            assert torch.equal(tf, sf) and tv.shape == sv.shape, "torch ops and the kernels disagree on the faces"
            row["torch_max_abs_position_difference"] = float((tv - sv).abs().max())
            row["torch_ops_ms"] = gs.gpu_ms(lambda: torch_simplify(v, f, cell, origin_t), max(3, opt.reps // 4))
            report = mesh_chamfer.compare_meshes(sv, sf, v, f, device=dev)
            row["chamfer_to_unsimplified"] = {key: report[key] for key in report if not isinstance(report[key], dict)}
            out["stage"][f"K={k:g}"] = row
            print(json.dumps({f"K={k:g}": row}), flush=True)
        if not opt.skip_export:
            stages = {"geometry_ms": "extract_geometry", "simplify_ms": "simplify_mesh", "obj_ms": "export_obj"}
            for k in [0.0] + list(opt.cells):
                d = tempfile.mkdtemp(prefix="nm_simplify_time_")
                row, res = gs.time_export(model, common + ["--save-dir", d, "--simplify-cell", str(k)], opt.runs, stages, dev,
                                          rest_key="appearance_and_rest_ms")
                out["export"][f"K={k:g}"] = dict(row, vertices=int(res[0].shape[0]), faces=int(res[1].shape[0]),
                                                 obj_bytes=os.path.getsize(os.path.join(d, "mesh.obj")))
                print(json.dumps({f"export K={k:g}": out["export"][f"K={k:g}"]}), flush=True)
    gs.write_json(out, opt.out)


if __name__ == "__main__":
    main()
