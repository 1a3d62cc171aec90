"""The mesh-component filter (mesh_nerf --min-component-faces / --keep-largest) at --res 480 --iso-level 32 --limit 1.2 on the
synthetic scene: the label + select + compact stage under HIP events (median), its pieces, the same stage done with
scipy.sparse.csgraph on the host including both copies, the geometry stage of the same run, and the whole export with and
without --keep-largest 1 (vertex counts beside the times, so the saved appearance work is visible).

    python tests/tools/time_mesh_components.py [--res 480] [--reps 21] [--runs 3] [--out profiles/r09_mesh_components.json]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nerfmeshes_amd import hip_ops, mesh_nerf  # noqa: E402
from tests import gpu_support as gs  # noqa: E402


def host_filter(v, f, n, keep_largest):
    """the stage on the host: D2H, scipy's components, the largest by (count, smallest vertex), numpy compaction, H2D"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    hv, hf, hn = v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy()
    nv = len(hv)
    rows = np.concatenate((hf[:, 0], hf[:, 1]))
    cols = np.concatenate((hf[:, 1], hf[:, 2]))
    count, lab = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(nv, nv)), directed=False)
    sizes = np.bincount(lab[hf[:, 0]], minlength=count)
    first = np.full(count, nv, np.int64)
    np.minimum.at(first, lab, np.arange(nv))
    best = np.lexsort((first, -sizes))[:keep_largest]
    keep_c = np.zeros(count, bool)
    keep_c[best] = True
    keep_v = keep_c[lab]
    new = np.cumsum(keep_v) - 1
    out_f = new[hf[keep_v[hf[:, 0]]]].astype(np.int32)
    dev = v.device
    return torch.from_numpy(hv[keep_v]).to(dev), torch.from_numpy(out_f).to(dev), torch.from_numpy(hn[keep_v]).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=480)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    model = gs.scene_model(dev)
    common = ["--res", str(opt.res), "--iso-level", "32", "--limit", "1.2"]
    out = {"res": opt.res, "scene": "synthetic.make_scene_weights (8x256)", "iso_level": 32, "limit": 1.2, "reps": opt.reps,
           "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        args = mesh_nerf.build_parser().parse_args(common)
        with gs.quiet():
            v, f, n, _ = mesh_nerf.extract_geometry(model, dev, args)
        nv, nf = int(v.shape[0]), int(f.shape[0])
        labels, counts = hip_ops.mesh_components(f, nv)
        sizes = torch.sort(counts[counts > 0], descending=True).values
        out.update(vertices=nv, faces=nf, components=int((labels == torch.arange(nv, device=dev)).sum()),
                   largest_components=[int(x) for x in sizes[:8]])
        stage = lambda k, m=0: hip_ops.mesh_filter_components(v, f, n, min_faces=m, keep_largest=k)      # noqa: E731
        kept = stage(1)[5]
        out["keep_largest_1"] = kept
        out["filter_ms"] = {f"keep_largest_{k}": gs.gpu_ms(lambda: stage(k), opt.reps) for k in (1, 3, 16)}
        out["filter_ms"]["min_faces_50"] = gs.gpu_ms(lambda: stage(0, 50), opt.reps)
        out["label_and_count_ms"] = gs.gpu_ms(lambda: hip_ops._mesh_components(hip_ops._lib.load(), f, nv, nf), opt.reps)
        # the pieces of the labelling on a permuted copy of the faces (the same graph, another arrival order)
        perm = torch.randperm(nf, device=dev)
        fp = f[perm].contiguous()
        out["label_and_count_ms_faces_permuted"] = gs.gpu_ms(lambda: hip_ops._mesh_components(hip_ops._lib.load(), fp, nv, nf), opt.reps)
        moved = 4 * (3 * nf * 3 + nv * 8 + 2 * (kept["vertices_kept"] * 6 + kept["faces_kept"] * 3))
        out["bytes_moved_estimate"] = moved
        try:
            a = host_filter(v, f, n, 1)
            b = stage(1)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), "host and device filters differ"
            out["host_scipy_ms"] = gs.wall_ms(lambda: host_filter(v, f, n, 1), max(3, opt.reps // 4))
        except ImportError:
            out["host_scipy_ms"] = None
        with gs.quiet():
            out["geometry_ms"] = gs.wall_ms(lambda: mesh_nerf.extract_geometry(model, dev, args), opt.runs)
        out["filter_over_geometry"] = out["filter_ms"]["keep_largest_1"] / out["geometry_ms"]
        for tag, extra in (("export_default", []), ("export_keep_largest_1", ["--keep-largest", "1"]),
                           ("export_min_faces_50", ["--min-component-faces", "50"])):
            d = tempfile.mkdtemp(prefix="nm_cc_time_")
            a = mesh_nerf.build_parser().parse_args(common + ["--save-dir", d, *extra])
            res = {}

            def run():
                with gs.quiet():
                    res["v"] = mesh_nerf.export_marching_cubes(model, a, model.cfg, dev)[0].shape[0]

            out[tag] = {"wall_ms": gs.wall_ms(run, opt.runs), "vertices": int(res["v"])}
        print(json.dumps(out), flush=True)
    gs.write_json(out, opt.out)


if __name__ == "__main__":
    main()
