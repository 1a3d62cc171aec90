"""The exact surface distance (mesh_chamfer --surface exact, mesh_nerf --target-surface exact) on the --res 480 --iso-level 32
--limit 1.2 mesh of the synthetic scene and on its `--simplify-cell 4` mesh, under HIP events after warm-up (median of --reps):

* `nm_points_to_mesh` at 100 000 queries (samples of the jittered mesh) against each mesh: the whole entry, the entry at 64
  queries (the prepass that writes the face records, plus one workgroup column of the hot kernel) and their difference, the
  hot kernel; pairs/s, and the fp32 operations per pair counted from the contract (115: 9 for ap / bp / cp, 19 per segment
  term, 14 per side test, 7 for the plane term) against the packed-fp32 VALU roof, which counts a fused multiply-add as two --
  the contract has none, so half of that roof is what it can reach;
* `nm_points_nearest` at 100 000 x 100 000 on the same box: what the sampled report costs today;
* the same contract in torch device ops at a size that fits, the outputs compared for equality;
* mesh_chamfer.compare_meshes of the dense mesh against itself and against the simplified one, sampled and exact side by side.

    python tests/tools/time_surface_distance.py [--res 480] [--reps 11] [--out profiles/r19_surface_distance.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nerfmeshes_amd import _lib, hip_ops, mesh_chamfer, mesh_nerf  # noqa: E402
from tests import gpu_support as gs  # noqa: E402

ROOF_FLOPS = 157.3e12          # packed fp32 vector peak of the MI355X, a fused multiply-add counted as two
FLOPS_PER_PAIR = 115


def raw_call(x, verts, faces):
    """the C entry alone on preallocated buffers: no read-back, no allocation inside the timed window"""
    lib = _lib.load()
    n, nv, nf = int(x.shape[0]), int(verts.shape[0]), int(faces.shape[0])
    dist2 = torch.empty(n, dtype=torch.float32, device=x.device)
    face = torch.empty(n, dtype=torch.int32, device=x.device)
    normals = torch.empty(n, 3, dtype=torch.float32, device=x.device)
    ws = torch.empty(int(lib.nm_points_to_mesh_workspace_bytes(n, nf)), dtype=torch.uint8, device=x.device)

    def run():
        _lib.check(lib.nm_points_to_mesh(hip_ops._ptr(x), n, hip_ops._ptr(verts), nv, hip_ops._ptr(faces), nf, hip_ops._ptr(dist2),
                                         hip_ops._ptr(face), hip_ops._ptr(normals), hip_ops._ptr(ws), hip_ops._stream()), "nm_points_to_mesh")
    return run


def torch_contract(x, verts, faces):
    """the contract of include/nerfmeshes_hip.h in torch device ops, one op per rounding -> (dist2, face)"""
    dot = lambda u, v: (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]   # noqa: E731
    cross = lambda u, v: torch.stack((u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],   # noqa: E731
                                      u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]), -1)
    a, b, c = (verts[faces[:, k].long()] for k in range(3))
    ab, ac, bc, ca = b - a, c - a, c - b, a - c
    n = cross(ab, ac)
    nn = dot(n, n)
    zero, one = torch.zeros((), device=x.device), torch.ones((), device=x.device)

    def seg(q, e):
        t = torch.fmin(torch.fmax(dot(q, e) * (1.0 / dot(e, e)), zero), one)
        d = q - t[..., None] * e
        return dot(d, d)

    p = x[:, None, :]
    ap, bp, cp = p - a, p - b, p - c
    s1, s2, s3 = seg(ap, ab[None]), seg(bp, bc[None]), seg(cp, ca[None])
    inside = (dot(n, cross(ab[None], ap)) >= 0) & (dot(n, cross(bc[None], bp)) >= 0) & (dot(n, cross(ca[None], cp)) >= 0) & (nn > 0)
    h = dot(n, ap)
    pl = (h * h) * (1.0 / nn)
    pl = torch.where(inside & (pl < float("inf")), pl, torch.full((), float("inf"), device=x.device))
    d2 = torch.minimum(torch.minimum(s1, s2), torch.minimum(s3, pl))
    best = torch.where(d2.isnan(), torch.full((), float("inf"), device=x.device), d2).min(1)[0]
    wins = (d2 == best[:, None]).to(torch.uint8)
    return best, torch.where(wins.any(1), wins.argmax(1), torch.full((), -1, device=x.device)).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=480)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--torch-queries", type=int, default=1024)
    ap.add_argument("--torch-faces", type=int, default=8192)
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    model = gs.scene_model(dev)
    common = ["--res", str(opt.res), "--iso-level", "32", "--limit", "1.2", "--simplify-cell", "4"]
    out = {"res": opt.res, "scene": "synthetic.make_scene_weights (8x256)", "iso_level": 32, "limit": 1.2, "reps": opt.reps,
           "device": torch.cuda.get_device_name(0), "roof_flops": ROOF_FLOPS, "flops_per_pair": FLOPS_PER_PAIR, "queries": opt.queries}

    def save():
        print(json.dumps(out), flush=True)
        gs.write_json(out, opt.out)

    with torch.no_grad():
        args = mesh_nerf.build_parser().parse_args(common)
        with gs.quiet():
            v, f, n, _ = mesh_nerf.extract_geometry(model, dev, args)
            f = f.to(torch.int32)
            sv, sf, _ = mesh_nerf.simplify_mesh(v, f, n, 4.0, args)
        sf = sf.to(torch.int32)
        gen = torch.Generator(device=dev)
        gen.manual_seed(0)
        jittered = v + 0.002 * torch.randn(v.shape, device=dev, generator=gen)
        x = hip_ops.mesh_sample_points(jittered, f, n=opt.queries, generator=gen)[0]
        y = hip_ops.mesh_sample_points(v, f, n=opt.queries, generator=gen)[0]
        out["points_to_mesh"] = {}
        for tag, (mv, mf) in (("dense", (v, f)), ("simplify_cell_4", (sv, sf))):
            nf = int(mf.shape[0])
            whole = gs.gpu_ms(raw_call(x, mv, mf), opt.reps)
            few = gs.gpu_ms(raw_call(x[:64].contiguous(), mv, mf), opt.reps)
            pairs = float(opt.queries) * nf / ((whole - few) * 1e-3)
            out["points_to_mesh"][tag] = {
                "vertices": int(mv.shape[0]), "faces": nf, "entry_ms": whole, "prepass_and_64_queries_ms": few, "hot_kernel_ms": whole - few,
                "pairs_per_s": pairs, "fraction_of_valu_roof": pairs * FLOPS_PER_PAIR / ROOF_FLOPS,
                "wrapper_ms": gs.gpu_ms(lambda: hip_ops.points_to_mesh(x, mv, mf, return_normals=True), opt.reps)}
            save()
        ms = gs.gpu_ms(lambda: hip_ops.points_nearest(x, y), opt.reps)
        out["points_nearest"] = {"n": opt.queries, "m": opt.queries, "ms": ms, "pairs_per_s": float(opt.queries) ** 2 / (ms * 1e-3)}
        save()
        tq, tf = x[:opt.torch_queries].contiguous(), f[:opt.torch_faces].contiguous()
        got, want = hip_ops.points_to_mesh(tq, v, tf), torch_contract(tq, v, tf)
        out["torch"] = {"queries": int(tq.shape[0]), "faces": int(tf.shape[0]),
                        "equal_dist2": float((got[0] == want[0]).float().mean()), "equal_face": float((got[1] == want[1]).float().mean()),
                        "max_abs_dist2_difference": float((got[0] - want[0]).abs().max()),
                        "torch_ms": gs.gpu_ms(lambda: torch_contract(tq, v, tf), 3, warm=1),
                        "kernel_ms": gs.gpu_ms(raw_call(tq, v, tf), opt.reps)}
        out["torch"]["torch_over_kernel"] = out["torch"]["torch_ms"] / out["torch"]["kernel_ms"]
        save()
        out["reports"] = {}
        for tag, (mv, mf) in (("dense_against_itself", (v, f)), ("simplify_cell_4_against_dense", (sv, sf))):
            row = {}
            for surface in mesh_chamfer.SURFACES:
                rep = mesh_chamfer.compare_meshes(mv, mf, v, f, samples=opt.queries, seed=0, device=dev, surface=surface,
                                                  fscore=(0.0025, 0.005) if surface == "exact" else ())
                row[surface] = {k: rep[k] for k in rep if k not in ("mesh", "target")}
                row[surface + "_wall_ms"] = gs.wall_ms(lambda: mesh_chamfer.compare_meshes(mv, mf, v, f, samples=opt.queries, seed=0,
                                                                                             device=dev, surface=surface), 3)
            out["reports"][tag] = row
            save()


if __name__ == "__main__":
    main()
