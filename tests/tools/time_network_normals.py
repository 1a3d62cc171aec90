"""Network normals (mesh_nerf --normals network) at --res 480 on the synthetic scene, plain and with --super-sampling: vertices,
the normals stage (HipMLP.density_gradient at the final vertices + the fp32 normalisation) under HIP events, its executed FLOP
and fraction of the fp32 MFMA peak, and the geometry stage (extract_geometry*) of the same run.

    python tests/tools/time_network_normals.py [--res 480] [--ss 0 2] [--reps 5] [--out FILE.json]
    python tests/tools/time_network_normals.py --stage-only [--ss 2]      # only the normals stage, for a rocprofv3 --kernel-trace run
"""
import argparse
import functools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchlib.common import FP32_MFMA_PEAK_TFLOPS  # noqa: E402
from nerfmeshes_amd import _lib, mesh_nerf  # noqa: E402
from tests import gpu_support as gs  # noqa: E402


def executed_flop_per_point(net):
    """the matrix work nm_mlp_density_grad runs per point: the full taping forward (trunk + view branch), the delta chain
    (layers_xyz[L-2 .. 1] -- or .. 0 when the chain does not stop at layers_xyz[0] -- fc_feat, layers_dir[0], the heads) and the
    contraction of the encoding's deltas (one block per skip layer plus layer1's)"""
    d = net.desc
    H, L = int(d["hidden_size"]), int(d["num_layers"])
    dx = 6 * int(d["num_encoding_fn_xyz"]) + 3
    stop = bool(_lib.load().nm_mlp_backward_stops_at_xyz0(net.handle))
    skips = sum(1 for i in range(L - 1) if i % int(d["skip_step"]) == 0 and i > 0 and i != L - 1)
    macs = (L - 2 if stop else L - 1) * H * H + H          # layers_xyz^T (hidden columns), fc_alpha^T
    if d.get("use_viewdirs", True):
        macs += H * H + (H // 2) * H + 3 * (H // 2)        # fc_feat^T, layers_dir[0]^T (hidden columns), fc_rgb^T
    macs += (1 + skips) * H * dx
    return net.flops_per_sample(density_only=False) + 2 * macs


gpu_ms = functools.partial(gs.gpu_ms, warm=1)                     # one warm-up call, as these figures were taken


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=480)
    ap.add_argument("--ss", type=int, nargs="+", default=[0, 2])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stage-only", action="store_true")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    model = gs.scene_model(dev)
    net = model.get_model().hip("f32")
    flop = executed_flop_per_point(net)
    out = {"res": opt.res, "scene": "synthetic.make_scene_weights (8x256)", "iso_level": 32, "limit": 1.2, "reps": opt.reps,
           "peak_tflops": FP32_MFMA_PEAK_TFLOPS, "device": torch.cuda.get_device_name(0), "kernel_variant": net.kernel_variant()[0],
           "stops_at_xyz0": bool(_lib.load().nm_mlp_backward_stops_at_xyz0(net.handle)), "executed_flop_per_point": flop,
           "per_ss": []}
    with torch.no_grad():
        for ss in opt.ss:
            args = mesh_nerf.build_parser().parse_args(["--res", str(opt.res), "--iso-level", "32", "--limit", "1.2",
                                                        "--super-sampling", str(ss)])
            geometry = mesh_nerf.extract_geometry_with_super_sampling if ss >= 1 else mesh_nerf.extract_geometry
            with gs.quiet():
                v, f, n, _ = geometry(model, dev, args)
            stage = lambda: mesh_nerf.network_normals(net, v, n)      # noqa: E731
            if opt.stage_only:
                for _ in range(opt.reps):
                    stage()
                torch.cuda.synchronize()
                continue
            row = {"ss": ss, "vertices": int(v.shape[0]), "faces": int(f.shape[0])}
            row["normals_ms"] = gpu_ms(stage, opt.reps)
            row["density_gradient_ms"] = gpu_ms(lambda: net.density_gradient(v), opt.reps)
            nn, kept = stage()
            row["kept_grid_normal"] = int(kept.sum())
            row["mean_cos_to_grid_normal"] = float((nn * n).sum(1).mean())
            row["tflops"] = row["vertices"] * flop / (row["density_gradient_ms"] * 1e-3) / 1e12
            row["frac_of_peak"] = row["tflops"] / FP32_MFMA_PEAK_TFLOPS
            with gs.quiet():
                row["geometry_ms"] = gs.wall_ms(lambda: geometry(model, dev, args), max(1, opt.reps // 2))
            row["normals_over_geometry"] = row["normals_ms"] / row["geometry_ms"]
            out["per_ss"].append(row)
            print(json.dumps(row), flush=True)
    if opt.stage_only:
        return
    text = json.dumps(out, indent=1)
    print(text)
    gs.write_json(out, opt.out)


if __name__ == "__main__":
    main()
