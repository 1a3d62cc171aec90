"""Ray-marched surface point cloud with the reference's function names (the reference's src/mesh_surface_ray.py:46-154):
orbit views -> rendered depth -> surface point of every ray -> neighbourhood vote -> oriented, coloured points -> PLY, all
on the MI355X.

    python -m nerfmeshes_amd.mesh_surface_ray --log-checkpoint <logdir>/<exp>/<run>/version_N

The reference script is dead code (it imports symbols that no longer exist and `plyfile`); this is what it set out to do.
Its constants are options with its values as defaults.  Every view is rendered by `NeRFModel.query_view` (rays generated in
the kernels), filtered and compacted by two HIP kernels (hip_ops.surface_filter / surface_gather: the 25 clamped gathers,
the compare / reduce chains and the boolean-mask indexing of mesh_surface_ray.py:115-141 in one pass, in row-major pixel
order), and only the kept rows leave the device.

A caveat that the default reproduces faithfully: the reference keeps a pixel only if `depth > 0`, and in eval mode the
renderer zeroes the depth of every ray with acc_map < 1.0 (modules.py:108-109).  An opaque ray has acc = 1 in exact
arithmetic and lands on either side of 1.0 by fp32 rounding, so WHICH opaque rays survive is decided by the summation order
of the renderer ("Surface point cloud": on the test scene no kept pixel is stable against a 1e-5 change of acc).
`--min-opacity T` (addition) is the well-conditioned rule: the depth is left as composited and a ray counts when
acc_map >= T.
"""
import argparse
import os

import numpy as np
import torch

from . import hip_ops, models
from .lightning_modules import PathParser
from .synthetic import pose_spherical


def get_grid(size):
    """mesh_surface_ray.py:61-65: the (size^2, 2) (row, column) index pairs of a square image, row-major."""
    x = torch.arange(size)
    a, b = torch.meshgrid(x, x, indexing="ij")
    return torch.stack([a.flatten(), b.flatten()], dim=-1)


def color_bytes(diffuse):
    """fp32 colours -> uint8 by the rule of hip_ops.surface_gather on the host: trunc(clamp(rgb * 255, 0, 255)), NaN -> 0."""
    c = np.asarray(diffuse, dtype=np.float32) * np.float32(255)
    return np.nan_to_num(np.clip(c, 0, 255), nan=0.0).astype(np.uint8)


def export_ply(vertices, diffuse, normals, filename, binary=False):
    """mesh_surface_ray.py:46-58 with its argument order: x y z nx ny nz (float) and red green blue (uchar) per vertex, ascii
    as the reference's `text = True` (or binary_little_endian).  `diffuse` is uint8, or fp32 in [0, 1] that `color_bytes`
    converts.  Written by the native library (nm_export_ply); `plyfile` is not needed."""
    d = diffuse.detach().cpu().numpy() if isinstance(diffuse, torch.Tensor) else np.asarray(diffuse)
    if d.dtype != np.uint8:
        d = color_bytes(d)
    hip_ops.export_ply(vertices, normals, d, filename, binary=binary)


def render_poses(args):
    """mesh_surface_ray.py:82-88: pose_spherical(angleY, angleX, radius), angleY outer, angleX inner."""
    return [pose_spherical(angle_y, angle_x, args.radius)
            for angle_y in np.linspace(-180, 180, args.views_y, endpoint=False)
            for angle_x in np.linspace(-90, 90, args.views_x, endpoint=True)]


def filter_view(model, pose, args, cfg):
    """One pose -> (filter state, rendered bundle): render, then the vote (mesh_surface_ray.py:97-136)."""
    size = int(args.img_size)
    focal = float(args.focal)
    bounds = torch.tensor([cfg.dataset.near, cfg.dataset.far], dtype=torch.float32)
    conditioned = args.min_opacity is not None
    out = model.query_view(torch.from_numpy(np.ascontiguousarray(pose)), size, size, focal, bounds, keep_depth=conditioned)
    view = hip_ops.make_view(pose, size, size, focal, ndc_near=1.0 if cfg.dataset.use_ndc else None)
    origins, dirs = hip_ops.view_rays(view, device=out.depth_map.device)
    if not cfg.dataset.use_ndc:
        origins = origins[:1]                     # one camera centre for the whole view
    flt = hip_ops.surface_filter(origins, dirs, out.depth_map, size, size, step=args.step_size,
                                 dist_threshold=args.dist_threshold,
                                 min_votes=hip_ops.surface_min_votes(args.step_size, args.prob_threshold),
                                 opacity=out.acc_map if conditioned else None,
                                 min_opacity=args.min_opacity if conditioned else None)
    return flt, out


def export_ray_trace(model, args, cfg, device):
    """mesh_surface_ray.py:68-154 -> (vertices (N,3) f32, normals (N,3) f32, diffuse (N,3) f32, diffuse (N,3) uint8) as numpy
    arrays, the views in pose order and the pixels of a view in row-major order; rank 0 writes the PLY.  Under
    torch.distributed (one process per GPU) the VIEWS are split over the ranks (dist.split_range), every rank filters its own
    views and one ragged all-gather assembles the rows in view order: the file is the single-rank file byte for byte."""
    from . import dist as nd
    from .mesh_nerf import network_normals
    if not (hasattr(model, "query_view") and model.can_query_view()):
        raise RuntimeError("mesh_surface_ray needs a model with the deterministic in-kernel view render (NeRFModel.query_view "
                           "in eval mode, no perturb / noise): there is no fallback")
    if not 0 <= int(args.step_size) <= hip_ops.SURFACE_STEP_MAX:
        raise ValueError(f"--step-size must be in [0, {hip_ops.SURFACE_STEP_MAX}], got {args.step_size}")
    rank, world = nd.world()
    poses = render_poses(args)
    lo, hi = nd.split_range(len(poses), rank, world)
    normals_mode = getattr(args, "normals", "ray")
    precision = getattr(args, "precision", "f32")
    if precision != "f32":
        model.set_precision(precision)
    rows = []
    try:
        for pose in poses[lo:hi]:
            flt, out = filter_view(model, pose, args, cfg)
            rows.append(hip_ops.surface_gather(flt, out.rgb_map))       # reads the view's count: one D2H copy per view
    finally:
        if precision != "f32":
            model.set_precision("f32")
    dev = torch.device(device)
    if rows:
        points, normals, colors, colors_u8 = (torch.cat(col, dim=0) for col in zip(*rows))
    else:                                                                  # more ranks than views
        points, normals, colors = (torch.empty(0, 3, dtype=torch.float32, device=dev) for _ in range(3))
        colors_u8 = torch.empty(0, 3, dtype=torch.uint8, device=dev)
    if normals_mode == "network":
        # the fp32 handle whatever --precision is; a zero or non-finite gradient keeps the ray normal
        normals, kept = network_normals(model.get_model().hip("f32"), points, normals)
        print(f"Network normals: {int(kept.sum())} of {points.shape[0]} points kept their ray normal")
    # one collective: the 36 bytes of the three fp32 triples and the 3 colour bytes of every row travel together
    packed = torch.cat((torch.cat((points, normals, colors), dim=1).contiguous().view(torch.uint8).view(-1, 36), colors_u8), dim=1)
    packed = nd.all_gather_ragged(packed.contiguous()).cpu()
    floats = packed[:, :36].contiguous().view(torch.float32).view(-1, 9).numpy()
    vertices, normals_np, diffuse = (np.ascontiguousarray(floats[:, 3 * k:3 * k + 3]) for k in range(3))
    diffuse_u8 = np.ascontiguousarray(packed[:, 36:].numpy())
    if rank == 0:
        path = os.path.join(args.save_dir, args.ply_name)
        export_ply(vertices, diffuse_u8, normals_np, path, binary=getattr(args, "ply_format", "ascii") == "binary")
        print(f"Finished writing to {path} with {len(vertices)} points from {len(poses)} views")
    return vertices, normals_np, diffuse, diffuse_u8


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--log-checkpoint", type=str, default=None)
    p.add_argument("--checkpoint", type=str, default="model_last.ckpt")
    p.add_argument("--save-dir", type=str, default=".")
    p.add_argument("--ply-name", type=str, default="lego-sampling.ply")
    # the reference's constants (mesh_surface_ray.py:71-78,90) as options with its values
    p.add_argument("--views-y", type=int, default=8, help="orbit angles around the vertical axis, linspace(-180, 180, N, endpoint=False)")
    p.add_argument("--views-x", type=int, default=4, help="elevation angles, linspace(-90, 90, N)")
    p.add_argument("--radius", type=float, default=4.0)
    p.add_argument("--img-size", type=int, default=800)
    p.add_argument("--focal", type=float, default=1111.1111)
    p.add_argument("--step-size", type=int, default=2, help="half width of the voting window: (2 step + 1)^2 neighbours")
    p.add_argument("--dist-threshold", type=float, default=0.002, help="SQUARED distance below which a neighbour's surface point votes")
    p.add_argument("--prob-threshold", type=float, default=0.6, help="share of the window's neighbours that must vote")
    p.add_argument("--min-opacity", type=float, default=None,
                   help="(addition) keep a ray when acc_map >= T, with the depth left as composited.  Default: the reference's "
                        "rule, depth > 0 after the eval-mode renderer zeroed the depth of every ray with acc_map < 1.0 -- which "
                        "opaque rays pass that test is decided by fp32 rounding of acc_map around 1.0, i.e. by the summation "
                        "order of the renderer; 0.99 is a well-conditioned choice")
    p.add_argument("--ply-format", choices=("ascii", "binary"), default="ascii",
                   help="(addition) ascii (default, as the reference's text = True) or binary_little_endian")
    p.add_argument("--normals", choices=("ray", "network"), default="ray",
                   help="(addition) ray (default): -direction of the ray, as the reference; network: -grad sigma / |grad sigma| of "
                        "the network at the points (a zero or non-finite gradient keeps the ray normal)")
    p.add_argument("--precision", choices=("f32", "bf16x3"), default="f32", help="(addition) arithmetic of the view render")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    path_parser = PathParser()
    cfg, _ = path_parser.parse(None, args.log_checkpoint, None, args.checkpoint)
    if not torch.cuda.is_available():
        raise SystemExit("mesh_surface_ray needs a MI355X: the HIP path has no CPU fallback")
    from . import dist as nd
    rank, world, device = nd.init_from_env()          # one process per GPU under torch.distributed.run
    print(f"Loading model from {path_parser.checkpoint_path}")
    model = getattr(models, cfg.experiment.model).load_from_checkpoint(path_parser.checkpoint_path)
    model = model.eval().to(device)
    try:
        with torch.no_grad():
            return export_ray_trace(model, args, cfg, device)
    finally:
        nd.shutdown()


if __name__ == "__main__":
    main()
