"""Draw a coloured mesh on the MI355X and score it in image space (addition: the reference cannot draw a mesh).

    python -m nerfmeshes_amd.mesh_render --mesh mesh.obj --log-checkpoint <run>/version_N                  # the config's test split
    python -m nerfmeshes_amd.mesh_render --mesh mesh.obj --log-checkpoint <run>/version_N --views 8 --compare-nerf
    python -m nerfmeshes_amd.mesh_render --mesh any.obj --views 16 --save-images --save-dir turntable     # no checkpoint: images

A deterministic software rasteriser (hip_ops.mesh_rasterize: exact integer coverage, a 64-bit minimum per pixel; the rule is in
include/nerfmeshes_hip.h) finds the face every pixel sees, hip_ops.mesh_interpolate blends the per-vertex colours of the OBJ
that `mesh_nerf` wrote -- or, for an OBJ with a texture (`mesh_nerf --texture-res`, or any other: `--appearance`),
hip_ops.mesh_texture_lookup fetches the image at the interpolated texture coordinates.  The pixel grid is get_ray_bundle's, so pixel (j, i) of the mesh image and of the network's render look
along the same ray.  The rasteriser's depth is measured along the camera's axis; the network's depth_map along the unit ray:
`ray_lengths` converts.  With a dataset the PSNR uses eval_nerf's bookkeeping (chunks of cfg.nerf.validation.chunksize, the
float batch count), so it compares with the PSNR eval_nerf prints for the network.  `--compare-nerf` renders every pose with
the network too (query_view, keep_depth) and reports the mesh against it.  `--ssim` scores the same image pairs with the
structural similarity too (hip_ops.image_ssim), `--save-ssim-maps` writes its per-pixel map.  Under torch.distributed.run the views are dealt
round-robin to the ranks and the per-view rows gathered; the report does not depend on the number of ranks."""
import argparse
import json
import os

import numpy as np
import torch

from . import hip_ops, models, synthetic
from .lightning_modules import PathParser

ROW = ("psnr_target", "psnr_nerf", "depth_mean", "depth_median", "depth_pixels", "iou") + hip_ops.RASTER_COUNTS
NAN = float("nan")


def ray_lengths(height, width, focal, device):
    """|(x, y, -1)| of get_ray_bundle's camera-space ray per pixel (H,W): depth along the camera's axis times this is the
    distance along the unit ray that the network's depth_map measures"""
    i = (torch.arange(width, dtype=torch.float64, device=device) - width * 0.5) / focal
    j = -(torch.arange(height, dtype=torch.float64, device=device) - height * 0.5) / focal
    return torch.sqrt(i[None, :] ** 2 + j[:, None] ** 2 + 1.0).to(torch.float32)


def device_texture(texture, device):
    """(face_uv (F,3,2), image (Ht,Wt,3) uint8) -> both on the device, as hip_ops.mesh_texture_lookup takes them"""
    face_uv, image = texture
    return (torch.as_tensor(face_uv, dtype=torch.float32).to(device).contiguous(),
            torch.as_tensor(image, dtype=torch.uint8).to(device).contiguous())


def render_mesh(verts, faces, colors, pose, height, width, focal, near, background, normals=None, cull_back=False, texture=None,
                vertex_too=False):
    """One view of a coloured mesh -> dict(rgb (H,W,3), depth (H,W): along the camera's axis, 0 where nothing was drawn,
    mask (H,W) bool, face_id (H,W) int32, counts: the rasteriser's; normals (H,W,3): interpolated, not normalised, zero in
    the background -- only when `normals` came).  verts (V,3), faces (F,3), colors (V,3) on the GPU (host arrays are copied);
    background: three floats.  texture = (face_uv (F,3,2), image (Ht,Wt,3) uint8): rgb is the bilinear fetch of the image at
    the interpolated coordinates (hip_ops.mesh_texture_lookup) instead of the blend of `colors`, which vertex_too adds as
    rgb_vertex from the same rasterisation."""
    verts, faces, _, _ = hip_ops._mesh_arrays(verts, faces, "render_mesh")
    view = hip_ops.make_view(pose, height, width, focal)
    raster = hip_ops.mesh_rasterize(verts, faces, view, near, cull_back=cull_back)
    colors = torch.as_tensor(colors, dtype=torch.float32).to(verts.device)
    if texture is None:
        rgb = hip_ops.mesh_interpolate(raster, faces, colors, background)
    else:
        face_uv, image = device_texture(texture, verts.device)
        if face_uv.shape[0] != faces.shape[0]:
            raise ValueError(f"render_mesh: texture coordinates of {face_uv.shape[0]} faces for a mesh of {faces.shape[0]}")
        rgb = hip_ops.mesh_texture_lookup(raster, face_uv, image, background)
    out = dict(rgb=rgb, depth=raster[1], mask=raster[0] >= 0, face_id=raster[0], counts=raster[3])
    if texture is not None and vertex_too:
        out["rgb_vertex"] = hip_ops.mesh_interpolate(raster, faces, colors, background)
    if normals is not None:
        out["normals"] = hip_ops.mesh_interpolate(raster, faces, torch.as_tensor(normals, dtype=torch.float32).to(verts.device),
                                                  (0.0, 0.0, 0.0))
    return out


def chunked_mse(rgb, targets, chunksize):
    """eval_nerf's per-image loss: the sum of the chunks' MSEs over the FLOAT batch count (eval_nerf.py:57)"""
    loss = 0
    for s in range(0, rgb.shape[0], chunksize):
        loss = loss + torch.nn.functional.mse_loss(rgb[s:s + chunksize], targets[s:s + chunksize])
    return loss / (rgb.shape[0] / chunksize)


def psnr(mse):
    mse = float(mse)
    return float("inf") if mse == 0.0 else -10.0 * float(np.log10(mse))


def compare_with_nerf(model, out, pose, height, width, focal, bounds, chunksize):
    """the mesh image against the network's own render of the pose -> (psnr, mean |depth difference|, median, pixels, iou,
    the network's bundle)"""
    pixels = height * width
    parts = [model.query_view(pose, height, width, focal, bounds, first=s, count=min(chunksize, pixels - s), keep_depth=True)
             for s in range(0, pixels, chunksize)]
    rgb = torch.cat([p.rgb_map for p in parts], 0)
    depth = torch.cat([p.depth_map for p in parts], 0).view(height, width)
    acc = torch.cat([p.acc_map for p in parts], 0).view(height, width)
    value = psnr(torch.nn.functional.mse_loss(out["rgb"].reshape(-1, 3), rgb))       # two renders of one pose: the plain MSE
    mask = out["mask"]
    both = mask & (acc >= 0.99)
    diff = (out["depth"] * ray_lengths(height, width, focal, depth.device) - depth).abs()[both]
    solid = acc >= 0.5
    union = int((mask | solid).sum())
    iou = float((mask & solid).sum()) / union if union else 1.0
    mean, median = (float(diff.double().mean()), float(diff.median())) if diff.numel() else (NAN, NAN)
    return value, mean, median, int(diff.numel()), iou, rgb, depth


def _imwrite(path, image):
    from .eval_nerf import _imwrite as write
    write(path, image)


def read_image(path):
    """an image file -> (H,W,3) uint8 on the host, row 0 on top"""
    from PIL import Image
    with Image.open(path) as im:
        return torch.from_numpy(np.array(im.convert("RGB"), dtype=np.uint8))


def _to_u8(rgb):
    return (rgb.clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8).cpu().numpy()


VERTEX_ROW = ("psnr_target_vertex", "psnr_nerf_vertex")
SSIM_ROW = ("ssim_target", "ssim_nerf")                          # only with ssim=True (--ssim, mesh_nerf --render-ssim)
SSIM_VERTEX_ROW = ("ssim_target_vertex", "ssim_nerf_vertex")     # ... and vertex_too


def ssim_gray_u8(ssim_map):
    """(H-10,W-10,C) fp64 S -> (H-10,W-10) uint8: the channel mean clamped to [0,1] as 8-bit grey (a NaN is black)"""
    grey = torch.nan_to_num(ssim_map.mean(dim=-1), nan=0.0).clamp(0.0, 1.0)
    return (grey * 255.0 + 0.5).to(torch.uint8).cpu().numpy()


def evaluate(verts, faces, colors, views, near, background, model=None, bounds=None, chunksize=None, compare_nerf=False,
             cull_back=False, save_dir=None, save_images=False, save_depth=False, device="cuda", texture=None, vertex_too=False,
             ssim=False, save_ssim_maps=False):
    """The report over an iterable of views `(pose, height, width, focal, targets | None)`: rank r draws views r, r + world,
    ...; the rows are gathered, so every rank returns the single-rank report.  targets: (H*W, 3) on any device.
    texture = (face_uv, image): the mesh is drawn with it (render_mesh) and every number describes the textured mesh;
    vertex_too then adds VERTEX_ROW -- the PSNR of the per-vertex colours from the same rasterisation against the same target and
    the same network render -- to every view and to the means.
    ssim adds SSIM_ROW (hip_ops.image_ssim of the mesh image against the target and, with compare_nerf, against the network's
    render; with vertex_too SSIM_VERTEX_ROW as well) to every view and to the means: the views must be at least 11 x 11.
    save_ssim_maps writes mesh_ssim/NNNN.png, the map against the target -- against the network's render for a view without
    one --, (H-10, W-10) in 8-bit grey.  Without ssim the columns do not exist."""
    from . import dist as nd
    rank, world = nd.world()
    verts, faces, _, _ = hip_ops._mesh_arrays(verts, faces, "mesh_render")
    colors = torch.as_tensor(colors, dtype=torch.float32).to(verts.device)
    if texture is not None:
        texture = device_texture(texture, verts.device)
    vertex_too = bool(vertex_too and texture is not None)
    ssim = bool(ssim or save_ssim_maps)
    columns = ROW + (VERTEX_ROW if vertex_too else ()) + ((SSIM_ROW + (SSIM_VERTEX_ROW if vertex_too else ())) if ssim else ())
    want_map = bool(save_dir and save_ssim_maps)
    rows, total = [], 0
    for nr, (pose, height, width, focal, targets) in enumerate(views):
        total += 1
        if nr % world != rank:
            continue
        out = render_mesh(verts, faces, colors, pose, height, width, focal, near, background, cull_back=cull_back, texture=texture,
                          vertex_too=vertex_too)
        chunk = chunksize or height * width
        row = dict.fromkeys(columns, NAN)
        row.update({k: float(v) for k, v in out["counts"].items()})
        if targets is not None:
            row["psnr_target"] = psnr(chunked_mse(out["rgb"].reshape(-1, 3), targets.to(verts.device).reshape(-1, 3), chunk))
        if compare_nerf:
            row["psnr_nerf"], row["depth_mean"], row["depth_median"], row["depth_pixels"], row["iou"], net_rgb, _ = compare_with_nerf(
                model, out, pose, height, width, focal, bounds, chunk)
            if vertex_too:
                row["psnr_nerf_vertex"] = psnr(torch.nn.functional.mse_loss(out["rgb_vertex"].reshape(-1, 3), net_rgb))
        if vertex_too and targets is not None:
            row["psnr_target_vertex"] = psnr(chunked_mse(out["rgb_vertex"].reshape(-1, 3), targets.to(verts.device).reshape(-1, 3), chunk))
        if ssim:
            image, ssim_map = out["rgb"].reshape(height, width, 3), None
            shots = ([("target", targets.to(verts.device).reshape(height, width, 3))] if targets is not None else []) + (
                [("nerf", net_rgb.reshape(height, width, 3))] if compare_nerf else [])
            for nr_shot, (name, other) in enumerate(shots):
                got = hip_ops.image_ssim(image, other, want_map=want_map and nr_shot == 0)
                row[f"ssim_{name}"] = got["ssim"]
                ssim_map = got["map"] if nr_shot == 0 else ssim_map
                if vertex_too:
                    row[f"ssim_{name}_vertex"] = hip_ops.image_ssim(out["rgb_vertex"].reshape(height, width, 3), other)["ssim"]
            if ssim_map is not None:
                os.makedirs(os.path.join(save_dir, "mesh_ssim"), exist_ok=True)
                _imwrite(os.path.join(save_dir, "mesh_ssim", f"{nr:04d}.png"), ssim_gray_u8(ssim_map))
        rows.append([row[k] for k in columns])
        if save_dir and save_images:
            os.makedirs(os.path.join(save_dir, "mesh_images"), exist_ok=True)
            _imwrite(os.path.join(save_dir, "mesh_images", f"{nr:04d}.png"), _to_u8(out["rgb"]))
        if save_dir and save_depth:
            os.makedirs(os.path.join(save_dir, "mesh_depth"), exist_ok=True)
            far = out["depth"].max().clamp_min(1e-12)
            shade = torch.where(out["mask"], 1.0 - out["depth"] / far, torch.zeros_like(out["depth"]))
            _imwrite(os.path.join(save_dir, "mesh_depth", f"{nr:04d}.png"), _to_u8(shade))
    mine = torch.tensor(rows, dtype=torch.float64, device=verts.device).reshape(-1, len(columns))
    if world > 1:
        counts = nd.round_robin_counts(total, world)
        flat = nd.all_gather_rows(mine, counts)
        starts = [sum(counts[:r]) for r in range(world)]
        mine = torch.stack([flat[starts[i % world] + i // world] for i in range(total)]) if total else flat
    return build_report(mine.cpu().numpy(), near, columns)


def build_report(table, near, columns=ROW):
    """per-view rows (views, len(columns)) fp64 -> the report: per-view dicts, means over the views that have the number, the
    reject counts summed"""
    integer = set(hip_ops.RASTER_COUNTS) | {"depth_pixels"}
    views = []
    for r in table:
        views.append({k: (int(v) if k in integer and not np.isnan(v) else (None if np.isnan(v) else float(v))) for k, v in zip(columns, r)})
    mean = {}
    for k in ("psnr_target", "psnr_nerf", "depth_mean", "depth_median", "iou") + tuple(
            k for k in VERTEX_ROW + SSIM_ROW + SSIM_VERTEX_ROW if k in columns):
        have = [v[k] for v in views if v[k] is not None]
        mean[k] = float(np.mean(have)) if have else None
    mse = [10.0 ** (-v["psnr_target"] / 10.0) for v in views if v["psnr_target"] is not None]
    if mse:                                                          # eval_nerf's dataset PSNR: of the mean loss
        mean["psnr_target_of_mean_mse"] = psnr(np.mean(mse))
    totals = {k: int(sum(v[k] for v in views)) for k in hip_ops.RASTER_COUNTS}
    return dict(near=float(near), views=views, mean=mean, counts=totals)


def format_report(report):
    lines = []
    for nr, v in enumerate(report["views"]):
        parts = [f"[MESH] View {nr}: covered {v['covered']} px, {v['drawn']} faces drawn"]
        if v["psnr_target"] is not None:
            parts.append(f"PSNR to the target {v['psnr_target']:.4f}")
        if v["psnr_nerf"] is not None:
            parts.append(f"PSNR to the network {v['psnr_nerf']:.4f}, |depth difference| mean "
                         f"{v['depth_mean'] if v['depth_mean'] is not None else NAN:.6f} median "
                         f"{v['depth_median'] if v['depth_median'] is not None else NAN:.6f} over {v['depth_pixels']} px, "
                         f"IoU {v['iou']:.4f}")
        if v.get("psnr_nerf_vertex") is not None:
            parts.append(f"per-vertex colours: PSNR to the network {v['psnr_nerf_vertex']:.4f}")
        have = [(what, v.get(key)) for what, key in (("the target", "ssim_target"), ("the network", "ssim_nerf"),
                                                     ("the target, per-vertex colours", "ssim_target_vertex"),
                                                     ("the network, per-vertex colours", "ssim_nerf_vertex"))]
        if any(value is not None for _, value in have):
            parts.append("SSIM to " + ", to ".join(f"{what} {value:.6f}" for what, value in have if value is not None))
        lines.append(", ".join(parts))
    mean = ", ".join(f"{k} {v:.6f}" for k, v in report["mean"].items() if v is not None)
    lines.append(f"Mesh render: {len(report['views'])} views" + (f", mean {mean}" if mean else ""))
    c = report["counts"]
    lines.append("Mesh render: faces rejected over all views: " + ", ".join(
        f"{k} {c[k]}" for k in hip_ops.RASTER_COUNTS[1:8]) + f" (near plane {report['near']:g}: no clipping)")
    return lines


def write_report(report, path):
    with open(path, "w") as fh:
        json.dump(report, fh, indent=1, sort_keys=True)
        fh.write("\n")


def orbit_views(count, height, width, focal, radius=4.0, phi=-30.0):
    for pose in synthetic.orbit_poses(count, phi=phi, radius=radius):
        yield pose, height, width, focal, None


def sphere_poses(count, centre, radius):
    """(count, 3, 4) fp32 camera-to-world matrices on a Fibonacci lattice of the sphere (centre, radius), every camera looking
    at the centre: z_k = 1 - (2k + 1) / count, a_k = k pi (3 - sqrt 5), d_k = (sqrt(1 - z^2) cos a, sqrt(1 - z^2) sin a, z); the
    eye is centre + radius d_k, the camera's backward axis d_k, right = unit(up x d_k), up' = d_k x right with up = (0, 0, 1),
    or (0, 1, 0) when |z_k| > 0.999.  fp64 on the host, cast to fp32 once."""
    centre = np.asarray(centre, np.float64).reshape(3)
    poses = np.zeros((int(count), 3, 4), np.float64)
    for k in range(int(count)):
        z = 1.0 - (2 * k + 1) / np.float64(count)
        a = k * (np.pi * (3.0 - np.sqrt(5.0)))
        s = np.sqrt(1.0 - z * z)
        d = np.array([s * np.cos(a), s * np.sin(a), z], np.float64)
        up = np.array([0.0, 1.0, 0.0] if abs(z) > 0.999 else [0.0, 0.0, 1.0], np.float64)
        right = np.cross(up, d)
        right /= np.sqrt((right * right).sum())
        poses[k, :, 0], poses[k, :, 1], poses[k, :, 2] = right, np.cross(d, right), d
        poses[k, :, 3] = centre + np.float64(radius) * d
    return poses.astype(np.float32)


def sphere_views(count, centre, radius, size, focal):
    """`count` square views of side `size` from all around (sphere_poses), in `orbit_views`' form"""
    for pose in sphere_poses(count, centre, radius):
        yield pose, size, size, focal, None


def frame_views(verts, cull_radius, size):
    """The framing of sphere_views for a mesh, done once: with lo and hi the fp32 extremes of the vertices, centre = (lo + hi) /
    2 in fp64, rb = half the box diagonal, radius = cull_radius rb, focal = 0.5 size sqrt(radius^2 - rb^2) / rb 0.95 and near =
    (float)((radius - rb) / 2): the bounding sphere fills 95 % of the image and no face can fail the near test.
    -> (centre (3,) fp64, radius, focal, near).  ValueError for no vertex, a vertex that is not finite, or a box without extent."""
    verts = torch.as_tensor(verts)
    if not 1.0 < float(cull_radius) < float("inf"):
        raise ValueError(f"frame_views: the radius must be finite and > 1 bounding radii, got {cull_radius}")
    if verts.shape[0] == 0:
        raise ValueError("frame_views: no vertex to frame")
    lo = verts.to(torch.float32).min(dim=0).values.cpu().numpy().astype(np.float64)
    hi = verts.to(torch.float32).max(dim=0).values.cpu().numpy().astype(np.float64)
    rb = 0.5 * np.sqrt(((hi - lo) ** 2).sum())
    if not (np.isfinite(rb) and rb > 0):
        raise ValueError(f"frame_views: the vertices' box [{lo}, {hi}] is not finite or has no extent")
    radius = np.float64(cull_radius) * rb
    focal = 0.5 * size * np.sqrt(radius * radius - rb * rb) / rb * 0.95
    return (lo + hi) / 2, float(radius), float(focal), float(np.float32((radius - rb) / 2))


def pose_from_rays(origins, directions, height, width, focal):
    """The (3,4) camera-to-world that get_ray_bundle made these rays from: a dataset (or its ray cache) keeps the rays of
    an image, not its pose.  directions (H*W,3) = R @ unit(x, y, -1): R^T is the least-squares solution over a grid of
    pixels, in fp64."""
    d = np.asarray(directions, np.float64).reshape(height, width, 3)
    rows = np.unique(np.linspace(0, height - 1, 9).round().astype(int))
    cols = np.unique(np.linspace(0, width - 1, 9).round().astype(int))
    jj, ii = np.meshgrid(rows, cols, indexing="ij")
    cam = np.stack(((ii - width * 0.5) / focal, -(jj - height * 0.5) / focal, -np.ones(ii.shape)), -1).reshape(-1, 3)
    cam /= np.linalg.norm(cam, axis=1, keepdims=True)
    rot_t = np.linalg.lstsq(cam, d[jj, ii].reshape(-1, 3), rcond=None)[0]
    origin = np.asarray(origins, np.float64).reshape(-1, 3)[0]
    return np.concatenate((rot_t.T, origin[:, None]), 1).astype(np.float32)


def dataset_views(cfg):
    """the config's test split, as eval_nerf walks it"""
    from torch.utils.data import DataLoader

    from .data.data_helpers import DataBundle
    from .data.datasets import BlenderDataset, DatasetType
    if cfg.dataset.use_ndc:
        raise ValueError("mesh_render: an NDC dataset has no pinhole view to rasterise with")
    dataset = BlenderDataset(cfg, type=DatasetType.TEST)
    for ray_batch in DataLoader(dataset, batch_size=1):
        bundle = DataBundle.deserialize(ray_batch).to_ray_batch()
        height, width, focal = int(bundle.hwf[0]), int(bundle.hwf[1]), float(bundle.hwf[2])
        pose = pose_from_rays(bundle.ray_origins.cpu().numpy(), bundle.ray_directions.cpu().numpy(), height, width, focal)
        yield pose, height, width, focal, bundle.ray_targets


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--mesh", type=str, required=True, help="an OBJ file; `v x y z r g b` lines give the colours")
    p.add_argument("--log-checkpoint", type=str, default=None, help="training log path: cameras of the config's test split")
    p.add_argument("--checkpoint", type=str, default="model_last.ckpt")
    p.add_argument("--views", type=int, default=0, help="this many orbit poses (as eval_nerf --views) instead of a dataset")
    p.add_argument("--radius", type=float, default=4.0, help="turntable without a checkpoint: the orbit's radius")
    p.add_argument("--img-size", type=int, default=800, help="side of the orbit views")
    p.add_argument("--focal", type=float, default=None, help="focal length in pixels of the orbit views (default: the lego focal scaled)")
    p.add_argument("--background", choices=("white", "black"), default=None,
                   help="default: cfg.dataset.white_background, white without a config")
    p.add_argument("--compare-nerf", action="store_true", default=False,
                   help="render every pose with the network too: PSNR, depth difference and IoU of the mesh against it")
    p.add_argument("--near", type=float, default=None, help="default: cfg.dataset.near / 4, 0.05 without a config")
    p.add_argument("--cull", choices=("none", "back"), default="none")
    p.add_argument("--appearance", choices=("auto", "vertex", "texture"), default="auto",
                   help="what colours the mesh: the OBJ's texture (its vt lines and the map_Kd image of its mtllib), its "
                        "per-vertex colours, or auto: the texture when the OBJ has one")
    p.add_argument("--save-dir", type=str, default=".")
    p.add_argument("--save-images", action="store_true", default=False)
    p.add_argument("--save-depth", action="store_true", default=False)
    p.add_argument("--out", type=str, default=None, help="write the report as JSON")
    p.add_argument("--ssim", action="store_true", default=False,
                   help="score every view with the structural similarity too (hip_ops.image_ssim: 11-tap Gaussian window, valid "
                        "windows, data range 1): ssim_target and, with --compare-nerf, ssim_nerf per view and in the means")
    p.add_argument("--save-ssim-maps", action="store_true", default=False,
                   help="implies --ssim: write <save-dir>/mesh_ssim/NNNN.png, the per-pixel SSIM (channel mean, clamped to "
                        "[0, 1]) as 8-bit grey, 10 pixels smaller than the view each way")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mesh_render needs a MI355X: the HIP path has no CPU fallback")
    if args.compare_nerf and not args.log_checkpoint:
        raise SystemExit("--compare-nerf needs --log-checkpoint")
    if not args.log_checkpoint and args.views <= 0:
        raise SystemExit("without --log-checkpoint there is no dataset: give --views N")
    from . import dist as nd
    from .nerf.nerf_helpers import load_obj_textured
    rank, world, device = nd.init_from_env()
    try:
        verts, faces, colors, _, face_uv, image_path = load_obj_textured(args.mesh)
        if colors is None:
            colors = torch.full_like(verts, 0.7)
        if args.appearance == "texture" and face_uv is None:
            raise SystemExit(f"--appearance texture: {args.mesh} has no texture (vt indices on every face corner and an mtllib "
                             "with a readable map_Kd image beside it)")
        texture = None
        if face_uv is not None and args.appearance != "vertex":
            texture = (face_uv, read_image(image_path))
        cfg = model = bounds = chunksize = None
        if args.log_checkpoint:
            pp = PathParser()
            cfg, _ = pp.parse(None, args.log_checkpoint, None, args.checkpoint)
            chunksize = cfg.nerf.validation.chunksize
            bounds = torch.tensor([cfg.dataset.near, cfg.dataset.far], dtype=torch.float32)
            if args.compare_nerf:
                model = getattr(models, cfg.experiment.model).load_from_checkpoint(pp.checkpoint_path).eval().to(device)
                with torch.no_grad():                                # query_view is an inference path: asked the way it is used
                    able = hasattr(model, "can_query_view") and model.can_query_view()
                if not able:
                    raise SystemExit("--compare-nerf needs a model that renders a view from its pose (query_view)")
        white = (args.background == "white") if args.background else (bool(cfg.dataset.white_background) if cfg else True)
        near = args.near if args.near is not None else (cfg.dataset.near / 4 if cfg else 0.05)
        size = args.img_size
        focal = args.focal if args.focal is not None else synthetic.LEGO_FOCAL_800 * size / 800.0
        views = orbit_views(args.views, size, size, focal, radius=args.radius) if args.views > 0 else dataset_views(cfg)
        with torch.no_grad():
            report = evaluate(verts, faces, colors, views, near, (1.0,) * 3 if white else (0.0,) * 3, model=model, bounds=bounds,
                              chunksize=chunksize, compare_nerf=args.compare_nerf, cull_back=args.cull == "back",
                              save_dir=args.save_dir, save_images=args.save_images, save_depth=args.save_depth, device=device,
                              texture=texture, ssim=args.ssim, save_ssim_maps=args.save_ssim_maps)
        report["mesh"] = dict(path=args.mesh, vertices=int(verts.shape[0]), faces=int(faces.shape[0]),
                              appearance="vertex" if texture is None else "texture")
        if texture is not None:
            report["mesh"]["atlas"] = dict(path=image_path, width=int(texture[1].shape[1]), height=int(texture[1].shape[0]))
        for line in format_report(report):
            print(line)
        if args.out and rank == 0:
            write_report(report, args.out)
            print(f"Mesh render report saved to {args.out}")
        return report
    finally:
        nd.shutdown()


if __name__ == "__main__":
    main()
