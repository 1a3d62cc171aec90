"""Mesh extraction with the reference's function names, arguments and CLI
(/root/reference/src/mesh_nerf.py:27-283): dense-grid density query -> adaptive iso level -> Lewiner
marching cubes -> per-vertex appearance -> OBJ, all on the MI355X.

    python -m nerfmeshes_amd.mesh_nerf --log-checkpoint <logdir>/<exp>/<run>/version_N --res 480 --iso-level 32

Differences in mechanism (not in results): the (res^3, 3) sample tensor is never materialised (grid points are
generated in the MLP kernel from the three axis arrays), the radiance stays in HBM (no per-batch D2H), and
marching cubes runs on the GPU grid directly.  `extract_radiance` still returns the same (n0,n1,n2,4) fp32
array for callers that want it; `extract_geometry` uses the density-only path (the colour branch of the MLP is
skipped; sigma is bit-identical to the full evaluation).

The geometry stage exists once (`_mesh_field`): a field given as a query of axis-0 planes, meshed on one rank, on the assembled
grid (`--gather grid`) or per slab (`--gather triangles`) and scaled to world units.  `extract_geometry` hands it the density,
`extract_geometry_with_super_sampling` the density and a vertex refinement, `extract_geometry_tsdf` the fused depth field and a
fixed level.

`--route script` (addition) runs the UNMODIFIED script's own call sequence over the same kernels instead -- host-built sample
points, `batchify` at `--batch-size`, `model.sample_points` + `.cpu()` per batch, numpy's iso level,
`skimage.measure.marching_cubes`, the per-vertex re-query in `--batch-size` calls -- i.e. INTEGRATION.md's route A without the
reference checkout: what a maintainer gets who changes nothing (tests/test_gpu_script_traces.py compares its call trace with the
one recorded from the reference's script; bench.py times its inner loop as `mesh.grid_query.at_reference_batch_1024`).
"""
import argparse
import json
import math
import os
import typing

import torch

from . import hip_ops, models
from .lightning_modules import PathParser
from .nerf.nerf_helpers import batchify, export_obj, export_obj_textured


def create_mesh(vertices, faces_idx):
    """mesh_nerf.py:14-24: the mesh centred and scaled into the unit sphere as a pytorch3d `Meshes` (only the chamfer
    branch of `validation_epoch_end` uses it; needs pytorch3d)."""
    from pytorch3d.structures import Meshes
    vertices = vertices - vertices.mean(0)
    return Meshes(verts=[vertices / max(vertices.abs().max(0)[0])], faces=[faces_idx])


def normalize_vertices(vertices):
    """`create_mesh`'s rule on plain tensors, wherever they live: subtract the vertex mean, then divide by the largest absolute
    coordinate, so the mesh fits [-1, 1]^3 around its vertex centroid (what the chamfer measure compares, mesh_chamfer)."""
    vertices = vertices - vertices.mean(0)
    return vertices / vertices.abs().max()


def _nums(nums):
    assert isinstance(nums, (tuple, list, int)), "Nums arg should be either iterable or int."
    if isinstance(nums, int):
        return (nums,) * 3
    assert len(nums) == 3, "Nums arg should be of length 3, number of axes for 3D"
    return tuple(int(n) for n in nums)


def _axes(args, nums, device):
    # mesh_nerf.py:37: torch.linspace on the host, then meshgrid 'ij' with the last axis fastest
    return [torch.linspace(-args.limit, args.limit, n).to(device) for n in nums]


def _grid_query(model, args, device, nums, density_only):
    nums = _nums(nums)
    net = model.get_model().hip("f32")
    ax = _axes(args, nums, device)
    return net.grid_query(ax[0], ax[1], ax[2], first=0, count=nums[0] * nums[1] * nums[2], density_only=density_only), nums


def _density_query(model, args, device, nums):
    """query(p_lo, p_hi) -> the raw sigma of the axis-0 planes [p_lo, p_hi) of the grid, flat fp32 on the device: what
    `_mesh_field` and the sharding helpers of nerfmeshes_amd.dist take"""
    net = model.get_model().hip("f32")
    ax = _axes(args, nums, device)
    plane = nums[1] * nums[2]
    return lambda p_lo, p_hi: net.grid_query(ax[0], ax[1], ax[2], first=p_lo * plane, count=(p_hi - p_lo) * plane, density_only=True)


def extract_radiance(model, args, device, nums):
    """(n0,n1,n2,4) numpy fp32 [rgb, raw sigma], as mesh_nerf.py:27-53."""
    if getattr(args, "route", "kernel") == "script":
        # the script's own loop (mesh_nerf.py:37-51): the (N,3) sample tensor on the host, one sample_points call and one D2H
        # copy per `--batch-size` points
        nums = _nums(nums)
        tiles = [torch.linspace(-args.limit, args.limit, n) for n in nums]
        samples = torch.stack(torch.meshgrid(*tiles, indexing="ij"), -1).view(-1, 3).float()
        parts = [model.sample_points(x, x).cpu() for (x,) in batchify(samples, batch_size=args.batch_size, device=device)]
        return torch.cat(parts, 0).view(*nums, 4).contiguous().numpy()
    out, nums = _grid_query(model, args, device, nums, density_only=False)
    return out.view(*nums, 4).cpu().numpy()


def extract_density(model, args, device, nums):
    """Density grid (n0,n1,n2) as a GPU tensor (radiance[..., 3] of the reference, mesh_nerf.py:73).
    Under torch.distributed (one process per GPU) every rank evaluates its slab of axis-0 planes and one
    all-gather (RCCL over xGMI) assembles the full grid on every rank; marching cubes then runs on the full
    grid, so the mesh is identical to the single-GPU one by construction."""
    from . import dist as nd
    nums = _nums(nums)
    query = _density_query(model, args, device, nums)
    if nd.world()[1] == 1:
        return query(0, nums[0]).view(*nums)
    return nd.density_grid_sharded(query, *nums)


def extract_iso_level(density, args):
    """mesh_nerf.py:56-65.  `density` may be a numpy array (the reference's own code path) or a GPU tensor: then the
    statistics are numpy's fp32 reductions replayed on the device (nm_np_stats: 8192-element chunks, pairwise sums,
    fp32 mean / variance) -- the SAME iso value bit for bit, which is what "bit-identical topology for the same
    iso-level" needs whenever the clamp to [min + std, max - std] is active."""
    if isinstance(density, torch.Tensor):
        st = hip_ops.np_stats(density)
        lo, hi, std, mean = st["min"], st["max"], st["std"], st["mean"]
    else:
        lo, hi, std, mean = density.min(), density.max(), density.std(), density.mean()
    iso_value = min(max(args.iso_level, lo + std), hi - std)
    print(f"Min density {lo}, Max density: {hi}, Mean density {mean}")
    print(f"Querying based on iso level: {iso_value}")
    return iso_value


def extract_iso_level_sharded(slab, first_plane, own_lo, own_hi, nums, args):
    """`extract_iso_level` of a grid that lives in slabs on several ranks: numpy's fp32 statistics of the WHOLE grid from
    per-rank chunk sums (hip_ops.np_stats_sharded), so that every rank gets the single-GPU level bit for bit."""
    from . import dist as nd
    n_total = nums[0] * nums[1] * nums[2]
    plane = nums[1] * nums[2]
    dev = slab.device if slab is not None else torch.device("cuda", torch.cuda.current_device())
    if plane < 8192:
        # numpy's 8192-element chunks are wider than the one-plane halo: a grid this small is simply assembled
        own = slab.reshape(-1)[own_lo - first_plane * plane:own_hi - first_plane * plane] if slab is not None else torch.empty(0, device=dev)
        st = hip_ops.np_stats(nd.all_gather_ragged(own.contiguous()))
    else:
        x = slab if slab is not None else torch.zeros(1, dtype=torch.float32, device=dev)
        st = hip_ops.np_stats_sharded(x, first_plane * plane, n_total, own_lo, own_hi, nd.all_gather_ragged)
    iso_value = min(max(args.iso_level, st["min"] + st["std"]), st["max"] - st["std"])
    print(f"Min density {st['min']}, Max density: {st['max']}, Mean density {st['mean']}")
    print(f"Querying based on iso level: {iso_value}")
    return iso_value


def _mesh_field(query, nums, args, level=None, refine=None):
    """The geometry stage of every route: the mesh of the scalar field whose axis-0 planes [p_lo, p_hi) `query(p_lo, p_hi)`
    returns (flat fp32 on the device) -> (vertices (V,3) f32 in world units, triangles (F,3) i32, normals (V,3) f32, the field).
    `level`: the level to mesh at; None is the numpy-exact adaptive iso level of the whole field (extract_iso_level).
    `refine(volume, z_global, iso, vertices, keys)` (optional) moves the vertices in place while they are in grid-index units,
    as dist.marching_cubes_sharded calls it.  One rank evaluates and meshes the whole field and issues no collective.  Under
    torch.distributed `--gather grid` assembles the field on every rank (dist.density_grid_sharded) and meshes it redundantly;
    `--gather triangles`, the default, meshes every rank's own slab of cube layers and only the triangles travel
    (dist.marching_cubes_sharded; the 4th value is then the rank's own slab, None on a rank without one).  All three give the
    same mesh bit for bit; an empty one is skimage's two errors on every rank."""
    from . import dist as nd
    world = nd.world()[1]
    if world > 1 and getattr(args, "gather", "triangles") == "triangles":
        if level is None:
            iso_fn = lambda slab, p_lo, own_lo, own_hi: extract_iso_level_sharded(slab, p_lo, own_lo, own_hi, nums, args)  # noqa: E731
        else:
            iso_fn = lambda *slab: level  # noqa: E731
        vertices, triangles, normals, _, field = nd.marching_cubes_sharded(query, *nums, iso_fn, refine=refine)
    else:
        field = nd.density_grid_sharded(query, *nums) if world > 1 else query(0, nums[0]).view(*nums)
        iso = extract_iso_level(field, args) if level is None else level
        if refine is None:
            vertices, triangles, normals, _ = hip_ops.marching_cubes(field, iso)
        else:
            vertices, triangles, normals, _, keys = hip_ops.marching_cubes(field, iso, return_keys=True)
            refine(field, 0, iso, vertices, keys)
    vertices = args.limit * (vertices / (args.res / 2.0) - 1.0)   # res/2, not (res-1)/2: as the reference
    return vertices, triangles, normals, field


def extract_geometry(model, device, args):
    """mesh_nerf.py:68-92 -> (vertices (V,3) f32, triangles (F,3) i32, normals (V,3) f32, density grid): `_mesh_field` of the
    density, whose three ways of running on one or several ranks are described there (under `--gather triangles` the 4th
    value is the rank's own slab of the grid)."""
    if getattr(args, "route", "kernel") == "script":
        # mesh_nerf.py:68-92 as written: the full radiance grid on the host, numpy's statistics, scikit-image's entry point
        # (the real package, or compat's nm_mc_* stand-in where it is not installed)
        import numpy as np
        try:
            from skimage import measure
            marching_cubes = measure.marching_cubes
        except ImportError:
            from .compat import marching_cubes
        density = extract_radiance(model, args, device, args.res)[..., 3]
        iso_value = extract_iso_level(density, args)
        vertices, triangles, normals, _ = [torch.from_numpy(np.ascontiguousarray(r)) for r in marching_cubes(density, iso_value)]
        vertices = args.limit * (vertices / (args.res / 2.0) - 1.0)
        return vertices, triangles, normals, density
    nums = _nums(args.res)
    return _mesh_field(_density_query(model, args, device, nums), nums, args)


def _assemble_grid_from_slabs(slab, nums, device):
    """The whole density grid from the slabs `--gather triangles` left on the ranks (only the mesh cache wants it): every
    rank contributes the planes it accounts for -- the lower planes of its own cube layers, the last non-empty rank also the
    top plane -- through ONE ragged all-gather; nothing is evaluated twice.  A rank without a cube layer (more ranks than
    layers) holds no slab (None) and contributes nothing, but still enters the collective."""
    from . import dist as nd
    rank, world = nd.world()
    n0, n1, n2 = nums
    lo, hi, below, above, p_lo, p_hi = nd.slab_layers(n0, rank, world)
    if slab is None or hi == lo:
        own = torch.empty(0, n1, n2, dtype=torch.float32, device=device)
    else:
        top = hi + (1 if hi == n0 - 1 else 0)
        own = slab.view(p_hi - p_lo, n1, n2)[lo - p_lo:top - p_lo]
    return nd.all_gather_ragged(own.contiguous()).view(n0, n1, n2)


def refine_vertices(net, args, nums, ss, volume, z_global, iso, vertices, keys):
    """Super-sampling of one marching-cubes result in place: the ss interior samples of every vertex's edge
    (hip_ops.mc_edge_points), their raw sigma (HipMLP.sample_density: the fp32 density kernels), and every edge vertex moved
    to the first sign change along its edge (hip_ops.mc_refine_vertices).  `vertices` are in grid-index units; `volume` holds
    the global planes [z_global, z_global + volume.shape[0])."""
    if keys.numel() == 0:
        return vertices
    base = _axes(args, nums, volume.device)
    fine = [hip_ops.fine_axis(args.limit, n, ss) for n in nums]
    points = hip_ops.mc_edge_points(keys, nums, ss, base, fine)
    sigma = net.sample_density(points.view(-1, 3))
    return hip_ops.mc_refine_vertices(volume, z_global, iso, keys, ss, sigma.view(-1, ss), vertices)


def extract_geometry_with_super_sampling(model, device, args):
    """mesh_nerf.py:95-128 (dead code there: it raises on its first line) as a working feature -> the same four values as
    `extract_geometry`.  The topology, normals and values are the plain res^3 mesh's, bit for bit; only an edge vertex's
    coordinate along its own edge changes: it moves to the first sign change among the `--super-sampling` samples strictly
    inside that edge (on the fine axis linspace(-limit, limit, (res-1)*(ss+1)+1)).  Only those samples are evaluated -- not
    the reference's three dense grids ("Super-sampled meshing").  Under torch.distributed, `--gather grid` refines
    after the redundant marching cubes, `--gather triangles` refines every slab's own vertices before they travel; both give
    the single-rank mesh bit for bit."""
    ss = int(args.super_sampling)
    if getattr(args, "route", "kernel") == "script":
        raise ValueError("--super-sampling has no --route script: the reference's script never runs it (mesh_nerf.py:95-96)")
    nums = _nums(args.res)
    hip_ops.check_super_sampling(nums, ss)
    net = model.get_model().hip("f32")
    return _mesh_field(_density_query(model, args, device, nums), nums, args,
                       refine=lambda volume, z_global, iso, v, keys: refine_vertices(net, args, nums, ss, volume, z_global, iso, v, keys))


def tsdf_focal(args):
    """`--tsdf-focal 0`: the synthetic scenes' 1111.1111 at 800 pixels, scaled to --tsdf-size"""
    from . import synthetic
    return float(args.tsdf_focal) or synthetic.LEGO_FOCAL_800 * int(args.tsdf_size) / 800.0


def tsdf_ray_lengths(size, focal):
    """(size, size) fp64 on the host: |(x, y, -1)| of get_ray_bundle's camera-space ray through every pixel of a square view --
    the distance along the unit ray over the depth along the camera's axis"""
    import numpy as np
    i = (np.arange(size, dtype=np.float64) - size * 0.5) / np.float64(focal)
    return np.sqrt(i[None, :] * i[None, :] + i[:, None] * i[:, None] + 1.0)


def check_tsdf(args, cfg=None):
    """What `--geometry tsdf` cannot be combined with (ValueError): --super-sampling, whose refinement reads density along the
    cut edges, and a scene in NDC, whose rays are not the pinhole rays the fusion projects along."""
    if int(getattr(args, "super_sampling", 0)) >= 1:
        raise ValueError("--geometry tsdf has no --super-sampling: the refinement moves a vertex to a sign change of the density, "
                         "and the fused field has none")
    if cfg is not None and cfg.dataset.use_ndc:
        raise ValueError("--geometry tsdf needs pinhole views: the scene is in normalised device coordinates (cfg.dataset.use_ndc)")


def tsdf_render_views(model, args, cfg, device):
    """The depth and the opacity of the --tsdf-views cameras -> (views: hip_ops.make_view results, depth (V,S,S), opacity (V,S,S)).
    `query_view(..., keep_depth=True)` measures the depth along the UNIT ray of each pixel (get_ray_bundle normalises its
    directions); the fusion compares it with a voxel's depth along the camera's axis, so every depth is divided by its pixel's
    |(x, y, -1)| (tsdf_ray_lengths) in fp64 and rounded to fp32 once.  Under torch.distributed the VIEWS are split over the
    ranks (dist.own_range) and ONE all-gather assembles both stacks on every rank."""
    from . import dist as nd
    from . import mesh_render
    count, size, focal = int(args.tsdf_views), int(args.tsdf_size), tsdf_focal(args)
    poses = mesh_render.sphere_poses(count, (0.0, 0.0, 0.0), float(args.tsdf_radius))
    bounds = torch.tensor([cfg.dataset.near, cfg.dataset.far], dtype=torch.float32)
    lo, hi, counts = nd.own_range(count)
    own = torch.empty(hi - lo, 2, size, size, dtype=torch.float32, device=device)
    lengths = torch.from_numpy(tsdf_ray_lengths(size, focal)).to(device)
    for k in range(lo, hi):
        out = model.query_view(torch.from_numpy(poses[k]), size, size, focal, bounds, keep_depth=True)
        own[k - lo, 0] = (out.depth_map.view(size, size).double() / lengths).float()
        own[k - lo, 1] = out.acc_map.view(size, size)
    if len(counts) > 1:                     # more than one rank
        own = nd.all_gather_rows(own, counts)
    views = [hip_ops.make_view(pose, size, size, focal) for pose in poses]
    return views, own[:, 0].contiguous(), own[:, 1].contiguous()


def extract_geometry_tsdf(model, device, args, cfg):
    """`--geometry tsdf` -> the four values of `extract_geometry`, the 4th being the fused field ("TSDF geometry"): the
    network's depth is rendered from --tsdf-views cameras all around the volume (tsdf_render_views), fused into a truncated
    signed distance field on the density grid's own axes (hip_ops.tsdf_integrate: inside-positive, so that marching cubes winds
    and orients the mesh as on the density path) and meshed at --tsdf-level -- no iso level to clamp.  Under torch.distributed
    the views are split for the render; `--gather triangles` then fuses and meshes per slab (dist.marching_cubes_sharded),
    `--gather grid` fuses slabs and assembles the field; both give the single-rank mesh bit for bit.  Rank 0 writes
    <save-dir>/<mesh-name stem>.tsdf.json."""
    import time
    from . import dist as nd
    check_tsdf(args, cfg)
    if not (hasattr(model, "can_query_view") and model.can_query_view()):
        raise RuntimeError("--geometry tsdf needs a model with the deterministic in-kernel view render (NeRFModel.query_view "
                           "in eval mode, no perturb / noise): there is no fallback")
    rank, world = nd.world()
    nums = _nums(args.res)
    if min(nums) < 2:
        raise ValueError("Input array must be at least 2x2x2.")
    plane = nums[1] * nums[2]
    ax = _axes(args, nums, device)
    level = float(args.tsdf_level)
    trunc = float(args.tsdf_trunc) * 2.0 * args.limit / (nums[0] - 1)        # --tsdf-trunc voxels of the grid's own spacing
    seconds = {}

    def clock(name, start):
        torch.cuda.synchronize(device)
        seconds[name] = seconds.get(name, 0.0) + time.perf_counter() - start

    start = time.perf_counter()
    views, depth, opacity = tsdf_render_views(model, args, cfg, device)
    clock("render", start)
    tally = torch.zeros(3, dtype=torch.int64, device=device)

    def integrate(p_lo, p_hi, counted):
        nonlocal tally
        out = hip_ops.tsdf_integrate(views, depth, opacity, ax, trunc, cfg.dataset.near, min_opacity=float(args.tsdf_min_opacity),
                                     first=p_lo * plane, count=(p_hi - p_lo) * plane)
        if counted:
            tally = tally + out["counts"]
        return out["field"]

    # the counters count every plane of the grid on exactly one rank: under `--gather triangles` a rank's ghost planes are fused
    # in calls of their own (voxels are independent, so the field is the same bytes) and not counted; elsewhere no plane is
    # fused twice
    own = None
    if world > 1 and getattr(args, "gather", "triangles") == "triangles":
        lo, hi = nd.slab_layers(nums[0], rank, world)[:2]
        own = lo, hi + (1 if hi == nums[0] - 1 else 0)

    def query(p_lo, p_hi):
        start = time.perf_counter()
        lo, top = own or (p_lo, p_hi)
        parts = [integrate(a, b, counted) for a, b, counted in ((p_lo, lo, False), (lo, top, True), (top, p_hi, False)) if b > a]
        clock("integrate", start)
        return torch.cat(parts) if len(parts) > 1 else parts[0]

    start = time.perf_counter()
    vertices, triangles, normals, field = _mesh_field(query, nums, args, level=level)
    clock("marching_cubes", start)
    seconds["marching_cubes"] -= seconds.get("integrate", 0.0)       # the stage without the fusion inside it (a rank may fuse nothing)
    if world > 1:
        nd.all_reduce(tally)
    counts = dict(zip(hip_ops.TSDF_COUNTS, (int(x) for x in tally.tolist())))
    print(f"TSDF: {len(views)} views of {int(args.tsdf_size)}² fused into {nums[0]} x {nums[1]} x {nums[2]} voxels: "
          f"{counts['observed']} observed, {counts['interior']} interior (occluded in every view), {counts['outside']} outside every "
          f"view; {vertices.shape[0]} vertices, {triangles.shape[0]} faces")
    if rank == 0:
        path = os.path.join(args.save_dir, os.path.splitext(args.mesh_name)[0] + ".tsdf.json")
        report = dict(geometry="tsdf", res=list(nums), limit=float(args.limit), views=len(views), size=int(args.tsdf_size),
                      radius=float(args.tsdf_radius), focal=tsdf_focal(args), trunc_voxels=float(args.tsdf_trunc), trunc=trunc,
                      near=float(cfg.dataset.near), min_opacity=float(args.tsdf_min_opacity), level=level, voxels=counts,
                      vertices=int(vertices.shape[0]), faces=int(triangles.shape[0]),
                      seconds={k: seconds.get(k, 0.0) for k in ("render", "integrate", "marching_cubes")})   # last: all that varies
        with open(path, "w") as fh:
            json.dump(report, fh, indent=1)
            fh.write("\n")
        print(f"TSDF report saved to {path}")
    return vertices, triangles, normals, field


def network_normals(net, vertices, normals):
    """`--normals network`: n = -grad / |grad| of the network's raw sigma at the world-space vertices (HipMLP.density_gradient),
    normalised in fp32 -- towards lower density, the orientation of skimage's default (gradient_direction="descent") and so of
    the grid normals.  A vertex whose gradient is zero or not finite keeps its grid normal.  -> (normals (V,3), kept (V,) bool:
    the vertices that kept theirs)."""
    normals = normals.to(dtype=torch.float32)
    if vertices.shape[0] == 0:
        return normals.reshape(0, 3), torch.zeros(0, dtype=torch.bool, device=normals.device)
    g = net.density_gradient(vertices)
    norm = torch.linalg.vector_norm(g, dim=1, keepdim=True)
    ok = torch.isfinite(norm) & (norm > 0)
    return torch.where(ok, -g / norm, normals.to(g.device)), ~ok[:, 0]


def filter_components(vertices, triangles, normals, min_faces, keep_largest):
    """`--min-component-faces N` / `--keep-largest K` on the device (hip_ops.mesh_filter_components): components -- vertices
    joined by triangles -- with fewer than N triangles go; of the rest the K with most triangles stay (ties: the one holding
    the smaller vertex index).  Kept vertices and triangles stay in their order.  ValueError when nothing is left."""
    vertices, triangles, normals, _, _, info = hip_ops.mesh_filter_components(
        vertices, triangles.to(torch.int32), normals, min_faces=min_faces, keep_largest=keep_largest)
    if info["faces_kept"] == 0:
        raise ValueError(f"no mesh component has at least {max(min_faces, 1)} faces: the filter (--min-component-faces {min_faces}, "
                         f"--keep-largest {keep_largest}) leaves nothing of {info['components']} components / {info['faces']} faces")
    print(f"Component filter: kept {info['components_kept']} of {info['components']} components, {info['faces_kept']} of "
          f"{info['faces']} faces, {info['vertices_kept']} of {info['vertices']} vertices")
    return vertices, triangles, normals


CULL_MAX_SIZE = 16384       # the rasteriser's largest image side


def cull_size(res):
    """`--cull-size 0`: the smallest multiple of 256 that gives a voxel of a res^3 grid at least 2 pixels when the grid's box
    fills 95 % of the image, at most the rasteriser's 16384 (1792 at --res 480)"""
    return min(int(math.ceil(2.0 * math.sqrt(3.0) * res / 0.95 / 256.0)) * 256, CULL_MAX_SIZE)


def cull_hidden(vertices, triangles, normals, args):
    """`--cull-hidden-views N` on the device (hip_ops.mesh_cull_hidden): the mesh is rasterised from N cameras all around it
    (mesh_render.sphere_views at --cull-radius bounding radii, --cull-size pixels square) and only the faces that win a pixel
    somewhere stay, with --cull-rings rounds of their vertex neighbours -- the faces too small to win a pixel centre.  Kept
    vertices and triangles stay in their order.  Rank 0 writes <save-dir>/<mesh-name stem>.visibility.json.  ValueError when
    nothing is left."""
    from . import dist as nd
    from . import mesh_render
    count, rings, radius = int(args.cull_hidden_views), int(args.cull_rings), float(args.cull_radius)
    res = max(_nums(args.res))
    size = int(args.cull_size) or cull_size(res)
    centre, distance, focal, near = mesh_render.frame_views(vertices, radius, size)
    views = [hip_ops.make_view(pose, h, w, f) for pose, h, w, f, _ in mesh_render.sphere_views(count, centre, distance, size, focal)]
    vertices, triangles, normals, _, info = hip_ops.mesh_cull_hidden(vertices, triangles.to(torch.int32), normals, views, near,
                                                                     rings=rings)
    # the bounding sphere, 2 distance / --cull-radius across, spans 0.95 size pixels
    per_voxel = 0.95 * size * (2.0 * args.limit / res) / (2.0 * distance / radius)
    if info["faces_kept"] == 0:
        raise ValueError(f"--cull-hidden-views {count} leaves nothing of {info['faces']} faces: no view of {size}^2 pixels sees one")
    print(f"Hidden-face filter: kept {info['faces_kept']} of {info['faces']} faces ({info['faces_seen']} seen), "
          f"{info['vertices_kept']} of {info['vertices']} vertices, {count} views of {size}\u00b2, {per_voxel:.2f} px/voxel")
    if per_voxel < 1.0:
        print(f"Warning: {per_voxel:.2f} pixels per voxel: faces smaller than a pixel are kept only through --cull-rings; raise "
              "--cull-size")
    if nd.world()[0] == 0:
        path = os.path.join(args.save_dir, os.path.splitext(args.mesh_name)[0] + ".visibility.json")
        report = dict(info, views=count, size=size, rings=rings, radius=radius, focal=focal, near=near, centre=[float(x) for x in centre],
                      distance=distance, pixels_per_voxel=per_voxel)
        with open(path, "w") as fh:
            json.dump(report, fh, indent=1)
            fh.write("\n")
        print(f"Hidden-face report saved to {path}")
    return vertices, triangles, normals


SMOOTH_FLIP = -1            # marching cubes winds its triangles against its normals (tests/test_mesh_smooth.py pins it)


def smooth_mesh(vertices, triangles, normals, args):
    """`--smooth-iters N` on the device (hip_ops.mesh_smooth): N iterations of Taubin's filter -- an umbrella half-step with
    `--smooth-lambda`, then one with `--smooth-mu` -- on the full-resolution mesh; boundary vertices (the grid box clips most
    exports) stay in place unless `--smooth-boundary free`.  The numbering and the triangles stay; the normals are recomputed
    from the smoothed triangles, on the side marching cubes' normals point to."""
    old = vertices
    vertices, normals, info = hip_ops.mesh_smooth(vertices, triangles.to(torch.int32), normals, iterations=args.smooth_iters,
                                                  lam=args.smooth_lambda, mu=args.smooth_mu,
                                                  free_boundary=args.smooth_boundary == "free", flip=SMOOTH_FLIP)
    voxel = 2.0 * args.limit / args.res
    moved = float(torch.linalg.vector_norm(vertices - old.to(vertices), dim=1).max()) / voxel if vertices.shape[0] else 0.0
    kept = 0 if args.smooth_boundary == "free" else info["boundary_vertices"]
    print(f"Smooth: {args.smooth_iters} iterations (lambda {args.smooth_lambda:g}, mu {args.smooth_mu:g}): {info['vertices']} vertices, "
          f"{kept} boundary vertices kept in place, {info['isolated_vertices']} isolated, {info['nonmanifold_edges']} non-manifold "
          f"edges, largest displacement {moved:.4f} voxels")
    return vertices, triangles, normals


def simplify_mesh(vertices, triangles, normals, cell_voxels, args):
    """`--simplify-cell K` on the device (hip_ops.mesh_simplify): vertex clustering on a grid of K-voxel cells, K * (2 * limit /
    res) world units, anchored at (-limit,)*3 -- the vertices of one cell become their exact mean (one alone stays bit for bit),
    degenerate and duplicate triangles go, kept ones stay in their order.  `--simplify-placement quadric` puts the vertex of a
    cell where the planes of the triangles around it meet instead (exact integer quadrics: the same bytes on every rank), which
    keeps creases and curved surfaces where they are.  `--simplify-levels L` with `--simplify-error E` (voxels) makes the
    clustering adaptive: the same on the nested grids of K * 2^l voxels, l = 0 .. L, every vertex in the coarsest cell whose
    quadric vertex lies within E of every triangle plane around it.  ValueError when no triangle is left."""
    voxel = 2.0 * args.limit / args.res
    cell = float(cell_voxels) * voxel
    v0, f0 = vertices.shape[0], triangles.shape[0]
    placement = getattr(args, "simplify_placement", "mean")
    levels = int(getattr(args, "simplify_levels", 0))
    adaptive = dict(levels=levels, max_error=float(getattr(args, "simplify_error", SIMPLIFY_ERROR_DEFAULT)) * voxel) if levels else {}
    vertices, triangles, normals, info = hip_ops.mesh_simplify(vertices, triangles.to(torch.int32), normals, cell=cell,
                                                               origin=(-args.limit,) * 3, placement=placement, **adaptive)
    if info["faces_kept"] == 0:
        raise ValueError(f"--simplify-cell {cell_voxels:g} leaves no triangle of {f0}: every one has two corners in one cell "
                         f"({info['clusters']} clusters of {v0} vertices)")
    print(f"Simplify: cell {cell_voxels:g} voxels: {v0} -> {info['vertices_kept']} vertices, {f0} -> {info['faces_kept']} faces "
          f"({info['degenerate_faces']} degenerate, {info['duplicate_faces']} duplicate)")
    if placement == "quadric":
        print(f"Simplify placement: quadric: {info['quadric_clusters']} clusters at their quadric's minimum "
              f"({info['clamped_clusters']} clamped to the cell), at the mean: {info['crowded_clusters']} crowded, "
              f"{info['singular_clusters']} singular; {info['far_corners']} far corners")
    if levels:
        print(f"Simplify levels: {levels} (cells of {cell_voxels:g} to {cell_voxels * 2 ** levels:g} voxels), error bound "
              f"{args.simplify_error:g} voxels, largest accepted error {info['largest_error'] / voxel:.4f} voxels")
        for l in range(levels, -1, -1):
            refused = ("" if l == 0 else
                       f"; refused: {info['refused_error'][l]} error, {info['refused_crowded'][l]} crowded, "
                       f"{info['refused_singular'][l]} singular, {info['refused_far'][l]} far, "
                       f"{info['refused_empty'][l]} no contributions")
            print(f"Simplify level {l}: {info['level_vertices'][l]} vertices in {info['level_clusters'][l]} clusters, "
                  f"{info['level_kept'][l]} kept{refused}")
    return vertices, triangles, normals


def chamfer_to_target(vertices, triangles, args, device):
    """`--target-mesh PATH`: the chamfer distance between the extracted mesh and an OBJ file, both in world coordinates
    (mesh_chamfer.compare_meshes with --chamfer-samples / --chamfer-seed / --target-surface / --target-fscore), printed; rank 0 writes
    <save-dir>/<mesh-name stem>.chamfer.json.  Under torch.distributed the searches are shared out over the ranks."""
    from . import dist as nd
    from . import mesh_chamfer
    from .nerf.nerf_helpers import load_obj
    target_vertices, target_faces = load_obj(args.target_mesh)
    report = mesh_chamfer.compare_meshes(vertices, triangles, target_vertices, target_faces, samples=args.chamfer_samples,
                                         seed=args.chamfer_seed, device=device, surface=getattr(args, "target_surface", "sampled"),
                                         fscore=getattr(args, "target_fscore", None))
    report["target"]["path"] = args.target_mesh
    for line in mesh_chamfer.format_report(report):
        print(line)
    if nd.world()[0] == 0:
        path = os.path.join(args.save_dir, os.path.splitext(args.mesh_name)[0] + ".chamfer.json")
        mesh_chamfer.write_report(report, path)
        print(f"Chamfer report saved to {path}")
    return report


class Feature(typing.NamedTuple):
    """One optional addition to the export, as data: what export_marching_cubes checks before anything is read or written, and
    for a geometry stage what postprocess calls."""
    what: str                   # the options' names, as the --route script refusal lists them
    options: dict               # option -> default; a namespace without the option has the default
    on: typing.Callable         # o -> switched on, with o = the options' values
    valid: typing.Callable = lambda o: True     # o -> every option is in range
    invalid: typing.Callable = None             # o -> the ValueError's text when not
    any_option: bool = False    # refused and range-checked as soon as ANY option differs from its default, not only when on
    script_has: str = "has no such step"        # what the reference's script has instead
    run: typing.Callable = None                 # a geometry stage: (vertices, triangles, normals, o, args) -> the three

    def values(self, args):
        return {name: getattr(args, name, default) for name, default in self.options.items()}

    def checked(self, o):
        return bool(self.on(o)) or (self.any_option and any(o[name] != default for name, default in self.options.items()))


def _finite(x, lo=float("-inf"), hi=float("inf")):
    return lo < float(x) < hi                       # a NaN fails both comparisons


def _target_surface_valid(o):
    from . import mesh_chamfer
    try:
        mesh_chamfer.check_surface(o["target_surface"], o["target_fscore"])
    except ValueError:
        return False
    return bool(o["target_mesh"])


# --simplify-error's default, in voxels: half of the tighter of the two distances the surface reports score at (F-score at half
# a voxel and at one), so a vertex that uses the whole bound still leaves every triangle plane around it well inside that
# band; it is also the accuracy uniform clustering with 4-voxel cells reaches on the synthetic scene (0.26 voxels, README)
SIMPLIFY_ERROR_DEFAULT = 0.25


def _simplify_levels_invalid(o):
    """the refusal of --simplify-levels L != 0 with the other simplify options as they are, or None"""
    levels, error = int(o["simplify_levels"]), float(o["simplify_error"])
    if not 0 <= levels <= hip_ops.SIMPLIFY_MAX_LEVELS:
        return f"--simplify-levels must be in [0, {hip_ops.SIMPLIFY_MAX_LEVELS}], got {levels}"
    if not 0.0 < float(o["simplify_cell"]) < float("inf"):
        return f"--simplify-levels {levels} needs --simplify-cell K > 0"
    if o["simplify_placement"] != "quadric":
        return f"--simplify-levels {levels} needs --simplify-placement quadric"
    if not 0.0 <= error < float("inf"):
        return f"--simplify-error must be finite and >= 0, got {error}"
    return None


TSDF_OPTIONS = {"geometry": "density", "tsdf_views": 32, "tsdf_size": 800, "tsdf_radius": 4.0, "tsdf_focal": 0.0, "tsdf_trunc": 3.0,
                "tsdf_min_opacity": 0.5, "tsdf_level": 0.0}

# The geometry stages run in this order (postprocess).  The component filter comes first: its thresholds count original
# triangles, and a filter that leaves nothing raises before anything is written.  The cull comes next, on the full-resolution
# geometry, so that the smoothing, the clustering, the appearance rays and the texture bake work on less.  Smoothing comes
# before the clustering, which then averages smoothed positions and the recomputed normals.  All four come before
# --target-mesh, the network normals and the appearance query, which see the final geometry and spend no ray on a dropped
# vertex.  The stage functions are looked up on this module when they are called, so that a tool can replace one.
FEATURES = {
    "tsdf": Feature(
        "--geometry tsdf / --tsdf-views / --tsdf-size / --tsdf-radius / --tsdf-focal / --tsdf-trunc / --tsdf-min-opacity / "
        "--tsdf-level", TSDF_OPTIONS, on=lambda o: o["geometry"] == "tsdf", any_option=True,
        valid=lambda o: (o["geometry"] in ("density", "tsdf") and 1 <= int(o["tsdf_views"]) <= hip_ops.TSDF_MAX_VIEWS
                         and 1 <= int(o["tsdf_size"]) <= 16384 and _finite(o["tsdf_radius"], lo=0.0)
                         and (float(o["tsdf_focal"]) == 0.0 or _finite(o["tsdf_focal"], lo=0.0)) and _finite(o["tsdf_trunc"], lo=0.0)
                         and _finite(o["tsdf_min_opacity"]) and _finite(o["tsdf_level"], -1.0, 1.0)),
        invalid=lambda o: (f"--geometry must be density or tsdf, --tsdf-views in [1, {hip_ops.TSDF_MAX_VIEWS}], --tsdf-size in "
                           "[1, 16384], --tsdf-radius and --tsdf-trunc finite and > 0, --tsdf-focal finite and >= 0, "
                           "--tsdf-min-opacity finite and --tsdf-level in (-1, 1)")),
    "normals": Feature(
        "--normals network", {"normals": "grid"}, on=lambda o: o["normals"] == "network",
        script_has="only has the grid's normals"),
    "components": Feature(
        "--min-component-faces / --keep-largest", {"min_component_faces": 0, "keep_largest": 0},
        on=lambda o: int(o["min_component_faces"]) or int(o["keep_largest"]),
        valid=lambda o: int(o["min_component_faces"]) >= 0 and 0 <= int(o["keep_largest"]) <= hip_ops.KEEP_LARGEST_MAX,
        invalid=lambda o: f"--min-component-faces must be >= 0 and --keep-largest in [0, {hip_ops.KEEP_LARGEST_MAX}]",
        run=lambda v, t, n, o, args: filter_components(v, t, n, int(o["min_component_faces"]), int(o["keep_largest"]))),
    "cull": Feature(
        "--cull-hidden-views / --cull-size / --cull-rings / --cull-radius",
        {"cull_hidden_views": 0, "cull_size": 0, "cull_rings": 1, "cull_radius": 3.0},
        on=lambda o: int(o["cull_hidden_views"]), any_option=True,
        valid=lambda o: (int(o["cull_hidden_views"]) >= 0 and 0 <= int(o["cull_size"]) <= CULL_MAX_SIZE
                         and 0 <= int(o["cull_rings"]) <= hip_ops.VISIBILITY_MAX_RINGS
                         and 1.0 < float(o["cull_radius"]) < float("inf")),
        invalid=lambda o: (f"--cull-hidden-views must be >= 0, --cull-size in [0, {CULL_MAX_SIZE}], --cull-rings in "
                           f"[0, {hip_ops.VISIBILITY_MAX_RINGS}] and --cull-radius finite and > 1"),
        run=lambda v, t, n, o, args: cull_hidden(v, t, n, args)),
    "smooth": Feature(
        "--smooth-iters / --smooth-lambda / --smooth-mu / --smooth-boundary",
        {"smooth_iters": 0, "smooth_lambda": 0.5, "smooth_mu": -0.53, "smooth_boundary": "fixed"},
        on=lambda o: int(o["smooth_iters"]), any_option=True,
        valid=lambda o: (0 <= int(o["smooth_iters"]) <= hip_ops.SMOOTH_MAX_ITERATIONS and 0.0 < o["smooth_lambda"] <= 1.0
                         and -1.0 <= o["smooth_mu"] <= 0.0),
        invalid=lambda o: (f"--smooth-iters must be in [0, {hip_ops.SMOOTH_MAX_ITERATIONS}], --smooth-lambda in (0, 1] and "
                           "--smooth-mu in [-1, 0]"),
        run=lambda v, t, n, o, args: smooth_mesh(v, t, n, args)),
    "simplify": Feature(
        "--simplify-cell", {"simplify_cell": 0.0, "simplify_placement": "mean"},
        on=lambda o: float(o["simplify_cell"]), any_option=True,      # a placement without a cell is refused, not ignored
        valid=lambda o: 0.0 < float(o["simplify_cell"]) < float("inf") and o["simplify_placement"] in hip_ops.SIMPLIFY_PLACEMENTS,
        invalid=lambda o: (f"--simplify-placement must be mean or quadric, got {o['simplify_placement']}"
                           if o["simplify_placement"] not in hip_ops.SIMPLIFY_PLACEMENTS else
                           f"--simplify-placement {o['simplify_placement']} needs --simplify-cell K > 0"
                           if float(o["simplify_cell"]) == 0.0 else
                           f"--simplify-cell must be finite and >= 0, got {float(o['simplify_cell'])}"),
        run=lambda v, t, n, o, args: simplify_mesh(v, t, n, float(o["simplify_cell"]), args)),
    "simplify_levels": Feature(
        "--simplify-levels / --simplify-error",
        {"simplify_levels": 0, "simplify_error": SIMPLIFY_ERROR_DEFAULT, "simplify_cell": 0.0, "simplify_placement": "mean"},
        # options of "simplify", which runs the stage: checked, never switched on; the cell and the placement are among the
        # options because the levels are valid only with them ("simplify", which comes first, speaks for the two themselves).
        # --simplify-error is read only with levels > 0: without them it is not even range-checked
        on=lambda o: False, any_option=True,
        valid=lambda o: int(o["simplify_levels"]) == 0 or _simplify_levels_invalid(o) is None,
        invalid=lambda o: _simplify_levels_invalid(o)),
    "target": Feature(
        "--target-mesh", {"target_mesh": None, "chamfer_samples": 100000}, on=lambda o: o["target_mesh"],
        valid=lambda o: int(o["chamfer_samples"]) >= 1,
        invalid=lambda o: f"--chamfer-samples must be >= 1, got {o['chamfer_samples']}"),
    "target_surface": Feature(
        "--target-surface / --target-fscore", {"target_surface": "sampled", "target_fscore": None, "target_mesh": None},
        # options of "target", which runs the measure: checked, never switched on; --target-mesh is among the options because
        # the two are valid only with it ("target", which comes first, speaks for --target-mesh itself)
        on=lambda o: False, any_option=True,
        valid=_target_surface_valid,
        invalid=lambda o: ("--target-surface / --target-fscore need --target-mesh PATH" if not o["target_mesh"] else
                           "--target-surface must be sampled or exact, and --target-fscore T1,T2,... (thresholds finite and > 0) "
                           "needs --target-surface exact")),
    "render": Feature(
        "--render-views", {"render_views": 0, "render_size": 800}, on=lambda o: int(o["render_views"]),
        valid=lambda o: int(o["render_views"]) >= 0 and 1 <= int(o["render_size"]) <= 16384,
        invalid=lambda o: "--render-views must be >= 0 and --render-size in [1, 16384]"),
    "render_ssim": Feature(
        "--render-ssim", {"render_ssim": False, "render_views": 0, "render_size": 800}, on=lambda o: bool(o["render_ssim"]),
        valid=lambda o: int(o["render_views"]) > 0 and int(o["render_size"]) >= hip_ops.SSIM_WINDOW,
        invalid=lambda o: f"--render-ssim needs --render-views N > 0 and --render-size >= {hip_ops.SSIM_WINDOW}"),
    "texture": Feature(
        "--texture-res", {"texture_res": 0}, on=lambda o: int(o["texture_res"]),
        valid=lambda o: 1 <= int(o["texture_res"]) <= hip_ops.TEXTURE_MAX_RES,
        invalid=lambda o: f"--texture-res must be in [0, {hip_ops.TEXTURE_MAX_RES}], got {int(o['texture_res'])}"),
}


def check_features(args):
    """Every record of FEATURES against `args`: a feature whose options are set refuses --route script, then range-checks them
    (ValueError).  -> the names of the features that are switched on."""
    script = getattr(args, "route", "kernel") == "script"
    on = set()
    for name, feature in FEATURES.items():
        o = feature.values(args)
        if feature.checked(o):
            if script:
                verb = "have" if " / " in feature.what else "has"
                raise ValueError(f"{feature.what} {verb} no --route script: the reference's script {feature.script_has}")
            if not feature.valid(o):
                raise ValueError(feature.invalid(o))
        if feature.on(o):
            on.add(name)
    return on


def postprocess(vertices, triangles, normals, args):
    """The geometry stages of FEATURES that are switched on, in its order, on the mesh the geometry stage or the cache gave.
    Under torch.distributed every rank runs every stage on the gathered mesh redundantly."""
    for feature in FEATURES.values():
        o = feature.values(args)
        if feature.run is not None and feature.on(o):
            vertices, triangles, normals = feature.run(vertices, triangles, normals, o, args)
    return vertices, triangles, normals


def export_marching_cubes(model, args, cfg, device):
    """mesh_nerf.py:131-201.  `--super-sampling N >= 1` refines the geometry (extract_geometry_with_super_sampling); the
    appearance, the cache and the OBJ are the same steps as without it.  The optional additions are the records of FEATURES:
    all are checked before anything is read or written, and the geometry stages among them run right after the geometry stage
    or the cache load (postprocess).  The cache keeps the geometry as it was before them -- grid normals, unfiltered, unculled,
    unsmoothed, unsimplified --, so that they can be tuned on it.
    `--geometry tsdf` takes the geometry from depth maps of the network fused into a truncated signed distance field instead
    of from the density grid (extract_geometry_tsdf); everything after the geometry stage is the same.
    `--normals network` replaces the grid normals by the network's (network_normals) before the appearance query and the OBJ.
    `--texture-res N` bakes a texture atlas after the per-vertex appearance (bake_texture), which stays: the `v` lines keep
    their colours, so a viewer without textures still shows them; the OBJ gains `vt` lines, an .mtl and a .png."""
    geometry = extract_geometry_with_super_sampling if args.super_sampling >= 1 else extract_geometry
    on = check_features(args)
    if "tsdf" in on:                                       # `--geometry tsdf`: the same four values from the fused depth maps
        check_tsdf(args)
        geometry = lambda model, device, args: extract_geometry_tsdf(model, device, args, cfg)  # noqa: E731
    from . import dist as nd
    cache_path = os.path.join(args.save_dir, args.cache_name)
    load = args.use_cached_mesh and os.path.exists(cache_path)
    if load:
        print("Loading cached mesh geometry...")
        vertices, triangles, normals, density = torch.load(cache_path, weights_only=False)
        unprocessed = tuple(torch.as_tensor(t).to(device) for t in (vertices, triangles, normals))
    else:
        print("Generating mesh geometry...")
        vertices, triangles, normals, density = geometry(model, device, args)
        unprocessed = vertices, triangles, normals         # what the cache keeps
    vertices, triangles, normals = postprocess(*unprocessed, args)   # a stage that leaves nothing raises before anything is written
    if not load and (args.use_cached_mesh or args.override_cache_mesh):
        if nd.world()[1] > 1 and getattr(args, "gather", "triangles") == "triangles":
            density = _assemble_grid_from_slabs(density, _nums(args.res), device)   # the cache holds the whole grid
        if nd.world()[0] == 0:
            torch.save(tuple(t.cpu() for t in unprocessed) + (
                        density.cpu().numpy() if isinstance(density, torch.Tensor) else density,), cache_path)
            print(f"Cached mesh geometry saved to {cache_path}")

    if "target" in on:                                     # the geometry is final here: judge it before any ray is spent
        chamfer_to_target(vertices, triangles, args, device)

    # Appearance: one query per vertex.  Vertices are independent, so under torch.distributed every rank queries a
    # contiguous range of them and one ragged all-gather assembles the (V,3) colours; rank 0 writes the file.
    rank, world = nd.world()
    lo, hi, counts = nd.own_range(vertices.shape[0])
    if "normals" in on:
        # the fp32 handle whatever --precision is (as the geometry); every rank its own vertex range, one ragged all-gather
        # (the fallback flag travels as a 4th column)
        own, kept = network_normals(model.get_model().hip("f32"), vertices[lo:hi], normals[lo:hi])
        rows = nd.all_gather_rows(torch.cat((own, kept[:, None].to(own.dtype)), dim=1).contiguous(), counts)
        normals = rows[:, :3].contiguous()
        print(f"Network normals: {int(rows[:, 3].sum())} of {vertices.shape[0]} vertices kept their grid normal "
              "(zero or non-finite gradient)")
    if getattr(args, "precision", "f32") != "f32":     # the geometry above is fp32 by contract; only the colours may use the mode
        model.set_precision(args.precision)
    targets, directions = vertices[lo:hi], -normals[lo:hi]
    # --batch-size bounds the reference's per-call memory (default 1024); on a 288 GB device the per-call overhead
    # of a 1024-ray launch sequence dominates, so at least 65 536 vertices go into one call
    chunk = max(int(args.batch_size), 65536)
    script = getattr(args, "route", "kernel") == "script"
    if script:
        if world > 1:
            raise ValueError("--route script is the unmodified script's single-process call sequence: run it on one rank")
        chunk = int(args.batch_size)                       # the script's calls as they are (mesh_nerf.py:172-191), D2H per batch
    diffuse = query_appearance(model, args, targets, directions, device, chunk, to_host=script)
    diffuse = torch.cat(diffuse, dim=0) if diffuse else torch.empty(0, 3, dtype=torch.float32, device=device)
    diffuse = nd.all_gather_rows(diffuse.contiguous(), counts).cpu().numpy()
    texture = bake_texture(model, vertices, triangles, normals, args, device, chunk) if "texture" in on else None
    if getattr(args, "precision", "f32") != "f32":
        model.set_precision("f32")
    path = os.path.join(args.save_dir, args.mesh_name)
    if rank == 0 and texture is None:
        export_obj(vertices.cpu(), triangles.cpu(), diffuse, normals.cpu(), path)
    elif rank == 0:
        export_obj_textured(vertices.cpu(), triangles.cpu(), diffuse, normals.cpu(), texture[0], texture[1], path)
    if "render" in on:
        render_report(model, vertices, triangles, diffuse, args, cfg, device, texture=texture)
    return vertices, triangles, normals, diffuse


def query_appearance(model, args, targets, directions, device, chunk, to_host=False, announce=True):
    """The colour the network gives each of `targets` (N,3) seen along `directions` (N,3), in calls of `chunk` points: the
    colour branch at the point itself under --no-view-dependence, else a full render of the short ray that starts
    --view-disparity in front of the point.  Vertices and texels both come through here.  -> the list of the calls' (n,3)
    results (to_host: each copied to the host as soon as it is there, the script route's D2H per batch)."""
    keep = (lambda t: t.cpu()) if to_host else (lambda t: t)
    colours = []
    if args.no_view_dependence:
        if announce:
            print("Diffuse map query directly  without specific-views...")
        for pos, dirs in batchify(targets, directions, batch_size=chunk, device=device, progress=False):
            colours.append(keep(model.sample_points(pos, dirs)[..., :3]))
    else:
        if announce:
            print("Diffuse map query with view dependence...")
        ray_bounds = torch.tensor([0.0, args.view_disparity_max_bound], dtype=directions.dtype)
        ray_origins = targets - args.view_disparity * directions
        for o, d in batchify(ray_origins, directions, batch_size=chunk, device=device, progress=False):
            colours.append(keep(model.query((o, d, ray_bounds)).rgb_map))
    return colours


TEXTURE_WINDOW_SAMPLES = 1 << 22        # samples generated and queried at a time: 48 MB of positions, as much of directions


def bake_texture(model, vertices, triangles, normals, args, device, chunk):
    """`--texture-res N`: the atlas of per-face charts ("Texture atlas") baked from the network.  The surface
    samples behind the texels are generated (hip_ops.mesh_texture_samples) and queried (query_appearance, the vertices' own
    query) in windows of whole faces, so the positions of all samples are never resident at once; the (F*T, 3) colours stay on
    the device.  Under torch.distributed every rank takes a contiguous face range and one all-gather assembles the colours;
    every rank then fills the atlas redundantly.  -> (face_uv (F,3,2) f32, atlas (H,W,3) uint8), both on the device."""
    from . import dist as nd
    n = int(args.texture_res)
    faces = triangles.to(device=device, dtype=torch.int32).contiguous()
    num_faces = int(faces.shape[0])
    layout = hip_ops.mesh_texture_layout(num_faces, n)                # ValueError: no face, or an atlas wider than 16384
    per_face = layout["samples_per_face"]
    vertices, normals = vertices.to(device), normals.to(device=device, dtype=torch.float32)
    lo, hi, counts = nd.own_range(num_faces)
    step = max(1, TEXTURE_WINDOW_SAMPLES // per_face)
    colours = torch.empty((hi - lo) * per_face, 3, dtype=torch.float32, device=device)
    fallback = bad = 0
    for first in range(lo, hi, step):
        count = min(step, hi - first)
        positions, directions, fb, bd = hip_ops.mesh_texture_samples(vertices, faces, normals, n, first, count, flip=SMOOTH_FLIP)
        fallback, bad = fallback + fb, bad + bd
        parts = query_appearance(model, args, positions, directions, device, chunk, announce=False)
        colours[(first - lo) * per_face:(first - lo + count) * per_face] = torch.cat(parts, dim=0)
    colours = nd.all_gather_rows(colours, [c * per_face for c in counts])
    tally = nd.all_gather_rows(torch.tensor([[fallback, bad]], dtype=torch.int64, device=device), [1] * len(counts)).sum(0).tolist()
    atlas = hip_ops.mesh_texture_fill(colours, num_faces, n)
    face_uv = hip_ops.mesh_texture_uv(num_faces, n, device=device)
    print(f"Texture atlas: {layout['width']} x {layout['height']} texels ({layout['cols']} x {layout['rows']} cells of {n + 3} x "
          f"{n + 2}) for {num_faces} faces at --texture-res {n}: {num_faces * per_face} samples, {int(tally[0])} with the face's "
          f"own normal (no usable vertex normal), {int(tally[1])} on faces with a bad index")
    return face_uv, atlas


def render_report(model, vertices, triangles, diffuse, args, cfg, device, texture=None):
    """`--render-views N`: the exported mesh drawn from N orbit poses at --render-size (mesh_render.evaluate) against the
    network's own render of each pose -- PSNR, depth difference, silhouette IoU --, printed; rank 0 writes
    <save-dir>/<mesh-name stem>.render.json.  Under torch.distributed the views are dealt out over the ranks.  With
    `--texture-res` the numbers describe the textured mesh, and the per-vertex colours' PSNR of the same views (one
    rasterisation, one network render) stands beside them.  `--render-ssim` adds the structural similarity to the network's render
    (mesh_render.SSIM_ROW) to every view and to the means."""
    from . import dist as nd
    from . import mesh_render, synthetic
    if not (hasattr(model, "can_query_view") and model.can_query_view()):
        raise ValueError("--render-views needs a model that renders a view from its pose (query_view)")
    size = int(args.render_size)
    views = mesh_render.orbit_views(int(args.render_views), size, size, synthetic.LEGO_FOCAL_800 * size / 800.0)
    bounds = torch.tensor([cfg.dataset.near, cfg.dataset.far], dtype=torch.float32)
    background = (1.0,) * 3 if cfg.dataset.white_background else (0.0,) * 3
    report = mesh_render.evaluate(vertices, triangles.to(torch.int32), torch.as_tensor(diffuse), views, cfg.dataset.near / 4,
                                  background, model=model, bounds=bounds, chunksize=cfg.nerf.validation.chunksize,
                                  compare_nerf=True, device=device, texture=texture, vertex_too=texture is not None,
                                  ssim=bool(getattr(args, "render_ssim", False)))
    if texture is not None:
        report["mesh"] = dict(appearance="texture", atlas=dict(width=int(texture[1].shape[1]), height=int(texture[1].shape[0])),
                              texture_res=int(args.texture_res))
    for line in mesh_render.format_report(report):
        print(line)
    if nd.world()[0] == 0:
        path = os.path.join(args.save_dir, os.path.splitext(args.mesh_name)[0] + ".render.json")
        mesh_render.write_report(report, path)
        print(f"Mesh render report saved to {path}")
    return report


def _non_negative(text):
    n = int(text)
    if n < 0:
        raise argparse.ArgumentTypeError(f"must be >= 0, got {n}")
    return n


def _cell_size(text):
    k = float(text)
    if not 0.0 <= k < float("inf"):                        # a NaN fails both comparisons
        raise argparse.ArgumentTypeError(f"must be finite and >= 0, got {text}")
    return k


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--log-checkpoint", type=str, default=None)
    p.add_argument("--checkpoint", type=str, default="model_last.ckpt")
    p.add_argument("--save-dir", type=str, default=".")
    p.add_argument("--mesh-name", type=str, default="mesh.obj")
    p.add_argument("--iso-level", type=float, default=32)
    p.add_argument("--limit", type=float, default=1.2)
    p.add_argument("--res", type=int, default=128)
    p.add_argument("--super-sampling", type=int, default=0)
    p.add_argument("--batch-size", type=int, default=1024)
    p.add_argument("--no-view-dependence", action="store_true", default=False)
    p.add_argument("--view-disparity", type=float, default=1e-2)
    p.add_argument("--view-disparity-max-bound", type=float, default=4e0)
    p.add_argument("--use-cached-mesh", action="store_true", default=False)
    p.add_argument("--override-cache-mesh", action="store_true", default=False)
    p.add_argument("--cache-name", type=str, default="mesh_cache.pt")
    p.add_argument("--precision", choices=("f32", "bf16x3"), default="f32",
                   help="(addition) arithmetic of the per-vertex appearance re-query; the density grid -- hence the mesh topology "
                        "-- is always computed in fp32")
    p.add_argument("--route", choices=("kernel", "script"), default="kernel",
                   help="(addition) kernel: one density-grid launch, GPU statistics and marching cubes (default); script: the "
                        "unmodified script's own call sequence -- sample_points + D2H per --batch-size points, numpy iso level, "
                        "skimage.measure.marching_cubes, the re-query in --batch-size calls (single process)")
    p.add_argument("--normals", choices=("grid", "network"), default="grid",
                   help="(addition) vertex normals of the appearance rays and the OBJ: grid (default) -- marching cubes' "
                        "gradient of the density grid -- or network: -grad sigma / |grad sigma| of the network at the final "
                        "vertices")
    p.add_argument("--min-component-faces", type=_non_negative, default=0,
                   help="(addition) drop every connected component of the mesh with fewer than this many triangles (0 = off)")
    p.add_argument("--keep-largest", type=_non_negative, default=0,
                   help="(addition) of the components left, keep only this many with the most triangles, ties going to the one "
                        "that holds the smaller vertex index (0 = off)")
    p.add_argument("--simplify-cell", type=_cell_size, default=0.0,
                   help="(addition) simplify the mesh by vertex clustering: the vertices in one cell of a grid of this many voxels "
                        "per edge become their mean, degenerate and duplicate triangles go; after the component filter, before "
                        "the normals and the appearance query (0 = off)")
    p.add_argument("--simplify-placement", choices=["mean", "quadric"], default="mean",
                   help="(addition) where --simplify-cell puts the vertex of a cell with several: mean (default) is their exact "
                        "mean; quadric is the point of the cell nearest to the planes of the triangles around it (exact integer "
                        "quadrics, a regularised 3 x 3 solve per cell), which keeps creases and curved surfaces where they are; "
                        "needs --simplify-cell")
    p.add_argument("--simplify-levels", type=_non_negative, default=0,
                   help="(addition) adaptive clustering: also cluster on this many coarser grids, each of twice the cell before, "
                        "and let every vertex join the coarsest cell whose vertex lies within --simplify-error of every triangle "
                        "plane around it; at most 8; needs --simplify-cell and --simplify-placement quadric (0 = off)")
    p.add_argument("--simplify-error", type=_cell_size, default=SIMPLIFY_ERROR_DEFAULT,
                   help="(addition) the error bound of --simplify-levels in voxels, finite and >= 0 (default "
                        f"{SIMPLIFY_ERROR_DEFAULT}: half of the half-voxel distance the surface reports score at); read only with "
                        "--simplify-levels > 0")
    p.add_argument("--cull-hidden-views", type=_non_negative, default=0,
                   help="(addition) drop the faces no outside camera sees: rasterise the mesh on the GPU from this many cameras "
                        "spread evenly over a sphere around it and keep the faces that win a pixel in at least one view; after "
                        "the component filter, before --smooth-iters, --simplify-cell and the appearance query; writes "
                        "<save-dir>/<mesh-name stem>.visibility.json (0 = off)")
    p.add_argument("--cull-size", type=_non_negative, default=0,
                   help="(addition) side in pixels of the --cull-hidden-views images; 0 (default): the smallest multiple of 256 "
                        "that gives every voxel at least 2 pixels, at most 16384")
    p.add_argument("--cull-rings", type=_non_negative, default=1,
                   help="(addition) rounds in which the faces that share a vertex with a kept face are kept too: the faces too "
                        "small to win a pixel centre next to visible ones (0: exactly the faces that won a pixel)")
    p.add_argument("--cull-radius", type=float, default=3.0,
                   help="(addition) distance of the --cull-hidden-views cameras from the centre of the mesh's bounding box, in "
                        "bounding radii; finite and > 1")
    p.add_argument("--smooth-iters", type=_non_negative, default=0,
                   help="(addition) smooth the mesh with this many iterations of Taubin's lambda | mu filter on the GPU: after "
                        "the component filter, before --simplify-cell, the normals and the appearance query; the vertex normals "
                        "are recomputed from the smoothed triangles (0 = off)")
    p.add_argument("--smooth-lambda", type=float, default=0.5,
                   help="(addition) factor of the first, shrinking half-step of every --smooth-iters iteration, in (0, 1]")
    p.add_argument("--smooth-mu", type=float, default=-0.53,
                   help="(addition) factor of the second, inflating half-step, in [-1, 0]; 0 skips it: plain Laplacian smoothing")
    p.add_argument("--smooth-boundary", choices=("fixed", "free"), default="fixed",
                   help="(addition) fixed (default): the vertices on an open edge of the mesh, where the grid box clips it, stay "
                        "in place; free: they move like any other vertex")
    p.add_argument("--target-mesh", type=str, default=None,
                   help="(addition) an OBJ file: print the chamfer distance between the extracted mesh and it (sampled and searched "
                        "on the GPU, world coordinates) and write <save-dir>/<mesh-name stem>.chamfer.json")
    p.add_argument("--chamfer-samples", type=int, default=100000, help="(addition) points sampled on each mesh for --target-mesh")
    p.add_argument("--chamfer-seed", type=int, default=0, help="(addition) seed of the device generator the samples are drawn from")
    p.add_argument("--target-surface", type=str, default="sampled",
                   help="(addition) sampled (default): --target-mesh compares two samplings; exact: every sample against the other "
                        "mesh's triangles (mesh_chamfer --surface exact), which adds accuracy / completeness, Hausdorff and normal "
                        "consistency to the report")
    p.add_argument("--target-fscore", type=str, default=None, metavar="T1,T2,...",
                   help="(addition) distance thresholds in world units for precision / recall / F-score against --target-mesh; "
                        "needs --target-surface exact")
    p.add_argument("--render-views", type=_non_negative, default=0,
                   help="(addition) after the OBJ is written, draw the mesh from this many orbit poses on the GPU and report it "
                        "against the network's own render of each pose: PSNR, depth difference, silhouette IoU; writes "
                        "<save-dir>/<mesh-name stem>.render.json (0 = off)")
    p.add_argument("--render-size", type=int, default=800, help="(addition) side in pixels of the --render-views images")
    p.add_argument("--render-ssim", action="store_true", default=False,
                   help="(addition) with --render-views: the structural similarity (SSIM, 11-tap Gaussian window) of every mesh "
                        "image to the network's render too, per view and in the means of <stem>.render.json")
    p.add_argument("--texture-res", type=_non_negative, default=0,
                   help="(addition) bake a texture atlas from the network: every face gets a chart of this many lattice "
                        "intervals per triangle side, (N+1)(N+2)/2 samples queried like the vertices; writes <stem>.obj with "
                        "vt lines, <stem>.mtl and <stem>.png, and --render-views scores the textured mesh (0 = off)")
    p.add_argument("--geometry", choices=("density", "tsdf"), default="density",
                   help="(addition) where the surface comes from: density (default) -- the density grid thresholded at --iso-level "
                        "-- or tsdf: the network's depth rendered from --tsdf-views cameras all around the volume, fused into a "
                        "truncated signed distance field on the --res grid on the GPU and meshed at its zero level; writes "
                        "<save-dir>/<mesh-name stem>.tsdf.json")
    p.add_argument("--tsdf-views", type=int, default=32, help="(addition) cameras of --geometry tsdf, spread evenly over a sphere")
    p.add_argument("--tsdf-size", type=int, default=800, help="(addition) side in pixels of the square depth images")
    p.add_argument("--tsdf-radius", type=float, default=4.0, help="(addition) radius of the camera sphere around the origin")
    p.add_argument("--tsdf-focal", type=float, default=0.0, help="(addition) focal length in pixels; 0 (default): 1111.1111 * size / 800")
    p.add_argument("--tsdf-trunc", type=float, default=3.0,
                   help="(addition) truncation distance of the field, in voxels of the --res grid")
    p.add_argument("--tsdf-min-opacity", type=float, default=0.5,
                   help="(addition) a ray counts as having hit a surface when its accumulated opacity is at least this")
    p.add_argument("--tsdf-level", type=float, default=0.0, help="(addition) level of the fused field handed to marching cubes, in (-1, 1)")
    p.add_argument("--gather", choices=("triangles", "grid"), default="triangles",
                   help="(addition, multi-GPU) what travels between the ranks: the emitted triangles of per-slab marching "
                        "cubes (default) or the density grid")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    path_parser = PathParser()
    cfg, _ = path_parser.parse(None, args.log_checkpoint, None, args.checkpoint)
    if not torch.cuda.is_available():
        raise SystemExit("mesh_nerf needs a MI355X: the HIP path has no CPU fallback")
    from . import dist as nd
    rank, world, device = nd.init_from_env()          # one process per GPU under torch.distributed.run
    print(f"Loading model from {path_parser.checkpoint_path}")
    model = getattr(models, cfg.experiment.model).load_from_checkpoint(path_parser.checkpoint_path)
    model = model.eval().to(device)
    try:
        with torch.no_grad():
            return export_marching_cubes(model, args, cfg, device)
    finally:
        nd.shutdown()


if __name__ == "__main__":
    main()
