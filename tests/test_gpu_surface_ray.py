"""GPU: the surface point cloud (mesh_surface_ray).  (1) The filter + ordered compaction kernels against the restated
reference filter (tests/surface_filter.py) bit for bit; (2) the reference rule end to end on the device's own renders;
(3) the well-conditioned rule (min_opacity 0.99) against the CPU oracle's render; (4) 2 / 3 / more ranks than views against
one rank, PLY files byte for byte; (5) the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nerfmeshes_amd import synthetic as S
from tests import surface_filter as SF
from tests.gpu_support import assert_ranks_ok, clean_env, launch_ranks, scene_model
from tests.gpu_support import ops  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (3, 7), (97, 131), (800, 800)]       # no multiple of the 16 x 64 tile; smaller than the halo


# ---- inputs (CPU tensors; a case = origins (1|H*W, 3), dirs (H, W, 3), depth (H, W), dist_threshold) ----------------------

def _camera_rays(ops, H, W):
    """real rays of the orbit camera, as hip_ops.view_rays generates them (focal chosen so that the object fills the view)"""
    view = ops.make_view(S.pose_spherical(30.0, -30.0, 4.0), H, W, 1.2 * max(H, W))
    o, d = ops.view_rays(view)
    return o[:1].cpu(), d.cpu().reshape(H, W, 3)


def _plane(ops, H, W):
    """a tilted plane through the origin: the spacing of the surface points grows with the depth across the image, and the
    limit is set to what the 21 nearest offsets of the 5 x 5 window need at the centre's spacing"""
    o, d = _camera_rays(ops, H, W)
    n = torch.tensor([0.9, 0.3, 0.5])
    n = n / n.norm()
    t = -(o[0] @ n) / (d @ n)
    spacing = float(t[H // 2, W // 2]) / (1.2 * max(H, W))
    return o, d, t, 5.2 * spacing ** 2


def _sphere(ops, H, W):
    """the unit sphere at the origin; rays that miss it have depth 0"""
    o, d = _camera_rays(ops, H, W)
    b = d @ o[0]
    disc = b * b - (o[0] @ o[0] - 1.0)
    t = torch.where(disc > 0, -b - disc.clamp(min=0).sqrt(), torch.zeros_like(b))
    return o, d, t, 12.0 * (3.0 / (1.2 * max(H, W))) ** 2


def _lattice(H, W, seed):
    """per-ray origins on a fine lattice, directions near +z (normalised): no camera"""
    g = torch.Generator().manual_seed(seed)
    rows, cols = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    o = torch.stack((cols * 1e-3, rows * 1e-3, torch.zeros(H, W)), -1).float().reshape(-1, 3)
    d = torch.tensor([0.0, 0.0, 1.0]) + 0.01 * torch.randn(H, W, 3, generator=g)
    return o, (d / d.norm(dim=-1, keepdim=True)).contiguous(), g


def _noise(H, W, seed=1, sigma=0.022, negative=0.15):
    """depth 1 + N(0, sigma): a neighbour votes with probability ~0.8 at the default limit (sqrt(0.002) = 0.045 against a
    difference of N(0, 2 sigma^2)); `negative` of the pixels get their depth negated (never kept, out of reach as voters)"""
    o, d, g = _lattice(H, W, seed)
    depth = 1.0 + sigma * torch.randn(H, W, generator=g)
    depth = torch.where(torch.rand(H, W, generator=g) < negative, -depth, depth)
    return o, d, depth, 0.002


def _steps(H, W, seed=2):
    """depth levels that change exactly at the tile borders (16 rows, 64 columns) and one pixel beside them"""
    o, d, g = _lattice(H, W, seed)
    rows, cols = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    level = ((rows // 16) + (cols // 64) + ((rows + 1) // 16) + ((cols - 1).clamp(min=0) // 64)) % 3
    return o, d, 1.0 + 0.25 * level.float(), 0.002


def _specials(H, W, seed=3):
    """the noise case with NaN, infinite, zero and negative depths sprinkled in"""
    o, d, depth, thr = _noise(H, W, seed, negative=0.0)
    g = torch.Generator().manual_seed(seed + 100)
    u = torch.rand(H, W, generator=g)
    depth = torch.where(u < 0.03, torch.full_like(depth, float("nan")), depth)
    depth = torch.where((u >= 0.03) & (u < 0.06), -depth, depth)
    depth = torch.where((u >= 0.06) & (u < 0.09), torch.zeros_like(depth), depth)
    depth = torch.where((u >= 0.09) & (u < 0.10), torch.full_like(depth, float("inf")), depth)
    return o, d, depth, thr


def _rgb(H, W, seed=7):
    g = torch.Generator().manual_seed(seed)
    rgb = 1.2 * torch.rand(H * W, 3, generator=g) - 0.1              # a little outside [0, 1]: the clamp of the uchar colours
    if H * W > 5:
        rgb[3, 1] = float("nan")
    return rgb


def _check(ops, case, step, prob=0.6, opacity=None, min_opacity=None, share=None):
    """HIP against the restated filter on identical inputs, bit for bit: votes, mask, count, and the gathered rows in order"""
    o, d, depth, thr = case
    H, W = depth.shape
    rgb = _rgb(H, W)
    votes, keep, points, normals = SF.surface_filter(o.reshape(-1, 3) if o.shape[0] == 1 else o.reshape(H, W, 3), d, depth, step,
                                                     thr, prob, opacity, min_opacity)
    flt = ops.surface_filter(o.cuda(), d.cuda(), depth.cuda(), H, W, step=step, dist_threshold=thr,
                             min_votes=ops.surface_min_votes(step, prob),
                             opacity=None if opacity is None else opacity.cuda(), min_opacity=min_opacity)
    assert flt["votes"].dtype == torch.int32 and flt["keep"].dtype == torch.bool
    assert torch.equal(flt["votes"].cpu().long(), votes), "votes"
    assert torch.equal(flt["keep"].cpu(), keep), "keep mask"
    n = int(keep.sum())
    assert int(flt["count"].item()) == n
    gp, gn, gc, gu = ops.surface_gather(flt, rgb.cuda())
    assert gp.shape == (n, 3) and gu.dtype == torch.uint8

    def bits(t):
        return t.contiguous().cpu().numpy().view(np.uint32)

    want_rgb = rgb[keep.reshape(-1)]
    assert np.array_equal(bits(gp), bits(points)), "points and their order"
    assert np.array_equal(bits(gn), bits(normals)), "normals"
    assert np.array_equal(bits(gc), bits(want_rgb)), "colours"
    assert np.array_equal(gu.cpu().numpy(), SF.color_bytes(want_rgb)), "uchar colours"
    frac = n / float(H * W)
    print(f"{H}x{W} step {step}: kept {n} of {H * W} ({frac:.3f})")
    if share:
        assert 0.10 <= frac <= 0.90, f"the case is trivial: kept share {frac}"
    return frac


# ---- 1. the stage, bit for bit ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("step", [0, 1, 2, 3])
def test_noise_every_size_and_step(ops, H, W, step):
    """per-ray origins.  The kept share is asserted on the images large enough for a share to mean something (a 1 x 1 or
    3 x 7 image is there for the halo and the bounds, not for statistics)."""
    _check(ops, _noise(H, W), step, share=H * W >= 1000)


@pytest.mark.parametrize("H,W", [(1024, 64), (1025, 64), (41, 1601)])
def test_noise_at_the_chunk_boundaries_of_the_scan(ops, H, W):
    """1024, 1025 and 1066 words of keep bits: exactly one full chunk of the one-workgroup scan (csrc/compact.h), the first
    word of the second chunk, where the carry is handed over, and a second chunk of 42 words that is a single partial wave.
    (The 800 x 800 image of SIZES has 10 400 words: the carry is carried ten times there.)"""
    assert H * ((W + 63) // 64) in (1024, 1025, 1066)
    _check(ops, _noise(H, W), 1, share=True)


@pytest.mark.parametrize("H,W", SIZES[2:])
@pytest.mark.parametrize("shape", ["plane", "sphere"])
def test_plane_and_sphere_on_real_rays(ops, shape, H, W):
    """shared origin, rays from hip_ops.view_rays; the reference's window (step 2, 0.6)"""
    _check(ops, (_plane if shape == "plane" else _sphere)(ops, H, W), 2, share=True)


@pytest.mark.parametrize("H,W", SIZES)
def test_real_rays_small_and_degenerate_depths(ops, H, W):
    o, d = _camera_rays(ops, H, W)
    frac = _check(ops, (o, d, torch.zeros(H, W), 0.002), 2)
    assert frac == 0.0, "all-zero depth: every point is the camera centre, all vote, none is kept"
    for step in (1, 3):
        _check(ops, _plane(ops, H, W), step)
        _check(ops, _sphere(ops, H, W), step)


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("step", [1, 2, 3])
def test_nan_negative_and_depth_steps_across_tile_borders(ops, H, W, step):
    _check(ops, _specials(H, W), step)
    _check(ops, _steps(H, W), step)
    o, d, depth, thr = _steps(H, W)
    _check(ops, (o[:1], d, depth, thr), step)                              # the same directions from one shared origin


@pytest.mark.parametrize("H,W", SIZES[1:])
def test_with_opacity(ops, H, W):
    o, d, depth, thr = _noise(H, W, seed=5, negative=0.0)
    g = torch.Generator().manual_seed(11)
    acc = torch.rand(H, W, generator=g)
    acc[0, 0] = float("nan")
    limit = 0.15
    acc.view(-1)[1] = float(np.float32(limit))                                  # fp32(0.15) > 0.15: equal after the rounding, passes
    frac = _check(ops, (o, d, depth, thr), 2, opacity=acc, min_opacity=limit, share=H * W >= 1000)
    full = _check(ops, (o, d, depth, thr), 2)
    assert frac <= full
    _check(ops, _sphere(ops, H, W)[:3] + (0.002,), 1, opacity=acc, min_opacity=0.5)      # shared origin, real rays


@pytest.mark.parametrize("thr,votes", [(0.25 + 1e-10, 6), (0.25 - 1e-10, 6), (0.2500001, 9), (0.002, 6)])
def test_threshold_is_compared_in_fp32(ops, thr, votes):
    """two points exactly 0.5 apart: `fp32 tensor < Python float` rounds the limit to fp32 once -- 0.25 + 1e-10 (fp32 below the
    double) and 0.25 - 1e-10 (fp32 above it) both become 0.25, which 0.25 is not below"""
    o = torch.zeros(1, 3)
    d = torch.tensor([[[0.0, 0.0, 1.0], [0.5, 0.0, 1.0]]])
    depth = torch.ones(1, 2)
    _check(ops, (o, d, depth, thr), 1, prob=0.0)
    flt = ops.surface_filter(o.cuda(), d.cuda(), depth.cuda(), 1, 2, step=1, dist_threshold=thr, min_votes=1)
    assert flt["votes"].cpu().tolist() == [[votes, votes]]


@pytest.mark.parametrize("step,prob", [(1, 0.625), (1, 0.6249999), (3, 0.5), (3, 0.4999999), (2, 0.6)])
def test_vote_limit_at_and_next_to_an_integer(ops, step, prob):
    _check(ops, _noise(97, 131, seed=9), step, prob=prob)


def test_entries_can_be_captured_in_a_graph(ops):
    """no allocation and no synchronisation inside the entries: filter + gather replayed from a captured graph on new inputs"""
    o, d, depth, thr = _noise(97, 131, seed=4)
    H, W = depth.shape
    rgb = _rgb(H, W).cuda()
    oc, dc, zc = o.cuda(), d.cuda(), depth.cuda()
    first = ops.surface_filter(oc, dc, zc, H, W, step=2, dist_threshold=thr, min_votes=15)
    n = int(first["count"].item())
    want = ops.surface_gather(first, rgb)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            flt = ops.surface_filter(oc, dc, zc, H, W, step=2, dist_threshold=thr, min_votes=15)
            got = ops.surface_gather(flt, rgb, count=n)
    zc.copy_(torch.zeros_like(zc))
    graph.replay()
    torch.cuda.synchronize()
    assert int(flt["count"].item()) == 0
    zc.copy_(depth.cuda())
    graph.replay()
    torch.cuda.synchronize()
    assert int(flt["count"].item()) == n
    for a, b in zip(got, want):                                            # bytes: the colours hold a NaN
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_gather_at_a_row_offset_and_within_the_capacity(ops):
    """the C entry appends a view's rows at a caller-given offset of larger arrays and never writes past `capacity` rows"""
    import ctypes as C
    from nerfmeshes_amd import _lib
    o, d, depth, thr = _noise(97, 131, seed=6)
    H, W = depth.shape
    rgb = _rgb(H, W).cuda()
    flt = ops.surface_filter(o.cuda(), d.cuda(), depth.cuda(), H, W, step=2, dist_threshold=thr, min_votes=15)
    n = int(flt["count"].item())
    want = ops.surface_gather(flt, rgb)
    lib, P = _lib.load(), (lambda t: C.c_void_p(t.data_ptr()))
    for offset, capacity in ((5, n + 9), (3, n - 40), (0, n), (n + 2, n + 2)):
        outs = [torch.full((n + 9, 3), -7.0, device="cuda") for _ in range(3)] + [torch.full((n + 9, 3), 9, dtype=torch.uint8, device="cuda")]
        rc = lib.nm_surface_gather(P(flt["workspace"]), P(flt["origins"]), flt["per_ray_o"], P(flt["dirs"]), P(flt["depth"]), None,
                                   0.0, P(rgb), H, W, offset, capacity, *[P(t) for t in outs], None)
        assert rc == 0
        torch.cuda.synchronize()
        rows = max(0, min(n, capacity - offset))
        for got, ref, fill in zip(outs, want, (-7.0, -7.0, -7.0, 9)):
            assert got[offset:offset + rows].cpu().numpy().tobytes() == ref[:rows].cpu().numpy().tobytes()
            assert bool((got[:offset] == fill).all()) and bool((got[offset + rows:] == fill).all()), "nothing outside the rows"


# ---- 2. the reference rule end to end on the device -------------------------------------------------------------------------

def _model(weights, **hparams):
    return scene_model("cuda", weights=weights, **hparams)


@pytest.fixture(scope="module")
def scene():
    return _model(S.make_scene_weights(), chunksize=3000)


def _args(tmp_path, *extra):
    from nerfmeshes_amd import mesh_surface_ray as msr
    return msr.build_parser().parse_args(["--save-dir", str(tmp_path), *extra])


def _restated_views(model, args, min_opacity=None):
    """the restated filter applied to the device's own query_view outputs, view after view"""
    from nerfmeshes_amd import hip_ops, mesh_surface_ray as msr
    size = args.img_size
    pts, nrm, col = [], [], []
    bounds = torch.tensor([model.cfg.dataset.near, model.cfg.dataset.far])
    for pose in msr.render_poses(args):
        with torch.no_grad():
            out = model.query_view(torch.from_numpy(pose), size, size, args.focal, bounds, keep_depth=min_opacity is not None)
        o, d = hip_ops.view_rays(hip_ops.make_view(pose, size, size, args.focal))
        depth = out.depth_map.cpu().reshape(size, size)
        acc = out.acc_map.cpu().reshape(size, size) if min_opacity is not None else None
        _, keep, p, n = SF.surface_filter(o[:1].cpu(), d.cpu().reshape(size, size, 3), depth, args.step_size, args.dist_threshold,
                                          args.prob_threshold, acc, min_opacity)
        pts.append(p)
        nrm.append(n)
        col.append(out.rgb_map.cpu()[keep.reshape(-1)])
    return torch.cat(pts).numpy(), torch.cat(nrm).numpy(), torch.cat(col).numpy()


@pytest.mark.parametrize("rule", ["reference", "min_opacity"])
def test_export_ray_trace_equals_the_restated_filter_on_the_device_renders(ops, scene, tmp_path, rule):
    from nerfmeshes_amd import mesh_surface_ray as msr
    extra = ["--min-opacity", "0.99"] if rule == "min_opacity" else []
    args = _args(tmp_path, "--views-y", "2", "--views-x", "1", "--img-size", "120", "--focal", str(1111.1111 * 120 / 800), *extra)
    with torch.no_grad():
        v, n, c, cu = msr.export_ray_trace(scene, args, scene.cfg, "cuda")
    wp, wn, wc = _restated_views(scene, args, 0.99 if extra else None)
    assert len(wp) > 200, "the views see the object"
    assert v.tobytes() == wp.tobytes() and n.tobytes() == wn.tobytes() and c.tobytes() == wc.tobytes()
    assert np.array_equal(cu, SF.color_bytes(wc))
    fmt, rp, rn, rc = SF.read_ply(tmp_path / "lego-sampling.ply")
    assert fmt == "ascii" and rp.tobytes() == v.tobytes() and rn.tobytes() == n.tobytes() and np.array_equal(rc, cu)


def test_models_without_the_view_render_are_refused(scene, tmp_path):
    from nerfmeshes_amd import mesh_surface_ray as msr
    args = _args(tmp_path, "--img-size", "16")
    with pytest.raises(RuntimeError, match="no fallback"):
        msr.export_ray_trace(torch.nn.Linear(1, 1), args, scene.cfg, "cuda")
    scene.train()
    try:
        assert not scene.can_query_view()          # the training config adds density noise
        with pytest.raises(RuntimeError, match="no fallback"):
            msr.export_ray_trace(scene, args, scene.cfg, "cuda")
    finally:
        scene.eval()


def test_keep_depth_changes_nothing_but_the_zeroing(scene):
    pose = torch.from_numpy(S.pose_spherical(30.0, -30.0, 4.0))
    bounds = torch.tensor([2.0, 6.0])
    with torch.no_grad():
        a = scene.query_view(pose, 64, 64, 90.0, bounds)
        b = scene.query_view(pose, 64, 64, 90.0, bounds, keep_depth=True)
    for name in ("rgb_map", "acc_map", "disp_map", "weights"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    zeroed = a.acc_map < 1.0
    assert bool(zeroed.any()) and bool((~zeroed).any())
    assert torch.equal(a.depth_map, torch.where(zeroed, torch.zeros_like(b.depth_map), b.depth_map))
    assert bool((b.depth_map[zeroed] > 0).any())


# ---- 3. against the CPU oracle under min_opacity = 0.99 ---------------------------------------------------------------------

TINY = dict(size=96, pose=(30.0, -30.0, 4.0), near=2.0, far=6.0, coarse=64, fine=128, min_opacity=0.99, band=1e-5)


def _oracle_view(w, kw):
    from oracle import nerf_oracle as O
    spec = O.MLPSpec(**kw)
    rs = O.RenderSpec(num_coarse=TINY["coarse"], num_fine=TINY["fine"], training=True)      # the un-zeroed depth
    size = TINY["size"]
    o, d = O.get_ray_bundle(size, size, 1111.1111 * size / 800, torch.from_numpy(S.pose_spherical(*TINY["pose"])))
    d = d.reshape(-1, 3)
    with torch.no_grad():
        parts = [O.query(w, w, spec, spec, rs, o[None], d[s:s + 2048], TINY["near"], TINY["far"]) for s in range(0, d.shape[0], 2048)]
    return o, d, {k: torch.cat([p[k] for p in parts]) for k in ("rgb_map", "depth_map", "acc_map")}


def _keep(o, d, depth, acc, thr_scale=1.0):
    size = TINY["size"]
    return SF.surface_filter(o[None], d.reshape(size, size, 3), depth.reshape(size, size), 2, 0.002 * thr_scale, 0.6,
                             acc.reshape(size, size), TINY["min_opacity"])


def _well_conditioned(o, d, b):
    """per pixel: its own acc farther than the band from the limit, and the same outcome under both extreme assignments of the
    rays inside the band and with the distance limit scaled by 0.99 and 1.01"""
    acc, lim, band = b["acc_map"], TINY["min_opacity"], TINY["band"]
    near_limit = (acc - lim).abs() <= band
    base = _keep(o, d, b["depth_map"], acc)[1]
    stable = ~near_limit.reshape(base.shape)
    for forced in (torch.where(near_limit, torch.full_like(acc, 1.0), acc), torch.where(near_limit, torch.zeros_like(acc), acc)):
        for scale in (0.99, 1.01):
            stable &= _keep(o, d, b["depth_map"], forced, scale)[1] == base
    return base, stable


def test_against_the_cpu_oracle_under_min_opacity(ops, tmp_path):
    """HIP render + HIP filter against oracle render + restated filter on the tiny_4x64 smooth scene: the keep masks agree on
    every well-conditioned pixel; the points of the pixels kept by both lie within 4x the oracle's own self-noise (the same
    network with its hidden units permuted: a different order of the same sums); colours within the render tests' parity bar.
    Figures go to profiles/r08_surface_ray.json through tests/tools/time_surface_ray.py (they are printed here)."""
    from oracle import parity
    from tests.golden.calibrate_scene import permute_hidden_units
    from nerfmeshes_amd import mesh_surface_ray as msr
    torch.set_num_threads(min(16, torch.get_num_threads()))
    w, kw = S.make_smooth_scene_weights("tiny_4x64")
    o, d, ref = _oracle_view(w, kw)
    base, stable = _well_conditioned(o, d, ref)
    share, kept_stable = float(stable.float().mean()), int((base & stable).sum())
    print(f"well-conditioned share {share:.4f}, kept and well conditioned {kept_stable}")
    assert share >= 0.99 and kept_stable >= 1000

    size = TINY["size"]
    model = _model(w, hidden_size=kw["hidden_size"], num_layers=kw["num_layers"], skip_step=kw["skip_step"],
                   num_encoding_fn_xyz=kw["num_encoding_fn_xyz"], num_encoding_fn_dir=kw["num_encoding_fn_dir"],
                   num_coarse=TINY["coarse"], num_fine=TINY["fine"], near=TINY["near"], far=TINY["far"])
    pose = S.pose_spherical(*TINY["pose"])
    args = _args(tmp_path, "--img-size", str(size), "--focal", str(1111.1111 * size / 800), "--min-opacity", str(TINY["min_opacity"]))
    with torch.no_grad():
        flt, out = msr.filter_view(model, pose, args, model.cfg)
        gp, _, gc, _ = ops.surface_gather(flt, out.rgb_map)
    keep_hip = flt["keep"].cpu()
    differ = (keep_hip != base) & stable
    print(f"HIP keeps {int(keep_hip.sum())}, oracle {int(base.sum())}; they differ on {int((keep_hip != base).sum())} pixels, "
          f"{int(differ.sum())} of them well conditioned")
    assert int(differ.sum()) == 0

    # the oracle's self-noise on this view: three permutations of the hidden units
    both = (keep_hip & base).reshape(-1)
    o3 = o[None].expand(d.shape[0], 3)
    pts_ref = o3 + d * ref["depth_map"][:, None]
    noise = 0.0
    for seed in (0, 1, 2):
        _, _, perm = _oracle_view(permute_hidden_units(w, kw["hidden_size"], kw["num_layers"], seed), kw)
        noise = max(noise, float((o3 + d * perm["depth_map"][:, None] - pts_ref)[both].norm(dim=1).max()))
    pts_hip = torch.zeros(size * size, 3)
    pts_hip[keep_hip.reshape(-1)] = gp.cpu()
    dist = float((pts_hip - pts_ref)[both].norm(dim=1).max())
    print(f"points kept by both: {int(both.sum())}; max distance HIP - oracle {dist:.3e}, oracle self-noise {noise:.3e}")
    assert noise > 0
    assert dist <= 4 * noise, (dist, noise)

    par = parity.psnr_parity(out.rgb_map.cpu(), ref["rgb_map"], chunk=2048)
    print("colours:", par)
    assert par["abs_dpsnr_db"] <= 1e-4 * max(1.0, 32768 / par["rays"]), par
    rgb_hip = torch.zeros(size * size, 3)
    rgb_hip[keep_hip.reshape(-1)] = gc.cpu()
    assert torch.equal(rgb_hip[both], out.rgb_map.cpu()[both])
    out_path = os.environ.get("NERFMESHES_SURFACE_RAY_FIGURES")
    if out_path:
        with open(out_path, "w") as fh:
            json.dump({"well_conditioned_share": share, "kept_and_well_conditioned": kept_stable, "kept_hip": int(keep_hip.sum()),
                       "kept_oracle": int(base.sum()), "masks_differ": int((keep_hip != base).sum()),
                       "masks_differ_well_conditioned": int(differ.sum()), "kept_by_both": int(both.sum()),
                       "max_point_distance_hip_vs_oracle": dist, "oracle_self_noise_max_point_distance": noise,
                       "colours": par}, fh, indent=1)


# ---- 4. ranks -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 3, 7])
def test_ranks_sharing_one_gpu_write_the_one_rank_file(world):
    """5 views: a ragged split over 2 and 3 ranks, and 7 ranks with two of them idle"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X")
    r = launch_ranks(os.path.join("tests", "tools", "sr_dist_worker.py"), world, timeout=600)
    assert_ranks_ok(r, f"SR_DIST_OK world={world}")


# ---- 5. the command line --------------------------------------------------------------------------------------------------------

def _cli(tmp_path, vdir, name, *extra):
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "nerfmeshes_amd.mesh_surface_ray", "--log-checkpoint", vdir,
           "--save-dir", str(tmp_path), "--ply-name", name, "--img-size", "100", "--focal", str(1111.1111 * 100 / 800),
           "--views-y", "3", "--views-x", "2", *extra]
    r = subprocess.run(cmd, cwd=ROOT, env=clean_env(), capture_output=True, text=True, timeout=700)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return SF.read_ply(tmp_path / name), r.stdout


def test_cli(ops, tmp_path):
    import importlib.util
    from nerfmeshes_amd import mesh_nerf, mesh_surface_ray as msr, models
    from nerfmeshes_amd.lightning_modules import PathParser
    spec = importlib.util.spec_from_file_location("make_ckpt", os.path.join(ROOT, "scripts", "make_synthetic_checkpoint.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    vdir = mk.write(str(tmp_path / "logs"))
    pp = PathParser()
    pp.parse(None, vdir, None, "model_last.ckpt")
    model = models.NeRFModel.load_from_checkpoint(pp.checkpoint_path).eval().to("cuda")
    common = ["--img-size", "100", "--focal", str(1111.1111 * 100 / 800), "--views-y", "3", "--views-x", "2"]

    def direct(*extra):
        args = _args(tmp_path / "direct", *common, *extra)
        os.makedirs(args.save_dir, exist_ok=True)
        with torch.no_grad():
            return msr.export_ray_trace(model, args, model.cfg, "cuda")

    (fmt, p, n, c), _ = _cli(tmp_path, vdir, "ascii.ply")
    v0, n0, _, cu0 = direct()
    assert fmt == "ascii" and len(p) > 100
    assert p.tobytes() == v0.tobytes() and n.tobytes() == n0.tobytes() and np.array_equal(c, cu0)
    (fmt, pb, nb, cb), _ = _cli(tmp_path, vdir, "binary.ply", "--ply-format", "binary")
    assert fmt == "binary" and pb.tobytes() == v0.tobytes() and nb.tobytes() == n0.tobytes() and np.array_equal(cb, cu0)

    (_, pn, nn, cn), stdout = _cli(tmp_path, vdir, "network.ply", "--normals", "network")
    assert "kept their ray normal" in stdout
    assert pn.tobytes() == v0.tobytes() and np.array_equal(cn, cu0), "points and colours do not depend on the normals"
    with torch.no_grad():
        want, kept = mesh_nerf.network_normals(model.get_model().hip("f32"), torch.from_numpy(pn).cuda(), torch.from_numpy(n0).cuda())
    assert nn.tobytes() == want.cpu().numpy().tobytes() and nn.tobytes() != n0.tobytes()
    assert not bool(kept.all())

    # under the reference rule only the rays whose acc rounded to >= 1.0 have a depth at all; acc >= 0.99 admits those and more
    (_, po, _, _), _ = _cli(tmp_path, vdir, "opacity.ply", "--min-opacity", "0.99")
    assert len(po) > len(p)
    (_, po2, _, _), _ = _cli(tmp_path, vdir, "opacity2.ply", "--min-opacity", "0.5")
    assert len(po2) >= len(po)
