"""CPU: the TSDF fusion's rule.  The vectorised numpy restatement (tests/tsdf_fuse.py) against its plain per-voxel loop, an
analytic scene of two spheres fused from exact depth maps and meshed with the oracle's marching cubes, the edge scenes the GPU
test runs (here: that they really contain every edge they are meant to), the argument errors of nm_tsdf_integrate on a host
without a GPU, and the command line."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import tsdf_fuse as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
SPECIAL_DEPTHS = (np.nan, np.inf, -np.inf, 0.0, -1.0)
OPACITIES = (0.0, 0.25, 0.5, 0.75, 1.0, np.nan)           # 0.5 is exactly min_opacity
TRUNC_KEPT, TRUNC_OCCLUDED = 0.25, float(np.nextafter(0.25, 0.0))   # s = 0.25 is kept by the first and one ulp above the second
GRIDS = ((2, 2, 2), (3, 5, 70), (2, 3, 300))
VIEW_COUNTS = (1, 2, 17)
IMAGES = ((8, 8, 4.0), (48, 64, 16.0))                    # height, width, focal: dyadic, so that projections land on exact halves


def look_at(eye, up=(0.0, 0.0, 1.0)):
    """(3,4) camera-to-world of a camera at `eye` that looks at the origin: columns right, up, backward, position"""
    eye = np.asarray(eye, F64)
    back = eye / np.sqrt((eye * eye).sum())
    right = np.cross(np.asarray(up, F64), back)
    right /= np.sqrt((right * right).sum())
    pose = np.zeros((3, 4), F64)
    pose[:, 0], pose[:, 1], pose[:, 2], pose[:, 3] = right, np.cross(back, right), back, eye
    return pose.astype(F32)


def edge_axes(grid):
    """dyadic coordinates: with the axis-aligned cameras of `edge_scene` the projections hit pixel centres, exact halves between
    two pixels and the two edges of the frustum; the long axis runs from behind the first camera to far in front of it"""
    n0, n1, n2 = grid
    x = np.array([0.125, -1.125, 0.875], F32)[:n0]
    y = np.array([0.0, 0.375, -0.875, 1.0, -1.125], F32)[:n1]
    z = np.array([1.0, 0.0], F32) if n2 == 2 else ((np.arange(n2) - n2 // 2) / 32.0).astype(F32)
    assert len(x) == n0 and len(y) == n1
    return [x, y, z]


def edge_scene(grid, num_views, image, with_opacity=True, seed=0):
    """-> dict(views, depth, opacity, axes, near, min_opacity): camera 0 at (0, 0, 2) with the identity rotation (z = 2 - pz: the
    voxels with pz = 1 are at z == near exactly, those with pz > 2 behind it), camera 1 at (2, 0, 0) looking along -x, the rest
    at seeded places all around.  Depths are multiples of 1/16 in [0.5, 3) -- so z - D == 0.25 happens --, every fifth pixel one
    of NaN, +inf, -inf, 0, -1; opacities are drawn from 0, 0.25, 0.5 (== min_opacity), 0.75, 1, NaN."""
    height, width, focal = image
    rng = np.random.default_rng(seed + 97 * num_views + height)
    poses = [np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 2]], F32), np.array([[0, 0, 1, 2], [0, 1, 0, 0], [-1, 0, 0, 0]], F32)]
    while len(poses) < num_views:
        eye = rng.normal(size=3)
        poses.append(look_at(3.0 * eye / np.sqrt((eye * eye).sum())))
    views = [TF.view(p, height, width, focal) for p in poses[:num_views]]
    depth = (rng.integers(8, 48, (num_views, height, width)) / 16.0).astype(F32)
    flat = depth.reshape(-1)
    flat[2::5] = np.resize(np.array(SPECIAL_DEPTHS, F32), flat[2::5].shape)
    opacity = rng.choice(np.array(OPACITIES, F32), (num_views, height, width)) if with_opacity else None
    return dict(views=views, depth=depth, opacity=opacity, axes=edge_axes(grid), near=1.0, min_opacity=0.5)


def edge_census(scene, trunc):
    """how often a scene meets each edge of the rule, counted with the rule's own operations"""
    px, py, pz = TF.voxel_points(scene["axes"], 0, int(np.prod([len(a) for a in scene["axes"]])))
    seen = dict.fromkeys(("behind", "at_near", "tie_col", "tie_row", "edge_low", "edge_high", "outside", "s_is_trunc", "s_above_trunc",
                          "clamped", "bad_depth", "opacity_at_threshold", "opacity_nan"), 0)
    in_any = np.zeros(len(px), bool)
    with np.errstate(all="ignore"):
        for v, vw in enumerate(scene["views"]):
            rot, c = vw["c2w"][:, :3].astype(F64), vw["c2w"][:, 3].astype(F64)
            dx, dy, dz = px - c[0], py - c[1], pz - c[2]
            cx, cy = (rot[0, 0] * dx + rot[1, 0] * dy) + rot[2, 0] * dz, (rot[0, 1] * dx + rot[1, 1] * dy) + rot[2, 1] * dz
            z = -((rot[0, 2] * dx + rot[1, 2] * dy) + rot[2, 2] * dz)
            ok = z >= scene["near"]
            u = (cx / z) * vw["focal"] + 0.5 * vw["width"]
            w = 0.5 * vw["height"] - (cy / z) * vw["focal"]
            seen["behind"] += int((z < 0).sum())
            seen["at_near"] += int((z == scene["near"]).sum())
            seen["tie_col"] += int((ok & (u - np.floor(u) == 0.5) & (u > 0) & (u < vw["width"] - 1)).sum())
            seen["tie_row"] += int((ok & (w - np.floor(w) == 0.5) & (w > 0) & (w < vw["height"] - 1)).sum())
            seen["edge_low"] += int((ok & ((u == -0.5) | (w == -0.5))).sum())
            seen["edge_high"] += int((ok & ((u == vw["width"] - 0.5) | (w == vw["height"] - 0.5))).sum())
            col, row = np.rint(u), np.rint(w)
            ok &= (col >= 0) & (col <= vw["width"] - 1) & (row >= 0) & (row <= vw["height"] - 1)
            in_any |= ok
            at = np.flatnonzero(ok)
            d = scene["depth"][v, row[at].astype(int), col[at].astype(int)]
            seen["bad_depth"] += int((~(np.isfinite(d) & (d > 0))).sum())
            good = np.isfinite(d) & (d > 0)
            if scene["opacity"] is not None:
                o = scene["opacity"][v, row[at].astype(int), col[at].astype(int)]
                seen["opacity_at_threshold"] += int((good & (o == F32(scene["min_opacity"]))).sum())
                seen["opacity_nan"] += int((good & np.isnan(o)).sum())
                good &= o.astype(F64) >= scene["min_opacity"]
            s = z[at] - d.astype(F64)
            seen["s_is_trunc"] += int((good & (s == trunc)).sum())
            seen["s_above_trunc"] += int((good & (s == np.nextafter(trunc, np.inf))).sum())
            seen["clamped"] += int((good & (s / trunc < -1)).sum())
    seen["outside"] = int((~in_any).sum())
    return seen


def test_restatement_against_the_scalar_loop():
    """5 x 4 x 3 voxels, three views, every special depth and opacity: two independent writings of the rule agree exactly"""
    rng = np.random.default_rng(5)
    axes = [np.linspace(-1.0, 1.0, 5).astype(F32), np.linspace(-0.9, 0.7, 4).astype(F32), np.linspace(-0.8, 1.1, 3).astype(F32)]
    views = [TF.view(look_at(eye), 12, 9, 12.0) for eye in ((0.0, -2.5, 0.5), (2.0, 1.0, 1.0), (0.3, 0.2, -2.2))]
    depth = rng.uniform(0.5, 3.5, (3, 12, 9)).astype(F32)
    depth.reshape(-1)[1::4] = np.resize(np.array(SPECIAL_DEPTHS, F32), depth.reshape(-1)[1::4].shape)
    opacity = rng.choice(np.array(OPACITIES, F32), (3, 12, 9))
    for op in (opacity, None):
        for first, count in ((0, None), (7, 41)):
            want = TF.integrate_scalar(views, depth, op, axes, 0.4, 0.5, 0.5, first, count)
            got = TF.integrate(views, depth, op, axes, 0.4, 0.5, 0.5, first, count)
            assert got[0].dtype == F32 and got[1].dtype == np.int32 and got[2].dtype == np.int64
            assert got[0].tobytes() == want[0].tobytes() and (got[1] == want[1]).all() and (got[2] == want[2]).all()
            assert got[2].sum() == len(got[0]) and (got[1] > 0).any() and (got[1] == 0).any()
    whole, part = TF.integrate(views, depth, opacity, axes, 0.4, 0.5), TF.integrate(views, depth, opacity, axes, 0.4, 0.5, 0.5, 7, 41)
    assert part[0].tobytes() == whole[0][7:48].tobytes() and (part[1] == whole[1][7:48]).all()


def test_the_edge_scenes_contain_the_edges_they_are_meant_to():
    """the GPU test runs these scenes against the kernel: between them they must meet every edge of the rule"""
    total = {}
    for grid in GRIDS:
        for image in IMAGES:
            for num_views in VIEW_COUNTS:
                for trunc in (TRUNC_KEPT, TRUNC_OCCLUDED):
                    census = edge_census(edge_scene(grid, num_views, image), trunc)
                    for k, n in census.items():
                        total[k] = total.get(k, 0) + n
                    # the tie at s == trunc: the same voxels and pixels are kept by one trunc and occluded by the other
                    if trunc == TRUNC_OCCLUDED:
                        assert census["s_above_trunc"] == edge_census(edge_scene(grid, num_views, image), TRUNC_KEPT)["s_is_trunc"]
    print(total)
    assert all(n > 0 for n in total.values()), total
    small = edge_census(edge_scene((2, 2, 2), 1, IMAGES[0]), TRUNC_KEPT)
    assert small["at_near"] and small["tie_col"] and small["edge_low"], small


RES, LIMIT, SPHERES = 48, 1.2, (((0.0, 0.0, 0.0), 0.7), ((0.9, 0.0, 0.0), 0.15))


def sphere_depth(pose, size, focal):
    """the exact depth along the camera's axis of the first sphere every pixel's ray meets, 0 where it meets none: the ray is
    c + t R (x, y, -1), whose parameter t is the depth along the axis"""
    i = (np.arange(size, dtype=F64) - size * 0.5) / focal
    x, y = np.meshgrid(i, -i, indexing="xy")
    rot, c = pose[:, :3].astype(F64), pose[:, 3].astype(F64)
    d = x[..., None] * rot[:, 0] + y[..., None] * rot[:, 1] - rot[:, 2]
    best = np.full((size, size), np.inf)
    for centre, radius in SPHERES:
        oc = c - np.asarray(centre, F64)
        a, b, k = (d * d).sum(-1), (d * oc).sum(-1), (oc * oc).sum() - radius * radius
        disc = b * b - a * k
        t = (-b - np.sqrt(np.where(disc >= 0, disc, np.nan))) / a
        best = np.where((disc >= 0) & (t > 0) & (t < best), t, best)
    return np.where(np.isfinite(best), best, 0.0).astype(F32)


@pytest.fixture(scope="module")
def analytic():
    size, count, focal = 128, 16, 1111.1111 * 128 / 800.0
    poses = []
    for k in range(count):                                  # a Fibonacci lattice on the sphere of radius 4
        z = 1.0 - (2 * k + 1) / count
        a, s = k * np.pi * (3.0 - np.sqrt(5.0)), np.sqrt(1.0 - z * z)
        poses.append(look_at(4.0 * np.array([s * np.cos(a), s * np.sin(a), z])))
    views = [TF.view(p, size, size, focal) for p in poses]
    depth = np.stack([sphere_depth(v["c2w"], size, focal) for v in views])
    opacity = (depth > 0).astype(F32)
    axes = [np.linspace(-LIMIT, LIMIT, RES).astype(F32)] * 3
    voxel = 2.0 * LIMIT / (RES - 1)
    field, obs, counts = TF.integrate(views, depth, opacity, axes, 3.0 * voxel, 2.0, 0.5)
    return field.reshape(RES, RES, RES), obs, counts, voxel


def components(mask):
    """6-connected components of a boolean grid, by flood fill"""
    todo, count = mask.copy(), 0
    while todo.any():
        count += 1
        stack = [tuple(np.argwhere(todo)[0])]
        todo[stack[0]] = False
        while stack:
            i, j, k = stack.pop()
            for a, b, c in ((i + 1, j, k), (i - 1, j, k), (i, j + 1, k), (i, j - 1, k), (i, j, k + 1), (i, j, k - 1)):
                if 0 <= a < mask.shape[0] and 0 <= b < mask.shape[1] and 0 <= c < mask.shape[2] and todo[a, b, c]:
                    todo[a, b, c] = False
                    stack.append((a, b, c))
    return count


def test_two_spheres_from_exact_depth_maps(analytic):
    """The cap of 0.75 voxel: the zero level of a mean of truncated distances along rays that are not normal to the surface is
    not the surface itself; a prototype of this rule measured 0.48 voxel at worst, a wrong projection or sign costs whole voxels."""
    from oracle import mc_oracle
    field, obs, counts, voxel = analytic
    verts, faces, normals, _ = mc_oracle.marching_cubes(field, 0.0)
    world = -LIMIT + verts.astype(F64) * voxel              # the grid's own coordinates
    dist = np.stack([np.abs(np.sqrt(((world - np.asarray(c)) ** 2).sum(1)) - r) for c, r in SPHERES])
    nearest = dist.argmin(0)
    worst, mean = dist.min(0).max() / voxel, dist.min(0).mean() / voxel
    print(f"{len(verts)} vertices, {len(faces)} faces, distance to the spheres: worst {worst:.3f} voxel, mean {mean:.3f}; counts {counts}")
    assert worst <= 0.75
    assert len(verts) - len(faces) / 2 == 4, "two closed surfaces of genus 0"
    assert components(field > 0) == 2
    outward = world - np.asarray([SPHERES[k][0] for k in nearest])
    assert ((normals.astype(F64) * outward).sum(1) > 0).all(), "normals point outward"
    assert counts[TF.OUTSIDE] == 0 and counts[TF.INTERIOR] > 0 and counts.sum() == RES ** 3
    assert (field[obs.reshape(field.shape) == 0] == 1.0).all(), "every unobserved voxel is interior"


def test_the_library_rejects_bad_arguments_without_a_gpu():
    from nerfmeshes_amd import _lib, hip_ops
    lib = _lib.load()
    null, one = C.c_void_p(None), C.c_void_p(8)                # never dereferenced: validation fails first
    pose = np.eye(4, dtype=F32)

    def err():
        return (lib.nm_last_error() or b"").decode()

    def call(views=None, count_views=None, depth=one, axes=(one, one, one), grid=(4, 4, 4), first=0, count=64, trunc=0.1, near=0.5,
             min_opacity=0.5, ws=one, field=one, counts=one):
        views = [hip_ops.make_view(pose, 8, 8, 10.0)] * 2 if views is None else views
        array = (_lib.View * max(len(views), 1))(*views)
        return lib.nm_tsdf_integrate(array if views else None, len(views) if count_views is None else count_views, depth, null, *axes,
                                     *grid, first, count, trunc, near, min_opacity, ws, field, null, counts, null)

    assert lib.nm_abi_version() == 6
    for bad in (dict(depth=null), dict(axes=(null, one, one)), dict(axes=(one, one, null)), dict(ws=null), dict(field=null),
                dict(counts=null), dict(views=[])):
        assert call(**bad) == 2 and "bad argument" in err(), bad
    for n in (0, -1, 1025):
        assert call(count_views=n) == 2 and "views must be in [1, 1024]" in err()
    assert call(views=[hip_ops.make_view(pose, 8, 8, 10.0), hip_ops.make_view(pose, 8, 9, 10.0)]) == 2 and "same height and width" in err()
    assert call(views=[hip_ops.make_view(pose, 8, 8, 10.0, ndc_near=1.0)]) == 2 and "NDC" in err()
    assert call(views=[hip_ops.make_view(pose, 0, 8, 10.0)]) == 2 and "sides must be in [1, 16384]" in err()
    for focal in (0.0, -1.0, float("inf"), float("nan")):
        assert call(views=[hip_ops.make_view(pose, 8, 8, focal)]) == 2 and "focal must be finite and > 0" in err()
    for value in (0.0, -0.1, float("inf"), float("nan")):
        assert call(trunc=value) == 2 and "trunc must be finite and > 0" in err()
        assert call(near=value) == 2 and "near must be finite and > 0" in err()
    assert call(min_opacity=float("nan")) == 2 and "min_opacity" in err()
    assert call(grid=(0, 4, 4)) == 2 and "at least one voxel" in err()
    for first, count in ((-1, 4), (0, -1), (0, 65), (60, 5), (65, 0), (2 ** 62, 2 ** 62)):
        assert call(first=first, count=count) == 2 and "outside the grid" in err(), (first, count)
    assert lib.nm_tsdf_workspace_bytes(0, 8, 8) == 0 and lib.nm_tsdf_workspace_bytes(1025, 8, 8) == 0
    assert lib.nm_tsdf_workspace_bytes(2, 0, 8) == 0 and lib.nm_tsdf_workspace_bytes(2, 8, 16385) == 0
    assert lib.nm_tsdf_workspace_bytes(32, 800, 800) == 32 * 128 + 32 * 800 * 800 * 4
    assert lib.nm_tsdf_workspace_bytes(1, 8, 8) == 256 + 256


def test_the_symbols_are_declared_exported_and_bound():
    from nerfmeshes_amd import _lib, build, hip_ops
    header = open(os.path.join(ROOT, "include", "nerfmeshes_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint nm_tsdf_integrate\s*\(const nm_view\* views, int64_t num_views,", code)
    assert re.search(r"\bint64_t nm_tsdf_workspace_bytes\s*\(int64_t num_views, int32_t height, int32_t width\);", code)
    assert "#define NM_ABI_VERSION 6" in header and "6, later: + nm_tsdf_integrate" in header
    assert "#define NM_TSDF_MAX_VIEWS 1024" in header and hip_ops.TSDF_MAX_VIEWS == 1024
    for k, name in enumerate(("OBSERVED", "INTERIOR", "OUTSIDE")):
        assert f"#define NM_TSDF_{name} {k}" in header and hip_ops.TSDF_COUNTS[k] == name.lower() and getattr(TF, name) == k
    lib = _lib.load()
    assert hasattr(lib, "nm_tsdf_integrate") and hasattr(lib, "nm_tsdf_workspace_bytes") and "tsdf_fuse.hip" in build.SOURCES
    restype, argtypes = _lib.SIGNATURES["nm_tsdf_integrate"]
    assert restype is C.c_int and len(argtypes) == 20 and argtypes[12:15] == [C.c_double] * 3


NO_STEP = "no --route script: the reference's script has no such step"
TSDF_WHAT = ("--geometry tsdf / --tsdf-views / --tsdf-size / --tsdf-radius / --tsdf-focal / --tsdf-trunc / --tsdf-min-opacity / "
             "--tsdf-level have ")


@pytest.mark.parametrize("option", [["--geometry", "tsdf"], ["--tsdf-views", "8"], ["--tsdf-level", "0.1"]], ids=lambda o: o[0])
def test_route_script_rejects_the_options_in_the_tables_words(tmp_path, option):
    from nerfmeshes_amd import mesh_nerf
    args = mesh_nerf.build_parser().parse_args([*option, "--route", "script", "--save-dir", str(tmp_path)])
    with pytest.raises(ValueError) as e:
        mesh_nerf.export_marching_cubes(None, args, None, "cpu")
    assert str(e.value) == TSDF_WHAT + NO_STEP
    assert not any(tmp_path.iterdir()), "rejected before anything is written"


def test_the_options_their_defaults_and_their_ranges():
    from nerfmeshes_amd import mesh_nerf
    args = mesh_nerf.build_parser().parse_args([])
    assert (args.geometry, args.tsdf_views, args.tsdf_size, args.tsdf_radius, args.tsdf_focal, args.tsdf_trunc, args.tsdf_min_opacity,
            args.tsdf_level) == ("density", 32, 800, 4.0, 0.0, 3.0, 0.5, 0.0)
    assert mesh_nerf.check_features(args) == set()
    assert mesh_nerf.check_features(argparse.Namespace()) == set(), "a namespace without the options passes"
    assert mesh_nerf.check_features(argparse.Namespace(geometry="tsdf")) == {"tsdf"}
    assert mesh_nerf.check_features(mesh_nerf.build_parser().parse_args(["--geometry", "tsdf", "--render-views", "2"])) == {"tsdf", "render"}
    assert mesh_nerf.check_features(argparse.Namespace(tsdf_views=8)) == set(), "the other options do not switch it on"
    assert abs(mesh_nerf.tsdf_focal(argparse.Namespace(tsdf_focal=0.0, tsdf_size=400)) - 555.55555) < 1e-9
    assert mesh_nerf.tsdf_focal(argparse.Namespace(tsdf_focal=90.0, tsdf_size=400)) == 90.0
    for bad in (dict(tsdf_views=0), dict(tsdf_views=1025), dict(tsdf_size=0), dict(tsdf_size=16385), dict(tsdf_radius=0.0),
                dict(tsdf_radius=float("inf")), dict(tsdf_focal=-1.0), dict(tsdf_focal=float("nan")), dict(tsdf_trunc=0.0),
                dict(tsdf_trunc=float("nan")), dict(tsdf_min_opacity=float("nan")), dict(tsdf_level=1.0), dict(tsdf_level=-1.0),
                dict(tsdf_level=float("nan")), dict(geometry="sdf")):
        with pytest.raises(ValueError, match=r"--tsdf-views in \[1, 1024\]"):       # also while the geometry is the density's
            mesh_nerf.check_features(argparse.Namespace(**bad))
        with pytest.raises(ValueError, match=r"--tsdf-views in \[1, 1024\]"):
            mesh_nerf.check_features(argparse.Namespace(**dict(dict(geometry="tsdf"), **bad)))
    with pytest.raises(SystemExit):
        mesh_nerf.build_parser().parse_args(["--geometry", "sdf"])


def test_super_sampling_and_ndc_scenes_are_refused(tmp_path):
    from nerfmeshes_amd import mesh_nerf
    args = mesh_nerf.build_parser().parse_args(["--geometry", "tsdf", "--super-sampling", "2", "--save-dir", str(tmp_path)])
    with pytest.raises(ValueError, match="--geometry tsdf has no --super-sampling"):
        mesh_nerf.export_marching_cubes(None, args, None, "cpu")
    with pytest.raises(ValueError, match="--geometry tsdf has no --super-sampling"):
        mesh_nerf.extract_geometry_tsdf(None, "cpu", args, None)
    assert not any(tmp_path.iterdir()), "rejected before anything is written"
    args = mesh_nerf.build_parser().parse_args(["--geometry", "tsdf"])
    cfg = argparse.Namespace(dataset=argparse.Namespace(use_ndc=True))
    with pytest.raises(ValueError, match="normalised device coordinates"):
        mesh_nerf.extract_geometry_tsdf(None, "cpu", args, cfg)

    class Jittered:
        def can_query_view(self):
            return False
    cfg.dataset.use_ndc = False
    with pytest.raises(RuntimeError, match="deterministic in-kernel view render"):
        mesh_nerf.extract_geometry_tsdf(Jittered(), "cpu", args, cfg)
