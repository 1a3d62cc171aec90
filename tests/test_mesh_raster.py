"""CPU: the rasteriser's rule as tests/mesh_raster.py restates it (exactly-once coverage, depth against an analytic sphere,
the winner's independence of the face order, the reject counts), load_obj_attributes, the argument errors of the C entries
(which return before any HIP call) and the new mesh_nerf option."""
import ctypes as C

import numpy as np
import pytest

from nerfmeshes_amd import synthetic as S
from tests import mesh_metrics as MM
from tests import mesh_raster as MR

F32 = np.float32


def sheet(seed=3, snap=None):
    """A 9 x 9 sheet of 128 triangles over [-1, 1]^2 at z = 0, the inner vertices jittered in the plane, every other
    triangle with the opposite winding; seen from (0, 0, 3) by a 48 x 48 camera with f = 60 it spans pixels [4, 44).
    snap: move every vertex onto the pixel centre nearest to it."""
    rng = np.random.default_rng(seed)
    g = np.linspace(-1.0, 1.0, 9)
    x, y = np.meshgrid(g, g, indexing="xy")
    jitter = rng.uniform(-0.1, 0.1, (9, 9, 2))
    jitter[[0, -1], :] = 0
    jitter[:, [0, -1]] = 0
    x, y = x + jitter[..., 0], y + jitter[..., 1]
    if snap:
        x, y = np.rint(x * 20.0) / 20.0, np.rint(y * 20.0) / 20.0         # 20 pixels per unit: 60 / 3
    verts = np.stack((x, y, np.zeros_like(x)), -1).reshape(-1, 3).astype(F32)
    idx = np.arange(81).reshape(9, 9)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel(), idx[1:, :-1].ravel()
    faces = np.concatenate((np.stack((a, b, c), 1), np.stack((a, c, d), 1))).astype(np.int32)
    faces[::2] = faces[::2][:, [0, 2, 1]]
    pose = np.eye(4, dtype=F32)
    pose[2, 3] = 3.0
    return verts, faces, pose


def coverage_count(verts, faces, pose, height, width, focal, near):
    """how many faces cover each pixel: every face drawn alone"""
    total = np.zeros((height, width), np.int64)
    for f in range(len(faces)):
        total += MR.rasterize(verts, faces[f:f + 1], pose, height, width, focal, near)[0] >= 0
    return total


@pytest.mark.parametrize("snap", [False, True], ids=["jittered", "on_pixel_centres"])
def test_a_sheet_covers_every_pixel_exactly_once(snap):
    verts, faces, pose = sheet(snap=snap)
    assert len(faces) == 128
    if snap:
        x, y, _, _, _ = MR.project(verts, pose, 48, 48, 60.0)
        assert (x % 256 == 0).all() and (y % 256 == 0).all()
    times = coverage_count(verts, faces, pose, 48, 48, 60.0, 0.1)
    assert times.max() == 1 and times.sum() == 1600
    assert times[4:44, 4:44].all(), "the top-left rule: rows and columns 4 .. 43"
    face_id, depth, bary, counts = MR.rasterize(verts, faces, pose, 48, 48, 60.0, 0.1)
    assert counts["covered"] == 1600 and counts["drawn"] + counts["degenerate"] == 128 and (face_id >= 0).sum() == 1600
    assert (depth[face_id >= 0] == F32(3.0)).all() and (depth[face_id < 0] == 0).all()
    assert np.abs(bary[face_id >= 0].sum(-1) - 1).max() < 1e-6


SPHERE_VIEWS = [((30.0, -30.0, 4.0), 64, 64, 70.0), ((-100.0, -60.0, 3.0), 50, 70, 55.0), ((170.0, 10.0, 2.5), 96, 96, 80.0)]


@pytest.fixture(scope="module")
def sphere():
    return MM.uv_sphere(64, 32)


@pytest.mark.parametrize("angles, height, width, focal", SPHERE_VIEWS)
def test_sphere_depth_and_planes(sphere, angles, height, width, focal):
    """The ray of a pixel is the camera-space (x, y, -1) of get_ray_bundle BEFORE its normalisation, turned into the world:
    its parameter is the distance along the camera's axis, which is what the rasteriser's depth measures."""
    verts, faces = sphere
    pose = S.pose_spherical(*angles)
    face_id, depth, bary, counts = MR.rasterize(verts, faces, pose, height, width, focal, 0.1)
    origin, dirs = MR.pixel_rays(pose, height, width, focal)
    # (a) the analytic hit |o + t d| = 1, where the ray meets the sphere at an incidence with |cos| >= 0.5
    a, b, c = (dirs * dirs).sum(-1), 2 * (dirs @ origin), origin @ origin - 1.0
    disc = b * b - 4 * a * c
    hit = disc > 0
    t = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0))) / (2 * a), 0)
    point = origin + t[..., None] * dirs
    cosine = np.abs((point * dirs).sum(-1) / np.sqrt(a))
    sure = hit & (cosine >= 0.5)
    assert sure.sum() > 100 and (face_id[sure] >= 0).all()
    err = np.abs(depth.astype(np.float64) - t)[sure].max()
    print(f"sphere {angles}: depth error {err:.3e}")
    assert err <= 2 * (1 - np.cos(np.sqrt(2) * np.pi / 64)) + 1e-4
    # (b) every covered pixel's point lies on its winning face's plane, up to the half sub-pixel snap at depth w_max
    covered = face_id >= 0
    p = origin + depth[covered].astype(np.float64)[:, None] * dirs[covered]
    tri = verts.astype(np.float64)[faces[face_id[covered]]]
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    w_max = float(depth[covered].max())
    off = np.abs(((p - tri[:, 0]) * normal).sum(-1)).max()
    print(f"sphere {angles}: plane distance {off:.3e} against {np.sqrt(2) * w_max / (512 * focal) + 1e-5 * w_max:.3e}")
    assert off <= np.sqrt(2) * w_max / (512 * focal) + 1e-5 * w_max
    assert counts["degenerate"] + counts["off_screen"] + counts["drawn"] == len(faces)


def soup(n=400, seed=5):
    """random triangles on a coarse lattice: many exact depth ties and shared edges"""
    rng = np.random.default_rng(seed)
    verts = (rng.integers(-4, 5, (n, 3)) * 0.25).astype(F32)
    faces = rng.integers(0, n, (2 * n, 3)).astype(np.int32)
    return verts, faces


def test_the_winner_depends_on_the_face_order_only_through_its_id():
    verts, faces = soup()
    pose = S.pose_spherical(20.0, -25.0, 4.0)
    first = MR.rasterize(verts, faces, pose, 40, 40, 45.0, 0.1)
    perm = np.random.default_rng(1).permutation(len(faces))
    other = MR.rasterize(verts, faces[perm], pose, 40, 40, 45.0, 0.1)
    assert first[1].tobytes() == other[1].tobytes() and first[3] == other[3], "depth and counts do not see the order"
    seen = first[0] >= 0
    assert seen.sum() > 200
    # under the permutation the winner is the tied face with the smallest NEW index: the same depth, maybe another face
    tri_a, tri_b = faces[first[0][seen]], faces[perm][other[0][seen]]
    same = (tri_a == tri_b).all(-1)
    for pix in np.argwhere(seen)[~same][:20]:
        alone_a = MR.rasterize(verts, faces[first[0][tuple(pix)]][None], pose, 40, 40, 45.0, 0.1)
        alone_b = MR.rasterize(verts, faces[perm][other[0][tuple(pix)]][None], pose, 40, 40, 45.0, 0.1)
        assert alone_a[1][tuple(pix)] == alone_b[1][tuple(pix)] == first[1][tuple(pix)], "only an exact tie changes hands"
    dup = np.concatenate((faces, faces))                            # every face twice: the smaller id wins everywhere
    twice = MR.rasterize(verts, dup, pose, 40, 40, 45.0, 0.1)
    assert twice[0].tobytes() == first[0].tobytes() and twice[2].tobytes() == first[2].tobytes()


def reject_mesh():
    """one face per reject reason, one drawn face and one drawn face for the large path"""
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0],              # 0-2: drawn (counter-clockwise as seen)
                      [np.nan, 0, 0], [0, 0, 3.95], [3e9, 0, 0],     # 3: not finite, 4: nearer than near, 5: out of range
                      [0.5, 0.5, 0], [1.0, 1.0, 0],                  # 6, 7: collinear with 0
                      [50, 50, 0], [51, 50, 0], [50, 51, 0],         # 8-10: beside the screen
                      [0.001, 0.001, 0], [0.002, 0.001, 0], [0.001, 0.002, 0]], F32)   # 11-13: between four pixel centres
    faces = np.array([[0, 1, 2], [0, 1, 14], [0, 3, 1], [0, 1, 4], [0, 5, 2], [0, 2, 1], [8, 9, 10], [0, 6, 7], [11, 12, 13],
                      [-1, 0, 1]], np.int32)
    pose = np.eye(4, dtype=F32)
    pose[2, 3] = 4.0
    return verts, faces, pose


def test_reject_counts():
    verts, faces, pose = reject_mesh()
    _, _, _, counts = MR.rasterize(verts, faces, pose, 32, 32, 40.0, 0.1, cull_back=True, large_threshold=16)
    assert counts == dict(drawn=1, bad_index=2, not_finite=1, near=1, out_of_range=1, culled=1, off_screen=2, degenerate=1,
                          large=1, covered=counts["covered"], fragments=counts["covered"]) and counts["covered"] > 30
    face_id, _, _, both = MR.rasterize(verts, faces, pose, 32, 32, 40.0, 0.1, large_threshold=10 ** 9)
    assert both["fragments"] == 2 * both["covered"] and both["culled"] == 0 and both["drawn"] == 2 and both["large"] == 0 and both["covered"] == counts["covered"]
    assert set(np.unique(face_id)) == {-1, 0}, "the same pixels twice: the smaller id wins"


def test_interpolate_restatement():
    verts, faces, pose = sheet()
    raster = MR.rasterize(verts, faces, pose, 48, 48, 60.0, 0.1)
    attr = np.concatenate((verts, verts[:, :1] * 2 + 1), 1)          # affine in the plane: reproduced up to rounding
    out = MR.interpolate(raster[0], raster[2], faces, attr, [9, 8, 7, 6])
    assert out.dtype == F32 and out.shape == (48, 48, 4)
    assert (out[raster[0] < 0] == np.array([9, 8, 7, 6], F32)).all()
    j, i = np.nonzero(raster[0] >= 0)
    want_x, want_y = (i - 24) / 20.0, -(j - 24) / 20.0
    got = out[raster[0] >= 0]
    snap = 1.0 / (512 * 20.0) + 1e-5                                 # half a sub-pixel step, in the sheet's units, and fp32 slack
    assert np.abs(got[:, 0] - want_x).max() < snap and np.abs(got[:, 1] - want_y).max() < snap
    assert np.abs(got[:, 3] - (2 * want_x + 1)).max() < 2 * snap


def test_load_obj_attributes_reads_back_what_export_obj_wrote(tmp_path):
    from nerfmeshes_amd.nerf.nerf_helpers import export_obj, load_obj, load_obj_attributes
    rng = np.random.default_rng(2)
    v = (rng.standard_normal((50, 3)) * 3).astype(F32)
    v[0] = [1e-30, -0.0, 123456.789]
    c = rng.random((50, 3), dtype=F32)
    n = rng.standard_normal((50, 3)).astype(F32)
    f = rng.integers(0, 50, (80, 3)).astype(np.int32)
    path = str(tmp_path / "m.obj")
    export_obj(v, f, c, n, path)
    rv, rf, rc, rn = load_obj_attributes(path)
    for got, want in ((rv, v), (rf, f), (rc, c), (rn, n)):
        got = got.numpy()
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
    pv, pf = load_obj(path)
    assert pv.numpy().tobytes() == v.tobytes() and pf.numpy().tobytes() == f.tobytes()
    bare = str(tmp_path / "bare.obj")
    open(bare, "w").write("v 0 0 0\nv 1 0 0 0.5 0.5 0.5\nv 0 1 0\nf 1 2 3\n")
    _, _, colors, normals = load_obj_attributes(bare)
    assert colors is None and normals is None


def test_pose_from_rays_recovers_the_pose_of_get_ray_bundle():
    """a dataset keeps an image's rays, not its pose: mesh_render gets the pose back from them"""
    from nerfmeshes_amd import mesh_render
    for angles, height, width, focal in SPHERE_VIEWS:
        pose = S.pose_spherical(*angles)[:3, :4]
        origin, dirs = MR.pixel_rays(pose, height, width, focal)
        dirs = (dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).astype(F32)     # get_ray_bundle's unit directions
        got = mesh_render.pose_from_rays(np.broadcast_to(origin.astype(F32), (1, 3)), dirs.reshape(-1, 3), height, width, focal)
        assert got.dtype == F32 and got.shape == (3, 4) and np.abs(got - pose).max() < 1e-6


@pytest.fixture(scope="module")
def lib():
    from nerfmeshes_amd import _lib
    return _lib.load()


def test_argument_errors_return_2_before_any_hip_call(lib):
    from nerfmeshes_amd import _lib, hip_ops
    view = hip_ops.make_view(np.eye(4, dtype=F32), 8, 8, 10.0)
    ndc = hip_ops.make_view(np.eye(4, dtype=F32), 8, 8, 10.0, ndc_near=1.0)
    p = C.c_void_p(256)                                              # never dereferenced: every call fails its checks first

    def raster(view=view, verts=p, nv=3, faces=p, nf=1, near=0.1, flags=0, threshold=16, ws=p, ids=p, depth=p, bary=p, counts=p):
        return lib.nm_mesh_rasterize(C.byref(view), verts, nv, faces, nf, near, flags, threshold, ws, ids, depth, bary, counts, None)

    for name in ("verts", "faces", "ws", "ids", "depth", "bary", "counts"):
        assert raster(**{name: None}) == 2, name
        assert b"bad argument" in lib.nm_last_error()
    assert raster(view=ndc) == 2 and b"NDC" in lib.nm_last_error()
    for near in (0.0, -1.0, float("nan"), float("inf")):
        assert raster(near=near) == 2 and b"near" in lib.nm_last_error()
    assert raster(flags=2) == 2 and raster(threshold=-1) == 2 and raster(nv=0) == 2 and raster(nf=-1) == 2
    assert raster(view=hip_ops.make_view(np.eye(4, dtype=F32), 0, 8, 10.0)) == 2
    assert raster(view=hip_ops.make_view(np.eye(4, dtype=F32), 8, 16385, 10.0)) == 2

    def interp(ids=p, bary=p, pixels=64, faces=p, nf=1, attr=p, nv=3, channels=3, background=p, out=p):
        return lib.nm_mesh_interpolate(ids, bary, pixels, faces, nf, attr, nv, channels, background, out, None)

    for channels in (0, -1, 17):
        assert interp(channels=channels) == 2 and b"channels" in lib.nm_last_error()
    for name in ("ids", "bary", "faces", "attr", "background", "out"):
        assert interp(**{name: None}) == 2, name
    size = lib.nm_mesh_raster_workspace_bytes
    assert size(10, 20, 8, 8) > 0 and size(0, 0, 1, 1) > 0
    for args in ((-1, 0, 8, 8), (0, -1, 8, 8), (2 ** 31 - 64, 0, 8, 8), (0, 2 ** 31 - 64, 8, 8), (1, 1, 0, 8), (1, 1, 8, 0),
                 (1, 1, 16385, 8), (1, 1, 8, 16385)):
        assert size(*args) == 0, args
    assert size(1000, 3000, 100, 200) >= 8 * 100 * 200 + 12 * 1000 + 4 * 3000


def test_mesh_nerf_takes_render_views_and_refuses_the_script_route():
    from nerfmeshes_amd import mesh_nerf
    args = mesh_nerf.build_parser().parse_args(["--render-views", "3", "--render-size", "100"])
    assert args.render_views == 3 and args.render_size == 100
    off = mesh_nerf.build_parser().parse_args([])
    assert off.render_views == 0 and off.render_size == 800
    bad = mesh_nerf.build_parser().parse_args(["--render-views", "2", "--route", "script", "--save-dir", "."])
    with pytest.raises(ValueError, match="--render-views has no --route script"):
        mesh_nerf.export_marching_cubes(None, bad, None, "cpu")
