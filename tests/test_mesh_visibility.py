"""CPU: the hidden-face rule as tests/mesh_visibility.py restates it (nested spheres with the exact counts, a shell with a window,
the rings, bad indices, the empty cases), mesh_render.sphere_views and its framing, the argument errors of the three C entries
(which return before any HIP call) and the new mesh_nerf options."""
import ctypes as C

import numpy as np
import pytest

from tests import mesh_metrics as MM
from tests import mesh_visibility as MV
from tests.test_mesh_raster import sheet

F32 = np.float32


def nested_spheres():
    """MM.uv_sphere(32, 16, 1.0) -- 1024 faces, 64 of them degenerate -- around MM.uv_sphere(16, 8, 0.5), 256 faces"""
    vo, fo = MM.uv_sphere(32, 16, 1.0)
    vi, fi = MM.uv_sphere(16, 8, 0.5)
    return np.concatenate((vo, vi)), np.concatenate((fo, fi + len(vo))).astype(np.int32)


def windowed_shell():
    """the nested spheres with a window in the outer one: its faces around the +x axis are gone"""
    verts, faces = nested_spheres()
    centroid = verts[faces[:1024]].astype(np.float64).mean(axis=1)
    window = np.zeros(len(faces), bool)
    window[:1024] = centroid[:, 0] > 0.75
    assert 40 < window.sum() < 200
    return verts, faces[~window], int((~window[:1024]).sum())


def vertex_normals(verts):
    """some per-vertex rows to carry through the compaction"""
    return np.random.default_rng(len(verts)).standard_normal((len(verts), 3)).astype(F32)


def framed(verts, views, size, cull_radius=3.0):
    """-> (poses, size, focal, near) of `views` cameras around the mesh"""
    centre, radius, focal, near = MV.frame(verts, cull_radius, size)
    return MV.sphere_poses(views, centre, radius), size, focal, near


def degenerate(verts, faces):
    t = verts[faces].astype(np.float64)
    return (np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]) ** 2).sum(-1) == 0


NESTED = [(8, 48, 0), (8, 48, 1), (24, 96, 0)]                       # views, size, rings


@pytest.fixture(scope="module")
def nested():
    """the restatement on the nested spheres, once per case: (verts, faces, normals, camera, result)"""
    verts, faces = nested_spheres()
    normals = vertex_normals(verts)
    out = {}
    for views, size, rings in NESTED:
        camera = framed(verts, views, size)
        out[views, size, rings] = verts, faces, normals, camera, MV.cull_hidden(verts, faces, normals, *camera, rings)
    return out


def test_nested_spheres_lose_the_inner_one_and_nothing_else(nested):
    verts, faces = nested_spheres()
    flat = degenerate(verts, faces)
    assert len(faces) == 1280 and flat[:1024].sum() == 64
    want = {(8, 48, 0): (37, 923), (8, 48, 1): (0, 1024), (24, 96, 0): (0, 960)}
    for case, (left_out, outer_kept) in want.items():
        _, _, _, _, (_, _, _, index, info) = nested[case]
        keep = np.zeros(len(faces), bool)
        keep[index] = True
        assert int((~keep[:1024] & ~flat[:1024]).sum()) == left_out, case
        assert int(keep[:1024].sum()) == outer_kept and int(keep[1024:].sum()) == 0, case
        assert info["faces_kept"] == outer_kept and info["faces"] == 1280 and info["bad_faces"] == 0
        assert sum(info["new_faces"]) == info["faces_seen"] and len(info["new_faces"]) == case[0]
    assert nested[8, 48, 0][4][4]["new_faces"][:6] == [300, 158, 117, 84, 86, 78]
    assert nested[8, 48, 1][4][4]["faces_seen"] == 923, "the rings do not change what was seen"
    assert nested[24, 96, 0][4][4]["faces_seen"] == 960 == int((~flat[:1024]).sum()), "every face with an area is seen"


def test_the_renumbering_is_numpys(nested):
    for verts, faces, normals, _, (ov, of, on, index, info) in nested.values():
        keep_f = np.zeros(len(faces), bool)
        keep_f[index] = True
        keep_v = np.zeros(len(verts), bool)
        keep_v[faces[keep_f].reshape(-1)] = True
        new = np.cumsum(keep_v) - 1
        assert (np.diff(index) > 0).all() and index.dtype == np.int32, "the kept faces in their original order"
        assert of.dtype == np.int32 and of.tobytes() == new[faces[keep_f]].astype(np.int32).tobytes()
        assert ov.tobytes() == verts[keep_v].tobytes() and on.tobytes() == normals[keep_v].tobytes()
        assert info["vertices_kept"] == keep_v.sum() == len(ov) and (ov[of] == verts[faces[index]]).all()


def test_a_shell_with_a_window_shows_part_of_the_inner_sphere():
    verts, faces, outer = windowed_shell()
    poses, size, focal, near = framed(verts, 8, 48)
    seen, new_faces, _ = MV.seen_faces(verts, faces, poses, size, focal, near)
    inner = seen[outer:]
    assert 0 < inner.sum() < len(inner) - 32, "some inner faces are seen through the window, some are not"
    kept = [MV.grow(faces, len(verts), seen, rings)[0] for rings in range(4)]
    assert (kept[0] == seen).all()
    for a, b in zip(kept, kept[1:]):
        assert (b[a]).all() and b.sum() > a.sum(), "the kept set grows with the rings"
    assert kept[3][outer:].sum() < len(inner), "three rings do not reach around the inner sphere"
    before = np.zeros(len(faces), bool)
    for k in (1, 3, 8):                                              # a prefix of the views sees a subset
        part, counts, _ = MV.seen_faces(verts, faces, poses[:k], size, focal, near)
        assert part[before].all() and counts == new_faces[:k]
        before = part
    assert (before == seen).all()
    first, _, _ = MV.seen_faces(verts, faces, poses[:3], size, focal, near)
    both, later, _ = MV.seen_faces(verts, faces, poses[3:], size, focal, near, seen=first)
    assert (both == seen).all() and later == new_faces[3:], "accumulating over two calls is one call over all views"
    ov, of, on, index, info = MV.cull_hidden(verts, faces, None, poses, size, focal, near, 1)
    assert on is None and (index == np.nonzero(kept[1])[0]).all() and info["faces_kept"] == kept[1].sum()


FIXED = (MV.sphere_poses(3, (0.0, 0.0, 0.0), 4.0), 32, 30.0, F32(0.1))   # a camera that needs no mesh to frame


def small_cases():
    """name -> (verts, faces, normals | None, (poses, size, focal, near), rings): fewer than 64 faces, a face count that is no
    multiple of 64, bad indices, and the three ways of being empty"""
    sv, sf, _ = sheet()
    tri = np.array([[-1, -1, 0], [1, -1, 0], [0, 1, 0]], F32)
    verts, faces = nested_spheres()
    bad = faces.copy()
    rows = np.random.default_rng(4).choice(len(bad), 30, replace=False)
    bad[rows, np.arange(30) % 3] = np.resize([-1, len(verts), 2 ** 31 - 1, -2 ** 31], 30)
    return {
        "one_face": (tri, np.array([[0, 1, 2]], np.int32), vertex_normals(tri), framed(tri, 2, 16), 0),
        "sheet_of_70": (sv, sf[:70], vertex_normals(sv), framed(sv, 4, 40), 0),
        "sheet_of_128_one_ring": (sv, sf, None, framed(sv, 4, 24), 1),
        "bad_indices": (verts, bad, vertex_normals(verts), framed(verts, 4, 48), 1),
        "no_faces": (sv, np.zeros((0, 3), np.int32), vertex_normals(sv), FIXED, 1),
        "nothing": (np.zeros((0, 3), F32), np.zeros((0, 3), np.int32), np.zeros((0, 3), F32), FIXED, 1),
        "no_views": (sv, sf, vertex_normals(sv), (FIXED[0][:0],) + FIXED[1:], 2),
    }


def test_small_bad_and_empty_inputs():
    cases = small_cases()
    results = {name: MV.cull_hidden(v, f, n, *camera, rings) for name, (v, f, n, camera, rings) in cases.items()}
    assert results["one_face"][4] == dict(faces=1, faces_seen=1, faces_kept=1, vertices=3, vertices_kept=3, bad_faces=0,
                                          new_faces=[1, 0])
    info = results["sheet_of_70"][4]
    assert info["faces_kept"] == info["faces_seen"] and 0 < info["faces_kept"] <= 70 and info["vertices_kept"] < 81
    assert results["sheet_of_128_one_ring"][4]["faces_kept"] == 128 and results["sheet_of_128_one_ring"][2] is None
    ov, of, on, index, info = results["bad_indices"]
    verts, faces = cases["bad_indices"][:2]
    assert info["bad_faces"] == 30 and info["faces_kept"] > 500
    assert ((faces[index] >= 0) & (faces[index] < len(verts))).all(), "a face with a bad index is never kept"
    assert (of >= 0).all() and (of < len(ov)).all()
    for name in ("no_faces", "nothing", "no_views"):
        ov, of, on, index, info = results[name]
        assert ov.shape == (0, 3) and of.shape == (0, 3) and on.shape == (0, 3) and index.shape == (0,), name
        assert info["faces_kept"] == info["faces_seen"] == info["vertices_kept"] == info["bad_faces"] == 0
    assert results["no_views"][4]["new_faces"] == [] and results["nothing"][4]["new_faces"] == [0, 0, 0]


def test_sphere_views_look_at_the_centre_from_all_around():
    from nerfmeshes_amd import mesh_render
    centre = np.array([0.3, -0.2, 0.1])
    for count in (1, 2, 7, 64, 500):
        poses = mesh_render.sphere_poses(count, centre, 2.5)
        assert poses.dtype == F32 and poses.shape == (count, 3, 4)
        assert poses.tobytes() == MV.sphere_poses(count, centre, 2.5).tobytes(), "the restatement's cameras are the product's"
        rot, eye = poses[:, :, :3].astype(np.float64), poses[:, :, 3].astype(np.float64)
        assert np.abs(rot.transpose(0, 2, 1) @ rot - np.eye(3)).max() < 1e-6, "orthonormal"
        assert np.abs(np.linalg.det(rot) - 1).max() < 1e-6, "right-handed"
        assert np.abs(np.linalg.norm(eye - centre, axis=1) - 2.5).max() < 1e-6
        assert np.abs((centre - eye) / 2.5 + rot[:, :, 2]).max() < 1e-6, "the camera looks along -z at the centre"
        assert abs(eye[:, 2].mean() - centre[2]) < 1e-6, "z_k = -z_(count-1-k): as many cameras above as below"
    views = list(mesh_render.sphere_views(5, centre, 2.5, 96, 120.0))
    assert len(views) == 5 and all(v[1:] == (96, 96, 120.0, None) for v in views)


def test_the_framing_shows_the_whole_mesh_and_clears_the_near_plane():
    import torch
    from nerfmeshes_amd import mesh_render
    verts, faces = nested_spheres()
    verts = verts * F32(0.7) + np.array([0.5, -1.0, 0.25], F32)
    got = mesh_render.frame_views(torch.from_numpy(verts), 3.0, 48)
    want = MV.frame(verts, 3.0, 48)
    assert (got[0] == want[0]).all() and got[1:] == (want[1], want[2], float(want[3])), "the restatement's framing is the product's"
    centre, radius, focal, near = want
    rb = radius / 3.0
    assert abs(focal * rb / np.sqrt(radius ** 2 - rb ** 2) - 0.95 * 24) < 1e-9, "the bounding sphere's outline: 95 % of the half side"
    assert near == F32((radius - rb) / 2)
    for pose in MV.sphere_poses(16, centre, radius):
        x, y, w, finite, in_range = MV.MR.project(verts, pose, 48, 48, focal)
        assert finite.all() and in_range.all() and (w > near).all() and w.min() >= radius - rb - 1e-5
        assert x.min() >= 0 and x.max() <= 47 * 256 and y.min() >= 0 and y.max() <= 47 * 256
    for bad in (1.0, 0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            mesh_render.frame_views(torch.from_numpy(verts), bad, 48)
    with pytest.raises(ValueError):
        mesh_render.frame_views(torch.zeros(0, 3), 3.0, 48)
    with pytest.raises(ValueError):
        mesh_render.frame_views(torch.ones(4, 3), 3.0, 48)


def test_mesh_nerf_takes_the_cull_options_and_refuses_the_script_route():
    from nerfmeshes_amd import mesh_nerf
    off = mesh_nerf.build_parser().parse_args([])
    assert (off.cull_hidden_views, off.cull_size, off.cull_rings, off.cull_radius) == (0, 0, 1, 3.0)
    on = mesh_nerf.build_parser().parse_args(["--cull-hidden-views", "64", "--cull-size", "512", "--cull-rings", "0",
                                              "--cull-radius", "2.5"])
    assert (on.cull_hidden_views, on.cull_size, on.cull_rings, on.cull_radius) == (64, 512, 0, 2.5)
    assert mesh_nerf.cull_size(480) == 1792 and mesh_nerf.cull_size(64) == 256 and mesh_nerf.cull_size(10 ** 6) == 16384
    assert all(mesh_nerf.cull_size(res) * 0.95 / (np.sqrt(3.0) * res) >= 2 for res in (16, 128, 480, 1000, 2000))
    helps = {a.option_strings[0]: a.help for a in mesh_nerf.build_parser()._actions if a.option_strings}
    for option in ("--cull-hidden-views", "--cull-size", "--cull-rings", "--cull-radius"):
        assert helps[option].startswith("(addition)"), option
    for extra in (["--cull-hidden-views", "2"], ["--cull-rings", "3"]):
        bad = mesh_nerf.build_parser().parse_args(extra + ["--route", "script", "--save-dir", "."])
        with pytest.raises(ValueError, match="--cull-hidden-views / --cull-size / --cull-rings / --cull-radius have no --route script"):
            mesh_nerf.export_marching_cubes(None, bad, None, "cpu")
    for extra in (["--cull-radius", "1.0"], ["--cull-radius", "nan"], ["--cull-size", "16385"], ["--cull-rings", "1025"]):
        bad = mesh_nerf.build_parser().parse_args(["--cull-hidden-views", "2", "--save-dir", "."] + extra)
        with pytest.raises(ValueError, match="--cull-radius finite and > 1"):
            mesh_nerf.export_marching_cubes(None, bad, None, "cpu")


@pytest.fixture(scope="module")
def lib():
    from nerfmeshes_amd import _lib
    return _lib.load()


def test_argument_errors_return_2_before_any_hip_call(lib):
    from nerfmeshes_amd import _lib, hip_ops
    good = hip_ops.make_view(np.eye(4, dtype=F32), 8, 8, 10.0)
    ndc = hip_ops.make_view(np.eye(4, dtype=F32), 8, 8, 10.0, ndc_near=1.0)
    p = C.c_void_p(256)                                              # never dereferenced: every call fails its checks first

    def views(views=(good, good), count=None, verts=p, nv=3, faces=p, nf=1, near=0.1, threshold=16, clear=1, ws=p, new=p, counts=p):
        array = (_lib.View * max(len(views), 1))(*views) if views is not None else None
        return lib.nm_mesh_visibility_views(array, len(views) if count is None else count, verts, nv, faces, nf, near, threshold,
                                            clear, ws, new, counts, None)

    for name in ("verts", "faces", "ws", "new"):
        assert views(**{name: None}) == 2, name
        assert b"bad argument" in lib.nm_last_error()
    assert views(views=None, count=2) == 2 and b"bad argument" in lib.nm_last_error()
    assert views(count=-1) == 2 and b"num_views" in lib.nm_last_error()
    assert views(views=(good, ndc)) == 2 and b"NDC" in lib.nm_last_error(), "the rasteriser's words"
    for near in (0.0, -1.0, float("nan"), float("inf")):
        assert views(near=near) == 2 and b"near" in lib.nm_last_error()
    assert views(threshold=-1) == 2 and b"large_threshold" in lib.nm_last_error()
    assert views(nv=0) == 2 and b"faces without vertices" in lib.nm_last_error()
    assert views(nf=-1) == 2 and views(nv=2 ** 31 - 64) == 2
    assert views(views=(good, hip_ops.make_view(np.eye(4, dtype=F32), 0, 8, 10.0))) == 2 and b"height and width" in lib.nm_last_error()
    assert views(views=(hip_ops.make_view(np.eye(4, dtype=F32), 8, 16385, 10.0),)) == 2
    assert views(views=(hip_ops.make_view(np.eye(4, dtype=F32), 8, 8, float("nan")),)) == 2 and b"focal" in lib.nm_last_error()

    out = [C.c_int64() for _ in range(4)]

    def select(faces=p, nf=1, nv=3, rings=1, ws=p, skip=None):
        refs = [None if k == skip else C.byref(o) for k, o in enumerate(out)]
        return lib.nm_mesh_visibility_select(faces, nf, nv, rings, ws, *refs, None)

    for kw in (dict(faces=None), dict(ws=None), dict(skip=0), dict(skip=1), dict(skip=2), dict(skip=3)):
        assert select(**kw) == 2 and b"bad argument" in lib.nm_last_error(), kw
    for rings in (-1, 1025):
        assert select(rings=rings) == 2 and b"rings" in lib.nm_last_error()
    assert select(nv=0) == 2 and select(nf=-1) == 2 and select(nf=2 ** 31 - 64) == 2

    def compact(ws=p, faces=p, nf=4, nv=6, verts=p, normals=p, kv=3, kf=1, out_verts=p, out_faces=p, out_normals=p, index=p):
        return lib.nm_mesh_visibility_compact(ws, faces, nf, nv, verts, normals, kv, kf, out_verts, out_faces, out_normals, index, None)

    for name in ("ws", "faces"):
        assert compact(**{name: None}) == 2 and b"bad argument" in lib.nm_last_error(), name
    for name in ("out_verts", "out_normals"):
        assert compact(**{name: None}) == 2 and b"an input array without its output" in lib.nm_last_error(), name
    assert compact(out_faces=None) == 2 and b"null face output" in lib.nm_last_error()
    for kw in (dict(kv=7), dict(kv=-1), dict(kf=5), dict(kf=-1)):
        assert compact(**kw) == 2 and b"kept counts" in lib.nm_last_error(), kw
    assert compact(nv=0) == 2 and compact(nf=-1) == 2

    size = lib.nm_mesh_visibility_workspace_bytes
    assert size(10, 20, 8, 8) > 0 and size(0, 0, 1, 1) > 0
    for args in ((-1, 0, 8, 8), (0, -1, 8, 8), (2 ** 31 - 64, 0, 8, 8), (0, 2 ** 31 - 64, 8, 8), (1, 1, 0, 8), (1, 1, 8, 0),
                 (1, 1, 16385, 8), (1, 1, 8, 16385)):
        assert size(*args) == 0, args
    words = lambda n: 8 * ((n + 63) // 64)                           # noqa: E731
    assert size(1000, 3000, 100, 200) >= lib.nm_mesh_raster_workspace_bytes(1000, 3000, 100, 200) + 3 * words(3000) + words(1000)
    assert size(1000, 3000, 100, 200) - size(1000, 3000, 1, 1) == 8 * 100 * 200 - 256, "only the pixels' words grow with the image"
