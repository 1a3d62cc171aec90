"""GPU: the mesh rasteriser (nm_mesh_rasterize, nm_mesh_interpolate, mesh_render, mesh_nerf --render-views).  Coverage is
integer work and visibility a 64-bit minimum, so every comparison with the numpy restatement (tests/mesh_raster.py) is exact
-- bytes, dtype, shape and the counts: single triangles, sheets, a sphere, a soup full of ties, bad vertices and indices,
duplicates, a face behind the near plane and one larger than the screen, both paths at every threshold, run after run; then
render_mesh on a colour ramp, the exporter and the command line end to end, 2 ranks against 1."""
import json
import os

import numpy as np
import pytest
import torch

from nerfmeshes_amd import synthetic as S
from tests import mesh_metrics as MM
from tests import mesh_raster as MR
from tests.test_mesh_raster import SPHERE_VIEWS, reject_mesh, sheet
from tests.gpu_support import assert_ranks_ok, export_mesh, launch_ranks, to_device as _dev
from tests.gpu_support import ops, scene  # noqa: F401

pytestmark = pytest.mark.gpu
F32 = np.float32


def _np(t):
    return t.cpu().numpy()


def _attributes(verts):
    rng = np.random.default_rng(len(verts))
    return rng.random((len(verts), 6), dtype=F32)


BACKGROUND = (0.25, 0.5, 0.75, 1.0, 0.0, -1.0)


def _device(ops, verts, faces, pose, height, width, focal, near, **kw):
    view = ops.make_view(pose, height, width, focal)
    raster = ops.mesh_rasterize(_dev(verts, F32).reshape(-1, 3), _dev(faces, np.int32).reshape(-1, 3), view, near, **kw)
    image = ops.mesh_interpolate(raster, _dev(faces, np.int32).reshape(-1, 3), _dev(_attributes(verts)), BACKGROUND)
    return _np(raster[0]), _np(raster[1]), _np(raster[2]), raster[3], _np(image)


def _check(ops, verts, faces, pose, height, width, focal, near, tag, **kw):
    """the device against the restatement -> the restatement's result"""
    want = MR.rasterize(verts, faces, pose, height, width, focal, near, **kw)
    want = want + (MR.interpolate(want[0], want[2], faces, _attributes(verts), BACKGROUND),)
    got = _device(ops, verts, faces, pose, height, width, focal, near, **kw)
    for name, a, b in zip(("face_id", "depth", "bary", "counts", "image"), got, want):
        if name == "counts":
            assert a == b, f"{tag}: counts {a} != {b}"
        else:
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{tag}: {name} differ"
    return want


def front_pose(distance):
    pose = np.eye(4, dtype=F32)
    pose[2, 3] = distance
    return pose


SIZES = [(1, 1), (7, 5), (64, 64), (65, 63)]


@pytest.mark.parametrize("height, width", SIZES)
def test_one_triangle_and_the_sheets(ops, height, width):
    focal = 0.9 * max(height, width)
    tri = np.array([[-0.8, -0.7, 0.1], [0.9, -0.5, -0.2], [0.1, 0.85, 0.3]], F32)
    one = _check(ops, tri, [[0, 1, 2]], front_pose(2.0), height, width, focal, 0.1, f"one triangle {height}x{width}")
    assert one[3]["drawn"] + one[3]["off_screen"] == 1 and (one[3]["covered"] > 0) == (min(height, width) > 1)
    _check(ops, tri, [[0, 2, 1]], front_pose(2.0), height, width, focal, 0.1, "the other winding", cull_back=True)
    for snap in (False, True):
        verts, faces, _ = sheet(snap=snap)
        _check(ops, verts, faces, front_pose(3.0), height, width, 1.25 * max(height, width), 0.1, f"sheet {snap} {height}x{width}")
    verts, faces, pose = sheet()
    own = _check(ops, verts, faces, pose, 48, 48, 60.0, 0.1, "the sheet at its own size")
    assert own[3]["covered"] == 1600


@pytest.mark.parametrize("angles, height, width, focal", SPHERE_VIEWS)
def test_the_sphere(ops, angles, height, width, focal):
    verts, faces = MM.uv_sphere(64, 32)
    want = _check(ops, verts, faces, S.pose_spherical(*angles), height, width, focal, 0.1, f"sphere {angles}")
    assert want[3]["covered"] > 500 and want[3]["degenerate"] > 0
    _check(ops, verts, faces, S.pose_spherical(*angles), height, width, focal, 0.1, f"sphere {angles} culled", cull_back=True)


def soup(n=1500, faces=5000, seed=5):
    """random triangles with vertices on a coarse lattice: massive depth and edge ties"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-4, 5, (n, 3)) * 0.25).astype(F32), rng.integers(0, n, (faces, 3)).astype(np.int32)


@pytest.fixture(scope="module")
def soup_case():
    verts, faces = soup()
    pose = S.pose_spherical(20.0, -25.0, 4.0)
    return verts, faces, pose, MR.rasterize(verts, faces, pose, 128, 128, 140.0, 0.1)


def test_a_soup_full_of_ties(ops, soup_case):
    verts, faces, pose, want = soup_case
    got = _device(ops, verts, faces, pose, 128, 128, 140.0, 0.1)
    assert got[3] == want[3] and all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], want[:3]))
    assert want[3]["covered"] > 3000 and want[3]["large"] > 100


def test_bad_vertices_and_indices_are_counted_not_accessed(ops):
    verts, faces = soup(seed=6)
    rng = np.random.default_rng(7)
    verts[rng.choice(len(verts), 15, replace=False), rng.integers(0, 3, 15)] = [np.nan, np.inf, -np.inf] * 5
    rows = rng.choice(len(faces), 50, replace=False)
    faces[rows, rng.integers(0, 3, 50)] = rng.choice([-1, len(verts), 2 ** 31 - 1, -2 ** 31], 50)
    want = _check(ops, verts, faces, S.pose_spherical(20.0, -25.0, 4.0), 128, 128, 140.0, 0.1, "bad soup")
    assert want[3]["bad_index"] == 50 and want[3]["not_finite"] > 0


def test_duplicates_the_near_plane_a_huge_face_and_the_reject_counts(ops):
    tri = np.array([[-1, -1, 0], [1, -1, 0], [0, 1, 0]], F32)
    twice = _check(ops, tri, [[0, 1, 2], [0, 1, 2], [1, 2, 0]], front_pose(3.0), 64, 64, 60.0, 0.1, "coplanar duplicates")
    assert set(np.unique(twice[0])) == {-1, 0}, "the smallest id wins every tie"
    near = np.array([[-1, -1, 0], [1, -1, 0], [0, 1, 2.95], [0, 1, 0]], F32)
    behind = _check(ops, near, [[0, 1, 2], [0, 1, 3]], front_pose(3.0), 64, 64, 60.0, 0.1, "a corner behind near")
    assert behind[3]["near"] == 1 and behind[3]["drawn"] == 1 and set(np.unique(behind[0])) == {-1, 1}
    huge = np.array([[-90, -80, 0], [95, -70, 1], [3, 99, -1]], F32)
    for size in SIZES:
        for threshold in (0, 2 ** 31 - 1):
            full = _check(ops, huge, [[0, 1, 2]], front_pose(3.0), *size, 60.0, 0.1, f"larger than the screen {size}",
                          large_threshold=threshold)
            assert full[3]["covered"] == size[0] * size[1] and full[3]["large"] == (threshold == 0)
    verts, faces, pose = reject_mesh()
    _check(ops, verts, faces, pose, 32, 32, 40.0, 0.1, "one face per reason", cull_back=True, large_threshold=16)


def test_both_paths_give_the_same_bytes_run_after_run(ops, soup_case):
    sphere = MM.uv_sphere(64, 32) + (S.pose_spherical(30.0, -30.0, 2.2),)
    for verts, faces, pose in (sphere, soup_case[:3]):
        runs = [_device(ops, verts, faces, pose, 128, 128, 140.0, 0.1, large_threshold=t) for t in (None, None, 0, 16, 2 ** 31 - 1)]
        assert runs[0][3]["covered"] > 3000
        for other in runs[1:]:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0][:3] + runs[0][4:], other[:3] + other[4:]))
            assert {k: v for k, v in other[3].items() if k != "large"} == {k: v for k, v in runs[0][3].items() if k != "large"}
        assert runs[2][3]["large"] == runs[2][3]["drawn"] and runs[4][3]["large"] == 0
        assert runs[3][3]["large"] >= runs[0][3]["large"]


def test_empty_inputs_draw_nothing(ops):
    view = ops.make_view(front_pose(3.0), 9, 11, 10.0)
    none = torch.zeros(0, 3, dtype=torch.int32, device="cuda")
    for verts in (torch.zeros(0, 3, device="cuda"), torch.rand(5, 3, device="cuda")):
        face_id, depth, bary, counts = ops.mesh_rasterize(verts, none, view, 0.1)
        assert (face_id == -1).all() and not depth.any() and not bary.any() and not any(counts.values())
        image = ops.mesh_interpolate((face_id, depth, bary), none, torch.zeros(verts.shape[0], 2, device="cuda"), (0.5, 2.0))
        assert image.shape == (9, 11, 2) and (image == torch.tensor([0.5, 2.0], device="cuda")).all()
    with pytest.raises(ValueError):
        ops.mesh_rasterize(torch.rand(5, 3, device="cuda"), none, ops.make_view(front_pose(3.0), 9, 11, 10.0, ndc_near=1.0), 0.1)
    with pytest.raises(ValueError):
        ops.mesh_rasterize(torch.rand(5, 3, device="cuda"), none, view, 0.0)


def test_both_entries_replay_from_a_captured_graph(ops):
    """nothing allocates and nothing waits for the host: the two C entries are captured once and replayed on other vertices"""
    import ctypes as C
    from nerfmeshes_amd import _lib
    lib = _lib.load()
    verts, faces = MM.uv_sphere(64, 32)
    pose, size = S.pose_spherical(30.0, -30.0, 4.0), 64
    view = ops.make_view(pose, size, size, 70.0)
    nv, nf = len(verts), len(faces)
    dv, df, attr = _dev(verts), _dev(faces), _dev(_attributes(verts))
    ws = torch.empty(int(lib.nm_mesh_raster_workspace_bytes(nv, nf, size, size)), dtype=torch.uint8, device="cuda")
    ids = torch.empty(size, size, dtype=torch.int32, device="cuda")
    depth, bary = torch.empty(size, size, device="cuda"), torch.empty(size, size, 3, device="cuda")
    counts = torch.empty(len(ops.RASTER_COUNTS), dtype=torch.int64, device="cuda")
    image, background = torch.empty(size, size, 6, device="cuda"), _dev(np.asarray(BACKGROUND, F32))
    ptr = ops._ptr

    def both():
        _lib.check(lib.nm_mesh_rasterize(C.byref(view), ptr(dv), nv, ptr(df), nf, 0.1, 0, 16, ptr(ws), ptr(ids), ptr(depth), ptr(bary),
                                         ptr(counts), ops._stream()), "nm_mesh_rasterize")
        _lib.check(lib.nm_mesh_interpolate(ptr(ids), ptr(bary), size * size, ptr(df), nf, ptr(attr), nv, 6, ptr(background), ptr(image),
                                           ops._stream()), "nm_mesh_interpolate")

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        both()                                                       # warm-up outside the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        both()
    for scale in (1.0, 0.5):
        dv.copy_(_dev(verts * F32(scale)))
        graph.replay()
        torch.cuda.synchronize()
        want = MR.rasterize(verts * F32(scale), faces, pose, size, size, 70.0, 0.1, large_threshold=16)
        assert _np(ids).tobytes() == want[0].tobytes() and _np(depth).tobytes() == want[1].tobytes()
        assert _np(bary).tobytes() == want[2].tobytes() and dict(zip(ops.RASTER_COUNTS, counts.tolist())) == want[3]
        assert _np(image).tobytes() == MR.interpolate(want[0], want[2], faces, _attributes(verts), BACKGROUND).tobytes()


def test_render_mesh_reproduces_an_affine_colour_ramp(ops):
    """a fronto-parallel quad whose corners lie on pixel centres (no snap), colours affine in the plane and in [0, 1]: three
    fp32 products and two sums per channel"""
    from nerfmeshes_amd import mesh_render
    verts = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], F32)          # 20 pixels per unit at depth 3, f = 60
    ramp = lambda x, y: np.stack((0.5 + 0.25 * x + 0.2 * y, 0.5 - 0.3 * x + 0.1 * y, 0.25 + 0.2 * (y + 1)), -1)  # noqa: E731
    colors = ramp(verts[:, 0].astype(np.float64), verts[:, 1].astype(np.float64)).astype(F32)
    out = mesh_render.render_mesh(verts, np.array([[0, 1, 2], [0, 2, 3]], np.int32), colors, front_pose(3.0), 48, 48, 60.0, 0.1,
                                  (1.0, 1.0, 1.0), normals=np.tile(np.array([[0, 0, 1]], F32), (4, 1)))
    mask = _np(out["mask"])
    assert mask.sum() == 1600 and mask[4:44, 4:44].all() and out["counts"]["covered"] == 1600
    j, i = np.nonzero(mask)
    want = ramp((i - 24) / 20.0, -(j - 24) / 20.0)
    assert np.abs(_np(out["rgb"])[mask] - want).max() <= 1e-5
    assert (_np(out["rgb"])[~mask] == 1.0).all() and (_np(out["depth"])[mask] == 3.0).all() and not _np(out["depth"])[~mask].any()
    assert np.abs(_np(out["normals"])[mask] - [0, 0, 1]).max() <= 1e-6 and (_np(out["face_id"])[mask] >= 0).all()


LIMIT, RES = 1.2, 64


def _run(model, tmp_path, tag, *extra):
    d = tmp_path / tag
    d.mkdir(exist_ok=True)
    return export_mesh(model, d, "--res", str(RES), "--limit", str(LIMIT), *extra), d


@pytest.fixture(scope="module")
def exported(scene, tmp_path_factory):
    """the exporter with and without the option, once"""
    import contextlib
    import io
    tmp = tmp_path_factory.mktemp("raster")
    texts = {}
    runs = {}
    for tag, extra in (("plain", []), ("zero", ["--render-views", "0"]), ("views", ["--render-views", "2", "--render-size", "100"])):
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            runs[tag] = _run(scene, tmp, tag, *extra)
        texts[tag] = text.getvalue()
    return runs, texts


def test_end_to_end_through_the_exporter(ops, scene, exported):
    from nerfmeshes_amd import mesh_render
    runs, texts = exported
    (v, f, n, c), d = runs["views"]
    report = json.load(open(d / "mesh.render.json"))
    assert len(report["views"]) == 2 and set(report) >= {"views", "mean", "counts", "near"}
    cfg = scene.cfg
    bounds = torch.tensor([cfg.dataset.near, cfg.dataset.far], dtype=torch.float32)
    focal = S.LEGO_FOCAL_800 * 100 / 800.0
    colors = torch.as_tensor(c).cuda()
    background = (1.0,) * 3 if cfg.dataset.white_background else (0.0,) * 3
    for nr, pose in enumerate(S.orbit_poses(2)):
        raster = ops.mesh_rasterize(v, f.to(torch.int32), ops.make_view(pose, 100, 100, focal), cfg.dataset.near / 4)
        rgb = ops.mesh_interpolate(raster, f.to(torch.int32), colors, background)
        row = report["views"][nr]
        assert {k: row[k] for k in raster[3]} == raster[3] and raster[3]["covered"] > 500
        with torch.no_grad():
            net = scene.query_view(pose, 100, 100, focal, bounds, keep_depth=True)
        a, b = _np(rgb).reshape(-1, 3).astype(np.float64), _np(net.rgb_map).astype(np.float64)
        want = -10 * np.log10(((a - b) ** 2).mean())
        print(f"view {nr}: PSNR to the network {row['psnr_nerf']} (fp64 {want}), depth {row['depth_mean']} / {row['depth_median']} "
              f"over {row['depth_pixels']} px, IoU {row['iou']}")
        assert abs(row["psnr_nerf"] - want) <= 1e-5 * abs(want)
        mask, acc = _np(raster[0]) >= 0, _np(net.acc_map).reshape(100, 100)
        both = mask & (acc >= 0.99)
        lengths = _np(mesh_render.ray_lengths(100, 100, focal, "cuda"))
        diff = np.abs(_np(raster[1]) * lengths - _np(net.depth_map).reshape(100, 100))[both]
        assert row["depth_pixels"] == both.sum() and row["psnr_target"] is None
        if both.sum():
            assert abs(row["depth_mean"] - diff.astype(np.float64).mean()) <= 1e-6 and row["depth_median"] == float(np.sort(diff)[(len(diff) - 1) // 2])
        solid = acc >= 0.5
        assert abs(row["iou"] - (mask & solid).sum() / max((mask | solid).sum(), 1)) <= 1e-12
    assert report["counts"]["covered"] == sum(r["covered"] for r in report["views"])
    assert "Mesh render: 2 views" in texts["views"] and "Mesh render report saved" in texts["views"]
    plain = open(runs["plain"][1] / "mesh.obj", "rb").read()
    assert open(d / "mesh.obj", "rb").read() == plain, "the OBJ does not see the option"
    assert open(runs["zero"][1] / "mesh.obj", "rb").read() == plain
    strip = lambda t, p: t.replace(str(p), "")                       # noqa: E731
    assert strip(texts["zero"], runs["zero"][1]) == strip(texts["plain"], runs["plain"][1]), "--render-views 0 prints nothing new"
    assert "Mesh render" not in texts["zero"] and not os.path.exists(runs["zero"][1] / "mesh.render.json")


def test_the_command_line_on_the_exported_obj(ops, scene, exported, tmp_path, monkeypatch):
    """mesh_render.main on the OBJ with --views 3 --compare-nerf --out --save-images: the checkpoint loading is replaced by
    the scene in memory (there is no training log here)"""
    from nerfmeshes_amd import mesh_render, models
    runs, _ = exported
    obj = runs["plain"][1] / "mesh.obj"

    class Parser:
        checkpoint_path = "memory"

        def parse(self, *a):
            return scene.cfg, None

    monkeypatch.setattr(mesh_render, "PathParser", Parser)            # the module's own name: nothing else sees the stand-in
    monkeypatch.setattr(getattr(models, scene.cfg.experiment.model), "load_from_checkpoint", classmethod(lambda cls, path: scene))
    out = tmp_path / "report.json"
    report = mesh_render.main(["--mesh", str(obj), "--log-checkpoint", "memory", "--views", "3", "--img-size", "80", "--compare-nerf",
                               "--out", str(out), "--save-images", "--save-depth", "--save-dir", str(tmp_path)])
    saved = json.load(open(out))
    assert len(saved["views"]) == 3 and saved["mesh"]["faces"] == runs["plain"][0][1].shape[0]
    for row in saved["views"]:
        assert set(row) == set(mesh_render.ROW) and row["psnr_nerf"] is not None and 0 <= row["iou"] <= 1 and row["covered"] > 300
    assert set(saved["mean"]) >= {"psnr_nerf", "depth_mean", "depth_median", "iou"} and set(saved["counts"]) == set(ops.RASTER_COUNTS)
    assert saved["views"] == json.loads(json.dumps(report["views"]))
    for nr in range(3):
        assert os.path.getsize(tmp_path / "mesh_images" / f"{nr:04d}.png") > 0 and os.path.getsize(tmp_path / "mesh_depth" / f"{nr:04d}.png") > 0
    turntable = mesh_render.main(["--mesh", str(obj), "--views", "2", "--img-size", "40", "--background", "black"])
    assert len(turntable["views"]) == 2 and turntable["views"][0]["psnr_nerf"] is None


def test_two_ranks_sharing_one_gpu_equal_one_rank():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X")
    world = 2
    r = launch_ranks(os.path.join("tests", "tools", "raster_dist_worker.py"), world, timeout=900)
    assert_ranks_ok(r, f"RASTER_DIST_OK world={world}")
