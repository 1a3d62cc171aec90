"""GPU: nm_tsdf_integrate against the numpy restatement (tests/tsdf_fuse.py) -- the field's bytes, the observation counts and the
three counters, exactly -- on the edge scenes of tests/test_tsdf_fuse.py (which checks on the CPU that they contain the edges:
voxels behind a camera and at z == near, outside every frustum, projections on exact halves and on the frustum's edges, depths
that are NaN, infinite, zero and negative, opacities at the threshold, NaN and absent, z - D exactly trunc and one ulp above),
sub-ranges off the wave and workgroup boundaries, repeated runs on two streams, and `mesh_nerf --geometry tsdf` end to end on
the suite's synthetic checkpoint, on one rank and on two."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

from tests import tsdf_fuse as TF
from tests.test_tsdf_fuse import GRIDS, IMAGES, TRUNC_KEPT, TRUNC_OCCLUDED, VIEW_COUNTS, edge_scene
from tests.gpu_support import assert_ranks_ok, export_args, export_mesh, launch_ranks, scene_model
from tests.gpu_support import ops  # noqa: F401

pytestmark = pytest.mark.gpu


def _device(ops, scene, trunc, first=0, count=None):
    views = [ops.make_view(v["c2w"], v["height"], v["width"], v["focal"]) for v in scene["views"]]
    opacity = None if scene["opacity"] is None else torch.from_numpy(scene["opacity"]).cuda()
    out = ops.tsdf_integrate(views, torch.from_numpy(scene["depth"]).cuda(), opacity, [torch.from_numpy(a).cuda() for a in scene["axes"]],
                             trunc, scene["near"], min_opacity=scene["min_opacity"], first=first, count=count, want_observations=True)
    return out["field"].cpu().numpy(), out["observations"].cpu().numpy(), out["counts"].cpu().numpy()


def _restated(scene, trunc, first=0, count=None):
    return TF.integrate(scene["views"], scene["depth"], scene["opacity"], scene["axes"], trunc, scene["near"], scene["min_opacity"],
                        first, count)


def _same(got, want, tag):
    assert got[0].dtype == want[0].dtype == np.float32 and got[0].shape == want[0].shape, tag
    bad = np.flatnonzero(got[0].view(np.uint32) != want[0].view(np.uint32))
    assert bad.size == 0, f"{tag}: {bad.size} field values differ, first at {bad[:5]}: {got[0][bad[:5]]} for {want[0][bad[:5]]}"
    assert got[1].dtype == np.int32 and (got[1] == want[1]).all(), f"{tag}: observations"
    assert got[2].dtype == np.int64 and got[2].tolist() == want[2].tolist(), f"{tag}: counts {got[2]} for {want[2]}"


@pytest.mark.parametrize("image", IMAGES, ids=lambda i: f"{i[0]}x{i[1]}")
@pytest.mark.parametrize("num_views", VIEW_COUNTS)
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_the_edge_scenes(ops, grid, num_views, image):
    for with_opacity in (True, False):
        scene = edge_scene(grid, num_views, image, with_opacity)
        for trunc in (TRUNC_KEPT, TRUNC_OCCLUDED):
            want = _restated(scene, trunc)
            print(f"opacity {with_opacity} trunc {trunc!r}: counts {want[2].tolist()}, observations up to {want[1].max()}")
            _same(_device(ops, scene, trunc), want, f"opacity {with_opacity}, trunc {trunc!r}")


# (2,3,300): 1800 voxels = 7 workgroups of 256 and a bit; starts and ends off the 64-lane and the 256-lane boundaries
RANGES = ((37, 300), (100, 1), (255, 513), (1, 1799), (1790, 10), (64, 192), (700, 0))


def test_sub_ranges_equal_the_slices_of_the_whole(ops):
    scene = edge_scene(GRIDS[2], 17, IMAGES[1])
    whole = _device(ops, scene, TRUNC_KEPT)
    _same(whole, _restated(scene, TRUNC_KEPT), "whole")
    for first, count in RANGES:
        got = _device(ops, scene, TRUNC_KEPT, first, count)
        assert got[0].tobytes() == whole[0][first:first + count].tobytes(), (first, count)
        assert (got[1] == whole[1][first:first + count]).all() and got[2].sum() == count, (first, count)
        _same(got, _restated(scene, TRUNC_KEPT, first, count), f"range {first}+{count}")


def test_three_runs_one_on_a_second_stream_give_the_same_bytes(ops):
    scene = edge_scene(GRIDS[1], 17, IMAGES[1])
    first = _device(ops, scene, TRUNC_KEPT)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        second = _device(ops, scene, TRUNC_KEPT)
    side.synchronize()
    third = _device(ops, scene, TRUNC_KEPT)
    for other in (second, third):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, other))


def test_what_the_wrapper_refuses(ops):
    scene = edge_scene(GRIDS[0], 2, IMAGES[0])
    for trunc, near in ((0.0, 1.0), (0.25, 0.0), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="finite and > 0"):
            ops.tsdf_integrate([ops.make_view(v["c2w"], 8, 8, 4.0) for v in scene["views"]], torch.from_numpy(scene["depth"]).cuda(), None,
                               [torch.from_numpy(a).cuda() for a in scene["axes"]], trunc, near)
    with pytest.raises(ValueError, match="outside the grid"):
        _device(ops, scene, 0.25, 4, 5)
    with pytest.raises(ValueError, match="one image per view"):
        ops.tsdf_integrate([ops.make_view(scene["views"][0]["c2w"], 8, 8, 4.0)], torch.from_numpy(scene["depth"]).cuda(), None,
                           [torch.from_numpy(a).cuda() for a in scene["axes"]], 0.25, 1.0)


@pytest.fixture(scope="module")
def model():
    return scene_model("cuda", chunksize=3000)


TSDF = ("--geometry", "tsdf", "--res", "24", "--tsdf-views", "6", "--tsdf-size", "48")


def _parse(directory, *extra):
    return export_args(directory, "--limit", "1.2", *extra)


def _run(model, tmp_path, tag, *extra):
    d = tmp_path / tag
    d.mkdir(exist_ok=True)
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        export_mesh(model, d, "--limit", "1.2", *extra)
    return d, text.getvalue()


def test_the_exporters_field_is_the_restatement_of_what_query_view_returned(model, tmp_path):
    """The depth enters the fusion along the camera's axis: query_view's, which is measured along the unit ray, over the length of
    the pixel's (x, y, -1) -- an fp64 division rounded to fp32, done here in numpy."""
    from nerfmeshes_amd import mesh_nerf, mesh_render
    args = _parse(tmp_path, *TSDF)
    cfg = model.cfg
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        vertices, triangles, normals, field = mesh_nerf.extract_geometry_tsdf(model, "cuda", args, cfg)
        size, focal = 48, mesh_nerf.tsdf_focal(args)
        poses = mesh_render.sphere_poses(6, (0.0, 0.0, 0.0), 4.0)
        bounds = torch.tensor([cfg.dataset.near, cfg.dataset.far], dtype=torch.float32)
        outs = [model.query_view(torch.from_numpy(p), size, size, focal, bounds, keep_depth=True) for p in poses]
    x = (np.arange(size, dtype=np.float64) - 24.0) / focal
    lengths = np.sqrt(x[None, :] ** 2 + x[:, None] ** 2 + 1.0)
    assert np.abs(lengths - mesh_render.ray_lengths(size, size, focal, "cpu").numpy()).max() < 1e-6, "the renderer's own ray lengths"
    depth = np.stack([(o.depth_map.view(size, size).cpu().numpy().astype(np.float64) / lengths).astype(np.float32) for o in outs])
    opacity = np.stack([o.acc_map.view(size, size).cpu().numpy() for o in outs])
    assert focal == 1111.1111 * 48 / 800.0 and (opacity >= 0.5).any() and (opacity < 0.5).any()
    axes = [torch.linspace(-1.2, 1.2, 24).numpy()] * 3         # the density grid's own axes: torch's fp32 linspace on the host
    assert all((a == t.cpu().numpy()).all() for a, t in zip(axes, mesh_nerf._axes(args, (24, 24, 24), "cuda")))
    want = TF.integrate([TF.view(p, size, size, focal) for p in poses], depth, opacity, axes, 3.0 * 2.4 / 23, cfg.dataset.near, 0.5)
    got = field.cpu().numpy()
    assert got.shape == (24, 24, 24) and got.tobytes() == want[0].tobytes()
    report = json.load(open(tmp_path / "mesh.tsdf.json"))
    assert [report["voxels"][k] for k in ("observed", "interior", "outside")] == want[2].tolist()
    assert report["vertices"] == vertices.shape[0] > 0 and report["faces"] == triangles.shape[0] > 0
    assert report["views"] == 6 and report["size"] == 48 and report["trunc_voxels"] == 3.0 and report["level"] == 0.0
    assert list(report)[-1] == "seconds" and sorted(report["seconds"]) == ["integrate", "marching_cubes", "render"]
    # the mesh is the field's zero level, in the exporter's coordinates
    from nerfmeshes_amd import hip_ops
    v, f, n, _ = hip_ops.marching_cubes(field, 0.0)
    assert torch.equal(vertices, 1.2 * (v / 12.0 - 1.0)) and torch.equal(triangles, f) and torch.equal(normals, n)


def test_end_to_end_and_the_density_geometry_is_untouched(model, tmp_path):
    plain, plain_text = _run(model, tmp_path, "plain", "--res", "24")
    named, named_text = _run(model, tmp_path, "named", "--res", "24", "--geometry", "density")
    assert open(named / "mesh.obj", "rb").read() == open(plain / "mesh.obj", "rb").read(), "--geometry density is today's OBJ byte for byte"
    assert named_text.replace(str(named), "") == plain_text.replace(str(plain), "") and sorted(os.listdir(named)) == sorted(os.listdir(plain))
    assert "TSDF" not in plain_text and not os.path.exists(plain / "mesh.tsdf.json")
    fused, text = _run(model, tmp_path, "fused", *TSDF, "--render-views", "2", "--render-size", "48")
    again, _ = _run(model, tmp_path, "again", *TSDF, "--render-views", "2", "--render-size", "48")
    lines = open(fused / "mesh.obj").read().splitlines()
    report = json.load(open(fused / "mesh.tsdf.json"))
    count = lambda key: sum(1 for row in lines if row.startswith(key + " "))   # noqa: E731
    assert report["vertices"] == count("v") == count("vn") > 0 and report["faces"] == count("f") > 0
    assert sum(report["voxels"].values()) == 24 ** 3
    assert (f"TSDF: 6 views of 48² fused into 24 x 24 x 24 voxels: {report['voxels']['observed']} observed, "
            f"{report['voxels']['interior']} interior") in text and "Querying based on iso level" not in text
    assert os.path.exists(fused / "mesh.render.json"), "the stages after the geometry run on the fused mesh"
    assert open(again / "mesh.obj", "rb").read() == open(fused / "mesh.obj", "rb").read()
    print(text)


def test_two_ranks_sharing_one_gpu_equal_one_rank():
    """both --gather modes in one launch of the worker: the OBJ byte for byte, and the report byte for byte up to its last entry,
    the seconds, which no two runs share"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X")
    world = 2
    r = launch_ranks(os.path.join("tests", "tools", "tsdf_dist_worker.py"), world, timeout=900)
    assert_ranks_ok(r, f"TSDF_DIST_OK world={world}")
