"""GPU: adaptive levels of mesh simplification (nm_mesh_simplify_adaptive_level / _faces / _emit, mesh_nerf --simplify-levels).
Every level's sums are exact integer sums, its error a maximum and its solve a fixed sequence of fp64 operations, so every
comparison with the numpy restatement (tests/mesh_simplify_adaptive.py) is exact -- bytes, dtype, shape and every key of the
info dict, with and without wave aggregation: the fixture meshes, generated volumes (a single root cell among them), levels = 0
against the quadric placement, a coarse cell that ends CROWDED, faces longer than two coarse cells, the same bytes run after run
and under a renumbering, and the exporter end to end, 2 ranks against 1."""
import os

import numpy as np
import pytest
import torch

from tests import mesh_simplify_adaptive as MA
from tests import mesh_simplify_quadric as MQ
from tests.helpers import load_golden
from tests.gpu_support import assert_ranks_ok, export_mesh, launch_ranks, to_device as _dev, to_numpy as _np
from tests.gpu_support import ops, scene  # noqa: F401

pytestmark = pytest.mark.gpu
INF = float("inf")


def _same(got, want, tag):
    for name, a, b in zip(("verts", "faces", "normals"), got[:3], want[:3]):
        if b is None:
            assert a is None, (tag, name)
            continue
        a = _np(a)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{tag}: {name} differ"
    assert got[3] == want[3] and tuple(got[3]) == tuple(want[3]), (tag, got[3], want[3])


def _check(ops, v, f, n, cell, origin, levels, error, tag, cache=None):
    """with and without wave aggregation against the restatement (computed once; cache: the levels' clusters that the cases of
    one mesh and origin share) -> the restatement's result"""
    want = MA.simplify(_np(v), _np(f), None if n is None else _np(n), cell=cell, origin=origin, levels=levels, max_error=error,
                       cache=cache)
    for aggregate in (False, True):
        got = ops.mesh_simplify(v, f, n, cell=cell, origin=origin, aggregate=aggregate, placement="quadric", levels=levels,
                                max_error=error)
        _same(got, want, f"{tag} aggregate={aggregate}")
    return want


def _cases():
    """the issue's matrix: cell x L x E, E in units of the cell"""
    return [(cell, levels, error) for cell in (1.5, 4.0) for levels in (1, 3) for error in (0.0, 0.05 * cell, INF)]


@pytest.mark.parametrize("part", range(4))
def test_every_fixture_mesh(ops, part):
    """every mesh of mc_cases.npz, the matrix's twelve cases dealt round over them, in four parts"""
    g = load_golden("mc_cases")
    cases = _cases()
    count = coarse = 0
    for i in range(int(g["count"])):
        if f"err_{i}" in g.files:
            continue
        count += 1
        if count % 4 != part:
            continue
        cell, levels, error = cases[(count // 4) % len(cases)]
        v, f, n = g[f"verts_{i}"].astype(np.float32), g[f"faces_{i}"].astype(np.int32), g[f"normals_{i}"].astype(np.float32)
        want = _check(ops, _dev(v), _dev(f), _dev(n), cell, (0, 0, 0), levels, error, f"golden {i} {cell} {levels} {error}")
        coarse += sum(want[3]["level_vertices"][1:])
    assert count == 667 and coarse > 100


def test_the_exported_fixture_mesh_over_the_whole_matrix(ops):
    g = load_golden("export_obj")
    v, f, n = g["vertices"].astype(np.float32), g["triangles"].astype(np.int32), g["normals"].astype(np.float32)
    span = float((v.max(axis=0) - v.min(axis=0)).max())
    for cell, levels, error in _cases():
        scale = cell * span / 40.0                                     # the matrix's cells on a mesh of any extent
        _check(ops, _dev(v), _dev(f), _dev(n), scale, None, levels, error / cell * scale, f"export_obj {cell} {levels} {error}")
    # without normals
    _check(ops, _dev(v), _dev(f), None, span / 20.0, None, 2, span / 400.0, "export_obj, bare")


def _volume(kind, shape, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.standard_normal(shape).astype(np.float32), 0.1
    if kind == "ties":
        return rng.integers(-2, 3, shape).astype(np.float32), 0.0
    g = np.stack(np.meshgrid(*[np.linspace(-1, 1, s) for s in shape], indexing="ij"), -1)
    return (np.sin(3 * g[..., 0]) * np.cos(2 * g[..., 1]) + g[..., 2] ** 2 - 0.3).astype(np.float32), float(np.float32(0.05))


@pytest.fixture(scope="module")
def volumes(ops):
    """(kind, shape) -> (verts, faces, normals, levels): the mesh, and the dict in which the restatement keeps the clusters of
    every level's grid for it (they depend on neither L nor E: computed once for the cases of the matrix); the latest mesh only"""
    cache = {}

    def get(kind, shape):
        if (kind, shape) not in cache:
            cache.clear()
            vol, iso = _volume(kind, shape, sum(shape) * 7 + len(kind))
            v, f, n = ops.marching_cubes(_dev(vol), iso)[:3]
            cache[kind, shape] = (v, f, n, {})
        return cache[kind, shape]
    return get


@pytest.mark.parametrize("error", [0.0, 0.05, INF], ids=["E=0", "E=0.05cell", "E=inf"])
@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("cell", [1.5, 4.0])
@pytest.mark.parametrize("shape", [(17, 5, 33), (33, 130, 77)])
@pytest.mark.parametrize("kind", ["noise", "ties", "smooth"])
def test_on_generated_volumes(ops, volumes, kind, shape, cell, levels, error):
    v, f, n, shared = volumes(kind, shape)
    info = _check(ops, v, f, n, cell, (0, 0, 0), levels, error * cell, f"{shape} {kind} cell {cell} L {levels} E {error}", shared)[3]
    assert info["faces"] > 0 and sum(info["level_vertices"]) == info["vertices"] and info["far_corners"] == 0
    if error == 0.0:
        assert info["largest_error"] == 0.0
    if error == INF and kind == "smooth":
        assert sum(info["level_vertices"][1:]) > 0
    if shape == (17, 5, 33) and cell == 4.0 and levels == 3:
        root = MA.level_clusters(_np(v), _np(f), None, np.zeros(3, np.float32), MA.level_cell(cell, levels))
        assert len(root["first"]) <= 2 and 4.0 * 8 > 17, "K * 2^L is larger than two of the axes: one or two root cells"


def test_levels_zero_is_the_quadric_placement_as_it_is(ops, volumes):
    v, f, n, _ = volumes("smooth", (33, 130, 77))
    want = ops.mesh_simplify(v, f, n, cell=3.0, origin=(0, 0, 0), placement="quadric")
    for kw in (dict(levels=0), dict(levels=0, max_error=0.5), dict(levels=0, max_error=float("nan")), dict(max_error=-3.0)):
        got = ops.mesh_simplify(v, f, n, cell=3.0, origin=(0, 0, 0), placement="quadric", **kw)
        assert all(_np(a).tobytes() == _np(b).tobytes() for a, b in zip(got[:3], want[:3])), kw
        assert got[3] == want[3] and tuple(got[3]) == MQ.INFO_KEYS
    mean = ops.mesh_simplify(v, f, n, cell=3.0, origin=(0, 0, 0), levels=0, max_error=1.0)
    plain = ops.mesh_simplify(v, f, n, cell=3.0, origin=(0, 0, 0))
    assert all(_np(a).tobytes() == _np(b).tobytes() for a, b in zip(mean[:3], plain[:3])) and mean[3] == plain[3]


def test_a_hot_coarse_cell_ends_crowded_and_its_vertices_fall_a_level(ops):
    """60 000 random points in 27 fine cells and one coarsest cell, strip faces along a sweep: every atomic of the coarsest
    level lands on one row, which ends far beyond 2^13 contributions (whatever its sums wrapped to) and is refused"""
    nv = 60_000
    rng = np.random.default_rng(3)
    v = (rng.random((nv, 3), dtype=np.float32) * 3).astype(np.float32)
    n = rng.standard_normal((nv, 3)).astype(np.float32)
    order = np.argsort(v[:, 0] + 3 * np.floor(v[:, 1] * 40), kind="stable").astype(np.int32)   # short faces: neighbours in a sweep
    f = order[np.stack((np.arange(nv - 2), np.arange(1, nv - 1), np.arange(2, nv)), 1)]
    want = _check(ops, _dev(v), _dev(f), _dev(n), 1.0, (0, 0, 0), 2, INF, "one coarse cell")
    info = want[3]
    assert info["refused_crowded"][2] == 1 and info["level_clusters"][2] == 0 and info["level_vertices"][2] == 0
    assert sum(info["level_vertices"]) == nv and info["vertices_kept"] > 0


def test_faces_longer_than_two_coarse_cells_mark_their_cells_far(ops):
    rng = np.random.default_rng(8)
    v = (rng.random((3000, 3)) * 24).astype(np.float32)               # 216 coarse cells of 4, random faces across all of them
    f = rng.integers(0, 3000, (9000, 3)).astype(np.int32)
    f[::50, 1] = f[::50, 0]                                          # and some with a repeated index
    info = _check(ops, _dev(v), _dev(f), None, 1.0, (0, 0, 0), 2, INF, "far")[3]
    assert info["far_corners"] > 9000 and info["refused_far"][2] + info["refused_empty"][2] > 100 and info["level_clusters"][2] < 216
    # a sheet of triangles exactly two coarse cells long: not far at the coarse level, far at the fine one
    k = 30
    gx, gy = np.meshgrid(np.arange(k, dtype=np.float32), np.arange(k, dtype=np.float32), indexing="ij")
    sheet = np.stack((4 * gx.ravel(), 4 * gy.ravel(), np.full(k * k, 0.5, np.float32)), 1)
    sheet = np.concatenate((sheet, sheet + np.float32([0.25, 0.5, 0.125])))          # two members per cell
    idx = np.arange(k * k).reshape(k, k)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    tris = np.concatenate((np.stack((a, b, c), 1), np.stack((a, c, d), 1))).astype(np.int32)
    info = _check(ops, _dev(sheet), _dev(tris), None, 1.0, (0, 0, 0), 1, INF, "two coarse cells")[3]
    assert info["refused_far"] == (0, 0) and info["level_clusters"] == (0, k * k) and info["far_corners"] == 3 * len(tris)


@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_runs_repeat_and_the_numbering_does_not_matter(ops, kind):
    vol, iso = _volume(kind, (64, 70, 50), 3)
    v, f, n, _ = ops.marching_cubes(_dev(vol), iso)
    kw = dict(cell=1.5, origin=(0, 0, 0), placement="quadric", levels=2, max_error=0.3)
    first = ops.mesh_simplify(v, f, n, **kw)
    assert first[3]["level_clusters"][1] > 0 and first[3]["refused_error"][2] > 0
    for aggregate in (False, True, False):
        again = ops.mesh_simplify(v, f, n, aggregate=aggregate, **kw)
        assert all(_np(a).tobytes() == _np(b).tobytes() for a, b in zip(first[:3], again[:3])) and first[3] == again[3]
    rng = np.random.default_rng(9)
    pv = torch.from_numpy(rng.permutation(v.shape[0])).cuda()
    pf = torch.from_numpy(rng.permutation(f.shape[0])).cuda()
    inverse = torch.empty_like(pv)
    inverse[pv] = torch.arange(v.shape[0], device="cuda")
    other = ops.mesh_simplify(v[pv].contiguous(), inverse[f[pf].long()].to(torch.int32).contiguous(), n[pv].contiguous(), **kw)
    assert other[3] == first[3]
    rows = lambda t: np.sort(np.ascontiguousarray(_np(t)).view([("x", "<u4"), ("y", "<u4"), ("z", "<u4")]).ravel())   # noqa: E731
    assert rows(other[0]).tobytes() == rows(first[0]).tobytes(), "the same set of vertex rows, bit for bit"
    assert rows(other[2]).tobytes() == rows(first[2]).tobytes()


LIMIT, RES = 1.2, 64


def _run(model, tmp_path, tag, *extra):
    d = tmp_path / tag
    d.mkdir(exist_ok=True)
    return export_mesh(model, d, "--res", str(RES), "--limit", str(LIMIT), *extra), d


def test_end_to_end_through_the_exporter(ops, scene, tmp_path, capsys):
    (v0, f0, n0, _), _ = _run(scene, tmp_path, "dense")
    quadric = ["--simplify-cell", "2", "--simplify-placement", "quadric"]
    _, d_plain = _run(scene, tmp_path, "plain", *quadric)
    plain_out = capsys.readouterr().out
    _, d_off = _run(scene, tmp_path, "off", *quadric, "--simplify-levels", "0", "--simplify-error", "0.7")
    off_out = capsys.readouterr().out
    assert "Simplify level" not in off_out
    assert [l for l in off_out.splitlines() if l.startswith("Simplify")] == [l for l in plain_out.splitlines() if l.startswith("Simplify")]
    assert open(d_plain / "mesh.obj", "rb").read() == open(d_off / "mesh.obj", "rb").read(), "options off: the former OBJ bytes"
    (v, f, n, c), d = _run(scene, tmp_path, "adaptive", *quadric, "--simplify-levels", "2", "--simplify-error", "0.25")
    out = capsys.readouterr().out
    voxel = 2.0 * LIMIT / RES
    wv, wf, wn, info = MA.simplify(_np(v0), _np(f0), _np(n0), cell=2.0 * voxel, origin=(-LIMIT,) * 3, levels=2, max_error=0.25 * voxel)
    assert 0 < info["faces_kept"] < len(f0) and sum(info["level_clusters"][1:]) > 0
    assert _np(v).tobytes() == wv.tobytes() and _np(f).tobytes() == wf.tobytes() and _np(n).tobytes() == wn.tobytes()
    assert v.shape == wv.shape and f.shape == wf.shape and c.shape == (len(wv), 3) and np.isfinite(c).all()
    lines = [f"Simplify: cell 2 voxels: {len(v0)} -> {len(wv)} vertices, {len(f0)} -> {len(wf)} faces "
             f"({info['degenerate_faces']} degenerate, {info['duplicate_faces']} duplicate)",
             f"Simplify placement: quadric: {info['quadric_clusters']} clusters at their quadric's minimum "
             f"({info['clamped_clusters']} clamped to the cell), at the mean: {info['crowded_clusters']} crowded, "
             f"{info['singular_clusters']} singular; {info['far_corners']} far corners",
             f"Simplify levels: 2 (cells of 2 to 8 voxels), error bound 0.25 voxels, largest accepted error "
             f"{info['largest_error'] / voxel:.4f} voxels"]
    for l in (2, 1):
        lines.append(f"Simplify level {l}: {info['level_vertices'][l]} vertices in {info['level_clusters'][l]} clusters, "
                     f"{info['level_kept'][l]} kept; refused: {info['refused_error'][l]} error, {info['refused_crowded'][l]} crowded, "
                     f"{info['refused_singular'][l]} singular, {info['refused_far'][l]} far, {info['refused_empty'][l]} no contributions")
    lines.append(f"Simplify level 0: {info['level_vertices'][0]} vertices in {info['level_clusters'][0]} clusters, "
                 f"{info['level_kept'][0]} kept")
    assert "\n".join(lines) + "\n" in out
    obj = open(d / "mesh.obj").read().splitlines()
    assert sum(l.startswith("v ") for l in obj) == len(wv) and sum(l.startswith("f ") for l in obj) == len(wf)
    assert len(wf) < sum(l.startswith("f ") for l in open(d_plain / "mesh.obj").read().splitlines())
    with pytest.raises(ValueError, match="--simplify-levels 2 needs --simplify-placement quadric"):
        _run(scene, tmp_path, "alone", "--simplify-cell", "2", "--simplify-levels", "2", "--override-cache-mesh")
    assert not any((tmp_path / "alone").iterdir()), "raised before anything was queried or written"


def test_two_ranks_sharing_one_gpu_equal_one_rank():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X")
    world = 2
    r = launch_ranks(os.path.join("tests", "tools", "simplify_adaptive_dist_worker.py"), world, timeout=600)
    assert_ranks_ok(r, f"SIMPLIFY_ADAPTIVE_DIST_OK world={world}")
