"""GPU: quadric placement of mesh simplification (nm_mesh_simplify_quadric_faces / nm_mesh_simplify_emit_quadric, mesh_nerf
--simplify-placement quadric).  The quadrics are exact integer sums and the solve is a fixed sequence of fp64 operations, so
every comparison with the numpy restatement (tests/mesh_simplify_quadric.py) is exact -- bytes, dtype, shape and the info
dict, with both insertion variants: the marching-cubes fixture, generated volumes, hot slots that end CROWDED, faces longer
than two cells, the same bytes run after run and under a renumbering, the default placement untouched, and the exporter end
to end, 2 ranks against 1."""
import os

import numpy as np
import pytest
import torch

from tests import mesh_simplify as MS
from tests import mesh_simplify_quadric as MQ
from tests.helpers import load_golden
from tests.gpu_support import assert_ranks_ok, export_mesh, launch_ranks, to_device as _dev, to_numpy as _np
from tests.gpu_support import ops, scene  # noqa: F401

pytestmark = pytest.mark.gpu


def _same(got, want, tag):
    for name, a, b in zip(("verts", "faces", "normals"), got[:3], want[:3]):
        if b is None:
            assert a is None, (tag, name)
            continue
        a = _np(a)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{tag}: {name} differ"
    assert got[3] == want[3] and tuple(got[3]) == tuple(want[3]), (tag, got[3], want[3])


def _check(ops, v, f, n, cell, origin, tag):
    """both insertion variants against the restatement (computed once) -> the restatement's result"""
    want = MQ.simplify(_np(v), _np(f), _np(n), cell=cell, origin=origin)
    for aggregate in (False, True):
        got = ops.mesh_simplify(v, f, n, cell=cell, origin=origin, aggregate=aggregate, placement="quadric")
        _same(got, want, f"{tag} aggregate={aggregate}")
    return want


def test_every_fixture_mesh(ops):
    g = load_golden("mc_cases")
    count = solved = clamped = 0
    for i in range(int(g["count"])):
        if f"err_{i}" in g.files:
            continue
        v, f, n = g[f"verts_{i}"].astype(np.float32), g[f"faces_{i}"].astype(np.int32), g[f"normals_{i}"].astype(np.float32)
        want = _check(ops, _dev(v), _dev(f), _dev(n), 2.0, (0, 0, 0), f"golden {i}")
        # without normals, the origin left to the wrapper (the vertices' minimum)
        _same(ops.mesh_simplify(_dev(v), _dev(f), cell=2.0, placement="quadric"), MQ.simplify(v, f, None, cell=2.0), f"golden {i}, bare")
        count, solved, clamped = count + 1, solved + want[3]["quadric_clusters"], clamped + want[3]["clamped_clusters"]
    assert count == 667 and solved > 1000 and clamped > 0


def _volume(kind, shape, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.standard_normal(shape).astype(np.float32), 0.1
    if kind == "ties":
        return rng.integers(-2, 3, shape).astype(np.float32), 0.0
    g = np.stack(np.meshgrid(*[np.linspace(-1, 1, s) for s in shape], indexing="ij"), -1)
    return (np.sin(3 * g[..., 0]) * np.cos(2 * g[..., 1]) + g[..., 2] ** 2 - 0.3).astype(np.float32), float(np.float32(0.05))


@pytest.mark.parametrize("cell", [1.5, 4.0])
@pytest.mark.parametrize("shape", [(17, 5, 33), (33, 130, 77)])
@pytest.mark.parametrize("kind", ["noise", "ties", "smooth"])
def test_on_generated_volumes(ops, shape, kind, cell):
    vol, iso = _volume(kind, shape, sum(shape) * 7 + len(kind))
    v, f, n, _ = ops.marching_cubes(_dev(vol), iso)
    info = _check(ops, v, f, n, cell, (0, 0, 0), f"{shape} {kind} cell {cell}")[3]
    assert 0 < info["faces_kept"] < info["faces"] and info["quadric_clusters"] > 0.5 * info["vertices_kept"]
    assert info["crowded_clusters"] == 0 and info["far_corners"] == 0


def test_hot_slots_end_crowded_and_equal_the_mean(ops):
    """200 003 points in eight cells, strip faces: every atomic of the face pass lands on eight rows, every cluster ends far
    beyond 2^13 contributions (whatever its sums wrapped to) and gets the mean, bit for bit"""
    nv = 200_003
    rng = np.random.default_rng(3)
    v = (rng.random((nv, 3), dtype=np.float32) * 2).astype(np.float32)
    n = rng.standard_normal((nv, 3)).astype(np.float32)
    perm = rng.permutation(nv).astype(np.int32)
    f = perm[np.stack((np.arange(nv - 2), np.arange(1, nv - 1), np.arange(2, nv)), 1)]
    dv, df, dn = _dev(v), _dev(f), _dev(n)
    want = _check(ops, dv, df, dn, 1.0, (0, 0, 0), "eight cells")
    assert want[3]["vertices_kept"] == 8 and want[3]["crowded_clusters"] == 8 and want[3]["quadric_clusters"] == 0
    mean = ops.mesh_simplify(dv, df, dn, cell=1.0, origin=(0, 0, 0))
    assert all(_np(a).tobytes() == b.tobytes() for a, b in zip(mean[:3], want[:3]))


def test_faces_longer_than_two_cells_contribute_nothing(ops):
    rng = np.random.default_rng(8)
    v = (rng.random((3000, 3)) * 6).astype(np.float32)                # 216 cells, random faces across all of them
    f = rng.integers(0, 3000, (9000, 3)).astype(np.int32)
    f[::50, 1] = f[::50, 0]                                          # and some with a repeated index
    info = _check(ops, _dev(v), _dev(f), None, 1.0, (0, 0, 0), "far")[3]
    assert info["far_corners"] > 9000 and info["quadric_clusters"] > 0
    # a sheet of triangles exactly two cells long: not far
    k = 30
    gx, gy = np.meshgrid(np.arange(k, dtype=np.float32), np.arange(k, dtype=np.float32), indexing="ij")
    sheet = np.stack((2 * gx.ravel(), 2 * gy.ravel(), np.full(k * k, 0.5, np.float32)), 1)
    sheet = np.concatenate((sheet, sheet + np.float32([0.25, 0.5, 0.125])))          # two members per cell
    idx = np.arange(k * k).reshape(k, k)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    tris = np.concatenate((np.stack((a, b, c), 1), np.stack((a, c, d), 1))).astype(np.int32)
    info = _check(ops, _dev(sheet), _dev(tris), None, 1.0, (0, 0, 0), "two cells")[3]
    assert info["far_corners"] == 0 and info["quadric_clusters"] == k * k


@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_runs_repeat_and_the_numbering_does_not_matter(ops, kind):
    vol, iso = _volume(kind, (64, 70, 50), 3)
    v, f, n, _ = ops.marching_cubes(_dev(vol), iso)
    first = ops.mesh_simplify(v, f, n, cell=3.0, origin=(0, 0, 0), placement="quadric")
    for aggregate in (False, True, False):
        again = ops.mesh_simplify(v, f, n, cell=3.0, origin=(0, 0, 0), aggregate=aggregate, placement="quadric")
        assert all(_np(a).tobytes() == _np(b).tobytes() for a, b in zip(first[:3], again[:3])) and first[3] == again[3]
    rng = np.random.default_rng(9)
    pv = torch.from_numpy(rng.permutation(v.shape[0])).cuda()
    pf = torch.from_numpy(rng.permutation(f.shape[0])).cuda()
    inverse = torch.empty_like(pv)
    inverse[pv] = torch.arange(v.shape[0], device="cuda")
    other = ops.mesh_simplify(v[pv].contiguous(), inverse[f[pf].long()].to(torch.int32).contiguous(), n[pv].contiguous(), cell=3.0,
                              origin=(0, 0, 0), placement="quadric")
    assert other[3] == first[3]
    rows = lambda t: np.sort(np.ascontiguousarray(_np(t)).view([("x", "<u4"), ("y", "<u4"), ("z", "<u4")]).ravel())   # noqa: E731
    assert rows(other[0]).tobytes() == rows(first[0]).tobytes(), "the same set of vertex rows, bit for bit"
    # the default placement is the call without the argument, keys included
    plain, mean = ops.mesh_simplify(v, f, n, cell=3.0, origin=(0, 0, 0)), ops.mesh_simplify(v, f, n, cell=3.0, origin=(0, 0, 0),
                                                                                             placement="mean")
    assert all(_np(a).tobytes() == _np(b).tobytes() for a, b in zip(plain[:3], mean[:3]))
    assert plain[3] == mean[3] and tuple(mean[3]) == MS.INFO_KEYS
    assert _np(plain[1]).tobytes() == _np(first[1]).tobytes() and _np(plain[0]).tobytes() != _np(first[0]).tobytes()


LIMIT, RES = 1.2, 64


def _run(model, tmp_path, tag, *extra):
    d = tmp_path / tag
    d.mkdir(exist_ok=True)
    return export_mesh(model, d, "--res", str(RES), "--limit", str(LIMIT), *extra), d


def test_end_to_end_through_the_exporter(ops, scene, tmp_path, capsys):
    (v0, f0, n0, _), _ = _run(scene, tmp_path, "dense")
    _, d_plain = _run(scene, tmp_path, "plain", "--simplify-cell", "4")
    capsys.readouterr()
    _, d_mean = _run(scene, tmp_path, "mean", "--simplify-cell", "4", "--simplify-placement", "mean")
    assert "Simplify placement" not in capsys.readouterr().out
    assert open(d_plain / "mesh.obj", "rb").read() == open(d_mean / "mesh.obj", "rb").read()
    (v, f, n, c), d = _run(scene, tmp_path, "quadric", "--simplify-cell", "4", "--simplify-placement", "quadric")
    out = capsys.readouterr().out
    wv, wf, wn, info = MQ.simplify(_np(v0), _np(f0), _np(n0), cell=4.0 * (2.0 * LIMIT / RES), origin=(-LIMIT,) * 3)
    assert 0 < info["faces_kept"] < len(f0) and info["quadric_clusters"] > 0.5 * len(wv)
    assert _np(v).tobytes() == wv.tobytes() and _np(f).tobytes() == wf.tobytes() and _np(n).tobytes() == wn.tobytes()
    assert v.shape == wv.shape and f.shape == wf.shape and c.shape == (len(wv), 3) and np.isfinite(c).all()
    first = (f"Simplify: cell 4 voxels: {len(v0)} -> {len(wv)} vertices, {len(f0)} -> {len(wf)} faces "
             f"({info['degenerate_faces']} degenerate, {info['duplicate_faces']} duplicate)\n")
    second = (f"Simplify placement: quadric: {info['quadric_clusters']} clusters at their quadric's minimum "
              f"({info['clamped_clusters']} clamped to the cell), at the mean: {info['crowded_clusters']} crowded, "
              f"{info['singular_clusters']} singular; {info['far_corners']} far corners\n")
    assert first + second in out
    lines = open(d / "mesh.obj").read().splitlines()
    assert sum(l.startswith("v ") for l in lines) == len(wv) and sum(l.startswith("f ") for l in lines) == len(wf)
    assert open(d / "mesh.obj", "rb").read() != open(d_mean / "mesh.obj", "rb").read()
    with pytest.raises(ValueError, match="--simplify-placement quadric needs --simplify-cell"):
        _run(scene, tmp_path, "alone", "--simplify-placement", "quadric", "--override-cache-mesh")
    assert not any((tmp_path / "alone").iterdir()), "raised before anything was queried or written"


def test_two_ranks_sharing_one_gpu_equal_one_rank():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X")
    world = 2
    r = launch_ranks(os.path.join("tests", "tools", "simplify_quadric_dist_worker.py"), world, timeout=600)
    assert_ranks_ok(r, f"SIMPLIFY_QUADRIC_DIST_OK world={world}")
