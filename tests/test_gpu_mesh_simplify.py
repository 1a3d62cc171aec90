"""GPU: mesh simplification by vertex clustering (nm_mesh_simplify_cluster / _emit, mesh_nerf --simplify-cell).  Every sum is
an exact integer sum and every fp operation is rounded on its own, so every comparison with the numpy restatement
(tests/mesh_simplify.py) is exact -- bytes, dtype, shape and the info dict: the marching-cubes fixture, generated volumes,
adversarial index and coordinate arrays, the same bytes run after run and under a renumbering, and the exporter end to end --
the cache, 2 ranks against 1.  Both insertion variants (lane atomics, wave aggregation) are held to the same bytes."""
import os

import numpy as np
import pytest
import torch

from tests import mesh_simplify as MS
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
    assert got[3] == want[3], (tag, got[3], want[3])


def _check(ops, v, f, n, cell, origin, tag, want=None):
    """both insertion variants against the restatement (computed once) -> the restatement's result"""
    if want is None:
        want = MS.simplify(_np(v), _np(f), _np(n), cell=cell, origin=origin)
    for aggregate in (False, True):
        _same(ops.mesh_simplify(v, f, n, cell=cell, origin=origin, aggregate=aggregate), want, f"{tag} aggregate={aggregate}")
    return want


@pytest.fixture(scope="module")
def meshes():
    g = load_golden("mc_cases")
    out = []
    for i in range(int(g["count"])):
        if f"err_{i}" in g.files:
            continue
        v, f, n = g[f"verts_{i}"].astype(np.float32), g[f"faces_{i}"].astype(np.int32), g[f"normals_{i}"].astype(np.float32)
        out.append((i, v, f, n, _dev(v), _dev(f), _dev(n)))
    assert len(out) == 667
    return out


@pytest.mark.parametrize("cell", [1.0, 2.0, 3.7])
def test_every_fixture_mesh(ops, meshes, cell):
    for i, v, f, n, dv, df, dn in meshes:
        want = MS.simplify(v, f, n, cell=cell, origin=(0, 0, 0))
        _same(ops.mesh_simplify(dv, df, dn, cell=cell, origin=(0, 0, 0)), want, f"golden {i} cell {cell}")
        # without normals, the origin left to the wrapper (the vertices' minimum), the other insertion variant
        want = MS.simplify(v, f, None, cell=cell)
        _same(ops.mesh_simplify(dv, df, cell=cell, aggregate=True), want, f"golden {i} cell {cell}, no normals")


def _volume(kind, shape, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.standard_normal(shape).astype(np.float32), 0.1
    if kind == "ties":
        return rng.integers(-2, 3, shape).astype(np.float32), 0.0
    g = np.stack(np.meshgrid(*[np.linspace(-1, 1, s) for s in shape], indexing="ij"), -1)
    return (np.sin(3 * g[..., 0]) * np.cos(2 * g[..., 1]) + g[..., 2] ** 2 - 0.3).astype(np.float32), float(np.float32(0.05))


@pytest.mark.parametrize("cell", [1.5, 2.0, 4.0])
@pytest.mark.parametrize("shape", [(17, 5, 33), (33, 130, 77), (90, 96, 80)])
@pytest.mark.parametrize("kind", ["noise", "ties", "smooth"])
def test_on_generated_volumes(ops, shape, kind, cell):
    vol, iso = _volume(kind, shape, sum(shape) * 7 + len(kind))
    v, f, n, _ = ops.marching_cubes(_dev(vol), iso)
    want = _check(ops, v, f, n, cell, (0, 0, 0), f"{shape} {kind} cell {cell}")
    info = want[3]
    assert 0 < info["faces_kept"] < info["faces"] and info["degenerate_faces"] > 0 and info["vertices_kept"] < info["vertices"]


def test_thin_sheet_keeps_both_sides_and_drops_same_winding_duplicates(ops):
    # two parallel 40 x 40 sheets 0.25 apart (a cell is 1): the upper one wound the other way, then the lower one once more
    k = 40
    gx, gy = np.meshgrid(np.arange(k, dtype=np.float32), np.arange(k, dtype=np.float32), indexing="ij")
    low = np.stack((gx.ravel() + 0.5, gy.ravel() + 0.5, np.full(k * k, 0.25, np.float32)), 1)
    idx = np.arange(k * k).reshape(k, k)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    tris = np.concatenate((np.stack((a, b, c), 1), np.stack((a, c, d), 1))).astype(np.int32)
    v = np.concatenate((low, low + np.float32([0, 0, 0.25]), low + np.float32([0, 0, 0.125])))
    f = np.concatenate((tris, tris[:, [0, 2, 1]] + k * k, tris[:, [1, 2, 0]] + 2 * k * k)).astype(np.int32)
    n = np.concatenate((np.tile(np.float32([0, 0, -1]), (k * k, 1)), np.tile(np.float32([0, 0, 1]), (k * k, 1)),
                        np.tile(np.float32([0, 0, -1]), (k * k, 1))))
    want = _check(ops, _dev(v), _dev(f), _dev(n), 1.0, (0, 0, 0), "sheets")
    assert want[3] == dict(vertices=3 * k * k, faces=3 * len(tris), clusters=k * k, vertices_kept=k * k, faces_kept=2 * len(tris),
                           degenerate_faces=0, duplicate_faces=len(tris))
    assert np.array_equal(want[1][:len(tris)], tris) and np.array_equal(want[1][len(tris):], tris[:, [0, 2, 1]]), "both sides stay"
    assert np.array_equal(want[0], low + np.float32([0, 0, 0.125]))
    assert np.array_equal(want[2], np.tile(np.float32([0, 0, -1]), (k * k, 1))), "(-1 + 1 - 1) normalised"


def _triangles_and_strips(nv):
    """test_gpu_mesh_components.py's family with coordinates: component k lives in the cells x in [4 k, 4 k + 2), a cell is 1.
    A triangle has its corners in three cells.  A strip (p0, p1, p2), (p1, p3, p2) has p0 and p1 in one cell: p1 merges into
    p0, the first face degenerates, the second stays, and p3 -- the mesh's last vertex -- stays.  The nv % 7 vertices in
    front are in no face, each in a cell of its own."""
    k = nv // 7
    x = 4.0 * np.arange(k)[:, None, None]
    corners = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5],                      # the triangle
                        [0.25, 0.25, 0.5], [0.75, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]])  # the strip, 2 cells further
    corners[3:, 0] += 2.0
    loose = np.stack((np.arange(nv % 7) + 0.5, np.full(nv % 7, 5.5), np.full(nv % 7, 0.5)), 1)
    verts = np.concatenate((loose, (corners + x * np.array([1.0, 0.0, 0.0])).reshape(-1, 3))).astype(np.float32)
    base = (nv % 7 + 7 * np.arange(k))[:, None, None]
    faces = (base + np.array([[0, 1, 2], [3, 4, 5], [4, 6, 5]])).astype(np.int32).reshape(-1, 3)
    normals = np.random.default_rng(nv).standard_normal((nv, 3)).astype(np.float32)
    return verts, faces, normals


@pytest.mark.parametrize("nv", [64, 65_536, 65_537, 131_073])
def test_compaction_at_the_chunk_boundaries_of_the_scan(ops, nv):
    """1, 1024, 1025 and 2049 words of used bits: a single partial wave, one full chunk of the one-workgroup scan
    (csrc/compact.h), the first word of the second chunk (the carry is handed over) and of the third (it is carried twice).
    Set and clear bits alternate in the vertex and in the face words, and the last vertex -- alone in the last word of the
    three larger meshes -- is kept: its new index needs that word's prefix."""
    v, f, n = _triangles_and_strips(nv)
    assert (nv + 63) // 64 in (1, 1024, 1025, 2049) and len(v) == nv and f.max() == nv - 1
    want = _check(ops, _dev(v), _dev(f), _dev(n), 1.0, (0, 0, 0), f"{nv} vertices")
    k = nv // 7
    assert want[3] == dict(vertices=nv, faces=3 * k, clusters=nv - k, vertices_kept=6 * k, faces_kept=2 * k, degenerate_faces=k,
                           duplicate_faces=0)
    assert want[0][-1].tobytes() == v[-1].tobytes() and want[1][-1].max() == 6 * k - 1, "the last vertex is the last row out"


def test_everything_in_one_cell_leaves_nothing(ops):
    rng = np.random.default_rng(2)
    v = rng.random((5000, 3), dtype=np.float32)
    f = rng.integers(0, 5000, (9000, 3)).astype(np.int32)
    for aggregate in (False, True):
        ov, of, on, info = ops.mesh_simplify(_dev(v), _dev(f), _dev(v), cell=4.0, origin=(-1, -1, -1), aggregate=aggregate)
        assert ov.shape == (0, 3) and of.shape == (0, 3) and on.shape == (0, 3) and of.dtype == torch.int32
        assert info == dict(vertices=5000, faces=9000, clusters=1, vertices_kept=0, faces_kept=0, degenerate_faces=9000,
                            duplicate_faces=0)


def test_a_million_points_in_eight_cells(ops):
    """hot slots: every atomic of the vertex pass lands on 8 slots, every face of the face pass on at most 8 * 7 * 6 / 3 triples"""
    nv = 1_000_003
    rng = np.random.default_rng(3)
    v = (rng.random((nv, 3), dtype=np.float32) * 2).astype(np.float32)
    n = rng.standard_normal((nv, 3)).astype(np.float32)
    perm = rng.permutation(nv).astype(np.int32)
    f = perm[np.stack((np.arange(nv - 2), np.arange(1, nv - 1), np.arange(2, nv)), 1)]
    want = _check(ops, _dev(v), _dev(f), _dev(n), 1.0, (0, 0, 0), "eight cells")
    assert want[3]["clusters"] == 8 and want[3]["vertices_kept"] == 8 and want[3]["faces_kept"] == 112
    assert want[3]["duplicate_faces"] + want[3]["degenerate_faces"] == nv - 2 - 112


def test_a_million_points_each_in_its_own_cell(ops):
    """long probe sequences (a million keys in a table of 2^21 slots), and the identity on rows"""
    nv = 1_000_003
    rng = np.random.default_rng(4)
    i = rng.permutation(nv)
    v = (np.stack((i % 128, (i // 128) % 128, i // 16384), 1) + rng.random((nv, 3)) * 0.5 + 0.25).astype(np.float32)
    n = rng.standard_normal((nv, 3)).astype(np.float32)
    n[5] = [np.nan, 0, 0]                                             # a single member's row is copied, whatever it holds
    f = np.stack((np.arange(nv - 2), np.arange(1, nv - 1), np.arange(2, nv)), 1).astype(np.int32)
    for aggregate in (False, True):
        ov, of, on, info = ops.mesh_simplify(_dev(v), _dev(f), _dev(n), cell=1.0, origin=(0, 0, 0), aggregate=aggregate)
        assert _np(ov).tobytes() == v.tobytes() and _np(on).tobytes() == n.tobytes() and _np(of).tobytes() == f.tobytes()
        assert info == dict(vertices=nv, faces=nv - 2, clusters=nv, vertices_kept=nv, faces_kept=nv - 2, degenerate_faces=0,
                            duplicate_faces=0)


def test_bad_vertices_and_faces_are_errors_not_accesses(ops):
    v = np.random.default_rng(5).random((300, 3), dtype=np.float32) * 8
    f = np.random.default_rng(6).integers(0, 300, (500, 3)).astype(np.int32)
    for aggregate in (False, True):
        bad = v.copy()
        bad[7, 1], bad[200, 2] = np.nan, np.inf
        with pytest.raises(ValueError, match=r"2 vertices have a non-finite coordinate or a cell index outside \[0, 2097152\)"):
            ops.mesh_simplify(_dev(bad), _dev(f), cell=1.0, aggregate=aggregate)
        far = v.copy()
        far[9, 0] = 2.0 ** 21                                         # cell 2^21 of [0, 2^21)
        far[10, 2] = -0.5                                             # below the origin
        far[11, 1] = 3e38
        with pytest.raises(ValueError, match=r"3 vertices have a non-finite coordinate or a cell index outside \[0, 2097152\)"):
            ops.mesh_simplify(_dev(far), _dev(f), cell=1.0, origin=(0, 0, 0), aggregate=aggregate)
        far[9, 0], far[10, 2], far[11, 1] = 2.0 ** 21 - 1, 0.0, 0.0   # the last cell is a cell
        ops.mesh_simplify(_dev(far), _dev(f), cell=1.0, origin=(0, 0, 0), aggregate=aggregate)
        out = f.copy()
        out[3, 2], out[400, 0] = 300, -1
        with pytest.raises(ValueError, match=r"2 faces have a vertex index outside \[0, 300\)"):
            ops.mesh_simplify(_dev(v), _dev(out), cell=1.0, aggregate=aggregate)
    empty = ops.mesh_simplify(_dev(v), torch.zeros(0, 3, dtype=torch.int32, device="cuda"), cell=1.0)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3) and empty[2] is None and empty[3]["clusters"] > 0
    none = ops.mesh_simplify(torch.zeros(0, 3, device="cuda"), torch.zeros(0, 3, dtype=torch.int32, device="cuda"), cell=1.0)
    assert none[0].shape == (0, 3) and none[3]["clusters"] == 0


@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_runs_repeat_and_the_numbering_does_not_matter(ops, kind):
    vol, iso = _volume(kind, (64, 70, 50), 3)
    v, f, n, _ = ops.marching_cubes(_dev(vol), iso)
    first = ops.mesh_simplify(v, f, n, cell=2.0, origin=(0, 0, 0))
    for aggregate in (False, True, False):
        again = ops.mesh_simplify(v, f, n, cell=2.0, origin=(0, 0, 0), aggregate=aggregate)
        assert all(_np(a).tobytes() == _np(b).tobytes() for a, b in zip(first[:3], again[:3])) and first[3] == again[3]
    # another numbering of the vertices, another order of the faces: the same clusters, the same exact means
    rng = np.random.default_rng(9)
    pv = torch.from_numpy(rng.permutation(v.shape[0])).cuda()
    pf = torch.from_numpy(rng.permutation(f.shape[0])).cuda()
    inverse = torch.empty_like(pv)
    inverse[pv] = torch.arange(v.shape[0], device="cuda")
    v2, n2 = v[pv].contiguous(), n[pv].contiguous()
    f2 = inverse[f[pf].long()].to(torch.int32).contiguous()
    other = ops.mesh_simplify(v2, f2, n2, cell=2.0, origin=(0, 0, 0))
    assert other[3] == first[3]
    rows = lambda t: np.sort(np.ascontiguousarray(_np(t)).view([("x", "<u4"), ("y", "<u4"), ("z", "<u4")]).ravel())   # noqa: E731
    assert rows(other[0]).tobytes() == rows(first[0]).tobytes(), "the same set of vertex rows, bit for bit"


LIMIT, RES = 1.2, 64


def _run(model, tmp_path, tag, *extra):
    d = tmp_path / tag
    d.mkdir(exist_ok=True)
    return export_mesh(model, d, "--res", str(RES), "--limit", str(LIMIT), *extra), d


def _restated(v0, f0, n0, k):
    return MS.simplify(_np(v0), _np(f0), _np(n0), cell=k * (2.0 * LIMIT / RES), origin=(-LIMIT,) * 3)


FILTER = ["--min-component-faces", "100", "--keep-largest", "2"]


@pytest.mark.parametrize("extra", [[], ["--normals", "network"], ["--super-sampling", "2"], FILTER],
                         ids=["plain", "network", "ss2", "filtered"])
def test_end_to_end_through_the_exporter(ops, scene, tmp_path, capsys, extra):
    (v0, f0, n0, _), _ = _run(scene, tmp_path, "dense", *extra)
    capsys.readouterr()
    (v, f, n, c), d = _run(scene, tmp_path, "simplified", *extra, "--simplify-cell", "2")
    out = capsys.readouterr().out
    grid_normals = "network" not in extra
    wv, wf, wn, info = _restated(v0, f0, n0 if grid_normals else None, 2.0)
    assert 0 < info["faces_kept"] < len(f0) and info["vertices_kept"] < len(v0) and info["degenerate_faces"] > 0
    assert _np(v).tobytes() == wv.tobytes() and _np(f).tobytes() == wf.tobytes() and v.shape == wv.shape and f.shape == wf.shape
    if grid_normals:
        assert _np(n).tobytes() == wn.tobytes()
    else:                                                            # the gradient is taken at the NEW positions
        from nerfmeshes_amd import mesh_nerf
        own, _ = mesh_nerf.network_normals(scene.get_model().hip("f32"), v, n)
        assert torch.equal(own, n) and "Network normals" in out
    assert c.shape == (len(wv), 3) and np.isfinite(c).all()
    assert (f"Simplify: cell 2 voxels: {len(v0)} -> {len(wv)} vertices, {len(f0)} -> {len(wf)} faces "
            f"({info['degenerate_faces']} degenerate, {info['duplicate_faces']} duplicate)") in out
    if extra == FILTER:                                              # the filter ran first, on the original triangles
        assert out.index("Component filter") < out.index("Simplify:")
    lines = open(d / "mesh.obj").read().splitlines()
    assert sum(l.startswith("v ") for l in lines) == len(wv) and sum(l.startswith("f ") for l in lines) == len(wf)


def test_zero_is_off_and_nothing_left_raises(ops, scene, tmp_path, capsys):
    _, d0 = _run(scene, tmp_path, "a")
    _, d1 = _run(scene, tmp_path, "b", "--simplify-cell", "0")
    assert "Simplify" not in capsys.readouterr().out
    assert open(d0 / "mesh.obj", "rb").read() == open(d1 / "mesh.obj", "rb").read()
    with pytest.raises(ValueError, match="--simplify-cell 1000 leaves no triangle"):
        _run(scene, tmp_path, "c", "--simplify-cell", "1000", "--override-cache-mesh")
    assert not any((tmp_path / "c").iterdir()), "raised before anything was queried or written"


def test_cache_keeps_the_unsimplified_geometry(ops, scene, tmp_path):
    (v0, f0, n0, _), _ = _run(scene, tmp_path, "dense")
    (v1, f1, n1, _), d = _run(scene, tmp_path, "cache", "--override-cache-mesh", "--simplify-cell", "2")
    assert v1.shape[0] < v0.shape[0]
    cv, cf, cn, _ = torch.load(d / "mesh_cache.pt", weights_only=False)
    assert torch.equal(cv, v0.cpu()) and torch.equal(cf, f0.cpu()) and torch.equal(cn, n0.cpu()), "the cache is the dense mesh"
    first = open(d / "mesh.obj", "rb").read()
    os.remove(d / "mesh.obj")
    (v2, f2, n2, _), _ = _run(scene, tmp_path, "cache", "--use-cached-mesh", "--simplify-cell", "2")
    assert torch.equal(v2, v1) and torch.equal(f2, f1) and torch.equal(n2, n1)
    assert open(d / "mesh.obj", "rb").read() == first, "the cached mesh simplified again gives the same OBJ bytes"
    (v3, f3, _, _), _ = _run(scene, tmp_path, "cache", "--use-cached-mesh", "--simplify-cell", "3")   # and the cell can be tuned on it
    assert 0 < f3.shape[0] < f1.shape[0]


def test_two_ranks_sharing_one_gpu_equal_one_rank():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X")
    world = 2
    r = launch_ranks(os.path.join("tests", "tools", "simplify_dist_worker.py"), world, timeout=900)
    assert_ranks_ok(r, f"SIMPLIFY_DIST_OK world={world}")
