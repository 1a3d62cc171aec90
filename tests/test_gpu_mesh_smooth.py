"""GPU: Taubin smoothing of a mesh (nm_mesh_smooth_build / _run, nm_mesh_vertex_normals, mesh_nerf --smooth-iters).  Every
per-vertex sum is an exact integer sum and every fp operation is rounded on its own, so every comparison with the numpy
restatement (tests/mesh_smooth.py) is exact -- bytes, dtype, shape and the info dict: the marching-cubes fixture, generated
volumes, the chunk boundaries of the degree scan, a hub of 100 000 neighbours, a million-vertex sheet, bad and empty inputs,
the same bytes run after run and under a renumbering, and the exporter end to end -- the stage order, the cache, 2 ranks
against 1."""
import os

import numpy as np
import pytest
import torch

from tests import mesh_simplify as MS
from tests import mesh_smooth as SM
from tests.helpers import load_golden
from tests.gpu_support import assert_ranks_ok, export_mesh, launch_ranks, to_device as _dev, to_numpy as _np
from tests.gpu_support import ops, scene  # noqa: F401

pytestmark = pytest.mark.gpu


def _same(got, want, tag):
    for name, a, b in zip(("verts", "normals"), got[:2], want[:2]):
        if b is None:
            assert a is None, (tag, name)
            continue
        a = _np(a)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{tag}: {name} differ"
    assert got[2] == want[2], (tag, got[2], want[2])


def _check(ops, v, f, n, tag, **kw):
    """the device against the restatement -> the restatement's result"""
    want = SM.smooth(_np(v), _np(f), _np(n), **kw)
    _same(ops.mesh_smooth(v, f, n, **kw), want, tag)
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


@pytest.mark.parametrize("free", [False, True], ids=["pinned", "free"])
@pytest.mark.parametrize("iterations", [1, 3])
def test_every_fixture_mesh(ops, meshes, iterations, free):
    for i, v, f, n, dv, df, dn in meshes:
        kw = dict(iterations=iterations, free_boundary=free)
        _same(ops.mesh_smooth(dv, df, dn, flip=-1, **kw), SM.smooth(v, f, n, flip=-1, **kw), f"golden {i} {kw}")
        _same(ops.mesh_smooth(dv, df, **kw), SM.smooth(v, f, **kw), f"golden {i} {kw}, no normals")


def _volume(kind, shape, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.standard_normal(shape).astype(np.float32), 0.1
    if kind == "ties":
        return rng.integers(-2, 3, shape).astype(np.float32), 0.0
    g = np.stack(np.meshgrid(*[np.linspace(-1, 1, s) for s in shape], indexing="ij"), -1)
    return (np.sin(3 * g[..., 0]) * np.cos(2 * g[..., 1]) + g[..., 2] ** 2 - 0.3).astype(np.float32), float(np.float32(0.05))


@pytest.mark.parametrize("shape", [(17, 5, 33), (33, 130, 77)])
@pytest.mark.parametrize("kind", ["noise", "ties", "smooth"])
def test_on_generated_volumes(ops, shape, kind):
    """the ties volumes emit coincident vertices and zero-area faces: faces without a normal, vertices that keep theirs"""
    vol, iso = _volume(kind, shape, sum(shape) * 7 + len(kind))
    v, f, n, _ = ops.marching_cubes(_dev(vol), iso)
    want = _check(ops, v, f, n, f"{shape} {kind}", iterations=5, flip=-1)
    assert want[2]["edges"] > 0 and not np.array_equal(want[0], _np(v))
    _check(ops, v, f, None, f"{shape} {kind} free", iterations=5, free_boundary=True)


def _tetrahedra_and_triangles(nv):
    """Units of seven vertices t0 p0 t1 p1 t2 p2 t3: a closed tetrahedron t (every edge on two faces: its vertices move) and an
    open triangle p (pinned) interleaved, so moving and pinned vertices alternate; the nv % 7 vertices in front are on no face.
    The mesh's last vertex is a tetrahedron's: it moves, and its neighbour list starts at the sum of all degrees before it."""
    k = nv // 7
    rng = np.random.default_rng(nv)
    verts = (rng.random((nv, 3)) * 8).astype(np.float32)
    base = (nv % 7 + 7 * np.arange(k))[:, None, None]
    t, p = [0, 2, 4, 6], [1, 3, 5]
    unit = np.array([[t[0], t[1], t[2]], [t[0], t[3], t[1]], [t[0], t[2], t[3]], [t[1], t[3], t[2]], p])
    return verts, (base + unit).astype(np.int32).reshape(-1, 3)


@pytest.mark.parametrize("nv", [1023, 1024, 1025, 2049])
def test_offsets_at_the_chunk_boundaries_of_the_scan(ops, nv):
    """chunk - 1, chunk, chunk + 1 and 2 chunks + 1 degrees for the one-workgroup scan (csrc/compact.h: 1024 per step): one
    partial chunk, one full one, the first value of the second chunk (the carry is handed over) and of the third"""
    v, f = _tetrahedra_and_triangles(nv)
    assert len(v) == nv and f.max() == nv - 1
    want = _check(ops, _dev(v), _dev(f), None, f"{nv} vertices", iterations=3, flip=1)
    k = nv // 7
    assert want[2] == dict(vertices=nv, faces=5 * k, edges=9 * k, boundary_edges=3 * k, nonmanifold_edges=0,
                           boundary_vertices=3 * k, isolated_vertices=nv % 7, degenerate_faces=0, exponent=3)
    moved = (want[0] != v).any(axis=1)
    assert moved[-1] and moved.sum() == 4 * k and not moved[-2], "the last vertex moves, its pinned neighbour in the numbering stays"


def test_a_hub_of_a_hundred_thousand_neighbours(ops):
    """a closed fan around vertex 0: 100 000 claims increment one degree counter, 100 000 fills advance one cursor, and one
    thread gathers 100 000 rows.  The rim's outer edges are on one face each: pinned by default, free on request."""
    k = 100_000
    rng = np.random.default_rng(11)
    angle = np.arange(k) * (2 * np.pi / k)
    rim = np.stack((np.cos(angle) * 50, np.sin(angle) * 50, rng.standard_normal(k)), 1)
    v = np.concatenate(([[0.3, -0.2, 7.0]], rim)).astype(np.float32)
    i = np.arange(k)
    f = np.stack((np.zeros(k, np.int64), 1 + i, 1 + (i + 1) % k), 1).astype(np.int32)
    dv, df = _dev(v), _dev(f[rng.permutation(k)])
    pinned = _check(ops, dv, df, None, "fan", iterations=2, flip=1)
    assert pinned[2] == dict(vertices=k + 1, faces=k, edges=2 * k, boundary_edges=k, nonmanifold_edges=0, boundary_vertices=k,
                             isolated_vertices=0, degenerate_faces=0, exponent=6)
    assert (pinned[0][0] != v[0]).any() and pinned[0][1:].tobytes() == v[1:].tobytes()
    free = _check(ops, dv, df, None, "free fan", iterations=2, free_boundary=True)
    assert (free[0][1:] != v[1:]).any(axis=1).all()


def test_a_million_vertex_sheet_and_its_duplicates(ops):
    """1000 x 1000 vertices, 1 996 002 faces, 2 996 001 edges in a table of 2^24 slots; every face listed twice and once more
    with the other winding brings every edge three or six times and must give the plain sheet's positions with a free
    boundary, bit for bit (no edge is on exactly one face any more, so nothing is pinned)."""
    k = 1000
    rng = np.random.default_rng(12)
    gx, gy = np.meshgrid(np.arange(k, dtype=np.float32), np.arange(k, dtype=np.float32), indexing="ij")
    v = np.stack((gx.ravel(), gy.ravel(), rng.standard_normal(k * k).astype(np.float32)), 1).astype(np.float32)
    idx = np.arange(k * k).reshape(k, k)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    f = np.concatenate((np.stack((a, b, c), 1), np.stack((a, c, d), 1))).astype(np.int32)
    dv, df = _dev(v), _dev(f)
    want = _check(ops, dv, df, None, "sheet", iterations=1, flip=1)
    assert want[2]["edges"] == 2_996_001 and want[2]["boundary_vertices"] == 4 * (k - 1) and want[2]["boundary_edges"] == 4 * (k - 1)
    free = ops.mesh_smooth(dv, df, iterations=1, free_boundary=True)
    thrice = ops.mesh_smooth(dv, torch.cat((df, df, df[:, [0, 2, 1]])).contiguous(), iterations=1)
    assert thrice[2]["edges"] == 2_996_001 and thrice[2]["boundary_edges"] == 0 and thrice[2]["nonmanifold_edges"] == 2_996_001
    assert _np(thrice[0]).tobytes() == _np(free[0]).tobytes()
    grid = lambda x: x.reshape(k, k, 3)                              # noqa: E731
    assert grid(want[0])[0].tobytes() == grid(v)[0].tobytes() and grid(want[0])[:, -1].tobytes() == grid(v)[:, -1].tobytes()
    assert (grid(_np(free[0]))[0] != grid(v)[0]).any(axis=1).all(), "pinned by default, moving when free"


def test_bad_vertices_and_faces_are_errors_not_accesses(ops):
    v = np.random.default_rng(5).random((300, 3), dtype=np.float32) * 8
    f = np.random.default_rng(6).integers(0, 300, (500, 3)).astype(np.int32)
    bad = v.copy()
    bad[7, 1], bad[200, 2], bad[299, 0] = np.nan, np.inf, -np.inf
    with pytest.raises(ValueError, match="3 vertices have a non-finite coordinate"):
        ops.mesh_smooth(_dev(bad), _dev(f), iterations=2)
    out = f.copy()
    out[3, 2], out[400, 0], out[499, 1] = 300, -1, 2 ** 31 - 1
    with pytest.raises(ValueError, match=r"3 faces have a vertex index outside \[0, 300\)"):
        ops.mesh_smooth(_dev(v), _dev(out), iterations=2)
    _check(ops, _dev(v), _dev(f), _dev(v), "random faces: fans, degenerate faces, both windings", iterations=2)
    none = torch.zeros(0, 3, dtype=torch.int32, device="cuda")
    empty = _check(ops, _dev(v), none, None, "no faces", iterations=3, flip=1)
    assert empty[0].tobytes() == v.tobytes() and empty[2]["isolated_vertices"] == 300 and not empty[1].any()
    nothing = ops.mesh_smooth(torch.zeros(0, 3, device="cuda"), none, iterations=3, flip=1)
    assert nothing[0].shape == (0, 3) and nothing[1].shape == (0, 3) and nothing[2]["vertices"] == 0 and nothing[2]["exponent"] == 0
    zeros = np.zeros((300, 3), np.float32)
    zeros[5, 1] = -0.0
    still = _check(ops, _dev(zeros), _dev(f), None, "all zero", iterations=3, free_boundary=True)
    assert still[0].tobytes() == zeros.tobytes() and still[2]["exponent"] == 0


@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_runs_repeat_and_the_numbering_does_not_matter(ops, kind):
    vol, iso = _volume(kind, (64, 70, 50), 3)
    v, f, n, _ = ops.marching_cubes(_dev(vol), iso)
    kw = dict(iterations=4, flip=-1)
    first = ops.mesh_smooth(v, f, n, **kw)
    again = ops.mesh_smooth(v, f, n, **kw)
    assert all(_np(a).tobytes() == _np(b).tobytes() for a, b in zip(first[:2], again[:2])) and first[2] == again[2]
    # another numbering of the vertices, another order of the faces: the same neighbour sets, the same exact sums
    rng = np.random.default_rng(9)
    pv = torch.from_numpy(rng.permutation(v.shape[0])).cuda()
    pf = torch.from_numpy(rng.permutation(f.shape[0])).cuda()
    inverse = torch.empty_like(pv)
    inverse[pv] = torch.arange(v.shape[0], device="cuda")
    v2, n2 = v[pv].contiguous(), n[pv].contiguous()
    f2 = inverse[f[pf].long()].to(torch.int32).contiguous()
    other = ops.mesh_smooth(v2, f2, n2, **kw)
    assert other[2] == first[2]
    assert torch.equal(other[0], first[0][pv]) and torch.equal(other[1], first[1][pv]), "row for row under the renumbering"
    rows = lambda t: np.sort(np.ascontiguousarray(_np(t)).view([("x", "<u4"), ("y", "<u4"), ("z", "<u4")]).ravel())   # noqa: E731
    assert rows(other[0]).tobytes() == rows(first[0]).tobytes(), "the same set of vertex rows, bit for bit"


def test_zero_iterations_and_plain_laplacian(ops):
    vol, iso = _volume("noise", (40, 33, 21), 5)
    v, f, n, _ = ops.marching_cubes(_dev(vol), iso)
    same = _check(ops, v, f, n, "zero iterations", iterations=0)
    assert same[0].tobytes() == _np(v).tobytes()
    laplace = _check(ops, v, f, None, "mu = 0", iterations=3, mu=0.0)
    taubin = _check(ops, v, f, None, "other factors", iterations=3, lam=1.0, mu=-1.0)
    assert laplace[0].tobytes() != taubin[0].tobytes()
    _check(ops, v, f, None, "mu = -0", iterations=2, mu=-0.0)


LIMIT, RES = 1.2, 64


def _run(model, tmp_path, tag, *extra):
    d = tmp_path / tag
    d.mkdir(exist_ok=True)
    return export_mesh(model, d, "--res", str(RES), "--limit", str(LIMIT), *extra), d


FILTER = ["--min-component-faces", "100", "--keep-largest", "2"]
SMOOTH = ["--smooth-iters", "5"]


@pytest.mark.parametrize("extra", [[], ["--normals", "network"], ["--super-sampling", "2"], FILTER, ["--simplify-cell", "2"]],
                         ids=["plain", "network", "ss2", "filtered", "simplified"])
def test_end_to_end_through_the_exporter(ops, scene, tmp_path, capsys, extra):
    from nerfmeshes_amd import mesh_nerf
    simplified = "--simplify-cell" in extra
    dense = FILTER if simplified else extra                          # the simplified case: filter, smooth, simplify
    (v0, f0, n0, _), _ = _run(scene, tmp_path, "dense", *dense)
    capsys.readouterr()
    (v, f, n, c), d = _run(scene, tmp_path, "smoothed", *dense, *(extra if simplified else []), *SMOOTH)
    out = capsys.readouterr().out
    grid_normals = "network" not in extra
    wv, wn, info = SM.smooth(_np(v0), _np(f0), _np(n0), iterations=5, flip=mesh_nerf.SMOOTH_FLIP)
    wf = _np(f0)
    moved = np.sqrt(((wv.astype(np.float32) - _np(v0)) ** 2).sum(1)).max() / (2 * LIMIT / RES)
    assert moved > 0
    if simplified:                                                   # the clustering averages smoothed positions and new normals
        wv, wf, wn, sinfo = MS.simplify(wv, wf, wn, cell=2.0 * (2.0 * LIMIT / RES), origin=(-LIMIT,) * 3)
        assert 0 < sinfo["faces_kept"] < len(f0)
        assert out.index("Component filter") < out.index("Smooth:") < out.index("Simplify:")
    assert _np(v).tobytes() == wv.tobytes() and _np(f).tobytes() == wf.tobytes() and v.shape == wv.shape and f.shape == wf.shape
    if grid_normals:
        assert _np(n).tobytes() == wn.tobytes()
    else:                                                            # the gradient is taken at the NEW positions
        own, _ = mesh_nerf.network_normals(scene.get_model().hip("f32"), v, n)
        assert torch.equal(own, n) and out.index("Smooth:") < out.index("Network normals")
    assert c.shape == (len(wv), 3) and np.isfinite(c).all()
    kept = info["boundary_vertices"]
    line = next(l for l in out.splitlines() if l.startswith("Smooth:"))
    assert line.startswith(f"Smooth: 5 iterations (lambda 0.5, mu -0.53): {len(v0)} vertices, {kept} boundary vertices kept in place, "
                           f"{info['isolated_vertices']} isolated, {info['nonmanifold_edges']} non-manifold edges, largest "
                           f"displacement ") and line.endswith(" voxels")
    assert abs(float(line.split()[-2]) - moved) < 1e-3
    if extra == FILTER:                                              # the filter ran first
        assert out.index("Component filter") < out.index("Smooth:")
    lines = open(d / "mesh.obj").read().splitlines()
    assert sum(l.startswith("v ") for l in lines) == len(wv) and sum(l.startswith("f ") for l in lines) == len(wf)
    assert sum(l.startswith("vn ") for l in lines) == len(wv)


def test_zero_is_off(ops, scene, tmp_path, capsys):
    _, d0 = _run(scene, tmp_path, "a")
    _, d1 = _run(scene, tmp_path, "b", "--smooth-iters", "0")
    assert "Smooth" not in capsys.readouterr().out
    assert open(d0 / "mesh.obj", "rb").read() == open(d1 / "mesh.obj", "rb").read()


def test_cache_keeps_the_unsmoothed_geometry(ops, scene, tmp_path):
    (v0, f0, n0, _), _ = _run(scene, tmp_path, "dense")
    (v1, f1, n1, _), d = _run(scene, tmp_path, "cache", "--override-cache-mesh", *SMOOTH)
    assert not torch.equal(v1, v0)
    cv, cf, cn, _ = torch.load(d / "mesh_cache.pt", weights_only=False)
    assert torch.equal(cv, v0.cpu()) and torch.equal(cf, f0.cpu()) and torch.equal(cn, n0.cpu()), "the cache is the unsmoothed mesh"
    first = open(d / "mesh.obj", "rb").read()
    os.remove(d / "mesh.obj")
    (v2, f2, n2, _), _ = _run(scene, tmp_path, "cache", "--use-cached-mesh", *SMOOTH)
    assert torch.equal(v2, v1) and torch.equal(f2, f1) and torch.equal(n2, n1)
    assert open(d / "mesh.obj", "rb").read() == first, "the cached mesh smoothed again gives the same OBJ bytes"


def test_two_ranks_sharing_one_gpu_equal_one_rank():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X")
    world = 2
    r = launch_ranks(os.path.join("tests", "tools", "smooth_dist_worker.py"), world, timeout=900)
    assert_ranks_ok(r, f"SMOOTH_DIST_OK world={world}")
