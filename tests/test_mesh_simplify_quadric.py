"""CPU: quadric placement of mesh simplification (--simplify-placement quadric) on the host side -- the numpy restatement
(tests/mesh_simplify_quadric.py) against a dict-and-loop implementation with Python's unbounded integers on every mesh of the
marching-cubes fixture, the bounds of the overflow proof on an adversarial mesh, the CROWDED and FAR rules, what the placement
gains on an analytic scene with a crease and a curved part, a planar sheet, a renumbering, mesh_nerf's option and the
argument checks of the three C entries."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import mc_oracle
from tests import mesh_simplify as MS
from tests import mesh_simplify_quadric as MQ
from tests.helpers import load_golden


@pytest.fixture(scope="module")
def meshes():
    g = load_golden("mc_cases")
    out = []
    for i in range(int(g["count"])):
        if f"err_{i}" in g.files:
            continue
        out.append((i, g[f"verts_{i}"].astype(np.float32), g[f"faces_{i}"].astype(np.int32), g[f"normals_{i}"].astype(np.float32)))
    return out


def _loop_vertex(x, origin, cell):
    """-> (cell index triple, lattice triple) of one vertex, as Python integers"""
    f32, f64 = np.float32, np.float64
    c = tuple(int(math.floor(f32(f32(x[k] - origin[k]) / cell))) for k in range(3))
    u = []
    for k in range(3):
        lo = f32(origin[k] + f32(f32(c[k]) * cell))
        t = f32(f32(x[k] - lo) / cell)
        u.append(int(np.rint(min(max(f64(t) * 256.0, -512.0), 512.0))))
    return c, tuple(u)


def _loop_corner(C0, u0, C1, u1, C2, u2):
    """one corner's nine terms with Python integers, or None when it is far"""
    e1 = [(C1[j] - C0[j]) * 256 + (u1[j] - u0[j]) for j in range(3)]
    e2 = [(C2[j] - C0[j]) * 256 + (u2[j] - u0[j]) for j in range(3)]
    if any(abs(e) > 512 for e in e1 + e2):
        return None
    n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
    d = -sum(n[j] * u0[j] for j in range(3))
    return [n[0] * n[0], n[0] * n[1], n[0] * n[2], n[1] * n[1], n[1] * n[2], n[2] * n[2], n[0] * d, n[1] * d, n[2] * d]


def _loop_sums(verts, faces, cell, origin):
    """-> ({cell: [nine sums, contributions]}, far corners), one corner at a time"""
    cell, origin = np.float32(cell), np.asarray(origin, np.float32)
    where = [_loop_vertex(x, origin, cell) for x in verts]
    sums, far = {}, 0
    for tri in faces.tolist():
        for k in range(3):
            (C0, u0), (C1, u1), (C2, u2) = where[tri[k]], where[tri[(k + 1) % 3]], where[tri[(k + 2) % 3]]
            terms = _loop_corner(C0, u0, C1, u1, C2, u2)
            if terms is None:
                far += 1
                continue
            row = sums.setdefault(C0, [[0] * 9, 0])
            row[0] = [a + b for a, b in zip(row[0], terms)]
            row[1] += 1
    return sums, far


def _restated_sums(verts, faces, cell, origin):
    origin, cell = MQ.grid(verts, cell, origin)
    Cv, u, _, cluster, first, _ = MQ.kept_clusters(verts, faces, origin, cell)
    sums, contributions, far = MQ.quadric_sums(faces, cluster, len(first), Cv, u)
    got = {tuple(Cv[first[k]].tolist()): [sums[k].tolist(), int(contributions[k])] for k in range(len(first)) if contributions[k]}
    return got, far, sums, contributions


@pytest.mark.parametrize("cell", [2.0, 3.7])
def test_integer_sums_match_unbounded_integers_on_every_fixture_mesh(meshes, cell):
    contributions = largest = 0
    for i, v, f, n in meshes:
        got, far, sums, counts = _restated_sums(v, f, cell, (0, 0, 0))
        want, want_far = _loop_sums(v, f, cell, (0, 0, 0))
        assert got == want and far == want_far, f"mesh {i}"        # Python's integers cannot wrap: neither did int64
        contributions += int(counts.sum())
        largest = max(largest, int(np.abs(sums).max()) if len(sums) else 0)
    assert contributions > 3 * 14881 * 0.9 and 0 < largest < 2 ** 51


def test_lattice_clamps_and_edges_of_exactly_two_cells_are_not_far():
    assert MQ.lattice_of(np.float32([0, 1, 0.5, 2, -2, 2.01, -7, 1e30, -1e30, np.nan, 1 / 512, 3 / 512])).tolist() == \
        [0, 256, 128, 512, -512, 512, -512, 512, -512, -512, 0, 2]                   # rint: ties to even
    # synthetic cells and lattice coordinates at the ends of their ranges: the proof's bounds hold and are reached
    # vertex 0 at u = +2^9, 1 and 2 at -2^9 six or two cells further: from corner 0, e1 = (512, -512, 512), e2 = (512, 512, -512),
    # so nrm = (0, 2^19, 2^19) and d = -2^29; vertex 3 makes an edge of 513
    Cv = np.array([[5, 5, 5], [11, 7, 11], [11, 11, 7], [8, 5, 5]], np.int64)
    u = np.array([[512, 512, 512], [-512, -512, -512], [-512, -512, -512], [257, 512, 512]], np.int64)
    faces = np.array([[0, 1, 2], [0, 3, 2], [0, 0, 1]], np.int32)
    terms, far = MQ.corner_terms(faces, Cv, u)
    for f, tri in enumerate(faces.tolist()):
        for k in range(3):
            a, b, c = tri[k], tri[(k + 1) % 3], tri[(k + 2) % 3]
            want = _loop_corner(Cv[a].tolist(), u[a].tolist(), Cv[b].tolist(), u[b].tolist(), Cv[c].tolist(), u[c].tolist())
            assert bool(far[f, k]) == (want is None) and terms[f, k].tolist() == ([0] * 9 if want is None else want), (f, k)
    assert not far[0, 0] and far[0, 1] and far[1, 0], "512 is near, 1024 and 513 are far"
    assert terms[0, 0].tolist() == [0, 0, 0, 2 ** 38, 2 ** 38, 2 ** 38, 0, -2 ** 48, -2 ** 48]
    assert not far[2].any() and not terms[2].any(), "a repeated index counts and adds zeros"
    assert np.abs(terms[..., :6]).max() <= 2 ** 38 and np.abs(terms[..., 6:]).max() < 2 ** 49


def _fan(count, shift, rng):
    """`count` faces with one corner in each of the cells (0,0,0), (1,0,0), (0,1,0) + shift (a cell is 1): each of the three
    clusters gets exactly `count` contributions and has 2 * count members"""
    corners = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    v = (corners[None] + rng.random((count, 3, 3)) * 0.8 + 0.1 + np.float32(shift)).astype(np.float32)
    spare = (corners[None] + rng.random((count, 3, 3)) * 0.8 + 0.1 + np.float32(shift)).astype(np.float32)
    return np.concatenate((v.reshape(-1, 3), spare.reshape(-1, 3))), np.arange(3 * count, dtype=np.int32).reshape(-1, 3)


def test_crowded_far_and_contribution_less_clusters_get_the_mean():
    rng = np.random.default_rng(11)
    va, fa = _fan(1 << 13, (0, 0, 0), rng)                           # 2^13 contributions: solved
    vb, fb = _fan((1 << 13) + 1, (10, 0, 0), rng)                    # one more: crowded
    # two faces whose corners are five cells apart, opposite windings so that both stay: every corner is far
    vc = np.float32([[0.2, 0.3, 20.4], [5.5, 0.5, 20.5], [0.5, 5.5, 20.5], [0.7, 0.6, 20.1], [5.1, 0.2, 20.8], [0.3, 5.9, 20.2]])
    fc = np.int32([[0, 1, 2], [3, 5, 4]])
    v = np.concatenate((va, vb, vc))
    f = np.concatenate((fa, fb + len(va), fc + len(va) + len(vb))).astype(np.int32)
    got, far, sums, contributions = _restated_sums(v, f, 1.0, (0, 0, 0))
    assert far == 6 and sorted(set(contributions.tolist())) == [0, 1 << 13, (1 << 13) + 1]
    want, want_far = _loop_sums(v, f, 1.0, (0, 0, 0))
    assert got == want and far == want_far
    assert np.abs(sums[:, :6]).max() <= 2 ** 51 and np.abs(sums[:, 6:]).max() < 2 ** 62
    qv, qf, _, info = MQ.simplify(v, f, None, cell=1.0, origin=(0, 0, 0))
    mv, mf, _, mean_info = MS.simplify(v, f, None, cell=1.0, origin=(0, 0, 0))
    assert qf.tobytes() == mf.tobytes() and {k: info[k] for k in MS.INFO_KEYS} == mean_info and tuple(info) == MQ.INFO_KEYS
    assert len(qv) == 9 and info["crowded_clusters"] == 3 and info["far_corners"] == 6
    assert info["quadric_clusters"] + info["singular_clusters"] == 3 and info["quadric_clusters"] >= 1
    shifted = qv[:, 0] > 9                                           # the crowded fan
    high = qv[:, 2] > 19                                             # the clusters without a contribution
    assert shifted.sum() == 3 and high.sum() == 3
    assert qv[shifted | high].tobytes() == mv[shifted | high].tobytes(), "the mean, bit for bit"
    assert (qv[~(shifted | high)] != mv[~(shifted | high)]).any()


R = (np.array([[math.cos(0.5), -math.sin(0.5), 0], [math.sin(0.5), math.cos(0.5), 0], [0, 0, 1]]) @
     np.array([[1, 0, 0], [0, math.cos(0.3), -math.sin(0.3)], [0, math.sin(0.3), math.cos(0.3)]]))
CENTRE = np.array([31.3, 32.1, 30.7])
HALF = np.array([18.0, 14.0, 10.0])


def _sdf(p):
    """min(box, sphere): a box of half-sizes HALF about CENTRE rotated by Rz(0.5) Rx(0.3), a sphere of radius 9 at CENTRE + (12, 0, 9)"""
    p = np.asarray(p, np.float64)
    q = np.abs((p - CENTRE) @ R) - HALF                              # R^T (p - c), row-wise
    box = np.sqrt((np.maximum(q, 0.0) ** 2).sum(-1)) + np.minimum(q.max(-1), 0.0)
    sphere = np.sqrt(((p - (CENTRE + np.array([12.0, 0.0, 9.0]))) ** 2).sum(-1)) - 9.0
    return np.minimum(box, sphere)


@pytest.fixture(scope="module")
def analytic():
    g = np.stack(np.meshgrid(*[np.arange(64, dtype=np.float64)] * 3, indexing="ij"), -1)
    v, f, n, _ = mc_oracle.marching_cubes(_sdf(g).astype(np.float32), 0.0)
    return v.astype(np.float32), f.astype(np.int32), n.astype(np.float32)


@pytest.mark.parametrize("cell", [4.0, 8.0])
def test_quadric_vertices_lie_closer_to_the_true_surface(analytic, cell):
    """quadric / mean of the mean |sdf| over the output vertices: 0.357 at cell 4, 0.278 at cell 8 (the bar is 0.5)"""
    v, f, n = analytic
    assert (len(v), len(f)) == (6894, 13784)
    mv, mf, mn, _ = MS.simplify(v, f, n, cell=cell, origin=(0, 0, 0))
    qv, qf, qn, info = MQ.simplify(v, f, n, cell=cell, origin=(0, 0, 0))
    assert qf.tobytes() == mf.tobytes() and qn.tobytes() == mn.tobytes() and qv.shape == mv.shape
    mean_error, quadric_error = np.abs(_sdf(mv)), np.abs(_sdf(qv))
    print(f"cell {cell:g}: mean placement {mean_error.mean():.4f} / {mean_error.max():.3f}, quadric {quadric_error.mean():.4f} / "
          f"{quadric_error.max():.3f} voxels (mean / max); {info}")
    assert quadric_error.mean() <= 0.5 * mean_error.mean()
    assert quadric_error.max() <= mean_error.max()
    assert info["quadric_clusters"] > 0.9 * info["vertices_kept"] and info["crowded_clusters"] == 0 and info["far_corners"] == 0
    # every vertex in the closed box of its cell, up to the final fp32 rounding
    origin, c32 = MQ.grid(v, cell, (0, 0, 0))
    reps = MQ.kept_clusters(v, f, origin, c32)[5]
    c, _ = MS.cells(v[reps], origin, c32)
    lo = (origin + c * c32).astype(np.float64)
    ulp = np.spacing(np.abs(qv).max(), dtype=np.float32).astype(np.float64)
    assert (qv >= lo - ulp).all() and (qv <= lo + np.float64(c32) + ulp).all()


def test_a_tilted_plane_keeps_the_mean():
    """every plane of a cluster is the sheet's own, and the members' mean lies in it: the residual is zero up to fp64 rounding"""
    k = 41
    i, j = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
    x, y = 0.25 + i * (19 / 64), 0.5 + j * (21 / 64)                 # multiples of 1 / 64 of a cell
    v = np.stack((x, y, 3.0 + (x + 2 * y) / 4), -1).reshape(-1, 3).astype(np.float32)   # z: a multiple of 1 / 256
    assert np.array_equal(v * 256, np.rint(v * 256)), "lattice-exact"
    idx = np.arange(k * k).reshape(k, k)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    f = np.concatenate((np.stack((a, b, c), 1), np.stack((a, c, d), 1))).astype(np.int32)
    mv, mf, _, _ = MS.simplify(v, f, None, cell=1.0, origin=(0, 0, 0))
    qv, qf, _, info = MQ.simplify(v, f, None, cell=1.0, origin=(0, 0, 0))
    assert qf.tobytes() == mf.tobytes() and info["quadric_clusters"] > 100 and info["singular_clusters"] == 0
    assert np.abs(qv.astype(np.float64) - mv.astype(np.float64)).max() <= 2.0 ** -20


@pytest.mark.parametrize("cell", [4.0, 2.5])
def test_a_renumbering_gives_the_same_vertex_rows(analytic, cell):
    v, f, n = analytic
    first = MQ.simplify(v, f, n, cell=cell, origin=(0, 0, 0))
    rng = np.random.default_rng(5)
    pv, pf = rng.permutation(len(v)), rng.permutation(len(f))
    inverse = np.empty_like(pv)
    inverse[pv] = np.arange(len(v))
    other = MQ.simplify(v[pv], inverse[f[pf]].astype(np.int32), n[pv], cell=cell, origin=(0, 0, 0))
    assert other[3] == first[3]
    rows = lambda a: np.sort(np.ascontiguousarray(a).view([("x", "<u4"), ("y", "<u4"), ("z", "<u4")]).ravel())   # noqa: E731
    assert rows(other[0]).tobytes() == rows(first[0]).tobytes(), "the same set of vertex rows, bit for bit"


def test_mean_placement_is_the_old_restatement_and_others_raise(meshes):
    _, v, f, n = meshes[40]
    a, b = MQ.simplify(v, f, n, cell=2.0, placement="mean"), MS.simplify(v, f, n, cell=2.0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3] and tuple(a[3]) == MS.INFO_KEYS
    with pytest.raises(ValueError, match="placement"):
        MQ.simplify(v, f, n, cell=2.0, placement="median")


def test_parser_and_feature_checks(tmp_path):
    import argparse
    from nerfmeshes_amd import mesh_nerf
    p = mesh_nerf.build_parser()
    assert p.parse_args([]).simplify_placement == "mean"
    assert p.parse_args(["--simplify-placement", "quadric"]).simplify_placement == "quadric"
    assert "(addition)" in next(a.help for a in p._actions if a.dest == "simplify_placement")
    with pytest.raises(SystemExit):
        p.parse_args(["--simplify-placement", "median"])
    assert "simplify_placement" in mesh_nerf.FEATURES["simplify"].options
    assert mesh_nerf.check_features(p.parse_args(["--simplify-cell", "4", "--simplify-placement", "quadric"])) == {"simplify"}
    assert mesh_nerf.check_features(p.parse_args(["--simplify-placement", "mean"])) == set()
    assert mesh_nerf.check_features(argparse.Namespace(simplify_cell=2.0)) == {"simplify"}
    with pytest.raises(ValueError, match="--simplify-placement quadric needs --simplify-cell"):
        mesh_nerf.check_features(p.parse_args(["--simplify-placement", "quadric"]))
    with pytest.raises(ValueError, match="--simplify-placement must be mean or quadric"):
        mesh_nerf.check_features(argparse.Namespace(simplify_cell=2.0, simplify_placement="median"))
    args = p.parse_args(["--simplify-placement", "quadric", "--save-dir", str(tmp_path)])
    with pytest.raises(ValueError, match="needs --simplify-cell"):
        mesh_nerf.export_marching_cubes(None, args, None, "cpu")
    args = p.parse_args(["--simplify-placement", "quadric", "--route", "script", "--save-dir", str(tmp_path)])
    with pytest.raises(ValueError, match="route script"):
        mesh_nerf.export_marching_cubes(None, args, None, "cpu")
    assert not any(tmp_path.iterdir()), "refused before anything is written"


def test_argument_errors_without_a_gpu():
    from nerfmeshes_amd import _lib
    lib = _lib.load()
    null, one = C.c_void_p(None), C.c_void_p(256)           # never dereferenced: validation fails first
    counts = (C.c_int64 * 5)(*([-7] * 5))

    def err():
        return (lib.nm_last_error() or b"").decode()

    def faces(ws=one, v=one, nv=20, f=one, nf=10, o=(0.0, 0.0, 0.0), cell=1.0, flags=0, qws=one):
        return lib.nm_mesh_simplify_quadric_faces(ws, v, nv, f, nf, *o, cell, flags, qws, null)

    def emit(ws=one, qws=one, v=one, nv=20, f=one, nf=10, n=null, o=(0.0, 0.0, 0.0), cell=1.0, kv=5, kf=5, ov=one, of=one, on=null,
             out=counts):
        return lib.nm_mesh_simplify_emit_quadric(ws, qws, v, nv, f, nf, n, *o, cell, kv, kf, ov, of, on, out, null)

    for fn in (faces, emit):
        for kw in (dict(v=null), dict(f=null), dict(ws=null), dict(qws=null)):
            assert fn(**kw) == 2 and "bad argument" in err(), (fn.__name__, kw)
        for kw in (dict(nf=-1), dict(nv=-1), dict(nv=1 << 31), dict(nf=(1 << 31) - 64)):
            assert fn(**kw) == 2 and "2^31" in err(), (fn.__name__, kw)
        assert fn(nf=3, nv=0) == 2 and "faces without vertices" in err()
        for cell in (0.0, -1.0, float("inf"), float("nan")):
            assert fn(cell=cell) == 2 and "cell size" in err(), (fn.__name__, cell)
        for o in ((float("nan"), 0.0, 0.0), (0.0, float("inf"), 0.0), (0.0, 0.0, float("-inf"))):
            assert fn(o=o) == 2 and "origin" in err(), (fn.__name__, o)
    assert faces(flags=2) == 2 and "flags" in err()
    assert emit(out=None) == 2 and "bad argument" in err()
    assert emit(kv=21) == 2 and "kept counts" in err()
    assert emit(kf=11) == 2 and "kept counts" in err()
    assert emit(ov=null) == 2 and "without its output" in err()
    assert emit(n=one) == 2 and "without its output" in err()
    assert emit(of=null) == 2 and "null face output" in err()
    assert list(counts) == [-7] * 5, "nothing is returned by a rejected call"
    # the second workspace: 128 bytes per slot of the vertex table; the first one is the size it was
    size = lib.nm_mesh_simplify_quadric_workspace_bytes
    assert size(-1, 0) == 0 and size(0, -1) == 0 and size(1 << 31, 0) == 0 and size(0, (1 << 31) - 64) == 0
    assert size(0, 0) == 256 + 128 * 64 and size(750_000, 1_500_000) == 256 + 128 * (1 << 21)
    assert 64 * (1 << 21) + 4 * (1 << 22) <= lib.nm_mesh_simplify_workspace_bytes(750_000, 1_500_000) <= \
        64 * (1 << 21) + 4 * (1 << 22) + 16 * 2_250_000
    assert lib.nm_abi_version() == 6


def test_wrapper_checks_the_placement_before_the_device():
    import torch
    from nerfmeshes_amd import hip_ops
    v, f = torch.zeros(8, 3), torch.zeros(4, 3, dtype=torch.int32)
    for placement in ("median", None, "Quadric"):
        with pytest.raises(ValueError, match="placement must be one of"):
            hip_ops.mesh_simplify(v, f, cell=1.0, placement=placement)
    assert hip_ops.SIMPLIFY_QUADRIC_COUNTS == MQ.COUNT_KEYS
