"""CPU: adaptive levels of mesh simplification (--simplify-levels / --simplify-error) on the host side -- the nesting of the
grids the partition argument rests on, the numpy restatement (tests/mesh_simplify_adaptive.py) against a dict-and-loop
implementation with Python's unbounded integers for the sums and the maxima, levels = 0 as the quadric placement, the
acceptance rules on constructed meshes (an unbounded error, two parallel sheets either side of the bound, a crowded coarse
cell, a far corner, a cell without a contribution, a singular status), a renumbering, what the levels gain on the analytic
scene, mesh_nerf's options and the argument checks of the wrapper and the C entries."""
import argparse
import ctypes as C
import math
import struct

import numpy as np
import pytest

from oracle import mc_oracle
from tests import mesh_simplify as MS
from tests import mesh_simplify_adaptive as MA
from tests import mesh_simplify_quadric as MQ
from tests.helpers import load_golden

INF = float("inf")


@pytest.fixture(scope="module")
def meshes():
    g = load_golden("mc_cases")
    out = []
    for i in range(int(g["count"])):
        if f"err_{i}" in g.files:
            continue
        out.append((i, g[f"verts_{i}"].astype(np.float32), g[f"faces_{i}"].astype(np.int32), g[f"normals_{i}"].astype(np.float32)))
    return out


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


# ---- nesting ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell, origin", [(1.0, (0.0, 0.0, 0.0)), (1.5, (-1.2, 0.3, 7.0)), (0.0375, (-1.2, -1.2, -1.2)),
                                          (4.0, (0.1, 0.2, 0.3)), (3.7, (-100.0, 5.5, 1e-3))])
def test_the_grids_nest_exactly(cell, origin):
    """c_l == c_0 >> l per axis, for vertices on the faces of the cells of every level, one ulp and two either side of them, and
    at random: cell * 2^l is exact in fp32, so (x - o) / (cell * 2^l) is the level-0 quotient scaled by a power of two"""
    cell32, o = np.float32(cell), np.float32(origin)
    rng = np.random.default_rng(7)
    steps = np.concatenate((np.arange(0, 70), rng.integers(0, 1 << 12, 200), [(1 << 21) - 1, (1 << 21) - 256, 1 << 20])).astype(np.float32)
    on = o[None, None, :] + steps[:, None, None] * cell32              # (N,1,3): on (or an ulp from) a face of a cell
    near = on
    for _ in range(2):
        near = np.concatenate((near, np.nextafter(near, np.float32(np.inf)), np.nextafter(near, np.float32(-np.inf))), 1)
    v = np.concatenate((near.reshape(-1, 3), (o + rng.random((4000, 3)) * 300 * cell32).astype(np.float32)))
    c0, bad0 = MS.cells(v, o, cell32)
    v, c0 = v[~bad0], c0[~bad0].astype(np.int64)
    assert len(v) > 5000 and (c0 % 8 == 7).any() and (c0 % 8 == 0).any()
    for level in range(1, MA.MAX_LEVELS + 1):
        cell_l = MA.level_cell(cell32, level)
        assert cell_l.dtype == np.float32 and float(cell_l) == float(cell32) * 2.0 ** level, "exact"
        c, bad = MS.cells(v, o, cell_l)
        assert not bad.any(), "good at level 0: good at every level"
        assert np.array_equal(c.astype(np.int64), c0 >> level), level


# ---- the restatement against loops with unbounded integers -------------------------------------------------------------------

def _loop_vertex(x, origin, cell):
    f32, f64 = np.float32, np.float64
    c = tuple(int(math.floor(f32(f32(x[k] - origin[k]) / cell))) for k in range(3))
    u = []
    for k in range(3):
        lo = f32(origin[k] + f32(f32(c[k]) * cell))
        t = f32(f32(x[k] - lo) / cell)
        u.append(int(np.rint(min(max(f64(t) * 256.0, -512.0), 512.0))))
    return c, tuple(u)


def _loop_level(verts, faces, origin, cell_l, frac_of):
    """One level, one corner at a time -> {cell: dict(members, sums (nine Python integers), contributions, far, error: the
    largest d2's bits as a Python integer)}.  frac_of(cell) -> (solved, frac): the placed point, which MQ's tests pin."""
    where = [_loop_vertex(x, origin, cell_l) for x in verts]
    rows = {}
    for i, (c, _) in enumerate(where):
        rows.setdefault(c, dict(members=[], sums=[0] * 9, contributions=0, far=False, error=0))["members"].append(i)
    for tri in faces.tolist():
        for k in range(3):
            (C0, u0), (C1, u1), (C2, u2) = where[tri[k]], where[tri[(k + 1) % 3]], where[tri[(k + 2) % 3]]
            e1 = [(C1[j] - C0[j]) * 256 + (u1[j] - u0[j]) for j in range(3)]
            e2 = [(C2[j] - C0[j]) * 256 + (u2[j] - u0[j]) for j in range(3)]
            row = rows[C0]
            if any(abs(e) > 512 for e in e1 + e2):
                row["far"] = True
                continue
            n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
            d = -sum(n[j] * u0[j] for j in range(3))
            terms = [n[0] * n[0], n[0] * n[1], n[0] * n[2], n[1] * n[1], n[1] * n[2], n[2] * n[2], n[0] * d, n[1] * d, n[2] * d]
            row["sums"] = [a + b for a, b in zip(row["sums"], terms)]
            row["contributions"] += 1
            solved, frac = frac_of(C0)
            if solved and any(n):
                x = [float(frac[j]) * 256.0 for j in range(3)]                 # Python floats: IEEE doubles, one rounding each
                nf = [float(n[j]) for j in range(3)]
                s = (nf[0] * (x[0] - float(u0[0])) + nf[1] * (x[1] - float(u0[1]))) + nf[2] * (x[2] - float(u0[2]))
                den = (nf[0] * nf[0] + nf[1] * nf[1]) + nf[2] * nf[2]
                row["error"] = max(row["error"], _bits((s * s) / den))
    return rows


def _restated_level(v, f, origin, cell_l):
    data = MA.level_clusters(v, f, None, origin, cell_l)
    cells = {tuple(data["C"][data["first"][k]].tolist()): k for k in range(len(data["first"]))}
    return data, cells


@pytest.mark.parametrize("cell, levels", [(2.0, 2), (1.5, 3)])
def test_levels_match_loops_with_unbounded_integers_on_fixture_meshes(meshes, cell, levels):
    """members, representatives, far marks and the error maxima (as bits) of every cluster of every level; then the choice:
    every vertex walks down from the coarsest level on its own"""
    checked = errors = 0
    for i, v, f, n in meshes[::9]:
        origin, cell32 = MQ.grid(v, cell, (0, 0, 0))
        error = 0.3 * cell
        out = MA.simplify(v, f, n, cell=cell, origin=(0, 0, 0), levels=levels, max_error=error, details=True)
        detail = out[4]
        per_level = {}
        for level in range(levels, -1, -1):
            cell_l = MA.level_cell(cell32, level)
            data, cells = _restated_level(v, f, origin, cell_l)
            solved = (data["status"] & MQ.SOLVED) != 0
            rows = _loop_level(v, f, origin, cell_l, lambda c: (bool(solved[cells[c]]), data["frac"][cells[c]]))
            assert set(rows) == set(cells), f"mesh {i} level {level}"
            for c, row in rows.items():
                k = cells[c]
                assert row["members"] == np.flatnonzero(data["cluster"] == k).tolist() and row["members"][0] == data["first"][k]
                assert row["far"] == bool(data["far"][k]) and row["error"] == _bits(data["error"][k]), (i, level, c)
                errors += row["error"] > 0
            per_level[level] = (rows, {m: c for c, row in rows.items() for m in row["members"]}, data, cells, solved)
        for vertex in range(len(v)):
            for level in range(levels, -1, -1):
                rows, cell_of, data, cells, solved = per_level[level]
                row = rows[cell_of[vertex]]
                tol2 = MA.tolerance2(error, MA.level_cell(cell32, level))
                ok = level == 0 or len(row["members"]) == 1 or (
                    bool(solved[cells[cell_of[vertex]]]) and not row["far"] and row["error"] <= _bits(tol2))
                if ok:
                    break
            assert detail["level"][vertex] == level and detail["rep"][vertex] == row["members"][0], (i, vertex)
        checked += 1
    assert checked >= 70 and errors > 50


def test_the_error_is_taken_in_the_stated_order():
    """one corner by hand: n = (3, -5, 7), u0 = (10, 20, 30), x = (10.5, 19.25, 31.125)"""
    n, u0 = np.array([[3, -5, 7]], np.int64), np.array([[10, 20, 30]], np.int64)
    x = np.array([[10.5, 19.25, 31.125]])
    s = (3 * 0.5 + -5 * -0.75) + 7 * 1.125
    assert MA.corner_d2(n, u0, x).tolist() == [(s * s) / ((9.0 + 25.0) + 49.0)]
    assert float(MA.tolerance2(0.3, np.float32(2.0))) == ((0.3 / 2.0) * 256.0) ** 2 and MA.tolerance2(INF, np.float32(2.0)) == INF
    assert MA.tolerance2(0.0, np.float32(1.5)) == 0.0


def test_levels_zero_is_the_quadric_placement(meshes):
    for _, v, f, n in meshes[5::50]:
        for placement in ("quadric", "mean"):
            a = MA.simplify(v, f, n, cell=2.0, placement=placement, levels=0, max_error=123.0)
            b = MQ.simplify(v, f, n, cell=2.0, placement=placement)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3] and tuple(a[3]) == tuple(b[3])


def test_info_keys_and_their_sums(meshes):
    _, v, f, n = meshes[40]
    info = MA.simplify(v, f, n, cell=1.5, levels=3, max_error=0.2)[3]
    assert tuple(info) == MA.INFO_KEYS and info["levels"] == 3
    assert all(len(info[k]) == 4 for k in MA.LEVEL_KEYS + ("level_kept",))
    assert sum(info["level_vertices"]) == info["vertices"] and sum(info["level_clusters"]) == info["clusters"]
    assert sum(info["level_kept"]) == info["vertices_kept"] and all(k <= c for k, c in zip(info["level_kept"], info["level_clusters"]))
    assert all(info[k][0] == 0 for k in MA.LEVEL_KEYS[2:]), "level 0 refuses nothing"
    assert 0.0 <= info["largest_error"] <= 0.2


# ---- the acceptance rules on constructed meshes ------------------------------------------------------------------------------

def _octahedron(centre, radius):
    c = np.float32(centre)
    v = np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]) * np.float32(radius) + c
    f = np.int32([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    return v.astype(np.float32), f


def test_a_mesh_inside_one_coarsest_cell_becomes_one_cluster_and_no_faces():
    v, f = _octahedron((2.0, 2.0, 2.0), 1.5)                          # inside the level-2 cell [0, 4)^3 of cell = 1
    out_v, out_f, _, info = MA.simplify(v, f, None, cell=1.0, origin=(0, 0, 0), levels=2, max_error=INF)
    assert info["clusters"] == 1 and info["level_clusters"] == (0, 0, 1) and info["level_vertices"] == (0, 0, 6)
    assert info["faces_kept"] == 0 and info["degenerate_faces"] == 8 and len(out_f) == 0
    assert len(out_v) == 0 and info["vertices_kept"] == 0, "a cluster no face is left on goes, as under uniform clustering"
    # with no error allowed the same mesh stays as fine as level 0 makes it
    fine = MA.simplify(v, f, None, cell=1.0, origin=(0, 0, 0), levels=2, max_error=0.0)
    uniform = MQ.simplify(v, f, None, cell=1.0, origin=(0, 0, 0))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(fine[:2], uniform[:2]))
    # level 1 (cells of 2): +x, +y and +z share the cell (1, 1, 1), refused; the other three are alone in theirs, hence taken there
    assert fine[3]["level_vertices"] == (3, 3, 0) and fine[3]["refused_error"] == (0, 1, 1) and fine[3]["largest_error"] == 0.0


R = (np.array([[math.cos(0.5), -math.sin(0.5), 0], [math.sin(0.5), math.cos(0.5), 0], [0, 0, 1]]) @
     np.array([[1, 0, 0], [0, math.cos(0.3), -math.sin(0.3)], [0, math.sin(0.3), math.cos(0.3)]]))
CENTRE = np.array([31.3, 32.1, 30.7])
HALF = np.array([18.0, 14.0, 10.0])


def _sdf(p):
    """min(box, sphere): a box of half-sizes HALF about CENTRE rotated by Rz(0.5) Rx(0.3), a sphere of radius 9 at CENTRE + (12, 0, 9):
    the analytic scene of tests/test_mesh_simplify_quadric.py"""
    p = np.asarray(p, np.float64)
    q = np.abs((p - CENTRE) @ R) - HALF
    box = np.sqrt((np.maximum(q, 0.0) ** 2).sum(-1)) + np.minimum(q.max(-1), 0.0)
    sphere = np.sqrt(((p - (CENTRE + np.array([12.0, 0.0, 9.0]))) ** 2).sum(-1)) - 9.0
    return np.minimum(box, sphere)


@pytest.fixture(scope="module")
def analytic():
    g = np.stack(np.meshgrid(*[np.arange(64, dtype=np.float64)] * 3, indexing="ij"), -1)
    v, f, n, _ = mc_oracle.marching_cubes(_sdf(g).astype(np.float32), 0.0)
    return v.astype(np.float32), f.astype(np.int32), n.astype(np.float32)


def _check_choice(detail, levels):
    """every vertex sits at the largest level whose cell is acceptable"""
    for level in range(levels, 0, -1):
        data = detail["data"][level]
        ok = MA.acceptable(data, detail["tol2"][level], level)[data["cluster"]]
        assert ok[detail["level"] == level].all(), "chosen: acceptable"
        assert not ok[detail["level"] < level].any(), "not chosen although no coarser level took it: not acceptable"


def test_an_unbounded_error_takes_every_solvable_cell(analytic):
    v, f, n = analytic
    out = MA.simplify(v, f, n, cell=2.0, origin=(0, 0, 0), levels=2, max_error=INF, details=True)
    _check_choice(out[4], 2)
    assert out[3]["level_vertices"] == (0, 0, len(v)) and out[3]["refused_error"] == (0, 0, 0)
    uniform = MQ.simplify(v, f, n, cell=8.0, origin=(0, 0, 0))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out[:3], uniform[:3])), "every cell solvable: uniform clustering at K * 2^L"


def _sheets(h, k=17):
    """two parallel sheets z = 0.5 and z = 0.5 + h over [0, 8]^2, vertices every 0.5: lattice-exact, the same x, y on both"""
    i, j = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
    idx = np.arange(k * k).reshape(k, k)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    tris = np.concatenate((np.stack((a, b, c), 1), np.stack((a, c, d), 1)))
    low = np.stack((i.ravel() * 0.5, j.ravel() * 0.5, np.full(k * k, 0.5)), 1)
    high = low + np.array([0.0, 0.0, h])
    return np.concatenate((low, high)).astype(np.float32), np.concatenate((tris, tris + k * k)).astype(np.int32)


def test_two_parallel_sheets_are_welded_iff_half_their_distance_is_within_the_bound():
    """cell 1, one coarser level: the sheets z = 0.5 and z = 1.25 share the coarse cells [0, 2) and no fine cell.  A coarse
    cluster's planes are the two sheets', its members' mean lies midway and is the quadric's minimum exactly (the residual
    there is zero in integers), so its error is h / 2 = 0.375 = 48 lattice units of the coarse cell, without rounding: the
    cells are taken at E = h / 2 and one lattice unit (1 / 128) above, refused one unit below"""
    h = 0.75
    v, f = _sheets(h)
    unit = 2.0 / 256
    for error, welded in ((h / 2 + unit, True), (h / 2, True), (h / 2 - unit, False), (0.0, False), (INF, True)):
        out_v, out_f, _, info = MA.simplify(v, f, None, cell=1.0, origin=(0, 0, 0), levels=1, max_error=error)
        z = set(out_v[:, 2].tolist())
        if welded:
            assert info["level_vertices"] == (0, len(v)) and info["refused_error"] == (0, 0), error
            assert z == {0.875} and info["largest_error"] == h / 2, "one sheet midway"
            assert info["duplicate_faces"] > 0, "the two sheets' triangles coincide"
        else:
            assert info["level_vertices"] == (len(v), 0) and info["refused_error"] == (0, 25) and info["level_clusters"] == (162, 0), error
            assert z == {0.5, 1.25} and info["largest_error"] == 0.0, "both sheets where they were"
            assert out_f.tobytes() == MQ.simplify(v, f, None, cell=1.0, origin=(0, 0, 0))[1].tobytes()


def test_crowded_far_and_contribution_less_coarse_cells_are_refused_and_counted():
    rng = np.random.default_rng(21)
    # 3000 small triangles inside the coarse cell [0, 2)^3: 9000 corners > 2^13 contributions there, far fewer in its fine cells
    base = rng.random((3000, 1, 3)) * 1.7 + 0.05
    va = (base + rng.random((3000, 3, 3)) * 0.2).astype(np.float32).reshape(-1, 3)
    fa = np.arange(9000, dtype=np.int32).reshape(-1, 3)
    # an octahedron in the coarse cell [10, 12)^3, one of its vertices also on a triangle that reaches 5 coarse cells away
    vb, fb = _octahedron((11.0, 1.0, 1.0), 0.75)
    vb = np.concatenate((vb, np.float32([[21.2, 0.5, 0.5], [21.4, 1.5, 0.5]])))
    fb = np.concatenate((fb, np.int32([[0, 6, 7]])))
    # four vertices on no face in the coarse cell [0, 2) x [20, 22) x [0, 2), two and two in fine cells
    vc = np.float32([[0.25, 20.25, 0.25], [0.5, 20.5, 0.5], [1.25, 21.25, 1.25], [1.5, 21.5, 1.5]])
    v = np.concatenate((va, vb, vc))
    f = np.concatenate((fa, fb + len(va))).astype(np.int32)
    out = MA.simplify(v, f, None, cell=1.0, origin=(0, 0, 0), levels=1, max_error=INF, details=True)
    info, detail = out[3], out[4]
    _check_choice(detail, 1)
    assert info["refused_crowded"] == (0, 1) and info["refused_error"] == (0, 0)
    assert info["refused_far"] == (0, 1), "the octahedron's cell"
    assert info["refused_empty"] == (0, 2), "the cell of the long triangle's other two corners has nothing but far corners"
    assert info["refused_singular"] == (0, 0)
    level = detail["level"]
    assert (level[:9000] == 0).all() and (level[9000:9008] == 0).all() and (level[-4:] == 0).all(), "they fall to the next level down"
    assert info["level_vertices"] == (len(v), 0)
    uniform = MQ.simplify(v, f, None, cell=1.0, origin=(0, 0, 0))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out[:2], uniform[:2])), "level 0 is uniform clustering"
    # without the long triangle the octahedron's cell is taken
    keep = np.ones(len(f), dtype=bool)
    keep[3000 + 8] = False
    info = MA.simplify(v, f[keep], None, cell=1.0, origin=(0, 0, 0), levels=1, max_error=INF)[3]
    assert info["refused_far"] == (0, 0) and info["level_vertices"][1] == 6 and info["refused_empty"] == (0, 2)


def test_a_singular_or_unsolved_status_is_refused():
    """no mesh makes the regularised matrix singular -- tr > 0 puts tr / 64 on the diagonal of a positive semi-definite matrix
    -- so the rule is checked on the statuses themselves"""
    data = dict(first=np.arange(7), count=np.array([1, 2, 2, 2, 2, 2, 2]), far=np.array([0, 0, 0, 0, 0, 1, 0], bool),
                status=np.array([0, MQ.SOLVED, MQ.SINGULAR, MQ.CROWDED, 0, MQ.SOLVED, MQ.SOLVED | MQ.CLAMPED]),
                error=np.array([0.0, 4.0, 0.0, 0.0, 0.0, 1.0, 9.0]))
    assert MA.acceptable(data, 9.0, 1).tolist() == [True, True, False, False, False, False, True]
    assert MA.acceptable(data, 3.9, 2).tolist() == [True, False, False, False, False, False, False]
    assert MA.acceptable(data, 0.0, 0).all(), "level 0 takes everything"


def test_a_renumbering_gives_the_same_vertex_rows(analytic):
    v, f, n = analytic
    first = MA.simplify(v, f, n, cell=2.0, origin=(0, 0, 0), levels=2, max_error=0.25)
    rng = np.random.default_rng(5)
    pv, pf = rng.permutation(len(v)), rng.permutation(len(f))
    inverse = np.empty_like(pv)
    inverse[pv] = np.arange(len(v))
    other = MA.simplify(v[pv], inverse[f[pf]].astype(np.int32), n[pv], cell=2.0, origin=(0, 0, 0), levels=2, max_error=0.25)
    assert other[3] == first[3]
    rows = lambda a: np.sort(np.ascontiguousarray(a).view([("x", "<u4"), ("y", "<u4"), ("z", "<u4")]).ravel())   # noqa: E731
    assert rows(other[0]).tobytes() == rows(first[0]).tobytes() and rows(other[2]).tobytes() == rows(first[2]).tobytes()


# ---- what the levels gain -------------------------------------------------------------------------------------------------

QUALITY_ERROR = 0.25           # voxels: mesh_nerf's default bound, chosen before anything was measured


def test_adaptive_levels_on_the_analytic_scene(analytic):
    """K = 2, L = 2, E = 0.25 voxels against uniform quadric clustering at K = 2 and at K * 2^L = 8, |sdf| of the output vertices
    in voxels (mean / worst), measured on the CPU:
        uniform K = 2      3142 faces   0.0121 / 0.300
        adaptive           2112 faces   0.0176 / 0.300      (levels 0 / 1 / 2: 848 / 182 / 18 clusters; largest error 0.232)
        uniform K = 8       192 faces   0.0761 / 0.881
    The relation asserted is the plain one, without a margin: the adaptive figures are no worse than uniform K = 8's.  None is
    needed: a cluster of a coarser level keeps every plane around it within E = 0.25, and the others are uniform K = 2's own
    clusters, whose worst vertex (0.300, on the crease between the box and the sphere) is the adaptive worst too; both lie a
    factor of three below what K = 8 gives."""
    v, f, n = analytic
    assert (len(v), len(f)) == (6894, 13784)
    fine = MQ.simplify(v, f, n, cell=2.0, origin=(0, 0, 0))
    coarse = MQ.simplify(v, f, n, cell=8.0, origin=(0, 0, 0))
    av, af, an, info, detail = MA.simplify(v, f, n, cell=2.0, origin=(0, 0, 0), levels=2, max_error=QUALITY_ERROR, details=True)
    e_fine, e_coarse, e = np.abs(_sdf(fine[0])), np.abs(_sdf(coarse[0])), np.abs(_sdf(av))
    print(f"uniform 2: {len(fine[1])} faces {e_fine.mean():.4f} / {e_fine.max():.3f}; adaptive: {len(af)} faces {e.mean():.4f} / "
          f"{e.max():.3f}; uniform 8: {len(coarse[1])} faces {e_coarse.mean():.4f} / {e_coarse.max():.3f}; {info}")
    assert len(af) < len(fine[1]), "strictly fewer faces than uniform K = 2"
    assert len(af) >= len(coarse[1]) and info["level_clusters"][1] > 0 and info["level_clusters"][2] > 0
    # every accepted cluster's error, recomputed corner by corner from the output position, is within the bound
    _check_choice(detail, 2)
    new = np.cumsum(np.isin(np.arange(len(v)), detail["reps"])) - 1
    worst = 0.0
    for level in (1, 2):
        data, cell_l = detail["data"][level], MA.level_cell(2.0, level)
        tol = (QUALITY_ERROR / float(cell_l)) * 256.0
        nrm, far = MA.corner_planes(f, data["C"], data["u"])
        at = detail["level"][f] == level                              # corners whose vertex chose this level
        big = data["count"][data["cluster"][f]] >= 2
        use = at & big & ~far & nrm.any(axis=2)
        assert not (at & big & far).any() and use.any()
        x = data["frac"][data["cluster"][f][use]] * 256.0
        d = np.sqrt(MA.corner_d2(nrm[use], data["u"][f][use], x))
        assert d.max() <= tol, (level, d.max(), tol)
        worst = max(worst, d.max() / 256.0 * float(cell_l))
        # and the emitted rows are those points
        heads = np.unique(detail["rep"][(detail["level"] == level) & np.isin(detail["rep"], detail["reps"])])
        k = data["cluster"][heads]
        lo = np.floor(v[heads] / cell_l) * cell_l
        want = np.where((data["count"][k] == 1)[:, None], v[heads], (lo.astype(np.float64) + np.float64(cell_l) * data["frac"][k]).astype(np.float32))
        assert av[new[heads]].tobytes() == want.tobytes()
    assert worst == info["largest_error"] <= QUALITY_ERROR
    # the reason for the feature
    assert e.mean() <= e_coarse.mean() and e.max() <= e_coarse.max()


# ---- mesh_nerf and the argument checks --------------------------------------------------------------------------------------

def test_parser_and_feature_checks(tmp_path):
    from nerfmeshes_amd import hip_ops, mesh_nerf
    p = mesh_nerf.build_parser()
    d = p.parse_args([])
    assert d.simplify_levels == 0 and d.simplify_error == mesh_nerf.SIMPLIFY_ERROR_DEFAULT == 0.25
    for dest in ("simplify_levels", "simplify_error"):
        assert "(addition)" in next(a.help for a in p._actions if a.dest == dest)
    for bad in (["--simplify-levels", "-1"], ["--simplify-levels", "1.5"], ["--simplify-error", "-0.1"], ["--simplify-error", "inf"],
                ["--simplify-error", "nan"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    # the pinned record stays; the new options are a record of their own
    assert set(mesh_nerf.FEATURES["simplify"].options) == {"simplify_cell", "simplify_placement"}
    record = mesh_nerf.FEATURES["simplify_levels"]
    assert record.what == "--simplify-levels / --simplify-error" and record.run is None
    assert {"simplify_levels", "simplify_error"} <= set(record.options)
    assert list(mesh_nerf.FEATURES).index("simplify_levels") == list(mesh_nerf.FEATURES).index("simplify") + 1, "the stage order stays"
    full = ["--simplify-cell", "2", "--simplify-placement", "quadric", "--simplify-levels", "2"]
    assert mesh_nerf.check_features(p.parse_args(full)) == {"simplify"}
    assert mesh_nerf.check_features(p.parse_args(full + ["--simplify-error", "0"])) == {"simplify"}
    assert mesh_nerf.check_features(p.parse_args(["--simplify-levels", str(hip_ops.SIMPLIFY_MAX_LEVELS)] + full[:4])) == {"simplify"}
    # levels = 0: the error is not read, whatever it is
    assert mesh_nerf.check_features(p.parse_args(["--simplify-error", "3"])) == set()
    assert mesh_nerf.check_features(argparse.Namespace(simplify_cell=2.0, simplify_error=float("nan"))) == {"simplify"}
    for options, text in ((["--simplify-levels", "2"], "--simplify-levels 2 needs --simplify-cell K > 0"),
                          (["--simplify-levels", "2", "--simplify-cell", "2"], "--simplify-levels 2 needs --simplify-placement quadric"),
                          (full[:4] + ["--simplify-levels", "9"], r"--simplify-levels must be in \[0, 8\], got 9")):
        with pytest.raises(ValueError, match=text):
            mesh_nerf.check_features(p.parse_args(options))
    with pytest.raises(ValueError, match="--simplify-error must be finite and >= 0"):
        mesh_nerf.check_features(argparse.Namespace(simplify_cell=2.0, simplify_placement="quadric", simplify_levels=1,
                                                    simplify_error=float("inf")))
    args = p.parse_args(["--simplify-levels", "2", "--save-dir", str(tmp_path)])
    with pytest.raises(ValueError, match="needs --simplify-cell"):
        mesh_nerf.export_marching_cubes(None, args, None, "cpu")
    args = p.parse_args(["--simplify-error", "0.5", "--route", "script", "--save-dir", str(tmp_path)])
    with pytest.raises(ValueError, match="--simplify-levels / --simplify-error have no --route script"):
        mesh_nerf.export_marching_cubes(None, args, None, "cpu")
    assert not any(tmp_path.iterdir()), "refused before anything is written"


def test_simplify_mesh_passes_the_options_on(monkeypatch, capsys):
    import torch
    from nerfmeshes_amd import hip_ops, mesh_nerf
    seen = {}

    def fake(vertices, triangles, normals, **kw):
        seen.update(kw)
        info = dict(zip(MQ.INFO_KEYS, range(1, 20)))
        if kw.get("levels"):
            info.update(levels=kw["levels"], largest_error=0.01, **{k: (5, 6, 7) for k in MA.LEVEL_KEYS + ("level_kept",)})
        return vertices, triangles, normals, info

    monkeypatch.setattr(hip_ops, "mesh_simplify", fake)
    v, t = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int64)
    p = mesh_nerf.build_parser()
    args = p.parse_args(["--res", "64", "--limit", "1.6", "--simplify-cell", "2", "--simplify-placement", "quadric"])
    mesh_nerf.simplify_mesh(v, t, None, 2.0, args)
    assert "levels" not in seen and "max_error" not in seen, "levels = 0 is the former call"
    plain = capsys.readouterr().out
    assert plain.count("\n") == 2 and "Simplify level" not in plain
    args = p.parse_args(["--res", "64", "--limit", "1.6", "--simplify-cell", "2", "--simplify-placement", "quadric",
                         "--simplify-levels", "2", "--simplify-error", "0.5"])
    mesh_nerf.simplify_mesh(v, t, None, 2.0, args)
    assert seen["levels"] == 2 and seen["max_error"] == 0.5 * (2.0 * 1.6 / 64) and seen["placement"] == "quadric"
    out = capsys.readouterr().out
    assert out.startswith(plain)
    assert out[len(plain):] == (
        "Simplify levels: 2 (cells of 2 to 8 voxels), error bound 0.5 voxels, largest accepted error 0.2000 voxels\n"
        "Simplify level 2: 7 vertices in 7 clusters, 7 kept; refused: 7 error, 7 crowded, 7 singular, 7 far, 7 no contributions\n"
        "Simplify level 1: 6 vertices in 6 clusters, 6 kept; refused: 6 error, 6 crowded, 6 singular, 6 far, 6 no contributions\n"
        "Simplify level 0: 5 vertices in 5 clusters, 5 kept\n")


def test_wrapper_checks_the_levels_before_the_device():
    import torch
    from nerfmeshes_amd import hip_ops
    v, f = torch.zeros(8, 3), torch.zeros(4, 3, dtype=torch.int32)
    for levels in (-1, 9, 1.0, "2", None, True):
        with pytest.raises(ValueError, match="levels must be an integer in"):
            hip_ops.mesh_simplify(v, f, cell=1.0, placement="quadric", levels=levels, max_error=0.1)
    for placement in ("mean",):
        with pytest.raises(ValueError, match="needs placement='quadric'"):
            hip_ops.mesh_simplify(v, f, cell=1.0, placement=placement, levels=1, max_error=0.1)
    with pytest.raises(ValueError, match="needs placement='quadric'"):
        hip_ops.mesh_simplify(v, f, cell=1.0, levels=1, max_error=0.1)
    with pytest.raises(ValueError, match="max_error is required"):
        hip_ops.mesh_simplify(v, f, cell=1.0, placement="quadric", levels=1)
    for error in (-1.0, float("nan"), -INF):
        with pytest.raises(ValueError, match="max_error must be >= 0"):
            hip_ops.mesh_simplify(v, f, cell=1.0, placement="quadric", levels=1, max_error=error)
    with pytest.raises(ValueError, match="coarsest cell size"):
        hip_ops.mesh_simplify(v, f, cell=3e38, placement="quadric", levels=1, max_error=0.1)
    # the restatement refuses the same
    for kw in (dict(levels=9, max_error=0.1), dict(levels=1), dict(levels=1, max_error=-1.0), dict(levels=1, max_error=0.1, placement="mean")):
        with pytest.raises(ValueError):
            MA.simplify(np.zeros((8, 3), np.float32), np.zeros((4, 3), np.int32), cell=1.0, **kw)
    assert hip_ops.SIMPLIFY_ADAPTIVE_KEYS == MA.ADAPTIVE_KEYS and hip_ops.SIMPLIFY_MAX_LEVELS == MA.MAX_LEVELS
    assert hip_ops.SIMPLIFY_LEVEL_FIELDS == MA.LEVEL_KEYS


def test_argument_errors_without_a_gpu():
    from nerfmeshes_amd import _lib
    lib = _lib.load()
    null, one = C.c_void_p(None), C.c_void_p(256)           # never dereferenced: validation fails first
    counts = (C.c_int64 * 79)(*([-7] * 79))
    tally = (C.c_int64 * 14)(*([-7] * 14))

    def err():
        return (lib.nm_last_error() or b"").decode()

    def level(v=one, nv=20, f=one, nf=10, n=null, o=(0.0, 0.0, 0.0), cell=1.0, l=1, levels=2, e=0.1, flags=0, ws=one, qws=one, aws=one):
        return lib.nm_mesh_simplify_adaptive_level(v, nv, f, nf, n, *o, cell, l, levels, e, flags, ws, qws, aws, null)

    def faces(f=one, nf=10, nv=20, levels=2, ws=one, aws=one, out=counts):
        return lib.nm_mesh_simplify_adaptive_faces(f, nf, nv, levels, ws, aws, out, null)

    def emit(ws=one, aws=one, f=one, nf=10, nv=20, levels=2, normals=0, kv=5, kf=5, ov=one, of=one, on=null, out=tally):
        return lib.nm_mesh_simplify_adaptive_emit(ws, aws, f, nf, nv, levels, normals, kv, kf, ov, of, on, out, null)

    for fn in (level, faces, emit):
        for kw in (dict(f=null), dict(ws=null), dict(aws=null)):
            assert fn(**kw) == 2 and "bad argument" in err(), (fn.__name__, kw)
        for kw in (dict(nf=-1), dict(nv=-1), dict(nv=1 << 31), dict(nf=(1 << 31) - 64)):
            assert fn(**kw) == 2 and "2^31" in err(), (fn.__name__, kw)
        assert fn(nf=3, nv=0) == 2 and "faces without vertices" in err()
        for levels in (0, -1, 9):
            assert fn(levels=levels) == 2 and "levels must be in [1, 8]" in err(), (fn.__name__, levels)
    assert level(v=null) == 2 and "bad argument" in err() and level(qws=null) == 2 and "bad argument" in err()
    for cell in (0.0, -1.0, INF, float("nan")):
        assert level(cell=cell) == 2 and "cell size" in err()
    assert level(cell=2e38, l=2) == 2 and "coarsest cell size" in err()
    for o in ((float("nan"), 0.0, 0.0), (0.0, INF, 0.0)):
        assert level(o=o) == 2 and "origin" in err()
    for l in (-1, 3):
        assert level(l=l) == 2 and "level must be in [0, levels]" in err()
    for e in (-1e-9, float("nan"), -INF):
        assert level(e=e) == 2 and "error bound" in err()
    assert level(flags=4) == 2 and "flags" in err()
    assert faces(out=None) == 2 and "bad argument" in err() and emit(out=None) == 2 and "bad argument" in err()
    assert emit(kv=21) == 2 and "kept counts" in err() and emit(kf=11) == 2 and "kept counts" in err()
    assert emit(ov=null) == 2 and "without its output" in err() and emit(normals=1) == 2 and "without its output" in err()
    assert emit(of=null) == 2 and "null face output" in err()
    assert list(counts) == [-7] * 79 and list(tally) == [-7] * 14, "nothing is returned by a rejected call"
    # the third workspace: a header and 30 bytes per vertex, each array padded to 256 bytes; it does not depend on the levels
    size = lib.nm_mesh_simplify_adaptive_workspace_bytes
    assert size(-1, 0) == 0 and size(0, -1) == 0 and size(1 << 31, 0) == 0 and size(0, (1 << 31) - 64) == 0
    header = size(0, 0)
    assert header == 768 and size(256, 7) == header + 256 * 30
    assert header + 30 * 750_000 <= size(750_000, 1_500_000) <= header + 30 * 750_000 + 5 * 256
    assert lib.nm_abi_version() == 6
