"""CPU: mesh simplification's host side -- the vectorised numpy restatement (tests/mesh_simplify.py) against a plain
dict-and-loop implementation on every mesh of the marching-cubes fixture, what that fixture exercises, the single-member rule,
the distance of every output vertex from its cell's centre, mesh_nerf's option (default, negatives, the --route script
rejection) and the argument checks of the three C entries."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import mesh_simplify as MS
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


def _loop_simplify(verts, faces, normals, cell, origin=None):
    """The contract once more, one vertex and one face at a time with Python dicts (no numpy sorting, no vector operation)."""
    f32, f64 = np.float32, np.float64
    verts, faces = np.asarray(verts, f32), np.asarray(faces, np.int32)
    cell = f32(cell)
    origin = verts.min(axis=0) if origin is None else np.asarray(origin, f32)
    cluster_of, members = {}, {}
    for v, x in enumerate(verts):
        c = tuple(int(math.floor(f32(f32(x[k] - origin[k]) / cell))) for k in range(3))
        assert all(0 <= ck < 1 << 21 for ck in c)
        cluster_of[v] = c
        members.setdefault(c, []).append(v)
    rep = {c: min(m) for c, m in members.items()}
    seen, kept, degenerate, duplicate = {}, [], 0, 0
    for f, tri in enumerate(faces.tolist()):
        r = [rep[cluster_of[v]] for v in tri]
        if len(set(r)) < 3:
            degenerate += 1
            continue
        k = r.index(min(r))
        key = (r[k], r[(k + 1) % 3], r[(k + 2) % 3])
        if key in seen:
            duplicate += 1
            continue
        seen[key] = f
        kept.append(r)
    used = sorted({r for tri in kept for r in tri})
    new = {r: i for i, r in enumerate(used)}
    out_v, out_n = [], []
    for r in used:
        c, m = cluster_of[r], members[cluster_of[r]]
        if len(m) == 1:
            out_v.append(verts[r])
            out_n.append(normals[r])
            continue
        lo = [f32(origin[k] + f32(f32(c[k]) * cell)) for k in range(3)]
        S, N = [0, 0, 0], [0, 0, 0]
        for v in m:
            for k in range(3):
                t = f32(f32(verts[v, k] - lo[k]) / cell)
                S[k] += int(np.rint(min(max(f64(t) * 2.0 ** 30, -2.0 ** 31), 2.0 ** 31)))
            if all(np.isfinite(normals[v, k]) and abs(normals[v, k]) <= 2 for k in range(3)):
                for k in range(3):
                    N[k] += int(np.rint(f64(normals[v, k]) * 2.0 ** 30))
        out_v.append([f32(f64(lo[k]) + f64(cell) * (f64(S[k]) / (f64(len(m)) * 2.0 ** 30))) for k in range(3)])
        if N == [0, 0, 0]:
            out_n.append(normals[r])
        else:
            s = np.array(N, np.int64).astype(f32)
            out_n.append(s / np.sqrt(f32(f32(s[0] * s[0]) + f32(s[1] * s[1])) + f32(s[2] * s[2])))
    info = dict(vertices=len(verts), faces=len(faces), clusters=len(members), vertices_kept=len(used), faces_kept=len(kept),
                degenerate_faces=degenerate, duplicate_faces=duplicate)
    return (np.array(out_v, f32).reshape(-1, 3), np.array([[new[r] for r in tri] for tri in kept], np.int32).reshape(-1, 3),
            np.array(out_n, f32).reshape(-1, 3), info)


def _same(got, want, tag):
    for name, a, b in zip(("verts", "faces", "normals"), got[:3], want[:3]):
        if b is None:
            assert a is None, (tag, name)
            continue
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{tag}: {name} differ"
    assert got[3] == want[3], (tag, got[3], want[3])


def test_restatement_matches_the_loop_on_every_fixture_mesh_and_what_the_fixture_covers(meshes):
    assert len(meshes) == 667 and sum(len(v) for _, v, _, _ in meshes) == 12610 and sum(len(f) for _, _, f, _ in meshes) == 14881
    degenerate = duplicate = dup_meshes = unreferenced = unref_meshes = 0
    for i, v, f, n in meshes:
        _same(MS.simplify(v, f, n, cell=2.0), _loop_simplify(v, f, n, 2.0), f"mesh {i}, origin = the vertices' minimum")
        got = MS.simplify(v, f, n, cell=2.0, origin=(0, 0, 0))       # the grid anchored at the volume's corner, as mesh_nerf's is
        _same(got, _loop_simplify(v, f, n, 2.0, origin=(0, 0, 0)), f"mesh {i}")
        info = got[3]
        assert info["faces_kept"] + info["degenerate_faces"] + info["duplicate_faces"] == len(f)
        degenerate += info["degenerate_faces"]
        duplicate += info["duplicate_faces"]
        dup_meshes += info["duplicate_faces"] > 0
        unreferenced += info["clusters"] - info["vertices_kept"]
        unref_meshes += info["clusters"] > info["vertices_kept"]
    # every branch is taken: degenerate faces, duplicates, clusters that no kept face references
    assert (degenerate, duplicate, dup_meshes, unreferenced, unref_meshes) == (12734, 5, 4, 837, 618)


def test_without_normals_the_geometry_is_the_same(meshes):
    for i, v, f, n in meshes[::7]:
        a, b = MS.simplify(v, f, n, cell=2.0), MS.simplify(v, f, None, cell=2.0)
        assert b[2] is None and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[3] == b[3], i


def test_a_cell_below_the_vertex_spacing_returns_the_input_rows(meshes):
    """The single-member rule at a cell of 2^-10: a mesh whose vertices all lie in cells of their own comes back row for row,
    bit for bit, faces unchanged.  33 of the 667 fixture meshes hold vertices closer than that (the tie volumes emit coincident
    ones): those must merge, and there the plain loop -- which copies a single member's rows -- is the reference."""
    cell, apart = np.float32(2.0 ** -10), 0
    for i, v, f, n in meshes:
        origin = v.min(axis=0)
        own = len({tuple(np.floor((x - origin) / cell).tolist()) for x in v}) == len(v)
        ov, of, on, info = MS.simplify(v, f, n, cell=cell)
        if not own:
            assert info["clusters"] < len(v), i
            _same((ov, of, on, info), _loop_simplify(v, f, n, cell), f"mesh {i}")
            continue
        apart += 1
        assert info["clusters"] == len(v) == info["vertices_kept"] and info["faces_kept"] == len(f), i
        assert ov.tobytes() == v.tobytes() and on.tobytes() == n.tobytes() and of.tobytes() == f.tobytes(), i
    assert apart == 634


@pytest.mark.parametrize("cell", [1.0, 2.0, 3.7])
def test_every_output_vertex_lies_in_its_cell(meshes, cell):
    bound = np.float64(cell) / 2 * (1 + 2.0 ** -20)
    for i, v, f, n in meshes:
        origin = v.min(axis=0)
        ov, _, _, _ = MS.simplify(v, f, n, cell=cell, origin=origin)
        c, bad = MS.cells(ov, origin, cell)
        assert not bad.any()
        centre = origin.astype(np.float64) + (c.astype(np.float64) + 0.5) * np.float64(np.float32(cell))
        assert (np.abs(ov.astype(np.float64) - centre) <= bound).all(), i


def test_hand_made_sheets_and_windings():
    # two unit squares one above the other, closer than a cell: the two sides of a thin sheet collapse onto the same clusters
    quad = np.array([[0, 0, 0], [4, 0, 0], [4, 4, 0], [0, 4, 0]], np.float32) + 0.5
    v = np.concatenate((quad, quad + np.float32([0, 0, 0.25])))
    up = [[0, 1, 2], [0, 2, 3]]
    f = np.array(up + [[4 + a, 4 + c, 4 + b] for a, b, c in up] + [[5, 6, 4]], np.int32)
    ov, of, _, info = MS.simplify(v, f, None, cell=1.0, origin=(0, 0, 0))
    assert info["clusters"] == 4 and info["vertices_kept"] == 4
    # the upper sheet's faces wind the other way: kept; [5, 6, 4] is face 0 rotated: a duplicate
    assert of.tolist() == [[0, 1, 2], [0, 2, 3], [0, 2, 1], [0, 3, 2]] and info["duplicate_faces"] == 1 and info["degenerate_faces"] == 0
    assert np.array_equal(ov, quad + np.float32([0, 0, 0.125]))
    # everything in one cell
    ov, of, _, info = MS.simplify(v, f, None, cell=64.0, origin=(0, 0, 0))
    assert ov.shape == (0, 3) and of.shape == (0, 3) and info["clusters"] == 1 and info["degenerate_faces"] == len(f)


def test_bad_inputs_raise():
    v = np.zeros((4, 3), np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    bad = v.copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError, match="1 vertices have a non-finite coordinate"):
        MS.simplify(bad, f, None, cell=1.0)
    far = v.copy()
    far[3, 0] = 2.0 ** 21
    with pytest.raises(ValueError, match=r"1 vertices .* outside \[0, 2097152\)"):
        MS.simplify(far, f, None, cell=1.0, origin=(0, 0, 0))
    with pytest.raises(ValueError, match="1 faces have a vertex index outside"):
        MS.simplify(v, np.array([[0, 1, 4]], np.int32), None, cell=1.0)
    for cell in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="cell size"):
            MS.simplify(v, f, None, cell=cell)


def test_parser_defaults_and_negatives():
    from nerfmeshes_amd import mesh_nerf
    p = mesh_nerf.build_parser()
    assert p.parse_args([]).simplify_cell == 0.0
    assert p.parse_args(["--simplify-cell", "2.5"]).simplify_cell == 2.5
    assert "(addition)" in next(a.help for a in p._actions if a.dest == "simplify_cell")
    for bad in ("-1", "-0.5", "nan", "inf", "-inf", "two"):
        with pytest.raises(SystemExit):
            p.parse_args(["--simplify-cell", bad])


def test_route_script_rejects_the_option(tmp_path):
    from nerfmeshes_amd import mesh_nerf
    args = mesh_nerf.build_parser().parse_args(["--simplify-cell", "2", "--route", "script", "--save-dir", str(tmp_path)])
    with pytest.raises(ValueError, match="route script"):
        mesh_nerf.export_marching_cubes(None, args, None, "cpu")
    assert not any(tmp_path.iterdir()), "rejected before anything is written"


def test_argument_errors_without_a_gpu():
    from nerfmeshes_amd import _lib
    lib = _lib.load()
    null, one = C.c_void_p(None), C.c_void_p(256)           # never dereferenced: validation fails first
    counts = (C.c_int64 * 7)(*([-7] * 7))

    def err():
        return (lib.nm_last_error() or b"").decode()

    def cluster(v=one, nv=20, f=one, nf=10, n=null, o=(0.0, 0.0, 0.0), cell=1.0, flags=0, ws=one, out=counts):
        return lib.nm_mesh_simplify_cluster(v, nv, f, nf, n, *o, cell, flags, ws, out, null)

    def emit(ws=one, v=one, nv=20, f=one, nf=10, n=null, o=(0.0, 0.0, 0.0), cell=1.0, kv=5, kf=5, ov=one, of=one, on=null):
        return lib.nm_mesh_simplify_emit(ws, v, nv, f, nf, n, *o, cell, kv, kf, ov, of, on, null)

    for fn in (cluster, emit):
        for kw in (dict(v=null), dict(f=null), dict(ws=null)):
            assert fn(**kw) == 2 and "bad argument" in err(), (fn.__name__, kw)
        for kw in (dict(nf=-1), dict(nv=-1), dict(nv=1 << 31), dict(nf=(1 << 31) - 64)):
            assert fn(**kw) == 2 and "2^31" in err(), (fn.__name__, kw)
        assert fn(nf=3, nv=0) == 2 and "faces without vertices" in err()
        for cell in (0.0, -1.0, float("inf"), float("nan")):
            assert fn(cell=cell) == 2 and "cell size" in err(), (fn.__name__, cell)
        for o in ((float("nan"), 0.0, 0.0), (0.0, float("inf"), 0.0), (0.0, 0.0, float("-inf"))):
            assert fn(o=o) == 2 and "origin" in err(), (fn.__name__, o)
    assert cluster(out=None) == 2 and "bad argument" in err()
    assert cluster(flags=2) == 2 and "flags" in err()
    assert list(counts) == [-7] * 7, "nothing is returned by a rejected call"
    assert emit(kv=21) == 2 and "kept counts" in err()
    assert emit(kf=11) == 2 and "kept counts" in err()
    assert emit(kv=-1) == 2 and emit(kf=-1) == 2
    assert emit(ov=null) == 2 and "without its output" in err()
    assert emit(n=one) == 2 and "without its output" in err()
    assert emit(of=null) == 2 and "null face output" in err()
    # the workspace: 64 bytes per slot of a table of >= 2 V slots, 4 per slot of one of >= 2 F
    size = lib.nm_mesh_simplify_workspace_bytes
    assert size(-1, 0) == 0 and size(0, -1) == 0 and size(1 << 31, 0) == 0 and size(0, (1 << 31) - 64) == 0
    assert size(0, 0) > 0
    assert 64 * (1 << 21) + 4 * (1 << 22) <= size(750_000, 1_500_000) <= 64 * (1 << 21) + 4 * (1 << 22) + 16 * 2_250_000
    assert lib.nm_abi_version() == 6


def test_wrapper_checks_its_arguments_before_the_device():
    import torch
    from nerfmeshes_amd import _lib, hip_ops
    v, f = torch.zeros(8, 3), torch.zeros(4, 3, dtype=torch.int32)
    with pytest.raises(_lib.HipLibraryError, match="GPU memory"):
        hip_ops.mesh_simplify(v, f, cell=1.0)
    for cell in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cell size"):
            hip_ops.mesh_simplify(v, f, cell=cell)
    with pytest.raises(ValueError, match="cell size is required"):
        hip_ops.mesh_simplify(v, f)
