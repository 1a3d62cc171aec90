"""GPU: connected components of the mesh and the filter on them (nm_mesh_components / _select / _compact, mesh_nerf
--min-component-faces / --keep-largest).  Everything is integer work, so every comparison with the numpy restatement
(tests/mesh_components.py) is exact: labels and counts on the marching-cubes fixture, the filter on generated volumes,
adversarial connectivity built as index arrays, canonical labels under a permutation of the faces, and the exporter end to
end -- geometry, normals and colours of the kept vertices bit for bit the unfiltered run's rows, the cache, 2 ranks against 1."""
import os

import numpy as np
import pytest
import torch

from tests import mesh_components as MC
from tests.helpers import load_golden
from tests.gpu_support import assert_ranks_ok, export_mesh, launch_ranks, to_device as _dev, to_numpy as _np
from tests.gpu_support import ops, scene  # noqa: F401

pytestmark = pytest.mark.gpu


def _same_filter(got, want, tag):
    for name, a, b in zip(("verts", "faces", "normals", "values", "keys"), got[:5], want[:5]):
        if b is None:
            assert a is None, (tag, name)
            continue
        a = _np(a)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{tag}: {name} differ"
    assert got[5] == want[5], (tag, got[5], want[5])


def test_labels_and_counts_on_every_fixture_mesh(ops):
    g = load_golden("mc_cases")
    checked = 0
    for i in range(int(g["count"])):
        if f"err_{i}" in g.files:
            continue
        f, nv = g[f"faces_{i}"].astype(np.int32), len(g[f"verts_{i}"])
        labels, counts = ops.mesh_components(_dev(f), nv)
        want_l, want_c = MC.components(f, nv)
        assert labels.dtype == torch.int32 and counts.dtype == torch.int32
        assert np.array_equal(_np(labels), want_l), f"golden {i}: labels"
        assert np.array_equal(_np(counts), want_c), f"golden {i}: counts"
        checked += 1
    assert checked == 667


def _volume(kind, shape, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.standard_normal(shape).astype(np.float32), 0.1
    if kind == "ties":
        return rng.integers(-2, 3, shape).astype(np.float32), 0.0
    g = np.stack(np.meshgrid(*[np.linspace(-1, 1, s) for s in shape], indexing="ij"), -1)
    return (np.sin(3 * g[..., 0]) * np.cos(2 * g[..., 1]) + g[..., 2] ** 2 - 0.3).astype(np.float32), float(np.float32(0.05))


@pytest.mark.parametrize("shape", [(17, 5, 33), (33, 130, 77), (90, 96, 80)])
@pytest.mark.parametrize("kind", ["noise", "ties", "smooth"])
def test_filter_on_generated_volumes(ops, shape, kind):
    vol, iso = _volume(kind, shape, hash((shape, kind)) % (2 ** 32))
    v, f, n, val, keys = ops.marching_cubes(_dev(vol), iso, return_keys=True)
    hv, hf, hn, hval, hkeys = (_np(t) for t in (v, f, n, val, keys))
    labelled = MC.components(hf, len(hv))
    labels, counts = ops.mesh_components(f, v.shape[0])
    assert np.array_equal(_np(labels), labelled[0]) and np.array_equal(_np(counts), labelled[1])
    for min_faces in (1, 4, 50):
        for keep_largest in (0, 1, 3):
            got = ops.mesh_filter_components(v, f, n, val, keys, min_faces=min_faces, keep_largest=keep_largest)
            want = MC.filter_components(hv, hf, hn, hval, hkeys, min_faces=min_faces, keep_largest=keep_largest, labelled=labelled)
            _same_filter(got, want, f"{shape} {kind} min_faces={min_faces} keep_largest={keep_largest}")
    # the optional arrays are optional
    got = ops.mesh_filter_components(v, f, n, min_faces=4, keep_largest=1)
    _same_filter(got, MC.filter_components(hv, hf, hn, min_faces=4, keep_largest=1, labelled=labelled), "no values, no keys")


def _rows(nv, seed=0):
    """per-vertex arrays that name their own row: any misplaced row shows"""
    idx = np.arange(nv, dtype=np.float32)
    v = np.stack((idx, idx + 0.25, idx + 0.5), 1)
    return v, -v, idx * 2, np.arange(nv, dtype=np.int64) * 7 + seed


def _filter_both(ops, faces, nv, **kw):
    v, n, val, keys = _rows(nv)
    got = ops.mesh_filter_components(_dev(v), _dev(faces, np.int32), _dev(n), _dev(val), _dev(keys), **kw)
    return got, (v, n, val, keys)


def test_one_strip_of_a_million_triangles_numbered_at_random(ops):
    """deep trees (a vertex's neighbours are anywhere in the index range) and one hot counter"""
    nv = 1_000_003
    perm = np.random.default_rng(5).permutation(nv).astype(np.int32)
    strip = np.stack((np.arange(nv - 2), np.arange(1, nv - 1), np.arange(2, nv)), 1)
    faces = perm[strip]
    labels, counts = ops.mesh_components(_dev(faces), nv)
    assert int(labels.max()) == 0, "one component, named by vertex 0"
    assert int(counts[0]) == nv - 2 and int(counts.sum()) == nv - 2
    got, (v, n, val, keys) = _filter_both(ops, faces, nv, min_faces=nv - 2, keep_largest=1)
    assert np.array_equal(_np(got[1]), faces) and np.array_equal(_np(got[0]), v) and np.array_equal(_np(got[4]), keys)
    assert got[5] == dict(components=1, components_kept=1, faces=nv - 2, faces_kept=nv - 2, vertices=nv, vertices_kept=nv)
    empty, _ = _filter_both(ops, faces, nv, min_faces=nv - 1)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3) and empty[5]["components_kept"] == 0


def test_many_isolated_triangles(ops):
    t = 120_000
    nv = 3 * t
    faces = np.random.default_rng(6).permutation(nv).astype(np.int32).reshape(t, 3)
    labels, counts = ops.mesh_components(_dev(faces), nv)
    low = faces.min(1)
    want_l = np.empty(nv, np.int32)
    want_l[faces] = low[:, None]
    want_c = np.zeros(nv, np.int32)
    want_c[low] = 1
    assert np.array_equal(_np(labels), want_l) and np.array_equal(_np(counts), want_c)
    assert np.array_equal(want_l, MC.labels(faces, nv))
    # all tie at one triangle: the 5 smallest labels win, and stay in face order
    got, rows = _filter_both(ops, faces, nv, keep_largest=5)
    want = MC.filter_components(rows[0], faces, rows[1], rows[2], rows[3], keep_largest=5, labelled=(want_l, want_c))
    _same_filter(got, want, "isolated triangles, keep_largest=5")
    assert got[5]["components"] == t and got[5]["faces_kept"] == 5 and got[5]["vertices_kept"] == 15
    assert sorted(set(want_l[_np(got[4]) // 7].tolist())) == np.sort(low)[:5].tolist(), "the kept rows belong to those five"
    none, _ = _filter_both(ops, faces, nv, min_faces=2)
    assert none[1].shape == (0, 3) and none[0].shape == (0, 3) and none[3].shape == (0,) and none[5]["vertices_kept"] == 0


def _triangles_and_strips(nv):
    """isolated components, alternately one triangle (3 vertices) and a strip of two (4 vertices), ending at the last vertex;
    the nv % 7 vertices in front are in no face"""
    base = (nv % 7 + 7 * np.arange(nv // 7))[:, None, None]
    return (base + np.array([[0, 1, 2], [3, 4, 5], [4, 6, 5]])).astype(np.int32).reshape(-1, 3)


@pytest.mark.parametrize("nv", [64, 65_536, 65_537, 131_073])
def test_compaction_at_the_chunk_boundaries_of_the_scan(ops, nv):
    """1, 1024, 1025 and 2049 words of vertex keep bits: a single partial wave, one full chunk of the one-workgroup scan
    (csrc/compact.h), the first word of the second chunk (the carry is handed over) and of the third (it is carried twice).
    min_faces = 2 keeps the strips alone, so set and clear bits alternate in the vertex and in the face words, and the last
    vertex -- alone in the last word of the three larger meshes -- is kept: its new index needs that word's prefix."""
    faces = _triangles_and_strips(nv)
    assert (nv + 63) // 64 in (1, 1024, 1025, 2049) and faces.max() == nv - 1
    got, rows = _filter_both(ops, faces, nv, min_faces=2)
    want = MC.filter_components(rows[0], faces, rows[1], rows[2], rows[3], min_faces=2)
    _same_filter(got, want, f"{nv} vertices")
    assert want[5]["vertices_kept"] == 4 * (nv // 7) and want[5]["faces_kept"] == 2 * (nv // 7)
    assert want[4][-1] == (nv - 1) * 7, "the last row out is the last vertex"


def test_unreferenced_vertices_and_k_beyond_the_components(ops):
    faces = np.array([[7, 3, 5], [5, 3, 8], [8, 10, 12], [1, 2, 6]], np.int32)         # 0, 4, 9, 11 are in no triangle
    nv = 13
    labels, counts = ops.mesh_components(_dev(faces), nv)
    assert _np(labels).tolist() == [0, 1, 1, 3, 4, 3, 1, 3, 3, 9, 3, 11, 3]
    assert _np(counts).tolist() == [0, 1, 0, 3] + [0] * 9
    for kw in (dict(), dict(min_faces=1), dict(keep_largest=1), dict(keep_largest=2), dict(keep_largest=4), dict(keep_largest=1000),
               dict(min_faces=1, keep_largest=1000), dict(min_faces=2, keep_largest=3), dict(min_faces=4), dict(min_faces=2 ** 40)):
        got, rows = _filter_both(ops, faces, nv, **kw)
        _same_filter(got, MC.filter_components(rows[0], faces, rows[1], rows[2], rows[3], **kw), str(kw))
    got, _ = _filter_both(ops, faces, nv)
    assert got[5]["components"] == 6 and got[5]["vertices_kept"] == 13, "a vertex in no triangle is a component of size 0"
    got, _ = _filter_both(ops, faces, nv, min_faces=1)
    assert got[5]["components_kept"] == 2 and got[5]["vertices_kept"] == 9
    # no faces at all, and no vertices at all
    got, rows = _filter_both(ops, np.zeros((0, 3), np.int32), 5, keep_largest=2)
    _same_filter(got, MC.filter_components(rows[0], np.zeros((0, 3), np.int32), rows[1], rows[2], rows[3], keep_largest=2), "no faces")
    got, _ = _filter_both(ops, np.zeros((0, 3), np.int32), 0)
    assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and got[5]["components"] == 0


def test_face_index_out_of_range_is_an_error_not_an_access(ops):
    faces = np.array([[0, 1, 2], [2, 3, 13], [4, -1, 5]], np.int32)
    with pytest.raises(ValueError, match="2 faces have a vertex index outside"):
        ops.mesh_components(_dev(faces), 13)
    v, n, val, keys = _rows(13)
    with pytest.raises(ValueError, match="2 faces have a vertex index outside"):
        ops.mesh_filter_components(_dev(v), _dev(faces), _dev(n))


@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_labels_do_not_depend_on_face_order_and_runs_repeat(ops, kind):
    vol, iso = _volume(kind, (64, 70, 50), 3)
    v, f, n, val = ops.marching_cubes(_dev(vol), iso)
    labels, counts = ops.mesh_components(f, v.shape[0])
    perm = torch.from_numpy(np.random.default_rng(9).permutation(f.shape[0])).cuda()
    for faces in (f[perm].contiguous(), f.flip(0).contiguous(), f[:, [2, 0, 1]].contiguous()):
        l2, c2 = ops.mesh_components(faces, v.shape[0])
        assert torch.equal(l2, labels) and torch.equal(c2, counts)
    a = ops.mesh_filter_components(v, f, n, val, min_faces=4, keep_largest=3)
    b = ops.mesh_filter_components(v, f, n, val, min_faces=4, keep_largest=3)
    for x, y in zip(a[:4], b[:4]):
        assert _np(x).tobytes() == _np(y).tobytes()
    roots = int((labels == torch.arange(v.shape[0], device="cuda", dtype=torch.int32)).sum())
    assert a[5] == b[5] and a[5]["components"] == roots >= 1
    if kind == "noise":                                              # the smooth volume's surface is a single sheet
        assert roots > 3, "the noise volume is there to give the races many trees to merge"


def _run(model, tmp_path, tag, *extra):
    d = tmp_path / tag
    d.mkdir(exist_ok=True)
    return export_mesh(model, d, "--res", "64", *extra), d


FILTER = ["--min-component-faces", "100", "--keep-largest", "2"]


@pytest.mark.parametrize("extra", [[], ["--normals", "network"], ["--super-sampling", "2"]], ids=["plain", "network", "ss2"])
def test_end_to_end_through_the_exporter(ops, scene, tmp_path, capsys, extra):
    (v0, f0, n0, c0), _ = _run(scene, tmp_path, "all", *extra)
    capsys.readouterr()
    (v, f, n, c), d = _run(scene, tmp_path, "filtered", *extra, *FILTER)
    out = capsys.readouterr().out
    hv0, hf0, hn0 = _np(v0), _np(f0), _np(n0)
    lab, counts = MC.components(hf0, len(hv0))
    assert int((lab == np.arange(len(hv0))).sum()) >= 2, "the unfiltered mesh has at least two components"
    wv, wf, wn, _, _, info = MC.filter_components(hv0, hf0, hn0, min_faces=100, keep_largest=2, labelled=(lab, counts))
    assert info["components_kept"] < info["components"] and 0 < info["faces_kept"] < len(hf0), "the options drop at least one"
    assert _np(v).tobytes() == wv.tobytes() and _np(f).tobytes() == wf.tobytes() and v.shape == wv.shape and f.shape == wf.shape
    # the normals (grid or network) and the colours of the kept vertices are the unfiltered run's rows, bit for bit
    keep_v = MC.select(lab, counts, 100, 2)[lab]
    assert _np(n).tobytes() == wn.tobytes()
    assert c.shape == (int(keep_v.sum()), 3) and c.tobytes() == np.ascontiguousarray(c0[keep_v]).tobytes()
    assert (f"Component filter: kept {info['components_kept']} of {info['components']} components, {info['faces_kept']} of "
            f"{info['faces']} faces, {info['vertices_kept']} of {info['vertices']} vertices") in out
    lines = open(d / "mesh.obj").read().splitlines()
    assert sum(l.startswith("v ") for l in lines) == len(wv) and sum(l.startswith("f ") for l in lines) == len(wf)


def test_defaults_leave_the_mesh_alone_and_nothing_left_raises(ops, scene, tmp_path, capsys):
    (v0, f0, n0, c0), d0 = _run(scene, tmp_path, "a")
    (v1, f1, n1, c1), d1 = _run(scene, tmp_path, "b", "--min-component-faces", "0", "--keep-largest", "0")
    assert "Component filter" not in capsys.readouterr().out
    assert open(d0 / "mesh.obj", "rb").read() == open(d1 / "mesh.obj", "rb").read()
    with pytest.raises(ValueError, match="no mesh component has at least 10000000 faces"):
        _run(scene, tmp_path, "c", "--min-component-faces", "10000000", "--override-cache-mesh")
    assert not any((tmp_path / "c").iterdir()), "raised before anything was queried or written"


def test_cache_keeps_the_unfiltered_geometry(ops, scene, tmp_path):
    (v0, f0, n0, _), _ = _run(scene, tmp_path, "all")
    (v1, f1, n1, _), d = _run(scene, tmp_path, "cache", "--override-cache-mesh", *FILTER)
    assert v1.shape[0] < v0.shape[0]
    cv, cf, cn, _ = torch.load(d / "mesh_cache.pt", weights_only=False)
    assert torch.equal(cv, v0.cpu()) and torch.equal(cf, f0.cpu()) and torch.equal(cn, n0.cpu()), "the cache is the unfiltered mesh"
    first = open(d / "mesh.obj", "rb").read()
    os.remove(d / "mesh.obj")
    (v2, f2, n2, _), _ = _run(scene, tmp_path, "cache", "--use-cached-mesh", *FILTER)
    assert torch.equal(v2, v1) and torch.equal(f2, f1) and torch.equal(n2, n1)
    assert open(d / "mesh.obj", "rb").read() == first, "the cached mesh filtered again gives the same OBJ bytes"
    # and the cache can be tuned on: another limit, no geometry stage
    (v3, f3, _, _), _ = _run(scene, tmp_path, "cache", "--use-cached-mesh", "--keep-largest", "1")
    assert 0 < f3.shape[0] < f1.shape[0]


def test_two_ranks_sharing_one_gpu_equal_one_rank():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X")
    world = 2
    r = launch_ranks(os.path.join("tests", "tools", "cc_dist_worker.py"), world, timeout=900)
    assert_ranks_ok(r, f"CC_DIST_OK world={world}")
