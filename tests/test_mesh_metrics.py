"""CPU: the host side of the chamfer measure -- the numpy restatement (tests/mesh_metrics.py) against independent references
(scipy's cKDTree in fp64, hand-made triangles), the OBJ reader, the parsers of mesh_chamfer and of mesh_nerf's three new
options, and the argument checks of the new C entries."""
import ctypes as C

import numpy as np
import pytest

from tests import mesh_metrics as MM
from tests.helpers import load_golden


def _ulps(a, b):
    ia, ib = (np.asarray(v, np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    return np.abs(ia - ib)


@pytest.mark.parametrize("n,m,kind", [(1000, 700, "gauss"), (513, 2049, "gauss"), (300, 300, "cube")])
def test_nearest_restatement_against_ckdtree(n, m, kind):
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(n + m)
    draw = rng.standard_normal if kind == "gauss" else (lambda s: rng.random(s) * 4 - 2)
    x, y = draw((n, 3)).astype(np.float32), draw((m, 3)).astype(np.float32)
    d2, idx = MM.nearest(x, y, rows=100)
    dist, want = cKDTree(y.astype(np.float64)).query(x.astype(np.float64), k=2)
    unique = dist[:, 1] - dist[:, 0] > 1e-6 * dist[:, 0]
    assert unique.sum() > 0.99 * n
    assert np.array_equal(idx[unique], want[unique, 0])
    assert _ulps(d2, (dist[:, 0] ** 2).astype(np.float32)).max() <= 4
    # the distance is the one of the index returned
    own = ((x.astype(np.float64) - y[idx].astype(np.float64)) ** 2).sum(1)
    assert _ulps(d2, own.astype(np.float32)).max() <= 4


def test_nearest_restatement_ties_nan_and_empty():
    y = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 1, 0]], np.float32)
    x = np.array([[1, 0, 0], [0.5, 0, 0], [np.nan, 1, 1], [0, 0.5, 0]], np.float32)
    d2, idx = MM.nearest(x, y)
    assert idx.tolist() == [1, 0, -1, 0] and d2[2] == np.inf and d2.tolist()[:2] == [0.0, 0.25]
    d2, idx = MM.nearest(x, np.zeros((0, 3), np.float32))
    assert (idx == -1).all() and np.isinf(d2).all()
    d2, idx = MM.nearest(np.zeros((0, 3), np.float32), y)
    assert d2.shape == (0,) and idx.shape == (0,)
    big = np.array([[3e38, 3e38, 0]], np.float32)                    # every d2 overflows: +inf still wins over nothing
    d2, idx = MM.nearest(big, -big.repeat(2, 0))
    assert d2[0] == np.inf and idx[0] == 0
    d2, idx = MM.nearest(big, np.concatenate((np.full((1, 3), np.nan, np.float32), -big)))
    assert d2[0] == np.inf and idx[0] == 1


def test_face_weights_on_hand_made_triangles():
    verts = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3], [0, 0, 1e-3]], np.float32)
    faces = np.array([[0, 1, 2], [3, 4, 5], [0, 1, 6], [0, 0, 1]], np.int32)
    areas, cdf, bad = MM.face_weights(verts, faces)
    assert bad == 0 and areas.dtype == np.float32 and cdf.dtype == np.uint64
    assert areas[0] == 6.0 and areas[1] == 0.0 and areas[3] == 0.0 and abs(areas[2] - 1.5e-3) < 1e-9
    w = np.diff(np.concatenate(([0], cdf.astype(np.int64))))
    assert w[1] == 0 and w[3] == 0 and 2 ** 31 <= w.max() < 2 ** 32
    assert w[0] == 6 * 2 ** 29                                       # 6 = 0.75 * 2^3: scaled by 2^(32-3)
    assert w[2] == int(np.trunc(float(areas[2]) * 2.0 ** 29))
    # a face below m * 2^-32 gets weight 0; an index out of range is counted and weighs nothing
    tiny = np.array([[0, 0, 0], [1e-6, 0, 0], [0, 1e-6, 0]], np.float32)
    a2, c2, bad2 = MM.face_weights(np.concatenate((verts, tiny)), np.array([[0, 1, 2], [7, 8, 9], [0, 1, 10], [-1, 0, 1]]))
    assert bad2 == 2 and a2[1] > 0 and c2.tolist() == [6 * 2 ** 29] * 4
    a3, c3, _ = MM.face_weights(verts, faces[[1, 3]])
    assert c3.tolist() == [0, 0]
    assert MM.face_weights(verts, np.zeros((0, 3), np.int32))[1].shape == (0,)


def test_sampling_restatement_follows_the_cdf():
    verts, faces = MM.uv_sphere()
    assert faces.shape == (4096, 3)
    areas, cdf, bad = MM.face_weights(verts, faces)
    assert bad == 0 and int((areas == 0).sum()) == 128
    assert abs(float(areas.astype(np.float64).sum()) - 4 * np.pi) < 0.02 * 4 * np.pi
    rng = np.random.default_rng(3)
    u = rng.random((20000, 3), dtype=np.float32)
    total = int(cdf[-1])
    first = np.flatnonzero(np.diff(np.concatenate(([0], cdf.astype(np.int64)))) > 0)
    edge = np.float32(int(cdf[first[5]]) / total)                    # a draw that lands on (or next to) a boundary
    u[:4, 0] = [0.0, np.nextafter(np.float32(1), np.float32(0)), edge, np.nextafter(edge, np.float32(0))]
    pts, fid, nrm = MM.sample_points(u, verts, faces, cdf)
    assert (areas[fid] > 0).all(), "a zero-weight face is never chosen"
    assert fid[0] == first[0] and fid[1] == first[-1]
    t = np.trunc(u[:, 0].astype(np.float64) * float(total)).astype(np.int64)
    lower = np.concatenate(([0], cdf.astype(np.int64)))[fid]
    assert ((lower <= t) & (t < cdf.astype(np.int64)[fid])).all()
    assert np.abs(np.linalg.norm(pts.astype(np.float64), axis=1) - 1).max() < 0.005      # chords of a 64 x 32 sphere
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1).max() < 1e-6
    # area-proportional: the share of the northern hemisphere
    assert abs((pts[:, 2] > 0).mean() - 0.5) < 0.02


OBJ_TEXT = """# a comment
mtllib none.mtl
v 0 0 0
v 1 0 0 0.5 0.25 1
v 1 1 0
v 0 1 0
vn 0 0 1
vt 0.5 0.5
o thing
f 1 2 3
f 1/1 3/1 4/1
f 1//1 2//1 4//1
f 1/1/1 2/1/1 3/1/1
f -4 -3 -2
v 0.5 0.5 1
f 1 2 3 4
f -1 1 2 3 4
f 5/1/1 -5//1 2/1
s off
l 1 2
"""


def test_load_obj_reads_every_face_form(tmp_path):
    import torch
    from nerfmeshes_amd.nerf.nerf_helpers import load_obj
    path = tmp_path / "forms.obj"
    path.write_text(OBJ_TEXT)
    v, f = load_obj(str(path))
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and not v.is_cuda
    assert v.tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1]]
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 1, 2],
                          [0, 1, 2], [0, 2, 3],                      # the quad
                          [4, 0, 1], [4, 1, 2], [4, 2, 3],           # the pentagon
                          [4, 0, 1]]
    empty = tmp_path / "empty.obj"
    empty.write_text("# nothing\n")
    v, f = load_obj(str(empty))
    assert v.shape == (0, 3) and f.shape == (0, 3)


@pytest.mark.parametrize("face,line", [("f 1 2 5", 4), ("f 1 2 0", 4), ("f -4 1 2", 4), ("f 1 2", 4), ("f 1 x 2", 4)])
def test_load_obj_rejects_a_bad_face_with_its_line_number(tmp_path, face, line):
    from nerfmeshes_amd.nerf.nerf_helpers import load_obj
    path = tmp_path / "bad.obj"
    path.write_text(f"v 0 0 0\nv 1 0 0\nv 0 1 0\n{face}\n")
    with pytest.raises(ValueError, match=f":{line}:"):
        load_obj(str(path))


def test_load_obj_round_trip_of_the_exporter_fixture():
    import os
    from nerfmeshes_amd.nerf.nerf_helpers import load_obj
    g = load_golden("export_obj")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "export_obj.obj")
    v, f = load_obj(path)
    assert v.numpy().tobytes() == g["vertices"].tobytes(), "repr of an fp32 reads back to the same fp32"
    assert np.array_equal(f.numpy(), g["triangles"])


def test_mesh_chamfer_parser_defaults():
    from nerfmeshes_amd import mesh_chamfer
    p = mesh_chamfer.build_parser()
    a = p.parse_args(["--mesh", "a.obj", "--target", "b.obj"])
    assert (a.mesh, a.target, a.samples, a.seed, a.normalize, a.out) == ("a.obj", "b.obj", 100000, 0, False, None)
    a = p.parse_args(["--mesh", "a.obj", "--target", "b.obj", "--samples", "5", "--seed", "7", "--normalize", "--out", "r.json"])
    assert (a.samples, a.seed, a.normalize, a.out) == (5, 7, True, "r.json")
    for bad in ([], ["--mesh", "a.obj"], ["--mesh", "a.obj", "--target", "b.obj", "--samples", "x"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_mesh_nerf_chamfer_options_and_the_route_script_rejection(tmp_path):
    from nerfmeshes_amd import mesh_nerf
    p = mesh_nerf.build_parser()
    a = p.parse_args([])
    assert (a.target_mesh, a.chamfer_samples, a.chamfer_seed) == (None, 100000, 0)
    a = p.parse_args(["--target-mesh", "t.obj", "--chamfer-samples", "20000", "--chamfer-seed", "3"])
    assert (a.target_mesh, a.chamfer_samples, a.chamfer_seed) == ("t.obj", 20000, 3)
    args = p.parse_args(["--target-mesh", "t.obj", "--route", "script", "--save-dir", str(tmp_path)])
    with pytest.raises(ValueError, match="route script"):
        mesh_nerf.export_marching_cubes(None, args, None, "cpu")
    args = p.parse_args(["--target-mesh", "t.obj", "--chamfer-samples", "0", "--save-dir", str(tmp_path)])
    with pytest.raises(ValueError, match="chamfer-samples"):
        mesh_nerf.export_marching_cubes(None, args, None, "cpu")
    assert not any(tmp_path.iterdir()), "rejected before anything is written"


def test_normalize_vertices_is_create_meshs_rule():
    import torch
    from nerfmeshes_amd import mesh_nerf
    v = torch.tensor([[0.0, 0, 0], [4, 0, 0], [0, 2, 0], [0, 0, -6]])
    got = mesh_nerf.normalize_vertices(v)
    centred = v - v.mean(0)
    assert torch.equal(got, centred / max(centred.abs().max(0)[0]))
    assert float(got.abs().max()) == 1.0 and torch.allclose(got.mean(0), torch.zeros(3), atol=1e-7)


def test_datasets_have_no_target_mesh_until_asked(tmp_path):
    from nerfmeshes_amd.data.datasets import CachingDataset, SynthesizableDataset
    from nerfmeshes_amd.nerf import CfgNode
    assert SynthesizableDataset.target_mesh is None and CachingDataset.target_mesh is None
    ds = SynthesizableDataset()
    ds.cfg = CfgNode({"dataset": {"basedir": str(tmp_path)}})
    assert ds.load_target_mesh() is None and ds.target_mesh is None
    (tmp_path / "model.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    v, f = ds.load_target_mesh()
    assert v.shape == (3, 3) and f.tolist() == [[0, 1, 2]] and ds.target_mesh is not None


def test_validation_needs_a_target_mesh_when_the_chamfer_loss_is_on():
    import torch
    from nerfmeshes_amd import models, synthetic as S
    hp = S.hparams(chunksize=3000)
    hp["experiment.chamfer_loss"] = True
    model = models.NeRFModel(hp)

    class NoMesh:
        target_mesh = None

    model.val_dataset = NoMesh()
    outputs = [{"log": {"validation/loss": torch.tensor(1.0)}, "val_loss": torch.tensor(1.0)}]
    with pytest.raises(AssertionError, match="a target mesh .obj must be provided in the dataset folder"):
        model.validation_epoch_end(outputs)
    hp["experiment.chamfer_loss"] = False
    off = models.NeRFModel(hp)
    off.val_dataset = NoMesh()
    got = off.validation_epoch_end(outputs + [{"log": {"validation/loss": torch.tensor(3.0)}, "val_loss": torch.tensor(2.0)}])
    assert set(got) == {"log", "val_loss"} and set(got["log"]) == {"validation/loss"}
    assert float(got["log"]["validation/loss"]) == 2.0 and float(got["val_loss"]) == 1.5


def test_argument_errors_of_the_new_entries_without_a_gpu():
    from nerfmeshes_amd import _lib
    lib = _lib.load()
    null, one = C.c_void_p(None), C.c_void_p(256)           # never dereferenced: validation fails first

    def err():
        return (lib.nm_last_error() or b"").decode()

    def weights(v=one, nv=20, f=one, nf=10, areas=null, cdf=one, ws=one):
        return lib.nm_mesh_face_weights(v, nv, f, nf, areas, cdf, ws, null)

    def sample(u=one, n=5, v=one, nv=20, f=one, nf=10, cdf=one, pts=one, ids=null, nrm=null):
        return lib.nm_mesh_sample_points(u, n, v, nv, f, nf, cdf, pts, ids, nrm, null)

    def nearest(x=one, n=5, y=one, m=7, d2=one, idx=one, ws=one):
        return lib.nm_points_nearest(x, n, y, m, d2, idx, ws, null)

    for kw in (dict(v=null), dict(f=null), dict(cdf=null), dict(ws=null)):
        assert weights(**kw) == 2 and "bad argument" in err(), kw
    for kw in (dict(u=null), dict(v=null), dict(f=null), dict(cdf=null)):
        assert sample(**kw) == 2 and "bad argument" in err(), kw
    for kw in (dict(x=null), dict(y=null), dict(d2=null), dict(idx=null), dict(ws=null)):
        assert nearest(**kw) == 2 and "bad argument" in err(), kw
    for kw in (dict(nv=-1), dict(nf=-1), dict(nv=1 << 31), dict(nf=(1 << 31) - 64)):
        assert weights(**kw) == 2 and "2^31" in err(), kw
        assert sample(**kw) == 2 and "2^31" in err(), kw
    assert sample(n=-1) == 2 and "2^31" in err()
    assert sample(n=1 << 31) == 2 and "2^31" in err()
    for kw in (dict(n=-1), dict(m=-1), dict(n=1 << 31), dict(m=(1 << 31) - 64)):
        assert nearest(**kw) == 2 and "2^31" in err(), kw
    assert weights(nf=3, nv=0) == 2 and "faces without vertices" in err()
    assert sample(nf=0) == 2 and "without faces" in err()
    assert sample(nv=0, nf=0) == 2 and "without faces" in err()
    # the workspaces: a header, and O(N) for the search whatever M is
    assert lib.nm_mesh_face_weights_workspace_bytes() >= 32
    assert lib.nm_points_nearest_workspace_bytes(-1, 0) == 0 and lib.nm_points_nearest_workspace_bytes(0, 1 << 31) == 0
    small, large = lib.nm_points_nearest_workspace_bytes(1000, 10), lib.nm_points_nearest_workspace_bytes(1000, 10 ** 9)
    assert small == large and 8 * 1000 <= small <= 8 * 1000 + 512
    assert lib.nm_points_nearest_workspace_bytes(0, 0) >= 0
    assert lib.nm_abi_version() == 6


def test_wrappers_check_their_arguments_before_the_device():
    import torch
    from nerfmeshes_amd import _lib, hip_ops
    with pytest.raises(_lib.HipLibraryError, match="GPU memory"):
        hip_ops.points_nearest(torch.zeros(4, 3), torch.zeros(4, 3))
    for name in ("mesh_face_weights", "mesh_sample_points", "points_nearest", "chamfer_distance"):
        assert callable(getattr(hip_ops, name))
