"""CPU: the exact point-to-mesh distance (nm_points_to_mesh, hip_ops.mesh_surface_distance, mesh_chamfer --surface exact /
--fscore, mesh_nerf --target-surface / --target-fscore) without a GPU: the numpy restatement of the arithmetic contract
(tests/mesh_surface_distance.py) against an independent fp64 Ericson routine, its degenerate / tie / NaN rules, the metric
reductions on hand-made arrays, the option plumbing, and the C ABI's argument checks."""
import argparse
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import mesh_metrics as MM
from tests import mesh_surface_distance as SD
from tests.mesh_surface_distance import ERICSON_BOUND, ON_SURFACE_BOUND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _queries(scale, n=2000, seed=0):
    return (np.random.default_rng(seed).uniform(-1.5, 1.5, (n, 3)) * scale).astype(F32)


@pytest.mark.parametrize("name", ["sphere", "soup", "soup 1e-3", "soup 1e3"])
def test_the_restatement_against_the_fp64_ericson_routine(name):
    scale = {"soup 1e-3": 1e-3, "soup 1e3": 1e3}.get(name, 1.0)
    verts, faces = MM.uv_sphere(32, 16) if name == "sphere" else SD.soup(500, 3, scale)
    x = _queries(scale)
    d2, face, _ = SD.points_to_mesh(x, verts, faces)
    assert not np.isnan(d2).any() and (face >= 0).all()
    want = SD.ericson(x, verts, faces)
    err = np.abs(np.sqrt(d2.astype(np.float64)) - want).max() / np.abs(verts).max()
    print(f"{name}: max |sqrt(d2_fp32) - d_fp64| / max|coordinate| = {err}")
    assert err <= ERICSON_BOUND
    # the same contract in fp64 is Ericson's answer up to fp64 rounding: the form, not only its fp32 evaluation, is right
    d64 = SD.pair_dist2(x[:300], verts, faces, np.float64)
    assert not np.isnan(d64).any()
    assert np.abs(np.sqrt(d64.min(1)) - want[:300]).max() <= 1e-13 * np.abs(verts).max()


def test_samples_of_a_mesh_lie_on_it_and_win_their_own_face():
    verts, faces = MM.uv_sphere(32, 16)
    cdf = MM.face_weights(verts, faces)[1]
    u = np.random.default_rng(1).random((2000, 3), dtype=F32)
    points, drawn, normals = MM.sample_points(u, verts, faces, cdf)
    d2, face, face_normals = SD.points_to_mesh(points, verts, faces)
    d = np.sqrt(d2.astype(np.float64))
    print(f"on-surface: max {d.max()}, mean {d.mean()}")
    assert d.max() <= ON_SURFACE_BOUND
    assert np.array_equal(face, drawn)
    assert normals.tobytes() == face_normals.tobytes(), "the winning face's normal is mm_sample's, bit for bit"
    # what the sampled measure reports for the same surface: orders of magnitude above
    other = MM.sample_points(np.random.default_rng(2).random((5000, 3), dtype=F32), verts, faces, cdf)[0]
    assert math.sqrt(MM.mean64(MM.nearest(points, other)[0])) > 1000 * d.max()


def _seg_dist(p, a, b):
    p, a, b = (np.asarray(t, np.float64) for t in (p, a, b))
    e = b - a
    t = np.clip(((p - a) * e).sum(-1) / max((e * e).sum(), 1e-300), 0, 1)
    return np.sqrt((((p - a) - t[:, None] * e) ** 2).sum(-1))


def test_degenerate_faces_are_their_point_or_segment():
    x = _queries(1.0, 300, 5)
    a, b = np.array([0.25, -0.5, 0.125], F32), np.array([-0.75, 0.5, 0.5], F32)
    mid = ((a + b) * F32(0.5)).astype(F32)
    cases = {"point": (np.stack((a, a, a)), _seg_dist(x, a, a)),
             "repeated first": (np.stack((a, a, b)), _seg_dist(x, a, b)),
             "repeated last": (np.stack((a, b, b)), _seg_dist(x, a, b)),
             "repeated ends": (np.stack((a, b, a)), _seg_dist(x, a, b)),
             "collinear": (np.stack((a, mid, b)), _seg_dist(x, a, b))}
    for name, (verts, want) in cases.items():
        d2, face, normals = SD.points_to_mesh(x, verts, np.array([[0, 1, 2]], np.int32))
        assert not np.isnan(d2).any() and (face == 0).all(), name
        assert np.abs(np.sqrt(d2.astype(np.float64)) - want).max() <= ERICSON_BOUND, name
        if name != "collinear":                                      # an exactly zero cross product: no normal
            assert np.isnan(normals).all(), name
    # exactly on the point / on a vertex: distance 0
    d2, face, _ = SD.points_to_mesh(np.stack((a, b)), np.stack((a, a, b)), np.array([[0, 1, 2]], np.int32))
    assert d2.tolist() == [0.0, 0.0]


def test_ties_nan_rules_and_empty_meshes():
    verts, faces = SD.soup(40, 7)
    x = _queries(1.0, 200, 8)
    d2, face, normals = SD.points_to_mesh(x, verts, faces)
    # every face twice: the smaller index wins, the values are the same
    twice = np.concatenate((faces, faces))
    d2_t, face_t, _ = SD.points_to_mesh(x, verts, twice)
    assert d2_t.tobytes() == d2.tobytes() and np.array_equal(face_t, face)
    flipped = np.concatenate((faces[::-1], faces))
    assert np.array_equal(SD.points_to_mesh(x, verts, flipped)[1], len(faces) - 1 - face)
    # a NaN vertex takes out its own face only
    bad = verts.copy()
    bad[3 * 5 + 1, 2] = np.nan
    d2_n, face_n, _ = SD.points_to_mesh(x, bad, faces)
    assert not (face_n == 5).any() and not np.isnan(d2_n).any()
    keep = face != 5
    assert keep.any() and (~keep).any(), "face 5 won somewhere before"
    assert d2_n[keep].tobytes() == d2[keep].tobytes() and np.array_equal(face_n[keep], face[keep])
    rest = np.delete(faces, 5, 0)
    d2_r, face_r, _ = SD.points_to_mesh(x, verts, rest)
    assert d2_n.tobytes() == d2_r.tobytes() and np.array_equal(face_n, face_r + (face_r >= 5))
    # a face with an index out of range is skipped, not read
    wild = faces.copy()
    wild[5] = [0, len(verts), 1]
    wild[6] = [-1, 2, 3]
    d2_w, face_w, _ = SD.points_to_mesh(x, verts, wild)
    assert not np.isin(face_w, (5, 6)).any() and np.isfinite(d2_w).all()
    # a NaN query, a mesh of NaN, no faces at all: (+inf, -1, NaN normal)
    xn = x.copy()
    xn[3, 1] = np.nan
    d2_q, face_q, nrm_q = SD.points_to_mesh(xn, verts, faces)
    assert d2_q[3] == np.inf and face_q[3] == -1 and np.isnan(nrm_q[3]).all()
    assert np.delete(d2_q, 3).tobytes() == np.delete(d2, 3).tobytes()
    for v, f in ((np.full_like(verts, np.nan), faces), (verts, faces[:0]), (verts[:0], faces[:0])):
        d2_e, face_e, nrm_e = SD.points_to_mesh(x, v, f)
        assert np.isinf(d2_e).all() and (face_e == -1).all() and np.isnan(nrm_e).all()
    assert SD.points_to_mesh(x[:0], verts, faces)[0].shape == (0,)


def test_metric_reductions_on_hand_made_arrays():
    nan = np.nan
    d2x, d2y = np.array([0.0, 0.25, 1.0, 4.0], F32), np.array([0.0625, 0.0625], F32)
    unit = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 0]], F32)
    other = np.array([[-1, 0, 0], [0, 0.5, 0], [nan, 0, 1], [0, 1, 0]], F32)
    m = SD.metrics(d2x, d2y, unit, other, unit[:2], np.full((2, 3), nan, F32), thresholds=(0.5, 0.25, 0.1))
    assert m["x_to_y"] == 5.25 / 4 and m["y_to_x"] == 0.0625 and m["chamfer"] == 5.25 / 4 + 0.0625
    assert m["accuracy"] == 3.5 / 4 and m["completeness"] == 0.25
    assert (m["hausdorff_x_to_y"], m["hausdorff_y_to_x"], m["hausdorff"]) == (2.0, 0.25, 2.0)
    # the pair with a NaN normal is left out and counted out: |-1|, |0.5|, |0| over 3 pairs
    assert m["normal_pairs_x_to_y"] == 3 and m["normal_consistency_x_to_y"] == 1.5 / 3
    assert m["normal_pairs_y_to_x"] == 0 and math.isnan(m["normal_consistency_y_to_x"]) and math.isnan(m["normal_consistency"])
    rows = {r["threshold"]: r for r in m["fscore"]}
    assert [r["threshold"] for r in m["fscore"]] == [0.5, 0.25, 0.1]
    # the comparison is inclusive: 0.25 = 0.5^2 counts at 0.5, 0.0625 = 0.25^2 counts at 0.25
    assert rows[0.5]["precision"] == 0.5 and rows[0.5]["recall"] == 1.0 and rows[0.5]["fscore"] == 2 * 0.5 / 1.5
    assert rows[0.25]["precision"] == 0.25 and rows[0.25]["recall"] == 1.0
    assert rows[0.1]["precision"] == 0.25 and rows[0.1]["recall"] == 0.0 and rows[0.1]["fscore"] == 0.0
    none = SD.metrics(d2x + 1, d2y, unit, unit, unit[:2], unit[:2], thresholds=(0.1,))["fscore"][0]
    assert none == dict(threshold=0.1, precision=0.0, recall=0.0, fscore=0.0), "0 when P + R = 0, not a division by zero"
    assert SD.metrics(d2x, d2y, unit, unit, unit[:2], unit[:2])["normal_consistency"] == 1.0


def test_hip_ops_reductions_are_the_restatements():
    """hip_ops.surface_metrics runs on any torch device: the same hand-made arrays on the CPU"""
    import torch
    from nerfmeshes_amd import hip_ops
    rng = np.random.default_rng(4)
    d2x, d2y = rng.random(301).astype(F32), rng.random(200).astype(F32)
    nx, fx, ny, fy = (rng.standard_normal((n, 3)).astype(F32) for n in (301, 301, 200, 200))
    fx[7] = np.nan
    ny[11, 2] = np.inf
    want = SD.metrics(d2x, d2y, nx, fx, ny, fy, thresholds=(0.3, 0.9))
    got = hip_ops.surface_metrics(*(torch.from_numpy(a) for a in (d2x, d2y, nx, fx, ny, fy)), thresholds=(0.3, 0.9))
    assert set(got) == set(want)
    for k, v in want.items():
        if isinstance(v, float):
            assert abs(got[k] - v) <= 1e-12 * abs(v), k
        else:
            assert got[k] == v, k
    assert got["normal_pairs_x_to_y"] == 300 and got["normal_pairs_y_to_x"] == 199
    d2y[5] = F32(0.3) * F32(0.3)                                     # fp32 0.09...: compared in fp64 against 0.3 * 0.3
    a = hip_ops.surface_metrics(*(torch.from_numpy(t) for t in (d2x, d2y, nx, fx, ny, fy)), thresholds=(0.3,))["fscore"]
    assert a == SD.metrics(d2x, d2y, nx, fx, ny, fy, thresholds=(0.3,))["fscore"]


# ---- option plumbing ---------------------------------------------------------------------------------
def test_mesh_chamfer_options():
    from nerfmeshes_amd import mesh_chamfer
    p = mesh_chamfer.build_parser()
    a = p.parse_args(["--mesh", "a.obj", "--target", "b.obj"])
    assert (a.surface, a.fscore) == ("sampled", None)
    a = p.parse_args(["--mesh", "a.obj", "--target", "b.obj", "--surface", "exact", "--fscore", "0.01,0.5"])
    assert (a.surface, a.fscore) == ("exact", "0.01,0.5")
    assert mesh_chamfer.check_surface(a.surface, a.fscore) == (0.01, 0.5)
    assert mesh_chamfer.check_surface("sampled", None) == () and mesh_chamfer.check_surface("exact", "") == ()
    with pytest.raises(SystemExit):
        p.parse_args(["--mesh", "a.obj", "--target", "b.obj", "--surface", "nearest"])
    with pytest.raises(ValueError, match="--surface exact"):
        mesh_chamfer.check_surface("sampled", "0.1")
    for bad in ("0", "-1", "nan", "inf", "0.1,x"):
        with pytest.raises(ValueError, match="thresholds"):
            mesh_chamfer.check_surface("exact", bad)
    with pytest.raises(ValueError, match="--surface exact"):
        mesh_chamfer.compare_meshes(None, None, None, None, fscore=(0.1,))


def test_mesh_chamfer_refuses_fscore_without_the_exact_surface(capsys):
    from nerfmeshes_amd import mesh_chamfer
    with pytest.raises(SystemExit) as e:
        mesh_chamfer.main(["--mesh", "a.obj", "--target", "b.obj", "--fscore", "0.1"])
    assert e.value.code == 2 and "--surface exact" in capsys.readouterr().err


def _sampled_report():
    return dict(chamfer=0.5, x_to_y=0.25, y_to_x=0.25, rms_x_to_y=0.5, rms_y_to_x=0.5, samples=7, seed=3, normalize=True,
                mesh=dict(vertices=4, faces=2, area=1.5), target=dict(vertices=5, faces=3, area=2.5))


def test_format_report_of_a_sampled_report_is_unchanged():
    from nerfmeshes_amd import mesh_chamfer
    assert mesh_chamfer.format_report(_sampled_report()) == [
        "Chamfer distance over 7 samples per mesh (seed 3, normalized): 0.5",
        "  mesh -> target: mean squared distance 0.25, rms 0.5",
        "  target -> mesh: mean squared distance 0.25, rms 0.5",
        "  mesh: 4 vertices, 2 faces, area 1.5",
        "  target: 5 vertices, 3 faces, area 2.5"]
    assert mesh_chamfer.KEYS == ("chamfer", "x_to_y", "y_to_x", "rms_x_to_y", "rms_y_to_x")


def test_format_report_of_an_exact_report():
    from nerfmeshes_amd import mesh_chamfer
    report = _sampled_report()
    report.update(surface="exact", accuracy=0.4, completeness=0.3, hausdorff_x_to_y=0.9, hausdorff_y_to_x=0.8, hausdorff=0.9,
                  normal_consistency_x_to_y=0.75, normal_consistency_y_to_x=0.25, normal_consistency=0.5, normal_pairs_x_to_y=7,
                  normal_pairs_y_to_x=6)
    assert set(mesh_chamfer.EXACT_KEYS) <= set(report)
    lines = mesh_chamfer.format_report(report)
    assert lines[:5] == mesh_chamfer.format_report(_sampled_report()) and len(lines) == 9
    assert "accuracy (mesh -> target) 0.4" in lines[5] and "completeness (target -> mesh) 0.3" in lines[5]
    assert "Hausdorff 0.9" in lines[6] and "Normal consistency 0.5" in lines[7] and "over 6 pairs" in lines[8]
    report["fscore"] = [dict(threshold=0.1, precision=0.5, recall=1.0, fscore=2 / 3), dict(threshold=0.2, precision=1.0, recall=1.0, fscore=1.0)]
    more = mesh_chamfer.format_report(report)
    assert more[:9] == lines and more[9:] == [f"F-score at 0.1: {2 / 3} (precision 0.5, recall 1.0)",
                                              "F-score at 0.2: 1.0 (precision 1.0, recall 1.0)"]


def test_mesh_nerf_target_surface_options(tmp_path):
    from nerfmeshes_amd import mesh_nerf
    p = mesh_nerf.build_parser()
    a = p.parse_args([])
    assert (a.target_surface, a.target_fscore) == ("sampled", None)
    record = mesh_nerf.FEATURES["target_surface"]
    assert record.what == "--target-surface / --target-fscore" and record.any_option
    assert mesh_nerf.FEATURES["target"].what == "--target-mesh" and "target_surface" not in mesh_nerf.FEATURES["target"].options
    ok = p.parse_args(["--target-mesh", "t.obj", "--target-surface", "exact", "--target-fscore", "0.01,0.02"])
    assert mesh_nerf.check_features(ok) == {"target"}
    assert mesh_nerf.check_features(p.parse_args(["--target-mesh", "t.obj", "--target-surface", "exact"])) == {"target"}
    assert mesh_nerf.check_features(p.parse_args(["--target-mesh", "t.obj"])) == {"target"}
    # a bare namespace, and one with only the new names at their defaults
    assert mesh_nerf.check_features(argparse.Namespace()) == set()
    assert mesh_nerf.check_features(argparse.Namespace(target_surface="sampled", target_fscore=None)) == set()
    assert mesh_nerf.check_features(argparse.Namespace(target_mesh="t.obj", target_surface="exact")) == {"target"}
    for argv, text in ((["--target-surface", "exact"], "need --target-mesh"),
                       (["--target-fscore", "0.1"], "need --target-mesh"),
                       (["--target-mesh", "t.obj", "--target-fscore", "0.1"], "needs --target-surface exact"),
                       (["--target-mesh", "t.obj", "--target-surface", "nearest"], "must be sampled or exact"),
                       (["--target-mesh", "t.obj", "--target-surface", "exact", "--target-fscore", "0"], "finite and > 0"),
                       (["--target-mesh", "t.obj", "--target-surface", "exact", "--target-fscore", "nan"], "finite and > 0"),
                       (["--target-mesh", "t.obj", "--target-surface", "exact", "--target-fscore", "a,b"], "finite and > 0")):
        args = p.parse_args(argv + ["--save-dir", str(tmp_path)])
        with pytest.raises(ValueError, match=text):
            mesh_nerf.export_marching_cubes(None, args, None, "cpu")
    for argv in (["--target-surface", "exact"], ["--target-fscore", "0.1"]):
        args = p.parse_args(argv + ["--route", "script", "--save-dir", str(tmp_path)])
        with pytest.raises(ValueError) as e:
            mesh_nerf.export_marching_cubes(None, args, None, "cpu")
        assert str(e.value) == "--target-surface / --target-fscore have no --route script: the reference's script has no such step"
    assert not any(tmp_path.iterdir()), "rejected before anything is written"


# ---- header, signatures, exports, argument checks ----------------------------------------------------------
NAMES = ("nm_points_to_mesh_workspace_bytes", "nm_points_to_mesh")


def test_header_signatures_and_exports_agree():
    from nerfmeshes_amd import _lib
    header = open(os.path.join(ROOT, "include", "nerfmeshes_hip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        m = re.search(r"^(int64_t|int) " + name + r"\(([^;]*)\);", header, re.M)
        assert m, f"{name} is declared in the header"
        params = [p.strip() for p in m.group(2).replace("\n", " ").split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is (C.c_int64 if m.group(1) == "int64_t" else C.c_int)
        assert len(args) == len(params), name
        for p, a in zip(params, args):
            assert (a is C.c_void_p) == ("*" in p) and (a is C.c_int64) == p.startswith("int64_t "), (name, p)
        assert getattr(lib, name) is not None
    assert "Point to mesh" in header and "tests/mesh_surface_distance.py" in header
    assert lib.nm_abi_version() == 6


def test_argument_errors_without_a_gpu():
    from nerfmeshes_amd import _lib
    lib = _lib.load()
    null, one = C.c_void_p(None), C.c_void_p(256)                    # never dereferenced: validation fails first

    def err():
        return (lib.nm_last_error() or b"").decode()

    def call(x=one, n=5, v=one, nv=20, f=one, nf=10, d2=one, face=one, nrm=null, ws=one):
        return lib.nm_points_to_mesh(x, n, v, nv, f, nf, d2, face, nrm, ws, null)

    for kw in (dict(x=null), dict(v=null), dict(f=null), dict(d2=null), dict(face=null), dict(ws=null)):
        assert call(**kw) == 2 and "bad argument" in err(), kw
    for kw in (dict(n=-1), dict(nv=-1), dict(nf=-1), dict(n=1 << 31), dict(nv=1 << 31), dict(nf=(1 << 31) - 64), dict(n=(1 << 31) - 64)):
        assert call(**kw) == 2 and "2^31" in err(), kw
    assert call(nv=0) == 2 and "faces without vertices" in err()
    assert call(n=0, x=null, d2=null, face=null, ws=null) == 0, "no query: nothing to do, nothing launched"
    size = lib.nm_points_to_mesh_workspace_bytes
    assert size(-1, 0) == 0 and size(0, -1) == 0 and size((1 << 31) - 64, 10) == 0 and size(10, (1 << 31) - 64) == 0
    assert size(0, 0) >= 0 and size((1 << 31) - 65, (1 << 31) - 65) > 0
    # one record per face, one key per query
    assert 112 * 1000 <= size(0, 1000) <= 112 * 1000 + 1024 and 8 * 1000 <= size(1000, 0) <= 8 * 1000 + 1024
    assert size(1000, 1000) <= size(0, 1000) + size(1000, 0)


def test_wrappers_check_their_arguments_before_the_device():
    import torch
    from nerfmeshes_amd import _lib, hip_ops
    with pytest.raises(_lib.HipLibraryError, match="GPU memory"):
        hip_ops.points_to_mesh(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match=">= 1"):
        hip_ops.mesh_surface_distance(None, None, None, None, n=0)
    with pytest.raises(ValueError, match="finite and > 0"):
        hip_ops.mesh_surface_distance(None, None, None, None, n=5, thresholds=(0.0,))
    for name in ("points_to_mesh", "mesh_surface_distance", "surface_metrics"):
        assert callable(getattr(hip_ops, name))
