"""GPU: the exact point-to-mesh distance (nm_points_to_mesh, hip_ops.points_to_mesh / mesh_surface_distance, mesh_chamfer
--surface exact / --fscore, mesh_nerf --target-surface / --target-fscore).  The kernel against the numpy restatement
(tests/mesh_surface_distance.py) byte for byte over the lane / tile / split remainders, every query and mesh kind; what the
feature is for (a mesh against itself has no noise floor); analytic values on two spheres; both CLIs end to end; 2 ranks
against 1."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import mesh_metrics as MM
from tests import mesh_surface_distance as SD
from tests.gpu_support import assert_ranks_ok, export_mesh, launch_ranks, scene_model, to_device as _dev
from tests.gpu_support import ops  # noqa: F401
from tests.mesh_surface_distance import ON_SURFACE_BOUND

pytestmark = pytest.mark.gpu
F32 = np.float32
MESHES = ("sphere", "soup", "degenerate", "duplicated", "nan vertex")
QUERIES = ("random", "vertices", "midpoints", "samples", "far")
# (face counts, query counts): the tile remainder of the index rescan with every lane / workgroup remainder; 4097 faces with
# few queries are split over blockIdx.y (two pieces of at least NN_MIN_CHUNK = 2048) and merged by atomicMin; 2049 faces with
# 2049 queries (three workgroups, the last one a remainder) stay in one piece
SHAPES = {"tiles": ((1, 63, 64, 65), (1, 63, 2049)), "split": ((4097,), (1, 63)), "unsplit": ((2049,), (2049,))}


def _np(t):
    return t.cpu().numpy()


def _mesh(kind, nf, seed):
    rng = np.random.default_rng(seed)
    if kind == "sphere":                                             # its first faces touch the pole: exactly degenerate
        verts, faces = MM.uv_sphere(16, 8) if nf <= 256 else MM.uv_sphere(64, 33)
        return verts, faces[:nf]
    if kind == "soup":
        return SD.soup(nf, seed)
    if kind == "duplicated":                                         # face i and face i + half are the same triangle
        half = (nf + 1) // 2
        verts, faces = SD.soup(half, seed)
        return verts, np.concatenate((faces, faces))[:nf]
    nv = nf // 2 + 3
    verts = rng.standard_normal((nv, 3)).astype(F32)
    if kind == "degenerate":                                         # points, and segments with each corner repeated
        i, j = rng.integers(0, nv, nf), rng.integers(0, nv, nf)
        forms = np.stack((np.stack((i, i, i), 1), np.stack((i, i, j), 1), np.stack((i, j, j), 1), np.stack((i, j, i), 1)))
        return verts, forms[rng.integers(0, 4, nf), np.arange(nf)].astype(np.int32)
    assert kind == "nan vertex"
    verts[1, rng.integers(0, 3)] = np.nan
    return verts, rng.integers(0, nv, (nf, 3)).astype(np.int32)


def _queries(kind, n, verts, faces, seed):
    rng = np.random.default_rng(seed)
    pick = faces[rng.integers(0, len(faces), n)]
    if kind == "samples":
        cdf = MM.face_weights(verts, faces)[1]
        if cdf[-1] > 0:
            with np.errstate(all="ignore"):
                return MM.sample_points(rng.random((n, 3), dtype=F32), verts, faces, cdf)[0]
        kind = "midpoints"                                           # a mesh without area: points of its segments
    if kind == "random":
        return rng.standard_normal((n, 3)).astype(F32)
    if kind == "vertices":
        return verts[pick[np.arange(n), rng.integers(0, 3, n)]]
    if kind == "midpoints":
        k = rng.integers(0, 3, n)
        return ((verts[pick[np.arange(n), k]] + verts[pick[np.arange(n), (k + 1) % 3]]) * F32(0.5)).astype(F32)
    assert kind == "far"
    return (rng.standard_normal((n, 3)) * 10 + 1e4).astype(F32)


def _same(got, want, tag):
    """bytes, except that a NaN equals a NaN (0 / 0 has the sign bit set on the host)"""
    got = _np(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, got.shape, want.dtype, want.shape)
    if got.dtype == F32:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), f"{tag}: the NaN differ"
        got, want = np.where(nan, F32(0), got), np.where(nan, F32(0), want)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.reshape(len(got), -1).view(np.uint8) != want.reshape(len(want), -1).view(np.uint8)).any(1))
        raise AssertionError(f"{tag}: {len(bad)} of {len(got)} rows differ, first {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")


def _check(ops, x, verts, faces, tag):
    d2, face, normals = ops.points_to_mesh(_dev(x), _dev(verts), _dev(faces), return_normals=True)
    assert d2.dtype == torch.float32 and face.dtype == torch.int32 and normals.shape == (len(x), 3)
    want = SD.points_to_mesh(x, verts, faces)
    _same(face, want[1], f"{tag}: face")
    _same(d2, want[0], f"{tag}: dist2")
    assert not np.isnan(want[0]).any()
    _same(normals, want[2], f"{tag}: normals")
    return want


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("queries", QUERIES)
@pytest.mark.parametrize("mesh", MESHES)
def test_points_to_mesh_matches_the_restatement_bitwise(ops, mesh, queries, shape):
    for nf in SHAPES[shape][0]:
        verts, faces = _mesh(mesh, nf, 100 + nf)
        for n in SHAPES[shape][1]:
            x = _queries(queries, n, verts, faces, 7 * nf + n)
            d2, face, _ = _check(ops, x, verts, faces, f"{mesh}, {queries} queries, N={n} F={nf}")
            nan_rows = np.isnan(x).any(1)
            assert (face[nan_rows] == -1).all() and np.isinf(d2[nan_rows]).all()
            if mesh == "nan vertex":
                assert not np.isnan(verts[faces[face[face >= 0]]]).any(), "a face with a NaN vertex never wins"
            if mesh == "duplicated" and nf > 1:
                assert (face[face >= 0] < (nf + 1) // 2).all(), "of two equal faces the smaller index wins"


def test_nan_queries_empty_inputs_repeatability_and_bad_indices(ops):
    verts, faces = _mesh("soup", 300, 1)
    x = _queries("random", 500, verts, faces, 2)
    x[17, 1] = np.nan
    x[256] = np.nan
    d2, face, normals = _check(ops, x, verts, faces, "NaN rows")
    assert face[17] == -1 and face[256] == -1 and d2[17] == np.inf and np.isnan(normals[256]).all() and (np.delete(face, [17, 256]) >= 0).all()
    none = torch.empty(0, 3, dtype=torch.int32, device="cuda")
    for v in (_dev(verts), torch.empty(0, 3, device="cuda")):                     # F = 0, with and without vertices
        d2, face, normals = ops.points_to_mesh(_dev(x), v, none, return_normals=True)
        assert d2.shape == (500,) and bool(torch.isinf(d2).all()) and bool((face == -1).all()) and bool(torch.isnan(normals).all())
    d2, face = ops.points_to_mesh(torch.empty(0, 3, device="cuda"), _dev(verts), _dev(faces))      # N = 0
    assert d2.shape == (0,) and face.shape == (0,)
    # without the normals: the same two arrays
    a = ops.points_to_mesh(_dev(x), _dev(verts), _dev(faces))
    assert len(a) == 2
    _same(a[0], SD.points_to_mesh(x, verts, faces)[0], "no normals: dist2")
    # two calls give identical bytes, split and unsplit
    for nf, n in ((4500, 40), (2500, 3000)):
        verts, faces = _mesh("duplicated", nf, 3)
        x = _dev(_queries("samples", n, verts, faces, 4))
        a, b = (ops.points_to_mesh(x, _dev(verts), _dev(faces), return_normals=True) for _ in range(2))
        assert all(_np(s).tobytes() == _np(t).tobytes() for s, t in zip(a, b))
    bad = faces.copy()
    bad[7, 2] = len(verts)
    with pytest.raises(ValueError, match="outside"):
        ops.points_to_mesh(x, _dev(verts), _dev(bad))
    bad[7, 2] = -1
    with pytest.raises(ValueError, match="outside"):
        ops.points_to_mesh(x, _dev(verts), _dev(bad))
    with pytest.raises(ValueError, match=r"\(N,3\)"):
        ops.points_to_mesh(torch.zeros(4, 2, device="cuda"), _dev(verts), _dev(faces))


# ---- the feature's point ---------------------------------------------------------------------------------
def _gen(seed):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return gen


def test_a_mesh_against_itself_has_no_noise_floor(ops):
    verts, faces = MM.uv_sphere(32, 16)
    v, f = _dev(verts), _dev(faces)
    n = 2000
    res = ops.mesh_surface_distance(v, f, v, f, n, generator=_gen(0))
    gen = _gen(0)
    a, fa, na = ops.mesh_sample_points(v, f, n=n, generator=gen, return_normals=True)
    b, fb, nb = ops.mesh_sample_points(v, f, n=n, generator=gen, return_normals=True)
    sampled = ops.chamfer_distance(a, b)
    print(f"exact accuracy {res['accuracy']} completeness {res['completeness']} hausdorff {res['hausdorff']}; sampled rms "
          f"{math.sqrt(sampled['x_to_y'])}; 1 - normal consistency {1 - res['normal_consistency']}")
    assert res["accuracy"] <= ON_SURFACE_BOUND and res["completeness"] <= ON_SURFACE_BOUND and res["hausdorff"] <= ON_SURFACE_BOUND
    assert math.sqrt(sampled["x_to_y"]) > 1000 * ON_SURFACE_BOUND and math.sqrt(sampled["y_to_x"]) > 1000 * ON_SURFACE_BOUND
    # every sample wins the face it was drawn from, whose normal it carries: |dot| of a unit fp32 vector with itself is 1 up
    # to its length's rounding, 3 products and 2 sums of relative error 2^-24 each on top of the normalisation's (measured on
    # the CPU: >= 1 - 2.4e-7)
    assert torch.equal(res["face_x"], fa) and torch.equal(res["face_y"], fb)
    assert res["normal_pairs_x_to_y"] == n and res["normal_pairs_y_to_x"] == n
    assert abs(res["normal_consistency"] - 1) <= 4 * 2.4e-7
    # the reductions are the restatement's, from the device arrays
    want = SD.points_to_mesh(_np(a), verts, faces)
    _same(res["dist2_x"], want[0], "dist2_x")
    m = SD.metrics(_np(res["dist2_x"]), _np(res["dist2_y"]), _np(na), want[2], _np(nb), SD.points_to_mesh(_np(b), verts, faces)[2])
    for k, val in m.items():
        if isinstance(val, float):
            assert abs(res[k] - val) <= 1e-12 * abs(val), k
        else:
            assert res[k] == val, k


def test_a_sphere_against_its_copy_scaled_by_1_05(ops):
    verts, faces = MM.uv_sphere(64, 32)
    big = (verts * F32(1.05)).astype(F32)
    # a point of the inner polyhedron lies at a radius in [1 - s, 1], the outer surface between 1.05 (1 - s) and 1.05, with
    # s the polyhedron's sag: 1 - the distance of its nearest face to the centre (about 0.0024: its two chords sag 0.0012
    # each).  So every distance is within 1.05 s of 0.05, far from both thresholds.
    centre = np.zeros((1, 3))
    sag = 1.05 * (1 - math.sqrt(np.nanmin(SD.pair_dist2(centre, verts, faces, np.float64))))
    assert 0.002 < sag < 0.003
    cdf = MM.face_weights(verts, faces)[1]
    some = MM.sample_points(np.random.default_rng(0).random((300, 3), dtype=F32), verts, faces, cdf)[0]
    for x, v in ((some, big), ((some * F32(1.05)).astype(F32), verts)):      # the CPU restatement first
        d = np.sqrt(SD.points_to_mesh(x, v, faces)[0].astype(np.float64))
        assert 0.04 < 0.05 - sag <= d.min() and d.max() <= 0.05 + sag < 0.06
    n = 20000
    res = ops.mesh_surface_distance(_dev(verts), _dev(faces), _dev(big), _dev(faces), n, generator=_gen(1), thresholds=(0.04, 0.06))
    print(f"accuracy {res['accuracy']} completeness {res['completeness']} hausdorff {res['hausdorff']}")
    assert res["fscore"] == [dict(threshold=0.04, precision=0.0, recall=0.0, fscore=0.0),
                             dict(threshold=0.06, precision=1.0, recall=1.0, fscore=1.0)]
    for k in ("accuracy", "completeness", "hausdorff_x_to_y", "hausdorff_y_to_x"):
        assert abs(res[k] - 0.05) <= sag, k
    assert res["chamfer"] == res["x_to_y"] + res["y_to_x"] and abs(res["chamfer"] - 2 * 0.05 ** 2) <= 2 * (0.1 * sag + sag * sag)
    assert res["normal_consistency"] > 0.999, "the nearest face of the other sphere is (nearly) parallel"


# ---- command lines -----------------------------------------------------------------------------------------
def _write_obj(path, verts, faces):
    with open(path, "w") as fh:
        for v in verts:
            fh.write("v " + " ".join(repr(float(c)) for c in v) + "\n")
        for f in faces:
            fh.write("f " + " ".join(f"{int(i) + 1}//{int(i) + 1}" for i in f) + "\n")


def _sampled_by_hand(ops, va, fa, vb, fb, samples, seed):
    """compare_meshes' report before the options existed, from the same calls in the same order"""
    gen = _gen(seed)
    clouds, info = [], {}
    for name, v, f in (("mesh", va, fa), ("target", vb, fb)):
        v, f = torch.as_tensor(v).to("cuda", torch.float32), torch.as_tensor(f).to("cuda", torch.int32)
        areas, _ = ops.mesh_face_weights(v, f)
        clouds.append(ops.mesh_sample_points(v, f, n=samples, generator=gen)[0])
        info[name] = dict(vertices=int(v.shape[0]), faces=int(f.shape[0]), area=float(areas.double().sum().item()))
    res = ops.chamfer_distance(*clouds)
    out = dict(chamfer=res["chamfer"], x_to_y=res["x_to_y"], y_to_x=res["y_to_x"], rms_x_to_y=math.sqrt(res["x_to_y"]),
               rms_y_to_x=math.sqrt(res["y_to_x"]), samples=samples, seed=seed, normalize=False)
    out.update(info)
    return out


def test_mesh_chamfer_cli_exact_and_default(ops, tmp_path, capsys):
    from nerfmeshes_amd import mesh_chamfer
    verts, faces = MM.uv_sphere(32, 16)
    other = (verts * F32(1.25) + F32(0.125)).astype(F32)
    a_obj, b_obj, out = str(tmp_path / "a.obj"), str(tmp_path / "b.obj"), str(tmp_path / "report.json")
    _write_obj(a_obj, verts, faces)
    _write_obj(b_obj, other, faces)
    argv = ["--mesh", a_obj, "--target", b_obj, "--samples", "3001", "--seed", "5", "--out", out]
    capsys.readouterr()
    report = mesh_chamfer.main(argv + ["--surface", "exact", "--fscore", "0.2,0.3,0.5"])
    printed = capsys.readouterr().out.splitlines()
    want = ops.mesh_surface_distance(_dev(verts), _dev(faces), _dev(other), _dev(faces), 3001, generator=_gen(5), thresholds=(0.2, 0.3, 0.5))
    saved = json.load(open(out))
    assert saved == report and report["surface"] == "exact" and report["samples"] == 3001
    for k in ("chamfer", "x_to_y", "y_to_x") + mesh_chamfer.EXACT_KEYS + ("fscore",):
        assert report[k] == want[k], k
    assert report["rms_x_to_y"] == math.sqrt(want["x_to_y"]) and report["rms_y_to_x"] == math.sqrt(want["y_to_x"])
    assert set(report) == set(_sampled_by_hand(ops, verts, faces, other, faces, 3001, 5)) | set(mesh_chamfer.EXACT_KEYS) | {"surface", "fscore"}
    assert printed == mesh_chamfer.format_report(report) + [f"Chamfer report saved to {out}"] and len(printed) == 5 + 4 + 3 + 1
    assert [r["precision"] for r in report["fscore"]] != [0.0] * 3 and report["fscore"][2]["fscore"] == 1.0
    # no threshold: no `fscore` key
    assert "fscore" not in mesh_chamfer.main(argv + ["--surface", "exact"])
    capsys.readouterr()
    # the default invocation: the report, the file and the lines of the code before the options, nothing added
    report = mesh_chamfer.main(argv)
    printed = capsys.readouterr().out.splitlines()
    old = _sampled_by_hand(ops, verts, faces, other, faces, 3001, 5)
    old["mesh"]["path"], old["target"]["path"] = a_obj, b_obj
    assert report == old and list(report) == list(old) and "surface" not in report
    assert open(out).read() == json.dumps(old, indent=1) + "\n"
    assert printed == mesh_chamfer.format_report(old) + [f"Chamfer report saved to {out}"] and len(printed) == 6
    assert mesh_chamfer.main(argv + ["--surface", "sampled"]) == old


def test_mesh_nerf_target_surface_end_to_end(ops, tmp_path, capsys):
    from nerfmeshes_amd import mesh_chamfer
    from nerfmeshes_amd.nerf.nerf_helpers import load_obj
    scene = scene_model("cuda", chunksize=3000)
    verts, faces = MM.uv_sphere(32, 16, radius=0.5)
    target = str(tmp_path / "target.obj")
    _write_obj(target, verts, faces)
    dirs = {k: tmp_path / k for k in ("sampled", "exact")}
    for d in dirs.values():
        d.mkdir()
    common = ["--res", "48", "--target-mesh", target, "--chamfer-samples", "5001", "--chamfer-seed", "3"]
    capsys.readouterr()
    v, t = export_mesh(scene, dirs["exact"], *common, "--target-surface", "exact", "--target-fscore", "0.05,0.5")[:2]
    printed = capsys.readouterr().out.splitlines()
    tv, tf = load_obj(target)
    want = mesh_chamfer.compare_meshes(v, t, tv, tf, samples=5001, seed=3, surface="exact", fscore=(0.05, 0.5))
    want["target"]["path"] = target
    path = dirs["exact"] / "mesh.chamfer.json"
    assert open(path).read() == json.dumps(want, indent=1) + "\n"
    assert want["surface"] == "exact" and len(want["fscore"]) == 2 and 0 < want["accuracy"] < 2 and want["normal_pairs_x_to_y"] > 0
    lines = mesh_chamfer.format_report(want) + [f"Chamfer report saved to {path}"]
    assert [ln for ln in printed if ln in set(lines)] == lines
    # without the new options: the file of the code before them
    v2, t2 = export_mesh(scene, dirs["sampled"], *common)[:2]
    assert torch.equal(torch.as_tensor(v2), torch.as_tensor(v)) and torch.equal(torch.as_tensor(t2), torch.as_tensor(t))
    old = _sampled_by_hand(ops, v, t, tv, tf, 5001, 3)
    old["target"]["path"] = target
    assert open(dirs["sampled"] / "mesh.chamfer.json").read() == json.dumps(old, indent=1) + "\n"
    assert open(dirs["sampled"] / "mesh.obj", "rb").read() == open(dirs["exact"] / "mesh.obj", "rb").read()


# ---- ranks ---------------------------------------------------------------------------------------------------
def test_two_ranks_sharing_one_gpu_equal_one_rank():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X")
    r = launch_ranks(os.path.join("tests", "tools", "surface_distance_dist_worker.py"), 2, timeout=600)
    assert_ranks_ok(r, "SURFACE_DISTANCE_DIST_OK world=2")
