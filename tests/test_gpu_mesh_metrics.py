"""GPU: the chamfer measure (nm_mesh_face_weights / nm_mesh_sample_points / nm_points_nearest, hip_ops.chamfer_distance,
mesh_chamfer, mesh_nerf --target-mesh, the validation chamfer branch).  The kernels against the numpy restatement
(tests/mesh_metrics.py) byte for byte -- `tobytes()` equality --, analytic values on a sphere, both CLIs end to end, the
validation hook, and 2 / 3 ranks against 1."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import mesh_metrics as MM
from tests.helpers import load_golden
from tests.gpu_support import assert_ranks_ok, launch_ranks, scene_model, to_device as _dev
from tests.gpu_support import ops  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _np(t):
    return t.cpu().numpy()


def _same(got, want, tag):
    got = _np(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.view(np.uint8).reshape(len(got), -1) != want.view(np.uint8).reshape(len(want), -1)).any(1))
        raise AssertionError(f"{tag}: {len(bad)} of {len(got)} rows differ, first {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")


# ---- nearest neighbour ---------------------------------------------------------------------------
def _cloud(kind, n, m, seed):
    rng = np.random.default_rng(seed)
    if kind == "lattice":                                            # massive exact ties: the smallest index must win
        return rng.integers(-2, 3, (n, 3)).astype(np.float32), rng.integers(-2, 3, (m, 3)).astype(np.float32)
    x, y = rng.standard_normal((n, 3)).astype(np.float32), rng.standard_normal((m, 3)).astype(np.float32)
    if kind == "dirty":                                              # 5 % of y duplicated, 1 % of the rows of x and y NaN
        dup = rng.random(m) < 0.05
        y[dup] = y[rng.integers(0, m, int(dup.sum()))]
        x[rng.random(n) < 0.01, rng.integers(0, 3)] = np.nan
        y[rng.random(m) < 0.01] = np.nan
        if n > 1:
            x[n // 2] = np.nan
        if m > 1:
            y[m // 3, 1] = np.nan
    return x, y


def _check_nearest(ops, x, y, tag):
    d2, idx = ops.points_nearest(_dev(x), _dev(y))
    assert d2.dtype == torch.float32 and idx.dtype == torch.int32
    want_d2, want_idx = MM.nearest(x, y)
    _same(idx, want_idx, f"{tag}: index")
    _same(d2, want_d2, f"{tag}: dist2")
    return want_d2, want_idx


@pytest.mark.parametrize("kind", ["gauss", "lattice", "dirty"])
@pytest.mark.parametrize("m", [1, 255, 256, 257, 5000])
def test_points_nearest_matches_the_restatement_bitwise(ops, kind, m):
    for n in (1, 63, 64, 65, 1000, 4097):
        x, y = _cloud(kind, n, m, 1000 * n + m)
        d2, idx = _check_nearest(ops, x, y, f"{kind} N={n} M={m}")
        nan_rows = np.isnan(x).any(1)
        if np.isnan(y).any(1).all():
            nan_rows[:] = True
        assert (idx[nan_rows] == -1).all() and np.isinf(d2[nan_rows]).all()
        assert (idx[~nan_rows] >= 0).all() and not np.isnan(y[idx[~nan_rows]]).any(), "a NaN row is never a winner"


@pytest.mark.parametrize("n,m", [(7, 200_000), (200_000, 7), (3000, 70_001)])
@pytest.mark.parametrize("kind", ["gauss", "lattice"])
def test_points_nearest_split_targets_and_many_queries(ops, kind, n, m):
    x, y = _cloud(kind, n, m, n + m)
    _check_nearest(ops, x, y, f"{kind} N={n} M={m}")


def test_points_nearest_empty_inputs_conversions_and_repeatability(ops):
    x, y = _cloud("gauss", 300, 900, 5)
    d2, idx = ops.points_nearest(_dev(x), torch.empty(0, 3, device="cuda"))
    assert d2.shape == (300,) and bool(torch.isinf(d2).all()) and bool((idx == -1).all())
    d2, idx = ops.points_nearest(torch.empty(0, 3, device="cuda"), _dev(y))
    assert d2.shape == (0,) and idx.shape == (0,)
    # a non-contiguous fp64 view goes through the wrapper's conversion
    wide = torch.from_numpy(np.concatenate((x, x), 1).astype(np.float64)).cuda()
    tall = torch.from_numpy(np.ascontiguousarray(y.T).astype(np.float64)).cuda().t()
    assert not tall.is_contiguous()
    got = ops.points_nearest(wide[:, 3:], tall)
    want = MM.nearest(x, y)
    _same(got[0], want[0], "converted: dist2")
    _same(got[1], want[1], "converted: index")
    # two calls give identical bytes, on the split path as well
    bx, by = _cloud("dirty", 1500, 50_000, 9)
    a, b = ops.points_nearest(_dev(bx), _dev(by)), ops.points_nearest(_dev(bx), _dev(by))
    assert _np(a[0]).tobytes() == _np(b[0]).tobytes() and torch.equal(a[1], b[1])
    with pytest.raises(ValueError, match=r"\(N,3\)"):
        ops.points_nearest(torch.zeros(4, 2, device="cuda"), _dev(y))
    # distances that overflow: +inf is still a valid minimum and the first such row wins
    big = np.array([[3e38, 3e38, 0]], np.float32)
    d2, idx = ops.points_nearest(_dev(big), _dev(np.concatenate((np.full((1, 3), np.nan, np.float32), -big, -big))))
    assert float(d2[0]) == float("inf") and int(idx[0]) == 1


# ---- face weights and sampling -------------------------------------------------------------------
def _draws(n, cdf, seed):
    """uniform draws plus the edge cases: 0, the largest fp32 below 1, and values whose t is exactly a cdf boundary"""
    rng = np.random.default_rng(seed)
    u = rng.random((n, 3), dtype=np.float32)
    u[0] = 0.0
    u[1] = np.nextafter(np.float32(1), np.float32(0))
    u[2, 1:] = [0.0, u[1, 0]]
    total = int(cdf[-1])
    bounds = np.unique(cdf.astype(np.int64))
    k = 3
    for b in bounds[:-1][:: max(1, len(bounds) // 40)]:
        # the fp32 draws around b / total: those whose trunc(u * total) is exactly b are what the case is about
        c = np.float32(b / total)
        for cand in (np.nextafter(c, np.float32(0)), c, np.nextafter(c, np.float32(1))):
            if k < n and 0 <= cand < 1:
                u[k, 0] = cand
                k += 1
    return u


def _check_mesh(ops, verts, faces, n, seed, tag, on_boundary=None):
    areas, cdf = ops.mesh_face_weights(_dev(verts), _dev(faces))
    want_areas, want_cdf, bad = MM.face_weights(verts, faces)
    assert bad == 0 and cdf.dtype == torch.int64
    _same(areas, want_areas, f"{tag}: areas")
    assert np.array_equal(_np(cdf).view(np.uint64), want_cdf), f"{tag}: cdf"
    u = _draws(n, want_cdf, seed)
    pts, fid, nrm = ops.mesh_sample_points(_dev(verts), _dev(faces), u=_dev(u), return_normals=True)
    want_pts, want_fid, want_nrm = MM.sample_points(u, verts, faces, want_cdf)
    assert np.array_equal(_np(fid), want_fid), f"{tag}: face ids"
    _same(pts, want_pts, f"{tag}: points")
    _same(nrm, want_nrm, f"{tag}: normals")
    two = ops.mesh_sample_points(_dev(verts), _dev(faces), u=_dev(u))
    assert len(two) == 2 and torch.equal(two[0], pts) and torch.equal(two[1], fid)
    assert (want_areas[want_fid] > 0).all(), f"{tag}: a zero-weight face was sampled"
    # t == cdf[i] selects face i + 1 (the next one with a weight)
    t = np.trunc(u[:, 0].astype(np.float64) * float(int(want_cdf[-1]))).astype(np.int64)
    hit = np.isin(t, want_cdf.astype(np.int64))
    if on_boundary is not None:
        on_boundary.append(int(hit.sum()))
    c64 = want_cdf.astype(np.int64)
    assert (c64[want_fid[hit]] > t[hit]).all() and (np.concatenate(([0], c64))[want_fid[hit]] == t[hit]).all()
    # every point lies on its face: the residual against the fp64 barycentric combination (weights >= 0 that sum to 1)
    tri = verts.astype(np.float64)[faces[want_fid]]
    s64 = np.sqrt(u[:, 1].astype(np.float64))
    bary = np.stack((1 - s64, s64 * (1 - u[:, 2].astype(np.float64)), s64 * u[:, 2].astype(np.float64)), 1)
    exact = np.einsum("ik,ikj->ij", bary, tri)
    extent = float(np.abs(verts.astype(np.float64)).max()) or 1.0
    resid = np.linalg.norm(_np(pts).astype(np.float64) - exact, axis=1)
    assert resid.max() <= 1e-6 * extent, f"{tag}: a point {resid.max()} off its face"
    return want_areas, want_cdf, want_fid


@pytest.mark.parametrize("nf", [1, 1023, 1024, 1025, 2049])
def test_face_weights_at_the_chunk_boundaries_of_the_scan(ops, nf):
    """the cumulative table of 1, 1023, 1024, 1025 and 2049 random triangles: a single partial wave, a chunk of the
    one-workgroup scan (csrc/compact.h) one short of full and exactly full, the first entry of the second chunk (the carry is
    handed over) and of the third (it is carried twice) -- against numpy's cumsum of the restated integer weights in uint64"""
    rng = np.random.default_rng(nf)
    verts = rng.random((3 * nf, 3)).astype(np.float32)
    faces = rng.permutation(3 * nf).astype(np.int32).reshape(nf, 3)
    want_areas, want_cdf, bad = MM.face_weights(verts, faces)
    weights = np.diff(np.concatenate((np.zeros(1, np.uint64), want_cdf)))
    assert bad == 0 and (weights > 0).all() and weights.max() >= 2 ** 31, "every prefix moves; the largest weight is in [2^31, 2^32)"
    assert np.array_equal(np.cumsum(weights, dtype=np.uint64), want_cdf)
    dv, df, nv, _ = ops._mesh_arrays(_dev(verts), _dev(faces), "test")
    areas, cdf, total = ops._mesh_face_weights(ops._lib.load(), dv, df, nv, nf, "test")
    _same(areas, want_areas, f"{nf} faces: areas")
    assert cdf.dtype == torch.int64 and np.array_equal(_np(cdf).view(np.uint64), want_cdf), f"{nf} faces: cdf"
    assert total == int(want_cdf[-1]) == int(_np(cdf)[-1])


def test_sampling_on_the_uv_sphere(ops):
    verts, faces = MM.uv_sphere()
    assert faces.shape == (4096, 3)
    areas, cdf, fid = _check_mesh(ops, verts, faces, 20000, 1, "uv sphere")
    assert int((areas == 0).sum()) == 128, "the pole triangles are degenerate"
    w = np.diff(np.concatenate(([0], cdf.astype(np.int64))))
    assert 2 ** 31 <= w.max() < 2 ** 32 and (w[areas == 0] == 0).all()


def test_sampling_draws_on_a_cdf_boundary(ops):
    """areas 8, 0, 4, 0, 0, 2, 2: the weights are 2^31, 0, 2^30, 0, 0, 2^29, 2^29 and the boundaries 1/2, 3/4, 7/8 are fp32
    draws whose t is exactly cdf[i]: they select the NEXT face that has a weight"""
    def right(x, a, b):
        return [[x, 0, 0], [x + a, 0, 0], [x, b, 0]]
    verts = np.array(right(0, 4, 4) + right(10, 1, 0) + right(20, 4, 2) + right(30, 0, 0) + right(40, 0, 3) + right(50, 2, 2)
                     + right(60, 2, 2), np.float32)
    faces = np.arange(21, dtype=np.int32).reshape(7, 3)
    seen = []
    areas, cdf, fid = _check_mesh(ops, verts, faces, 200, 6, "powers of two", seen)
    assert areas.tolist() == [8, 0, 4, 0, 0, 2, 2] and cdf.tolist() == [2 ** 31, 2 ** 31, 3 * 2 ** 30, 3 * 2 ** 30, 3 * 2 ** 30,
                                                                         7 * 2 ** 29, 2 ** 32]
    assert seen[0] >= 3
    u = np.zeros((6, 3), np.float32)
    u[:, 0] = [0.5, np.nextafter(np.float32(0.5), np.float32(0)), 0.75, 0.875, np.nextafter(np.float32(0.875), np.float32(0)), 0]
    got = ops.mesh_sample_points(_dev(verts), _dev(faces), u=_dev(u))[1]
    assert got.tolist() == [2, 0, 5, 6, 5, 0]


def test_sampling_on_every_fixture_mesh(ops):
    g = load_golden("mc_cases")
    checked = 0
    for i in range(int(g["count"])):
        if f"err_{i}" in g.files or len(g[f"faces_{i}"]) == 0:
            continue
        _check_mesh(ops, np.ascontiguousarray(g[f"verts_{i}"], np.float32), g[f"faces_{i}"].astype(np.int32), 1000, i, f"golden {i}")
        checked += 1
    assert checked == 667


def test_sampling_one_huge_and_many_tiny_faces(ops):
    rng = np.random.default_rng(4)
    k = 3000
    tiny = rng.random((k, 1, 3)) * 50 + (rng.random((k, 3, 3)) - 0.5) * rng.random((k, 1, 1)) ** 4 * 0.5
    verts = np.concatenate((np.array([[0, 0, 0], [1000, 0, 0], [0, 1000, 0]], np.float64), tiny.reshape(-1, 3))).astype(np.float32)
    faces = np.concatenate((np.array([[0, 1, 2]]), 3 + np.arange(3 * k).reshape(k, 3))).astype(np.int32)
    order = rng.permutation(len(faces))                              # the huge face somewhere in the middle
    areas, cdf, fid = _check_mesh(ops, verts, faces[order], 5000, 2, "huge + tiny")
    w = np.diff(np.concatenate(([0], cdf.astype(np.int64))))
    small = w[areas < areas.max()]
    assert (small < 2 ** 12).all() and (small == 0).any() and (small > 0).any(), "tiny faces on both sides of m * 2^-32"
    # the tiny faces together weigh less than 3000 * 2^12 / 2^31 = 0.6 % of the total, and at most 3 + 3 * 41 = 126 of the 5000
    # draws (2.5 %) are planted next to a cdf boundary by _draws
    assert (fid == int(np.argmax(areas))).mean() > 0.96
    # only faces far below the largest: they alone are sampled, in proportion
    areas2, cdf2, fid2 = _check_mesh(ops, verts, faces[1:], 5000, 3, "tiny only")
    assert len(np.unique(fid2)) > 100


def test_sampling_argument_errors(ops):
    verts, faces = MM.uv_sphere(8, 4)
    v, f = _dev(verts), _dev(faces)
    with pytest.raises(ValueError, match="no area"):
        ops.mesh_sample_points(_dev(np.zeros((5, 3), np.float32)), _dev(np.array([[0, 1, 2], [2, 3, 4]], np.int32)), n=10)
    with pytest.raises(ValueError):
        ops.mesh_sample_points(v, torch.empty(0, 3, dtype=torch.int32, device="cuda"), n=10)
    bad = faces.copy()
    bad[3, 1] = len(verts)
    with pytest.raises(ValueError, match="outside"):
        ops.mesh_sample_points(v, _dev(bad), n=10)
    bad[3, 1] = -1
    with pytest.raises(ValueError, match="outside"):
        ops.mesh_face_weights(v, _dev(bad))
    with pytest.raises(ValueError, match="give the number"):
        ops.mesh_sample_points(v, f)
    # the default draws come from the generator: the same seed, the same points
    gens = [torch.Generator(device="cuda") for _ in range(2)]
    for gen in gens:
        gen.manual_seed(11)
    a, b = (ops.mesh_sample_points(v, f, n=777, generator=gen) for gen in gens)
    assert a[0].shape == (777, 3) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    areas, cdf = ops.mesh_face_weights(v, torch.empty(0, 3, dtype=torch.int32, device="cuda"))
    assert areas.shape == (0,) and cdf.shape == (0,)


# ---- chamfer distance: analytic values -----------------------------------------------------------
@pytest.fixture(scope="module")
def sphere_clouds(ops):
    verts, faces = MM.uv_sphere()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    n = 20000
    a = ops.mesh_sample_points(_dev(verts), _dev(faces), n=n, generator=gen)[0]
    b = ops.mesh_sample_points(_dev(verts), _dev(faces), n=n, generator=gen)[0]
    c = ops.mesh_sample_points(_dev(verts * np.float32(1.1)), _dev(faces), n=n, generator=gen)[0]
    return n, a, b, c


def test_chamfer_of_two_samplings_of_a_sphere(ops, sphere_clouds):
    n, a, b, _ = sphere_clouds
    res = ops.chamfer_distance(a, b)
    ratio = res["chamfer"] * n / 8                                   # E[d^2] = area / (pi N) = 4 / N per direction
    print(f"two samplings of the unit sphere, N = {n}: chamfer * N / 8 = {ratio}")
    assert 0.8 <= ratio <= 1.2
    assert isinstance(res["chamfer"], float) and res["chamfer"] == res["x_to_y"] + res["y_to_x"]
    assert res["dist2_x"].shape == (n,) and res["dist2_y"].shape == (n,) and res["dist2_x"].is_cuda


def test_chamfer_of_a_sphere_and_its_scaled_copy(ops, sphere_clouds):
    n, a, _, c = sphere_clouds
    res = ops.chamfer_distance(a, c)
    print(f"unit sphere against radius 1.1, N = {n}: chamfer = {res['chamfer']}")
    assert 0.019 <= res["chamfer"] <= 0.022                          # 2 * 0.1^2 + 8 / N


def test_chamfer_identities_and_the_fp64_mean(ops, sphere_clouds):
    n, a, b, c = sphere_clouds
    same = ops.chamfer_distance(a, a)
    assert same["chamfer"] == 0.0 and same["x_to_y"] == 0.0 and not bool(same["dist2_x"].any())
    ab, ba = ops.chamfer_distance(a, b), ops.chamfer_distance(b, a)
    assert ab["chamfer"] == ba["chamfer"] and ab["x_to_y"] == ba["y_to_x"] and ab["y_to_x"] == ba["x_to_y"]
    assert torch.equal(ab["dist2_x"], ba["dist2_y"]) and torch.equal(ab["dist2_y"], ba["dist2_x"])
    for key, name in (("dist2_x", "x_to_y"), ("dist2_y", "y_to_x")):
        want = MM.mean64(_np(ab[key]))
        assert abs(ab[name] - want) <= 1e-10 * want
    # against the restatement on a smaller pair, unequal sizes
    x, y = _np(a[:3001]), _np(c[:1777])
    got, want = ops.chamfer_distance(_dev(x), _dev(y)), MM.chamfer(x, y)
    _same(got["dist2_x"], want["dist2_x"], "chamfer: dist2_x")
    _same(got["dist2_y"], want["dist2_y"], "chamfer: dist2_y")
    for name in ("chamfer", "x_to_y", "y_to_x"):
        assert abs(got[name] - want[name]) <= 1e-10 * want[name]
    with pytest.raises(ValueError, match="empty"):
        ops.chamfer_distance(a, torch.empty(0, 3, device="cuda"))


# ---- end to end ----------------------------------------------------------------------------------
def _scene(**experiment):
    return scene_model("cuda", chunksize=3000, **{f"experiment.{k}": v for k, v in experiment.items()})


@pytest.fixture(scope="module")
def scene(ops):
    return _scene()


def _report_lines(report):
    from nerfmeshes_amd import mesh_chamfer
    return set(mesh_chamfer.format_report(report))


def test_mesh_nerf_target_mesh_end_to_end(ops, tmp_path, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_ckpt", os.path.join(ROOT, "scripts", "make_synthetic_checkpoint.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    vdir = mk.write(str(tmp_path / "logs"))
    from nerfmeshes_amd import mesh_nerf
    n = 20000
    dirs = {k: tmp_path / k for k in ("plain", "same", "ss2")}
    for d in dirs.values():
        d.mkdir()
    common = ["--log-checkpoint", vdir, "--res", "48", "--batch-size", "4096", "--view-disparity-max-bound", "1.0"]
    capsys.readouterr()
    mesh_nerf.main(common + ["--save-dir", str(dirs["plain"])])
    plain_out = capsys.readouterr().out
    target = str(dirs["plain"] / "mesh.obj")
    chamfer = ["--target-mesh", target, "--chamfer-samples", str(n)]
    mesh_nerf.main(common + ["--save-dir", str(dirs["same"])] + chamfer)
    same_out = capsys.readouterr().out
    assert not (dirs["plain"] / "mesh.chamfer.json").exists()
    report = json.load(open(dirs["same"] / "mesh.chamfer.json"))
    assert report["samples"] == n and report["seed"] == 0 and report["normalize"] is False
    assert report["mesh"]["faces"] == report["target"]["faces"] > 100 and report["target"]["path"] == target
    assert abs(report["mesh"]["area"] - report["target"]["area"]) <= 1e-6 * report["mesh"]["area"]
    for k in ("x_to_y", "y_to_x"):
        assert abs(report["rms_" + k] ** 2 - report[k]) <= 1e-12 * report[k]
    assert report["chamfer"] == report["x_to_y"] + report["y_to_x"]
    ratio = report["chamfer"] * n / 8 / (report["mesh"]["area"] / (4 * np.pi))
    print(f"the same surface sampled twice: chamfer = {report['chamfer']}, area = {report['mesh']['area']}, ratio = {ratio}")
    assert 0.5 <= ratio <= 2
    # the OBJ and every other printed line are those of the run without --target-mesh
    assert open(dirs["same"] / "mesh.obj", "rb").read() == open(target, "rb").read()
    new = _report_lines(report) | {f"Chamfer report saved to {dirs['same'] / 'mesh.chamfer.json'}"}
    kept = [l for l in same_out.splitlines() if l not in new]
    assert len(kept) == len(same_out.splitlines()) - len(new), "every new line was printed"
    assert [l.replace(str(dirs["same"]), "DIR") for l in kept] == [l.replace(str(dirs["plain"]), "DIR") for l in plain_out.splitlines()]
    # the refined mesh against the plain one: further than a resampling of the same surface, within one cell
    mesh_nerf.main(common + ["--save-dir", str(dirs["ss2"]), "--super-sampling", "2"] + chamfer)
    capsys.readouterr()
    ss2 = json.load(open(dirs["ss2"] / "mesh.chamfer.json"))
    print(f"--super-sampling 2 against the plain mesh: chamfer = {ss2['chamfer']}")
    assert report["chamfer"] < ss2["chamfer"] < (2.4 / 48) ** 2


def _write_obj(path, verts, faces):
    with open(path, "w") as fh:
        for v in verts:
            fh.write("v " + " ".join(repr(float(c)) for c in v) + "\n")
        for f in faces:
            fh.write("f " + " ".join(f"{int(i) + 1}//{int(i) + 1}" for i in f) + "\n")


@pytest.mark.parametrize("normalize", [False, True])
def test_mesh_chamfer_cli_reproduces_hip_ops_by_hand(ops, tmp_path, capsys, normalize):
    from nerfmeshes_amd import mesh_chamfer, mesh_nerf
    verts, faces = MM.uv_sphere(32, 16)
    other = (verts * np.float32(1.25) + np.float32(0.125)).astype(np.float32)
    _write_obj(tmp_path / "a.obj", verts, faces)
    _write_obj(tmp_path / "b.obj", other, faces)
    out = tmp_path / "report.json"
    argv = ["--mesh", str(tmp_path / "a.obj"), "--target", str(tmp_path / "b.obj"), "--samples", "5000", "--seed", "5", "--out", str(out)]
    report = mesh_chamfer.main(argv + (["--normalize"] if normalize else []))
    printed = capsys.readouterr().out
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    clouds = []
    for v in (verts, other):
        v = _dev(v)
        if normalize:
            v = mesh_nerf.normalize_vertices(v)
        clouds.append(ops.mesh_sample_points(v, _dev(faces), n=5000, generator=gen)[0])
    want = ops.chamfer_distance(*clouds)
    saved = json.load(open(out))
    for k in ("chamfer", "x_to_y", "y_to_x"):
        assert report[k] == want[k] == saved[k], k
    assert saved["rms_x_to_y"] == math.sqrt(want["x_to_y"]) and saved["samples"] == 5000 and saved["normalize"] is normalize
    assert saved["mesh"]["vertices"] == len(verts) and saved["target"]["faces"] == len(faces)
    scale = 1.0 if normalize else 1.25 ** 2
    assert abs(saved["target"]["area"] / saved["mesh"]["area"] - scale) < 1e-4
    assert f"{want['chamfer']}" in printed and str(out) in printed
    if normalize:
        assert saved["chamfer"] < 0.01, "the two spheres coincide once normalised"
    else:
        assert saved["chamfer"] > 0.05


# ---- the validation hook -------------------------------------------------------------------------
class _StubDataset:
    def __init__(self, target_mesh):
        self.target_mesh = target_mesh


def _outputs():
    return [{"log": {"validation/loss": torch.tensor(0.5), "validation/psnr": torch.tensor(20.0)}, "val_loss": torch.tensor(0.5)},
            {"log": {"validation/loss": torch.tensor(1.5), "validation/psnr": torch.tensor(30.0)}, "val_loss": torch.tensor(1.5)}]


@pytest.fixture(scope="module")
def own_mesh(scene):
    from nerfmeshes_amd import mesh_nerf
    args = mesh_nerf.build_parser().parse_args(["--res", "48", "--iso-level", "32"])
    with torch.no_grad():
        v, f = mesh_nerf.extract_geometry(scene, "cuda", args)[:2]
    return v.cpu(), f.cpu()


def test_validation_epoch_end_logs_the_chamfer_loss(ops, own_mesh, capsys):
    model = _scene(chamfer_loss=True, chamfer_res=48)
    model.val_dataset = _StubDataset(own_mesh)
    got = model.validation_epoch_end(_outputs())
    loss = got["log"]["validation/chamfer_loss"]
    print(f"validation/chamfer_loss of the model's own mesh, {model.cfg.experiment.chamfer_sampling_size} samples: {float(loss)}")
    assert isinstance(loss, torch.Tensor) and loss.dim() == 0 and bool(torch.isfinite(loss))
    assert 0 < float(loss) < (2 / 48) ** 2
    assert float(got["log"]["validation/loss"]) == 1.0 and float(got["val_loss"]) == 1.0
    # a level above the grid's range: the adaptive clamp still finds a surface
    high = _scene(chamfer_loss=True, chamfer_res=48, chamfer_iso_level=1.0e9)
    high.val_dataset = _StubDataset(own_mesh)
    loss = high.validation_epoch_end(_outputs())["log"]["validation/chamfer_loss"]
    assert bool(torch.isfinite(loss)) and float(loss) > 0


def test_validation_epoch_end_without_the_chamfer_loss_is_unchanged(ops, own_mesh, scene):
    scene.val_dataset = _StubDataset(own_mesh)
    got = scene.validation_epoch_end(_outputs())
    assert set(got) == {"log", "val_loss"} and set(got["log"]) == {"validation/loss", "validation/psnr"}
    assert float(got["log"]["validation/psnr"]) == 25.0 and float(got["val_loss"]) == 1.0


def test_validation_epoch_end_skips_a_grid_without_a_surface(ops, own_mesh, monkeypatch, capsys):
    from nerfmeshes_amd import mesh_nerf
    model = _scene(chamfer_loss=True, chamfer_res=48)
    model.val_dataset = _StubDataset(own_mesh)

    def no_surface(*a, **k):
        raise RuntimeError("No surface found at the given iso value.")

    monkeypatch.setattr(mesh_nerf, "extract_geometry", no_surface)
    capsys.readouterr()
    got = model.validation_epoch_end(_outputs())
    assert "validation/chamfer_loss" not in got["log"] and set(got["log"]) == {"validation/loss", "validation/psnr"}
    assert capsys.readouterr().out.count("Chamfer loss skipped") == 1

    def other(*a, **k):
        raise RuntimeError("something else")

    monkeypatch.setattr(mesh_nerf, "extract_geometry", other)
    with pytest.raises(RuntimeError, match="something else"):
        model.validation_epoch_end(_outputs())
    model.val_dataset = _StubDataset(None)
    with pytest.raises(AssertionError, match="a target mesh .obj must be provided"):
        model.validation_epoch_end(_outputs())


# ---- ranks ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_ranks_sharing_one_gpu_equal_one_rank(world):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X")
    r = launch_ranks(os.path.join("tests", "tools", "chamfer_dist_worker.py"), world, timeout=900)
    assert_ranks_ok(r, f"CHAMFER_DIST_OK world={world}")
