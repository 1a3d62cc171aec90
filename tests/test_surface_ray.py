"""CPU: the surface point cloud's host side -- the PLY writer (nm_export_ply) through the reader of tests/surface_filter.py,
the argument checks of the three new C entries, the pose list, the vote limit, the parser's defaults against the reference's
constants, and the restated filter on a hand-made case."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from nerfmeshes_amd import _lib, hip_ops, mesh_surface_ray as msr, synthetic as S
from tests import surface_filter as SF


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _cloud(n, seed=0):
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal((n, 3)) * rng.choice([1e-6, 1e-3, 1.0, 1e5, 1e20], (n, 1))).astype(np.float32)
    nrm = rng.standard_normal((n, 3)).astype(np.float32)
    special = np.array([0.0, -0.0, 1.0, -1.0, 1e-4, 9.999e-5, 1e16, 1.5e16, np.inf, -np.inf, 1e-45, 3.4028235e38, 0.1, 123456.0, 0.002],
                       dtype=np.float32)
    k = min(n, len(special) // 3)
    p[:k] = special[:3 * k].reshape(k, 3)
    c = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    if n >= 2:
        c[0], c[1] = (0, 0, 0), (255, 255, 255)
    return p, nrm, c


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("n", [0, 1, 2, 1000, 50001])
def test_ply_round_trip_bit_for_bit(tmp_path, binary, n):
    p, nrm, c = _cloud(n)
    path = tmp_path / "cloud.ply"
    hip_ops.export_ply(p, nrm, c, str(path), binary=binary)
    fmt, rp, rn, rc = SF.read_ply(path)
    assert fmt == ("binary" if binary else "ascii")
    assert rp.shape == (n, 3) and rn.shape == (n, 3) and rc.shape == (n, 3)
    assert np.array_equal(_bits(rp), _bits(p)) and np.array_equal(_bits(rn), _bits(nrm)) and np.array_equal(rc, c)
    if binary:
        assert os.path.getsize(path) == open(path, "rb").read().index(b"end_header\n") + 11 + 27 * n


def test_ply_header_and_ascii_lines(tmp_path):
    p = np.array([[1.0, -0.5, 1e-5], [0.1, 2.0, 1e20]], np.float32)
    nrm = np.array([[0.0, 0.0, -1.0], [0.25, -0.0, 3.0]], np.float32)
    c = np.array([[0, 128, 255], [7, 8, 9]], np.uint8)
    path = tmp_path / "two.ply"
    msr.export_ply(p, c, nrm, str(path))                                   # the reference's argument order
    text = open(path).read()
    assert text == ("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
                    "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\n"
                    "property uchar blue\nend_header\n"
                    "1.0 -0.5 9.999999747378752e-06 0.0 0.0 -1.0 0 128 255\n"
                    "0.10000000149011612 2.0 1.0000000200408773e+20 0.25 -0.0 3.0 7 8 9\n")
    for line, row in zip(text.splitlines()[13:], np.concatenate((p, nrm), 1)):
        assert line.split()[:6] == [repr(float(x)) for x in row], "floats as Python prints the widened fp32"
    msr.export_ply(p, c, nrm, str(path), binary=True)
    assert open(path, "rb").read().startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 2\n")


def test_export_ply_converts_float_colours_by_the_documented_rule(tmp_path):
    rgb = np.array([[0.0, 1.0, 0.5], [0.999, -0.2, 1.7], [np.nan, 0.00392, 0.00393]], np.float32)
    want = np.array([[0, 255, 127], [254, 0, 255], [0, 0, 1]], np.uint8)
    assert np.array_equal(msr.color_bytes(rgb), want) and np.array_equal(SF.color_bytes(rgb), want)
    path = tmp_path / "c.ply"
    msr.export_ply(np.zeros((3, 3), np.float32), rgb, np.ones((3, 3), np.float32), str(path), binary=True)
    assert np.array_equal(SF.read_ply(path)[3], want)
    with pytest.raises(ValueError, match="uint8"):
        hip_ops.export_ply(np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32), rgb, str(path))


def test_argument_errors_without_a_gpu(tmp_path):
    lib = _lib.load()
    null, one = C.c_void_p(None), C.c_void_p(16)           # never dereferenced: validation fails first

    def err():
        return (lib.nm_last_error() or b"").decode()

    def flt(o=one, d=one, z=one, h=8, w=8, step=2, ws=one):
        return lib.nm_surface_filter(o, 0, d, z, null, 0.0, h, w, step, 0.002, 15, null, null, null, ws, null)

    for kw in (dict(o=null), dict(d=null), dict(z=null), dict(ws=null)):
        assert flt(**kw) == 2 and "bad argument" in err(), kw
    assert flt(step=-1) == 2 and "step must be in [0, 8]" in err()
    assert flt(step=9) == 2 and "step must be in [0, 8]" in err()
    for h, w in ((0, 8), (8, 0), (-3, 8), (1 << 16, 1 << 16)):
        assert flt(h=h, w=w) == 2 and "height and width" in err()
        assert lib.nm_surface_filter_workspace_bytes(h, w) == 0
    # one 8-byte word and one 4-byte prefix per 64-pixel row segment, plus the count
    assert lib.nm_surface_filter_workspace_bytes(800, 800) >= 800 * 13 * 12 + 8
    assert lib.nm_surface_filter_workspace_bytes(1, 1) >= 20

    def gat(ws=one, o=one, d=one, z=one, rgb=one, h=8, w=8, off=0, cap=64, cu8=one):
        return lib.nm_surface_gather(ws, o, 0, d, z, null, 0.0, rgb, h, w, off, cap, one, one, one, cu8, null)

    for kw in (dict(ws=null), dict(o=null), dict(d=null), dict(z=null)):
        assert gat(**kw) == 2 and "bad argument" in err(), kw
    assert gat(rgb=null) == 2 and "colour outputs need" in err()
    assert gat(h=0) == 2 and gat(w=-1) == 2
    assert gat(off=-1) == 2 and "row offset" in err()
    assert gat(off=65, cap=64) == 2 and "row offset" in err()

    ok = (C.c_float * 3)(1.0, 2.0, 3.0)
    col = (C.c_uint8 * 3)(1, 2, 3)
    p = lambda a: C.cast(a, C.c_void_p)   # noqa: E731
    assert lib.nm_export_ply(null, p(ok), p(col), 1, 0, b"/nonexistent-dir/x.ply") == 2 and "null array" in err()
    assert lib.nm_export_ply(p(ok), null, p(col), 1, 0, b"/nonexistent-dir/x.ply") == 2 and "null array" in err()
    assert lib.nm_export_ply(p(ok), p(ok), null, 1, 1, b"/nonexistent-dir/x.ply") == 2 and "null array" in err()
    assert lib.nm_export_ply(p(ok), p(ok), p(col), 1, 0, b"/nonexistent-dir/x.ply") == 6 and "cannot open" in err()
    assert lib.nm_export_ply(p(ok), p(ok), p(col), -1, 0, str(tmp_path / "x.ply").encode()) == 2
    assert lib.nm_export_ply(null, null, null, 0, 0, str(tmp_path / "empty.ply").encode()) == 0
    assert lib.nm_abi_version() == 6


def test_wrappers_refuse_host_tensors():
    with pytest.raises(_lib.HipLibraryError, match="GPU memory"):
        hip_ops.surface_filter(torch.zeros(1, 3), torch.zeros(16, 3), torch.zeros(16), 4, 4)


def test_pose_list_is_the_reference_orbit():
    args = msr.build_parser().parse_args([])
    poses = msr.render_poses(args)
    assert len(poses) == 32
    ys, xs = [-180.0, -135.0, -90.0, -45.0, 0.0, 45.0, 90.0, 135.0], [-90.0, -30.0, 30.0, 90.0]
    k = 0
    for y in ys:                                   # angleY outer, angleX inner (mesh_surface_ray.py:85-86)
        for x in xs:
            want = S.pose_spherical(y, x, 4.0)
            assert poses[k].dtype == np.float32 and poses[k].shape == (4, 4)
            assert np.allclose(poses[k], want, rtol=0, atol=1e-6), (y, x)
            k += 1
    assert np.array_equal(poses[5], S.pose_spherical(np.linspace(-180, 180, 8, endpoint=False)[1], np.linspace(-90, 90, 4)[1], 4.0))
    five = msr.render_poses(msr.build_parser().parse_args(["--views-y", "5", "--views-x", "1", "--radius", "3"]))
    assert len(five) == 5 and np.array_equal(five[2], S.pose_spherical(np.linspace(-180, 180, 5, endpoint=False)[2], -90.0, 3.0))
    for p in poses:
        assert abs(np.linalg.norm(p[:3, 3]) - 4.0) < 1e-5


def test_min_votes_is_the_reference_comparison_in_python_doubles():
    mv = hip_ops.surface_min_votes
    assert 24 * 0.6 == 14.399999999999999 and mv(2, 0.6) == 15
    for step, prob in ((2, 0.6), (1, 0.5), (1, 0.625), (1, math.nextafter(0.625, 0)), (1, math.nextafter(0.625, 1)),
                       (3, 0.5), (3, math.nextafter(0.5, 0)), (3, math.nextafter(0.5, 1)), (3, 0.6), (0, 0.6), (2, 0.0),
                       (2, 1.0), (1, 0.9999)):
        limit = ((2 * step + 1) ** 2 - 1) * prob
        got = mv(step, prob)
        for count in range(0, (2 * step + 1) ** 2 + 2):
            assert (count >= got) == (count > limit), (step, prob, count)
    assert mv(1, 0.625) == 6 and mv(1, math.nextafter(0.625, 0)) == 5          # 8 * 0.625 = 5.0: "more than 5"
    assert mv(3, 0.5) == 25 and mv(3, math.nextafter(0.5, 0)) == 24 and mv(3, math.nextafter(0.5, 1)) == 25
    assert mv(1, 0.5) == 5 and mv(0, 0.6) == 1 and mv(2, 1.0) == 25           # step 0: no neighbours, the centre's own vote


def test_parser_defaults_are_the_reference_constants():
    a = msr.build_parser().parse_args([])
    # mesh_surface_ray.py:71-78, :90, :154
    assert (a.views_y, a.views_x, a.radius, a.img_size, a.step_size) == (8, 4, 4.0, 800, 2)
    assert (a.dist_threshold, a.prob_threshold, a.focal) == (0.002, 0.6, 1111.1111)
    assert a.ply_name == "lego-sampling.ply" and a.save_dir == "." and a.checkpoint == "model_last.ckpt"
    assert a.min_opacity is None and a.ply_format == "ascii" and a.normals == "ray" and a.precision == "f32"
    assert a.focal == S.LEGO_FOCAL_800
    helptext = msr.build_parser().format_help()
    assert helptext.count("(addition)") == 4 and "summation" in helptext


def test_get_grid_is_row_major():
    g = msr.get_grid(3)
    assert g.tolist() == [[0, 0], [0, 1], [0, 2], [1, 0], [1, 1], [1, 2], [2, 0], [2, 1], [2, 2]]


def _hand_case():
    """6 x 6 pixels 0.01 apart in x / y, looking down z: depth 1 on the left three columns, 2 on the right three, a hole
    (depth 0) at (2, 1) and a spike (depth 3) at (4, 4).  Window 3 x 3, squared distance limit 0.002: neighbours on the same
    level vote (at most 2e-4 apart), the others do not (at least 1 apart)."""
    H = W = 6
    rows, cols = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    o = torch.stack((cols * 0.01, rows * 0.01, torch.zeros(H, W)), -1).float()
    d = torch.tensor([0.0, 0.0, 1.0]).expand(H, W, 3).contiguous()
    depth = torch.ones(H, W)
    depth[:, 3:] = 2.0
    depth[2, 1], depth[4, 4] = 0.0, 3.0
    return o, d, depth


HAND_VOTES = [[9, 9, 6, 6, 9, 9],      # clamped duplicates count: a corner still has 9 votes
              [8, 8, 5, 6, 9, 9],      # next to the hole: one vote fewer; at the step: the three across do not vote
              [8, 1, 5, 6, 9, 9],      # the hole itself: only its own vote
              [8, 8, 5, 5, 8, 8],
              [9, 9, 6, 5, 1, 8],      # the spike: only its own vote
              [9, 9, 6, 5, 8, 8]]


def test_restated_filter_on_the_hand_made_case():
    o, d, depth = _hand_case()
    votes, keep, points, normals = SF.surface_filter(o, d, depth, 1, 0.002, 0.6)          # 8 * 0.6 = 4.8: five votes
    assert votes.tolist() == HAND_VOTES
    want = torch.ones(6, 6, dtype=torch.bool)
    want[2, 1] = want[4, 4] = False
    assert torch.equal(keep, want)
    assert points.shape == (34, 3) and torch.equal(normals, torch.tensor([-0.0, -0.0, -1.0]).expand(34, 3))
    kept = [(r, c) for r in range(6) for c in range(6) if (r, c) not in ((2, 1), (4, 4))]   # row-major
    want_pts = torch.tensor([[np.float32(0.01) * c, np.float32(0.01) * r, 1.0 if c < 3 else 2.0] for r, c in kept])
    assert torch.equal(points, want_pts.float())
    # 8 * 0.625 = 5.0 exactly: "more than five"
    v2, k2, p2, _ = SF.surface_filter(o, d, depth, 1, 0.002, 0.625)
    assert v2.tolist() == HAND_VOTES and torch.equal(k2, torch.tensor(HAND_VOTES) >= 6) and p2.shape[0] == 28   # six pixels with five votes, the hole, the spike
    # the well-conditioned rule: opacity below the limit behaves as depth 0
    acc = torch.ones(6, 6)
    acc[0, 0] = 0.98
    v3, k3, p3, _ = SF.surface_filter(o, d, depth, 1, 0.002, 0.6, opacity=acc, min_opacity=0.99)
    assert not bool(k3[0, 0]) and int(v3[0, 0]) == 4 and int(v3[0, 1]) == 7 and int(v3[1, 1]) == 7 and p3.shape[0] == 33
    # a negative depth votes like any other point but is never kept; NaN never votes
    depth2 = depth.clone()
    depth2[0, 5], depth2[5, 0] = -2.0, float("nan")
    v4, k4, _, _ = SF.surface_filter(o, d, depth2, 1, 0.002, 0.6)
    assert int(v4[0, 5]) == 4 and not bool(k4[0, 5]) and int(v4[5, 0]) == 0 and not bool(k4[5, 0])


def test_threshold_compares_in_fp32_as_torch_does():
    """`fp32 tensor < Python float` rounds the float to fp32 first: two points exactly 0.5 apart (0.25 squared) are NOT closer
    than a limit of 0.25 + 1e-10 (its fp32 rounding, 0.25, lies below the double) nor than 0.25 - 1e-10 (rounds up to 0.25)."""
    o = torch.zeros(1, 2, 3)
    d = torch.tensor([[[0.0, 0.0, 1.0], [0.5, 0.0, 1.0]]])
    depth = torch.ones(1, 2)
    for thr, votes in ((0.25 + 1e-10, 6), (0.25 - 1e-10, 6), (0.2500001, 9), (0.002, 6)):
        assert np.float32(0.25) == np.float32(0.25 + 1e-10) == np.float32(0.25 - 1e-10)
        v, _, _, _ = SF.surface_filter(o, d, depth, 1, thr, 0.0)
        assert v.tolist() == [[votes, votes]], thr
