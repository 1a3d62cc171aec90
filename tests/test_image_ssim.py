"""CPU: the image SSIM's rule.  The numpy restatement (tests/image_ssim.py) against the same formula over scipy's Gaussian
filter, its exact values on identical images, the argument errors of nm_image_ssim on a host without a GPU, and the command
lines: the options parse, and with them off the report has exactly the columns it had."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import image_ssim as IS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SIZES = [(11, 11), (12, 75), (40, 73), (26, 74), (27, 139), (64, 64)]
KINDS = ("identical", "inverted", "noisy", "constant", "quantised")


def pair(kind, height, width, channels=3, seed=0):
    rng = np.random.default_rng(seed + 1000 * height + width)
    a = rng.random((height, width, channels), dtype=F32)
    if kind == "identical":
        return a, a.copy()
    if kind == "inverted":
        return a, (F32(1.0) - a).astype(F32)
    if kind == "noisy":
        return a, (a + rng.normal(0.0, 0.1, a.shape)).astype(F32)
    if kind == "constant":
        return np.full_like(a, 0.25), np.full_like(a, 0.75)
    if kind == "quantised":
        q = (np.round(a * 255.0) / 255.0).astype(F32)
        return q, (np.round(np.clip(a + rng.normal(0.0, 0.05, a.shape), 0.0, 1.0) * 255.0) / 255.0).astype(F32)
    raise KeyError(kind)


def test_the_taps_are_the_normalised_gaussian():
    k = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-0.5 * (k / 1.5) ** 2)
    assert np.abs(IS.W - g / g.sum()).max() < 1e-16 and IS.W.shape == (11,) and (IS.W == IS.W[::-1]).all()
    assert IS.C1 == 0.01 * 0.01 and IS.C2 == 0.03 * 0.03


@pytest.mark.parametrize("height, width", SIZES)
def test_restatement_against_scipy(height, width):
    """Bars (derived, not measured): each filtered value carries about 22 fp64 roundings of at most 1.1e-16 of values <= 1;
    the quotient amplifies them by at most a 1 / (C1 C2)-class factor when both variances vanish: 1e-9 for the map.  The fixed
    point rounds every S to a multiple of 2^-32, so its mean is within 2^-33 of the plain mean."""
    ndimage = pytest.importorskip("scipy.ndimage")
    for kind in KINDS:
        a, b = pair(kind, height, width)
        x, y = a.astype(np.float64), b.astype(np.float64)
        smooth = [ndimage.gaussian_filter(f, (1.5, 1.5, 0.0), truncate=3.5, mode="reflect")[5:height - 5, 5:width - 5]
                  for f in (x, y, x * x, y * y, x * y)]
        want = IS.ssim_map(*smooth)
        got, sums, value = IS.ssim(a, b)
        assert got.shape == want.shape == (height - 10, width - 10, 3) and got.dtype == np.float64
        worst = np.abs(got - want).max()
        print(f"{kind} {height}x{width}: map differs by {worst:.3g}, mean by {abs(value - got.mean(axis=(0, 1)).mean()):.3g}")
        assert worst <= 1e-9, (kind, worst)
        assert (sums[:, 1] == 0).all() and sums.dtype == np.int64 and sums.shape == (3, 2)
        assert abs(value - got.mean(axis=(0, 1)).mean()) <= 2.0 ** -33, kind


@pytest.mark.parametrize("height, width", SIZES)
def test_identical_images_are_exactly_one(height, width):
    a, b = pair("identical", height, width)
    got, sums, value = IS.ssim(a, b)
    assert (got == 1.0).all()
    assert sums[:, 0].tolist() == [(height - 10) * (width - 10) * 2 ** 32] * 3 and value == 1.0


def test_negative_values_round_half_to_even_and_non_finite_pixels_are_counted():
    a, b = pair("inverted", 26, 74)
    got, sums, value = IS.ssim(a, b)
    assert (got < 0).all() and (sums[:, 0] < 0).all() and value < -0.9
    assert sums[:, 0].tolist() == [int(np.rint(got[..., c] * 2.0 ** 32).astype(np.int64).sum()) for c in range(3)]
    a = a.copy()
    a[3, 4, 0], a[20, 70, 2] = np.nan, np.inf
    got, sums, value = IS.ssim(a, b)
    assert sums[:, 1].tolist() == [4 * 5, 0, 6 * 4] and np.isnan(value)
    assert np.isfinite(got[..., 1]).all() and (~np.isfinite(got[..., 0])).sum() == 20


def test_the_library_rejects_bad_arguments_without_a_gpu():
    from nerfmeshes_amd import _lib
    lib = _lib.load()
    null, one = C.c_void_p(None), C.c_void_p(8)                # never dereferenced: validation fails first

    def err():
        return (lib.nm_last_error() or b"").decode()

    assert lib.nm_abi_version() == 6
    for bad in ((null, one, 16, 16, 3, null, one), (one, null, 16, 16, 3, null, one), (one, one, 16, 16, 3, null, null)):
        assert lib.nm_image_ssim(*bad, null) == 2 and "bad argument" in err()
    for height, width in ((10, 16), (16, 10), (0, 0), (-5, 16)):
        assert lib.nm_image_ssim(one, one, height, width, 3, null, one, null) == 2
        assert "image must be at least 11x11" in err()
    for height, width in ((16385, 16), (16, 16385)):
        assert lib.nm_image_ssim(one, one, height, width, 3, null, one, null) == 2 and "at most 16384" in err()
    for channels in (0, 5, -1):
        assert lib.nm_image_ssim(one, one, 16, 16, channels, null, one, null) == 2 and "channels must be in [1, 4]" in err()


def test_the_symbol_is_declared_exported_and_bound():
    from nerfmeshes_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "nerfmeshes_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint nm_image_ssim\s*\(const float\* d_a, const float\* d_b, int32_t height, int32_t width, int32_t channels,"
                     r"\s*double\* d_map,\s*int64_t\* d_sums, void\* stream\);", code)
    assert "#define NM_ABI_VERSION 6" in header and "6, later: + nm_image_ssim" in header
    assert hasattr(_lib.load(), "nm_image_ssim") and "image_ssim.hip" in build.SOURCES
    restype, argtypes = _lib.SIGNATURES["nm_image_ssim"]
    assert restype is C.c_int and argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                               C.c_void_p]
    for tap in IS.HALF:                                        # the rule in the header and the kernel name the same constants
        assert tap.hex() in header
        assert tap.hex() in open(os.path.join(ROOT, "nerfmeshes_amd", "csrc", "image_ssim.hip")).read()


TODAYS_ROW = ("psnr_target", "psnr_nerf", "depth_mean", "depth_median", "depth_pixels", "iou", "drawn", "bad_index", "not_finite",
              "near", "out_of_range", "culled", "off_screen", "degenerate", "large", "covered", "fragments")


def test_the_options_parse_and_are_off_by_default():
    from nerfmeshes_amd import eval_nerf, mesh_nerf, mesh_render
    args = mesh_render.build_parser().parse_args(["--mesh", "m.obj"])
    assert args.ssim is False and args.save_ssim_maps is False
    args = mesh_render.build_parser().parse_args(["--mesh", "m.obj", "--ssim", "--save-ssim-maps"])
    assert args.ssim is True and args.save_ssim_maps is True
    assert eval_nerf.build_parser().parse_args([]).ssim is False and eval_nerf.build_parser().parse_args(["--ssim"]).ssim is True
    assert mesh_nerf.build_parser().parse_args([]).render_ssim is False
    args = mesh_nerf.build_parser().parse_args(["--render-views", "2", "--render-ssim"])
    assert args.render_ssim is True and mesh_nerf.check_features(args) == {"render", "render_ssim"}
    assert mesh_nerf.check_features(mesh_nerf.build_parser().parse_args(["--render-views", "2"])) == {"render"}


def test_render_ssim_needs_render_views(tmp_path):
    from nerfmeshes_amd import mesh_nerf
    args = mesh_nerf.build_parser().parse_args(["--render-ssim", "--save-dir", str(tmp_path)])
    with pytest.raises(ValueError) as e:
        mesh_nerf.export_marching_cubes(None, args, None, "cpu")
    assert str(e.value) == "--render-ssim needs --render-views N > 0 and --render-size >= 11"
    assert not any(tmp_path.iterdir()), "rejected before anything is written"
    args = mesh_nerf.build_parser().parse_args(["--render-ssim", "--render-views", "2", "--render-size", "10"])
    with pytest.raises(ValueError, match="--render-size >= 11"):
        mesh_nerf.check_features(args)
    args = mesh_nerf.build_parser().parse_args(["--render-ssim", "--render-views", "2", "--route", "script"])
    with pytest.raises(ValueError) as e:
        mesh_nerf.check_features(args)
    assert str(e.value) == "--render-views has no --route script: the reference's script has no such step"
    assert mesh_nerf.check_features(argparse.Namespace()) == set()


def test_without_the_options_the_report_has_todays_columns():
    from nerfmeshes_amd import hip_ops, mesh_render
    assert mesh_render.ROW == TODAYS_ROW and TODAYS_ROW[6:] == hip_ops.RASTER_COUNTS
    assert mesh_render.VERTEX_ROW == ("psnr_target_vertex", "psnr_nerf_vertex")
    table = np.full((2, len(mesh_render.ROW)), np.nan)
    table[:, 6:] = 3.0
    table[0, :6] = (20.0, 30.0, 0.01, 0.005, 100.0, 0.9)
    report = mesh_render.build_report(table, 0.5)
    assert sorted(report) == ["counts", "mean", "near", "views"]
    assert list(report["mean"]) == ["psnr_target", "psnr_nerf", "depth_mean", "depth_median", "iou", "psnr_target_of_mean_mse"]
    assert [tuple(v) for v in report["views"]] == [mesh_render.ROW] * 2
    lines = mesh_render.format_report(report)
    assert len(lines) == 4 and not any("SSIM" in line or "ssim" in line for line in lines)
    # ... and with them the columns stand behind today's
    columns = mesh_render.ROW + mesh_render.SSIM_ROW
    table = np.concatenate((table, [[0.75, 0.5], [0.25, np.nan]]), axis=1)
    report = mesh_render.build_report(table, 0.5, columns)
    assert report["mean"]["ssim_target"] == 0.5 and report["mean"]["ssim_nerf"] == 0.5
    assert report["views"][1]["ssim_nerf"] is None and tuple(report["views"][0]) == columns
    lines = mesh_render.format_report(report)
    assert "SSIM to the target 0.750000, to the network 0.500000" in lines[0] and lines[1].endswith("SSIM to the target 0.250000")
