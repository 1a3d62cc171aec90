"""GPU: the image SSIM (nm_image_ssim, hip_ops.image_ssim, mesh_render --ssim, eval_views(metrics=), 2 ranks against 1).  The
kernel works in fp64 with every operation rounded on its own and sums integers, so every comparison with the numpy restatement
(tests/image_ssim.py) is exact: the bytes of the map, both int64 columns and the mean -- at every tile boundary of the 24 x 32
tile, for 1, 3 and 4 channels, run after run and on a second stream."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from nerfmeshes_amd import synthetic as S
from tests import image_ssim as IS
from tests.test_image_ssim import TODAYS_ROW, pair
from tests.test_mesh_raster import sheet
from tests.gpu_support import assert_ranks_ok, export_mesh, launch_ranks, scene_model
from tests.gpu_support import ops  # noqa: F401

pytestmark = pytest.mark.gpu
F32 = np.float32
TH, TW = 24, 32                          # IS_TH, IS_TW of nerfmeshes_amd/csrc/image_ssim.hip


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def images(kind, height, width, channels):
    if kind == "outside":
        rng = np.random.default_rng(height * 7 + width)
        return (rng.normal(0.5, 2.0, (height, width, channels)).astype(F32), rng.normal(0.5, 2.0, (height, width, channels)).astype(F32))
    if kind == "random":
        rng = np.random.default_rng(height * 11 + width)
        return rng.random((height, width, channels), dtype=F32), rng.random((height, width, channels), dtype=F32)
    return pair(kind, height, width, channels)


def check(ops, a, b, tag):
    """the device against the restatement: map bytes, sums, mean; want_map=False gives the same sums; a second run the same
    bytes -> the restatement's result"""
    want_map, want_sums, want = IS.ssim(a, b)
    da, db = _dev(a), _dev(b)
    second = torch.cuda.Stream()
    runs = []
    for nr in range(3):
        with torch.cuda.stream(second) if nr == 2 else contextlib.nullcontext():
            if nr == 2:
                second.wait_stream(torch.cuda.default_stream())
            runs.append(ops.image_ssim(da, db, want_map=True))
    bare = ops.image_ssim(da, db)
    for nr, got in enumerate(runs):
        m = got["map"].cpu().numpy()
        assert m.dtype == np.float64 and m.shape == want_map.shape, f"{tag} run {nr}: {m.shape}"
        assert m.tobytes() == want_map.tobytes(), f"{tag} run {nr}: the map differs, worst {np.abs(m - want_map).max()}"
        assert got["sums"].dtype == np.int64 and got["sums"].tolist() == want_sums.tolist(), f"{tag} run {nr}: sums"
        assert got["ssim"] == want and got["nonfinite"] == 0, f"{tag} run {nr}: {got['ssim']} != {want}"
        assert got["per_channel"] == IS.mean_of_sums(want_sums, want_map.shape[0] * want_map.shape[1])[1]
    assert bare["map"] is None and bare["sums"].tolist() == want_sums.tolist() and bare["ssim"] == want, f"{tag}: without the map"
    return want_map, want_sums, want


# (H - 10, W - 10): every tile boundary in both directions, thinned from the full product
OUTPUTS = [(1, 1), (1, TW), (2, 2 * TW + 3), (2, 2), (TH - 1, TW - 1), (TH - 1, TW + 1), (TH, 1), (TH, TW), (TH + 1, TW - 1),
           (TH + 1, TW + 1), (2 * TH + 3, 2), (2 * TH + 3, 2 * TW + 3), (1, 290), (290, 1)]
KINDS = ("random", "inverted", "constant", "quantised", "outside")


@pytest.mark.parametrize("out_h, out_w", OUTPUTS)
def test_bit_for_bit_against_the_restatement(ops, out_h, out_w):
    for channels in (1, 3, 4):
        for kind in KINDS:
            _, sums, value = check(ops, *images(kind, out_h + 10, out_w + 10, channels), f"{kind} {out_h + 10}x{out_w + 10}x{channels}")
            if kind == "inverted":
                assert (sums[:, 0] < 0).all() and value < 0, "negative S: the rounding of negatives"


def test_flat_images_take_a_height(ops):
    a, b = images("random", 40, 73, 3)
    want = IS.ssim(a, b)
    got = ops.image_ssim(_dev(a.reshape(-1, 3)), _dev(b.reshape(-1, 3)), want_map=True, height=40)
    assert got["map"].cpu().numpy().tobytes() == want[0].tobytes() and got["ssim"] == want[2]
    with pytest.raises(ValueError, match="image must be at least 11x11"):
        ops.image_ssim(_dev(a[:10]), _dev(b[:10]))
    with pytest.raises(ValueError, match="channels must be in"):
        ops.image_ssim(_dev(np.zeros((16, 16, 5), F32)), _dev(np.zeros((16, 16, 5), F32)))
    with pytest.raises(ValueError, match="one shape"):
        ops.image_ssim(_dev(a), _dev(b[:, :70]))
    with pytest.raises(ValueError, match="height="):
        ops.image_ssim(_dev(a.reshape(-1, 3)), _dev(b.reshape(-1, 3)))


def test_non_finite_pixels_are_counted_and_left_out(ops):
    a, b = images("random", 60, 90, 3)
    a[0, 0, 0], a[30, 45, 0], a[59, 89, 2] = np.nan, np.inf, -np.inf
    want_map, want_sums, want = IS.ssim(a, b)
    assert want_sums[:, 1].tolist() == [1 + 11 * 11, 0, 1] and np.isnan(want)
    for want_it in (True, False):
        got = ops.image_ssim(_dev(a), _dev(b), want_map=want_it)
        assert got["sums"].tolist() == want_sums.tolist() and np.isnan(got["ssim"]) and got["nonfinite"] == 1 + 121 + 1
    m = ops.image_ssim(_dev(a), _dev(b), want_map=True)["map"].cpu().numpy()
    finite = np.isfinite(want_map)
    assert (np.isfinite(m) == finite).all() and m[finite].tobytes() == want_map[finite].tobytes()


def test_full_size_identical_and_noisy(ops):
    """the one full-size case: 800 x 800 x 3"""
    rng = np.random.default_rng(800)
    a = rng.random((800, 800, 3), dtype=F32)
    got = ops.image_ssim(_dev(a), _dev(a.copy()), want_map=True)
    assert got["ssim"] == 1.0 and got["sums"].tolist() == [[790 * 790 * 2 ** 32, 0]] * 3 and bool((got["map"] == 1.0).all())
    b = (a + rng.normal(0.0, 0.05, a.shape)).astype(F32)
    want_map, want_sums, want = IS.ssim(a, b)
    got = ops.image_ssim(_dev(a), _dev(b), want_map=True)
    assert got["map"].cpu().numpy().tobytes() == want_map.tobytes() and got["sums"].tolist() == want_sums.tolist()
    assert got["ssim"] == want and 0.0 < want < 1.0


# ---- mesh_render ------------------------------------------------------------------------------------------------------------

def _views(count=2, size=64):
    poses = [sheet()[2], S.pose_spherical(25.0, -20.0, 3.0)]
    for nr in range(count):
        yield poses[nr], size, size, 80.0, torch.from_numpy(S.pseudo_targets(size * size, seed=5 + nr))


def test_mesh_render_scores_with_ssim_only_when_asked(ops, tmp_path):
    from nerfmeshes_amd import mesh_render
    verts, faces, _ = sheet()
    colors = np.random.default_rng(1).random((len(verts), 3), dtype=F32)
    background = (1.0, 1.0, 1.0)
    off = mesh_render.evaluate(verts, faces, colors, _views(), 0.1, background)
    assert [tuple(v) for v in off["views"]] == [TODAYS_ROW] * 2 and sorted(off) == ["counts", "mean", "near", "views"]
    assert list(off["mean"]) == ["psnr_target", "psnr_nerf", "depth_mean", "depth_median", "iou", "psnr_target_of_mean_mse"]
    assert not any("SSIM" in line for line in mesh_render.format_report(off))
    on = mesh_render.evaluate(verts, faces, colors, _views(), 0.1, background, ssim=True, save_dir=str(tmp_path), save_ssim_maps=True)
    assert [tuple(v) for v in on["views"]] == [TODAYS_ROW + mesh_render.SSIM_ROW] * 2
    for nr, (pose, height, width, focal, targets) in enumerate(_views()):
        rgb = mesh_render.render_mesh(verts, faces, colors, pose, height, width, focal, 0.1, background)["rgb"]
        want_map, _, want = IS.ssim(rgb.cpu().numpy(), targets.numpy().reshape(height, width, 3))
        row = on["views"][nr]
        assert row["ssim_target"] == want and row["ssim_nerf"] is None and -1.0 < want < 1.0
        assert {k: row[k] for k in TODAYS_ROW} == off["views"][nr], "the other columns do not see the option"
        image = mesh_render.read_image(str(tmp_path / "mesh_ssim" / f"{nr:04d}.png")).numpy()
        assert image.shape == (54, 54, 3)
        grey = np.clip(want_map.mean(axis=-1), 0.0, 1.0)
        assert np.abs(image[..., 0].astype(np.float64) - grey * 255.0).max() <= 0.5 + 1e-4 and (image[..., 0] == image[..., 1]).all()
    assert on["mean"]["ssim_target"] == float(np.mean([v["ssim_target"] for v in on["views"]])) and on["mean"]["ssim_nerf"] is None
    assert {k: v for k, v in on["mean"].items() if k not in mesh_render.SSIM_ROW} == off["mean"]
    assert sum("SSIM to the target" in line for line in mesh_render.format_report(on)) == 2
    assert not os.path.exists(tmp_path / "mesh_images")


# ---- eval_views -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene(ops):
    return scene_model("cuda", chunksize=1500)


def test_eval_views_fills_the_metrics_and_is_silent_without(ops, scene):
    from nerfmeshes_amd import eval_nerf
    model = scene
    views = list(eval_nerf.synthetic_views(2, height=40, width=52, focal=70.0))
    texts, results = {}, {}
    for tag, metrics in (("plain", None), ("ssim", {})):
        text = io.StringIO()
        with torch.no_grad(), contextlib.redirect_stdout(text):
            results[tag] = eval_nerf.eval_views(model, views, model.cfg, "cuda", metrics=metrics)
        texts[tag] = text.getvalue()
        if metrics is not None:
            filled = metrics
    plain, scored = results["plain"], results["ssim"]
    assert len(scored) == len(plain) == 4 and [float(x) for x in scored[0]] == [float(x) for x in plain[0]]
    assert float(scored[1]) == float(plain[1]) and scored[2] == plain[2] and torch.equal(scored[3], plain[3])
    plain_lines, lines = texts["plain"].splitlines(), texts["ssim"].splitlines()
    assert "SSIM" not in texts["plain"] and sum(line.startswith(("[EVAL]", "Dataset")) for line in plain_lines) == 3
    assert sorted(filled) == ["ssim", "ssim_mean"] and len(filled["ssim"]) == 2
    last = ops.image_ssim(scored[3], views[1][4].cuda(), height=40)["ssim"]
    assert filled["ssim"][1] == last and filled["ssim_mean"] == (filled["ssim"][0] + filled["ssim"][1]) / 2
    want = IS.ssim(scored[3].cpu().numpy().reshape(40, 52, 3), views[1][4].numpy().reshape(40, 52, 3))[2]
    assert last == want
    assert [line for line in lines if line.startswith("[EVAL]")][1].endswith(f" / SSIM: {filled['ssim'][1]}")
    assert lines[-1] == f"Dataset SSIM: {filled['ssim_mean']}"
    assert [line.split(" / SSIM")[0] for line in lines[:-1]] == plain_lines, "the other lines are the ones printed without"


# ---- mesh_nerf --render-ssim --------------------------------------------------------------------------------------------------

def test_the_exporter_adds_the_columns_only_with_render_ssim(ops, scene, tmp_path):
    import json
    from nerfmeshes_amd import mesh_render
    reports, texts = {}, {}
    for tag, extra in (("plain", []), ("ssim", ["--render-ssim"])):
        d = tmp_path / tag
        d.mkdir()
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            v, f, _, c = export_mesh(scene, d, "--res", "48", "--render-views", "2", "--render-size", "64", *extra)
        reports[tag], texts[tag] = json.load(open(d / "mesh.render.json")), text.getvalue().replace(str(d), "")
    assert [tuple(sorted(r)) for r in reports["plain"]["views"]] == [tuple(sorted(TODAYS_ROW))] * 2 and "SSIM" not in texts["plain"]
    rows = reports["ssim"]["views"]
    assert [set(r) for r in rows] == [set(TODAYS_ROW) | set(mesh_render.SSIM_ROW)] * 2
    assert [{k: r[k] for k in TODAYS_ROW} for r in rows] == reports["plain"]["views"]
    assert {k: m for k, m in reports["ssim"]["mean"].items() if k not in mesh_render.SSIM_ROW} == reports["plain"]["mean"]
    cfg = scene.cfg
    bounds = torch.tensor([cfg.dataset.near, cfg.dataset.far], dtype=torch.float32)
    background = (1.0,) * 3 if cfg.dataset.white_background else (0.0,) * 3
    for row, pose in zip(rows, S.orbit_poses(2)):
        focal = S.LEGO_FOCAL_800 * 64 / 800.0
        rgb = mesh_render.render_mesh(v, f.to(torch.int32), torch.as_tensor(c), pose, 64, 64, focal, cfg.dataset.near / 4, background)["rgb"]
        with torch.no_grad():
            chunk = cfg.nerf.validation.chunksize                    # the calls compare_with_nerf makes
            net = torch.cat([scene.query_view(pose, 64, 64, focal, bounds, first=s, count=min(chunk, 4096 - s), keep_depth=True).rgb_map
                             for s in range(0, 4096, chunk)])
        assert row["ssim_nerf"] == IS.ssim(rgb.cpu().numpy(), net.cpu().numpy().reshape(64, 64, 3))[2] and row["ssim_target"] is None
    assert texts["ssim"].count("SSIM to the network") == 2
    assert [line for line in texts["ssim"].splitlines() if not line.startswith(("[MESH]", "Mesh render: 2 views"))] == [
        line for line in texts["plain"].splitlines() if not line.startswith(("[MESH]", "Mesh render: 2 views"))]


# ---- two ranks ---------------------------------------------------------------------------------------------------------------

def test_two_ranks_sharing_one_gpu_equal_one_rank():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X")
    world = 2
    r = launch_ranks(os.path.join("tests", "tools", "ssim_dist_worker.py"), world, timeout=900)
    assert_ranks_ok(r, f"SSIM_DIST_OK world={world}")
