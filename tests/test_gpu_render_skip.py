"""The render path's skip of workgroup tiles without density (MI355X).

Inside `nm_render_rays` / `nm_render_view` the two network calls write workspace radiance that only the compositor reads, and
a sample with raw sigma <= 0 has alpha == weight == 0 exactly.  A workgroup tile (128 samples: 8 adjacent rays x 16 consecutive
samples where samples % 16 == 0, else 128 consecutive samples) on which NO sample has density therefore writes {0, 0, 0, sigma}
and skips fc_feat, the view layer and fc_rgb.  Nothing an entry point returns may change: the reference of every case here is
the unchanged public path on the same handles, which never skips --

    coarse_intervals -> eval_rays -> composite -> sample_pdf -> eval_rays -> composite

-- and all six maps of both bundles must be equal BIT FOR BIT.  The tiles the library reports as skipped must be exactly the
all-empty tiles of that path's sigma under the documented tiling."""
import numpy as np
import pytest
import torch

from nerfmeshes_amd import synthetic as S

pytestmark = pytest.mark.gpu

MLP_KW = dict(num_layers=8, hidden_size=256, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
SIDE, FIRST, RAYS = 800, 400 * 800, 2051          # 2051 consecutive pixels of the middle row: not a multiple of 8
NEAR, FAR = 2.0, 6.0


def _dev():
    return torch.device("cuda")


def _rays(count=RAYS):
    from nerfmeshes_amd import hip_ops
    o, d = hip_ops.ray_bundle(S.orbit_poses(1)[0], SIDE, SIDE, S.LEGO_FOCAL_800, FIRST, count, device=_dev())
    return o[None].contiguous(), d


def _bounds():
    return torch.tensor([NEAR], device=_dev()), torch.tensor([FAR], device=_dev())


def _u(nc, nf):
    return torch.linspace(0.0, 1.0, nc).to(_dev()), torch.linspace(0.0, 1.0, nf).to(_dev())


def public_path(coarse, fine, o, d, u_c, u_f):
    """The six maps of both bundles and the raw sigma of both passes, from the public entry points (no tile is ever skipped)."""
    from nerfmeshes_amd import hip_ops
    near, far = _bounds()
    t_c = hip_ops.coarse_intervals(u_c, near, far, d.shape[0])
    rad_c = coarse.eval_rays(o, d, t_c)
    cb = hip_ops.composite(rad_c, t_c, d)
    if fine is None:
        return cb, None, rad_c[..., 3], None
    t_f = hip_ops.sample_pdf(t_c, cb["weights"], u_f)
    rad_f = fine.eval_rays(o, d, t_f)
    fb = hip_ops.composite(rad_f, t_f, d)
    return cb, fb, rad_c[..., 3], rad_f[..., 3]


def tile_classes(sigma):
    """(empty, full, mixed) workgroup tiles of a (rays, samples) sigma under the kernel's tiling.  A sample has density unless
    sigma <= 0 (so a NaN has); the padding of the last ray block / the last linear tile has none."""
    sigma = sigma.detach().cpu().numpy()
    rays, samples = sigma.shape
    dense = ~(sigma <= 0.0)
    real = np.ones_like(dense)
    if samples % 16 == 0:                           # 8 adjacent rays x 16 consecutive samples
        pad = (-rays) % 8
        dense = np.pad(dense, ((0, pad), (0, 0)))
        real = np.pad(real, ((0, pad), (0, 0)))
        shape = (dense.shape[0] // 8, 8, samples // 16, 16)
        dense, real = dense.reshape(shape).transpose(0, 2, 1, 3).reshape(-1, 128), real.reshape(shape).transpose(0, 2, 1, 3).reshape(-1, 128)
    else:                                           # linear order
        pad = (-dense.size) % 128
        dense, real = np.pad(dense.reshape(-1), (0, pad)).reshape(-1, 128), np.pad(real.reshape(-1), (0, pad)).reshape(-1, 128)
    n_dense, n_real = dense.sum(1), real.sum(1)
    empty = int((n_dense == 0).sum())
    full = int((n_dense == n_real).sum())
    return empty, full, dense.shape[0] - empty - full


def assert_bundles_equal(got, want, what):
    assert sorted(got) == sorted(want)
    for k in want:
        assert torch.equal(got[k], want[k]), (what, k, float((got[k] - want[k]).abs().max()))


def render_counted(render, model, samples_per_ray, rays):
    """render() under the profiling hook: (its result, tiles the library skipped)."""
    from nerfmeshes_amd import hip_ops
    torch.cuda.synchronize()
    hip_ops.mlp_profile_enable(True)
    try:
        hip_ops.mlp_profile_read()
        out = render()
        skipped = hip_ops.mlp_profile_read_skipped(model, rays * samples_per_ray)[3]
    finally:
        hip_ops.mlp_profile_enable(False)
    return out, skipped


@pytest.fixture(scope="module")
def scene():
    """The benchmark's networks, the test rays and the public path's results on them (computed once, never modified)."""
    from nerfmeshes_amd import hip_ops
    w = S.make_scene_weights(**MLP_KW)
    coarse, fine = hip_ops.HipMLP(w, MLP_KW, _dev()), hip_ops.HipMLP(w, MLP_KW, _dev())
    o, d = _rays()
    u_c, u_f = _u(64, 128)
    cb, fb, sig_c, sig_f = public_path(coarse, fine, o, d, u_c, u_f)
    return dict(coarse=coarse, fine=fine, o=o, d=d, u_c=u_c, u_f=u_f, cb=cb, fb=fb, sig_c=sig_c, sig_f=sig_f)


def test_scene_render_is_bit_equal_and_skips_exactly_the_empty_tiles(scene):
    from nerfmeshes_amd import hip_ops
    s = scene
    near, far = _bounds()
    classes_c, classes_f = tile_classes(s["sig_c"]), tile_classes(s["sig_f"])
    print("coarse tiles (empty, full, mixed):", classes_c, " fine:", classes_f)
    assert sum(classes_c) == 257 * 4 and sum(classes_f) == 257 * 12
    assert min(classes_c) > 0 and min(classes_f) > 0        # empty, full and mixed tiles are all present
    (cb, fb), skipped = render_counted(lambda: hip_ops.render_rays(s["coarse"], s["fine"], s["o"], s["d"], near, far, s["u_c"], s["u_f"]),
                                       s["coarse"], 64 + 192, RAYS)
    print("skipped tiles:", skipped, "of", 257 * 16)
    assert_bundles_equal(cb, s["cb"], "coarse")
    assert_bundles_equal(fb, s["fb"], "fine")
    assert skipped == classes_c[0] + classes_f[0]
    assert float(fb["acc_map"].max()) > 0.1                  # not a comparison of zeros


def test_render_view_equals_render_rays(scene):
    from nerfmeshes_amd import hip_ops
    s = scene
    near, far = _bounds()
    view = hip_ops.make_view(S.orbit_poses(1)[0], SIDE, SIDE, S.LEGO_FOCAL_800)
    (cb, fb), skipped = render_counted(lambda: hip_ops.render_view(s["coarse"], s["fine"], view, near, far, s["u_c"], s["u_f"], first=FIRST, count=RAYS),
                                       s["coarse"], 64 + 192, RAYS)
    assert_bundles_equal(cb, s["cb"], "coarse")
    assert_bundles_equal(fb, s["fb"], "fine")
    assert skipped == tile_classes(s["sig_c"])[0] + tile_classes(s["sig_f"])[0]


def test_coarse_only(scene):
    from nerfmeshes_amd import hip_ops
    s = scene
    near, far = _bounds()
    (cb, fb), skipped = render_counted(lambda: hip_ops.render_rays(s["coarse"], None, s["o"], s["d"], near, far, s["u_c"], None),
                                       s["coarse"], 64, RAYS)
    assert fb is None
    assert_bundles_equal(cb, s["cb"], "coarse")
    assert skipped == tile_classes(s["sig_c"])[0]


def test_sample_counts_that_are_no_multiple_of_16_keep_linear_order(scene):
    """60 coarse samples: tiles of 128 consecutive samples (the 160 of the fine pass are ray tiles again)."""
    from nerfmeshes_amd import hip_ops
    s = scene
    near, far = _bounds()
    u_c, u_f = _u(60, 100)
    cb_w, fb_w, sig_c, sig_f = public_path(s["coarse"], s["fine"], s["o"], s["d"], u_c, u_f)
    (cb, fb), skipped = render_counted(lambda: hip_ops.render_rays(s["coarse"], s["fine"], s["o"], s["d"], near, far, u_c, u_f),
                                       s["coarse"], 60 + 160, RAYS)
    assert_bundles_equal(cb, cb_w, "coarse")
    assert_bundles_equal(fb, fb_w, "fine")
    classes_c, classes_f = tile_classes(sig_c), tile_classes(sig_f)
    assert sum(classes_c) == -(-RAYS * 60 // 128) and sum(classes_f) == 257 * 10
    assert classes_c[0] > 0 and classes_f[0] > 0
    assert skipped == classes_c[0] + classes_f[0]


@pytest.mark.parametrize("bias", [-1.0, 1.0])
def test_all_tiles_empty_and_no_tile_empty(bias):
    from nerfmeshes_amd import hip_ops
    rays = 203
    w = S.make_mlp_weights(2, density_gain=1.0, density_bias=bias, **MLP_KW)
    coarse, fine = hip_ops.HipMLP(w, MLP_KW, _dev()), hip_ops.HipMLP(w, MLP_KW, _dev())
    o, d = _rays(rays)
    u_c, u_f = _u(64, 128)
    near, far = _bounds()
    cb_w, fb_w, sig_c, sig_f = public_path(coarse, fine, o, d, u_c, u_f)
    tiles = 26 * (4 + 12)
    want_empty = tiles if bias < 0 else 0
    assert tile_classes(sig_c)[0] + tile_classes(sig_f)[0] == want_empty
    (cb, fb), skipped = render_counted(lambda: hip_ops.render_rays(coarse, fine, o, d, near, far, u_c, u_f), coarse, 64 + 192, rays)
    assert_bundles_equal(cb, cb_w, "coarse")
    assert_bundles_equal(fb, fb_w, "fine")
    assert skipped == want_empty
    if bias < 0:
        assert not cb["rgb_map"].any() and not fb["rgb_map"].any()      # exactly zero: the skipped colours are finite


def test_8x128_handle():
    from nerfmeshes_amd import hip_ops
    w, kw = S.make_smooth_scene_weights("fern_8x128")
    coarse, fine = hip_ops.HipMLP(w, kw, _dev()), hip_ops.HipMLP(w, kw, _dev())
    rays = 515
    o, d = _rays(rays)
    u_c, u_f = _u(64, 128)
    near, far = _bounds()
    cb_w, fb_w, sig_c, sig_f = public_path(coarse, fine, o, d, u_c, u_f)
    (cb, fb), skipped = render_counted(lambda: hip_ops.render_rays(coarse, fine, o, d, near, far, u_c, u_f), coarse, 64 + 192, rays)
    assert_bundles_equal(cb, cb_w, "coarse")
    assert_bundles_equal(fb, fb_w, "fine")
    classes_c, classes_f = tile_classes(sig_c), tile_classes(sig_f)
    print("8x128 coarse tiles (empty, full, mixed):", classes_c, " fine:", classes_f)
    assert classes_c[0] + classes_f[0] > 0 and classes_c[2] + classes_f[2] > 0
    assert skipped == classes_c[0] + classes_f[0]


@pytest.mark.parametrize("which", ["tiny_4x64", "bf16x3"])
def test_families_without_the_skip_evaluate_every_tile(which):
    """mlp_kernel<64, ...> and the bf16x3 kernel ignore the flag: the same bits as the public path, nothing skipped."""
    from nerfmeshes_amd import hip_ops
    if which == "bf16x3":
        w, kw, prec = S.make_scene_weights(**MLP_KW), MLP_KW, "bf16x3"
    else:
        (w, kw), prec = S.make_smooth_scene_weights(which), "f32"
    coarse, fine = hip_ops.HipMLP(w, kw, _dev(), precision=prec), hip_ops.HipMLP(w, kw, _dev(), precision=prec)
    rays = 515
    o, d = _rays(rays)
    u_c, u_f = _u(64, 128)
    near, far = _bounds()
    cb_w, fb_w, sig_c, sig_f = public_path(coarse, fine, o, d, u_c, u_f)
    assert tile_classes(sig_c)[0] + tile_classes(sig_f)[0] > 0           # there would be tiles to skip
    (cb, fb), skipped = render_counted(lambda: hip_ops.render_rays(coarse, fine, o, d, near, far, u_c, u_f), coarse, 64 + 192, rays)
    assert_bundles_equal(cb, cb_w, "coarse")
    assert_bundles_equal(fb, fb_w, "fine")
    assert skipped == 0


def test_eval_rays_still_writes_every_colour(scene):
    """The public entry points never skip: eval_rays' rgb on scene rays (most of whose samples have no density) is what
    sample_points computes for the same points, and no colour is the placeholder zero."""
    from nerfmeshes_amd import hip_ops
    s = scene
    near, far = _bounds()
    t = hip_ops.coarse_intervals(s["u_c"], near, far, RAYS)
    rad = s["coarse"].eval_rays(s["o"], s["d"], t)
    pts = s["o"] + s["d"][:, None, :] * t[..., None]                    # two roundings, as the kernel's ray-mode prologue
    ref = s["coarse"].sample_points(pts, s["d"][:, None, :])
    assert torch.equal(rad, ref)
    assert tile_classes(rad[..., 3])[0] > 0
    assert float(rad[..., :3].min()) > 0.0                              # a sigmoid, never the skip's 0
