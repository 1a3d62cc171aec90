"""The skipping render kernel draws its tiles from a device counter (MI355X; DESIGN.md 3.9, `MlpArgs::tile_queue`).

`mlp_kernel3<..., SKIP>` is launched with one workgroup per resident slot; a workgroup's first tile is its block index, every
further one is claimed with an atomicAdd on a counter word of the handle that is zeroed in stream order in front of the launch.
Which workgroup evaluates a tile must not matter: as in test_gpu_render_skip.py the reference of every case is the public path

    coarse_intervals -> eval_rays -> composite -> sample_pdf -> eval_rays -> composite

which neither skips nor queues, all six maps of both bundles must be equal BIT FOR BIT, and the tiles the library reports as
skipped must be exactly the all-empty tiles of that path's sigma.  The ray counts are chosen around the grid size (CUs workgroups
for the 8x256 network): fewer tiles than workgroups, exactly as many, and more (the queue is drawn from)."""
import numpy as np
import pytest
import torch

from nerfmeshes_amd import synthetic as S
from tests.test_gpu_render_skip import (FIRST, MLP_KW, SIDE, _bounds, _dev, _rays, _u, assert_bundles_equal, public_path,
                                        render_counted, tile_classes)

pytestmark = pytest.mark.gpu


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ragged():
    return 8 * (_cus() + 1) - 3         # CUs + 1 ray blocks, the last one with 5 of its 8 rays


def _pair(w, kw):
    from nerfmeshes_amd import hip_ops
    return hip_ops.HipMLP(w, kw, _dev()), hip_ops.HipMLP(w, kw, _dev())


def _check(coarse, fine, rays, nc, nf, want=None, expect_skips=None):
    """One counted render against the public path on the same handles.  Returns the reference (for reuse)."""
    from nerfmeshes_amd import hip_ops
    o, d = _rays(rays)
    u_c, u_f = _u(nc, nf)
    near, far = _bounds()
    if want is None:
        want = public_path(coarse, fine, o, d, u_c, u_f)
    cb_w, fb_w, sig_c, sig_f = want
    empty = tile_classes(sig_c)[0] + (tile_classes(sig_f)[0] if fine is not None else 0)
    total = sum(tile_classes(sig_c)) + (sum(tile_classes(sig_f)) if fine is not None else 0)
    per_ray = nc + (nc + nf if fine is not None else 0)
    (cb, fb), skipped = render_counted(lambda: hip_ops.render_rays(coarse, fine, o, d, near, far, u_c, u_f if fine is not None else None),
                                       coarse, per_ray, rays)
    print(f"{rays} rays, {nc}+{nf}: {total} tiles, {empty} empty, {skipped} skipped")
    assert_bundles_equal(cb, cb_w, "coarse")
    if fine is not None:
        assert_bundles_equal(fb, fb_w, "fine")
    assert skipped == (empty if expect_skips is None else expect_skips)
    return want


@pytest.fixture(scope="module")
def scene():
    """The benchmark's networks and the public path's results on the ragged ray set (computed once, never modified)."""
    w = S.make_scene_weights(**MLP_KW)
    coarse, fine = _pair(w, MLP_KW)
    rays = _ragged()
    o, d = _rays(rays)
    u_c, u_f = _u(64, 128)
    want = public_path(coarse, fine, o, d, u_c, u_f)
    return dict(coarse=coarse, fine=fine, rays=rays, o=o, d=d, u_c=u_c, u_f=u_f, want=want)


def test_fewer_tiles_than_workgroups(scene):
    """13 rays: two ray blocks (the second with 5 rays), 8 + 24 tiles -- every workgroup's first claim is past the end."""
    want = _check(scene["coarse"], scene["fine"], 13, 64, 128)
    assert sum(tile_classes(want[2])) == 8 and sum(tile_classes(want[3])) == 24


def test_exactly_one_tile_per_resident_workgroup(scene):
    """8 CUs / 4 rays x 64 coarse samples = CUs tiles: wg_iters == grid."""
    rays = 8 * _cus() // 4
    want = _check(scene["coarse"], None, rays, 64, 0)
    assert sum(tile_classes(want[2])) == _cus()


def test_more_tiles_than_workgroups_ragged(scene):
    s = scene
    sig_c, sig_f = s["want"][2], s["want"][3]
    assert sum(tile_classes(sig_c)) == 4 * (_cus() + 1) and sum(tile_classes(sig_f)) == 12 * (_cus() + 1)
    assert min(tile_classes(sig_c)) > 0 and min(tile_classes(sig_f)) > 0     # empty, full and mixed tiles: unequal tile times
    _check(s["coarse"], s["fine"], s["rays"], 64, 128, want=s["want"])
    assert float(s["want"][1]["acc_map"].max()) > 0.1                        # not a comparison of zeros


def test_linear_tile_order(scene):
    """60 + 100 samples: the coarse pass runs tiles of 128 consecutive samples (`ray_tiles == 0`), the 160-sample fine pass ray tiles."""
    want = _check(scene["coarse"], scene["fine"], scene["rays"], 60, 100)
    assert sum(tile_classes(want[2])) == -(-scene["rays"] * 60 // 128) > _cus()


@pytest.mark.parametrize("bias", [-1.0e3, 1.0e3])
def test_all_empty_and_no_empty_network(bias):
    """fc_alpha.bias = -1e3: every tile is empty and restarts the weight stream for a CLAIMED next tile; +1e3: none does."""
    w = S.make_mlp_weights(2, **MLP_KW)
    w["fc_alpha.bias"] = np.full_like(w["fc_alpha.bias"], bias)
    coarse, fine = _pair(w, MLP_KW)
    want = _check(coarse, fine, _ragged(), 64, 128)
    tiles = 16 * (_cus() + 1)
    assert tile_classes(want[2])[0] + tile_classes(want[3])[0] == (tiles if bias < 0 else 0)
    if bias < 0:
        assert not want[0]["rgb_map"].any() and not want[1]["rgb_map"].any()


def test_render_view(scene):
    from nerfmeshes_amd import hip_ops
    s = scene
    near, far = _bounds()
    view = hip_ops.make_view(S.orbit_poses(1)[0], SIDE, SIDE, S.LEGO_FOCAL_800)
    (cb, fb), skipped = render_counted(lambda: hip_ops.render_view(s["coarse"], s["fine"], view, near, far, s["u_c"], s["u_f"],
                                                                   first=FIRST, count=s["rays"]), s["coarse"], 64 + 192, s["rays"])
    assert_bundles_equal(cb, s["want"][0], "coarse")
    assert_bundles_equal(fb, s["want"][1], "fine")
    assert skipped == tile_classes(s["want"][2])[0] + tile_classes(s["want"][3])[0]


def test_8x128_with_10_frequencies_queues():
    """The 128-wide skip kernel: two workgroups per CU are resident, so 2 CUs + 1 ray blocks draw from the queue in both passes."""
    w, kw = S.make_smooth_scene_weights("fern_8x128")
    coarse, fine = _pair(w, kw)
    want = _check(coarse, fine, 8 * (2 * _cus() + 1) - 3, 64, 128)
    assert tile_classes(want[2])[0] + tile_classes(want[3])[0] > 0


def test_8x128_with_6_frequencies_runs_as_before():
    """That shape has no skip kernel: the plain kernel with its static stride, nothing skipped, the same bits."""
    kw = dict(MLP_KW, hidden_size=128, num_encoding_fn_xyz=6)
    coarse, fine = _pair(S.make_mlp_weights(3, density_gain=30.0, density_bias=-1.0, **kw), kw)   # sigma in about [-1.1, 0.6]
    want = _check(coarse, fine, _ragged(), 64, 128, expect_skips=0)
    assert tile_classes(want[2])[0] + tile_classes(want[3])[0] > 0           # there would be tiles to skip


def test_counter_reuse(scene):
    """Three renders in a row on the same pair of handles, then one under the profiling hook: the counter starts from zero each time."""
    from nerfmeshes_amd import hip_ops
    s = scene
    near, far = _bounds()
    for turn in range(3):
        cb, fb = hip_ops.render_rays(s["coarse"], s["fine"], s["o"], s["d"], near, far, s["u_c"], s["u_f"])
        assert_bundles_equal(cb, s["want"][0], f"coarse, run {turn}")
        assert_bundles_equal(fb, s["want"][1], f"fine, run {turn}")
    _check(s["coarse"], s["fine"], s["rays"], 64, 128, want=s["want"])


def test_interleaved_renders(scene):
    """Two renders with different ray counts queued back to back, no synchronisation between them: each equals its own reference."""
    from nerfmeshes_amd import hip_ops
    s = scene
    near, far = _bounds()
    small = _cus() * 8 // 4 + 11
    o2, d2 = _rays(small)
    want2 = public_path(s["coarse"], s["fine"], o2, d2, s["u_c"], s["u_f"])
    torch.cuda.synchronize()
    cb1, fb1 = hip_ops.render_rays(s["coarse"], s["fine"], s["o"], s["d"], near, far, s["u_c"], s["u_f"])
    cb2, fb2 = hip_ops.render_rays(s["coarse"], s["fine"], o2, d2, near, far, s["u_c"], s["u_f"])
    cb3, fb3 = hip_ops.render_rays(s["coarse"], s["fine"], s["o"], s["d"], near, far, s["u_c"], s["u_f"])
    torch.cuda.synchronize()
    for got, want, what in ((cb1, s["want"][0], "first coarse"), (fb1, s["want"][1], "first fine"), (cb2, want2[0], "second coarse"),
                            (fb2, want2[1], "second fine"), (cb3, s["want"][0], "third coarse"), (fb3, s["want"][1], "third fine")):
        assert_bundles_equal(got, want, what)
