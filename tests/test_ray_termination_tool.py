"""tests/tools/ray_termination_count.py (CPU only): the kernel's conservative rule for ray termination never calls a tile dead
on which the compositor's fp32 transmittance is not exactly 0.

The rule: per sample c = log2f((1 - alpha) + 1e-10f + 2^-23) + 2^-8, att[k] = the sum over the ray's depth slots 0..k, tile
(block, k) dead when att[k - 1] < -160 on all 8 rays.  Checked on oracle-rendered rays of the benchmark scene (32 blocks of 8
adjacent rays per view, spread evenly) and on synthetic sequences placed where alpha rounds to 1.0f."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import ray_termination_count as RT  # noqa: E402


# bench.py's orbit of 4 poses: the warm-up view and view 2; and the pose where most dies (view 2 of an orbit of 3: 42 % of the tile time)
@pytest.mark.parametrize("views,view,expect_dead", [(4, 0, False), (4, 2, False), (3, 2, True)])
def test_rule_implies_zero_transmittance_on_scene_rays(views, view, expect_dead):
    rec = RT.count_view(view, views, 32)          # count_view runs check_rule_is_safe on both passes
    for name in ("coarse", "fine"):
        r = rec[name]
        print(views, view, name, r["dead_exact"], r["dead_rule"], r["tiles"])
        assert r["dead_rule"] <= r["dead_exact"] <= r["tiles"]
        assert r["dead_exact_share_per_depth_slot"][0] == 0.0           # nothing is in front of slot 0
    assert 0.0 <= rec["time_share_rule"] <= rec["time_share_exact"] < 1.0
    if expect_dead:
        assert rec["fine"]["dead_rule"] > 0.2 * rec["fine"]["tiles"] and rec["time_share_rule"] > 0.25


def test_rule_on_the_alpha_rounding_boundary():
    """x = sigma * dist in [16.6, 17.4]: expf(-x) is around 2^-24, so 1 - alpha is 0 or one quantum (2^-24) from sample to sample
    and log2 of the factor jumps between -33.2 and -24.  Mixed with transparent stretches of random length in front."""
    rng = np.random.Generator(np.random.PCG64(7))
    rays, samples = 4096, 192
    x = rng.uniform(16.6, 17.4, (rays, samples)).astype(np.float32)
    start = rng.integers(0, samples, rays)
    x[np.arange(samples)[None, :] < start[:, None]] = 0.0
    x[rng.random((rays, samples)) < 0.3] = 0.0
    t = np.broadcast_to(np.arange(samples, dtype=np.float32)[None], (rays, samples))
    f = RT.factors(x, t, np.ones(rays, dtype=np.float32))             # dist = 1: sigma is x (the last sample's dist is 1e10)
    one_minus_alpha = f[:, :-1][x[:, :-1] > 0] - np.float32(1e-10)
    assert (one_minus_alpha <= np.float32(2.0 ** -23)).all() and len(np.unique(f[:, :-1][x[:, :-1] > 0])) >= 2    # both roundings occur
    rule, exact = RT.check_rule_is_safe(f)
    print("boundary sequences:", rule, "tiles dead by the rule,", exact, "exactly, of", rays // 8 * samples // 16)
    assert 0 < rule <= exact


def test_nan_sigma_is_no_density():
    sigma = np.full((8, 32), np.nan, dtype=np.float32)
    t = np.broadcast_to(np.linspace(2, 6, 32, dtype=np.float32)[None], (8, 32))
    f = RT.factors(sigma, t, np.ones(8, dtype=np.float32))
    assert (f == 1.0).all()
    exact, rule = RT.dead_tiles(f)
    assert not exact.any() and not rule.any()
