"""Ray termination in the render path's network launches (MI355X; DESIGN.md 3.9, `MlpArgs::att`).

In a render call of at least two 8-ray blocks per resident workgroup, `mlp_kernel3<256, ..., SKIP>` keeps, per ray and depth
slot, an upper bound of log2 of the product of the compositor's transmittance factors, claims its tiles slot-major and does not
evaluate a tile whose 8 rays all have that bound below -160 in front of it: the compositor's fp32 transmittance is 0 there, so
the tile's weights are +0 whatever the network gives.  Nothing an entry point returns may change.  As in
test_gpu_render_skip.py the reference of every case is the public path on the same handles, which neither skips nor terminates,

    coarse_intervals -> eval_rays -> composite -> sample_pdf -> eval_rays -> composite

and all six maps of both bundles must be equal BIT FOR BIT.  The tiles the library reports as terminated must be tiles at whose
first sample that path's transmittance is exactly 0 on every ray (counted with tests/tools/ray_termination_count.py), and the
executed FLOPs it reports must be the full count minus what its two tile counts stand for.

The scene run: view 2 of bench.py's default orbit of 4 poses, the 16 CUs + 3 consecutive pixels from pixel 400 * 800 on (the
middle rows of the image: rays into the object, 290 of their 8208 tiles lie behind transmittance 0 at 256 CUs)."""
import os
import sys

import numpy as np
import pytest
import torch

from nerfmeshes_amd import synthetic as S
from tests.test_gpu_render_skip import FIRST, MLP_KW, NEAR, FAR, SIDE, assert_bundles_equal, tile_classes

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import ray_termination_count as RT  # noqa: E402

pytestmark = pytest.mark.gpu

BENCH_VIEWS, BENCH_VIEW = 4, 2


def _dev():
    return torch.device("cuda")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ragged():
    return 8 * 2 * _cus() + 5           # 2 CUs + 1 ray blocks, the last one with 5 of its 8 rays


def _pose(view=BENCH_VIEW):
    return S.orbit_poses(BENCH_VIEWS)[view]


def _rays(count, first=FIRST):
    from nerfmeshes_amd import hip_ops
    o, d = hip_ops.ray_bundle(_pose(), SIDE, SIDE, S.LEGO_FOCAL_800, first, count, device=_dev())
    return o[None].contiguous(), d


def _bounds():
    return torch.tensor([NEAR], device=_dev()), torch.tensor([FAR], device=_dev())


def _u(nc=64, nf=128):
    return torch.linspace(0.0, 1.0, nc).to(_dev()), torch.linspace(0.0, 1.0, nf).to(_dev())


def _pair(w, kw):
    from nerfmeshes_amd import hip_ops
    return hip_ops.HipMLP(w, kw, _dev()), hip_ops.HipMLP(w, kw, _dev())


def public_path(coarse, fine, o, d):
    """Both bundles from the public entry points, and per pass (sigma, t) for the tile counts."""
    from nerfmeshes_amd import hip_ops
    near, far = _bounds()
    u_c, u_f = _u()
    t_c = hip_ops.coarse_intervals(u_c, near, far, d.shape[0])
    rad_c = coarse.eval_rays(o, d, t_c)
    cb = hip_ops.composite(rad_c, t_c, d)
    if fine is None:
        return dict(cb=cb, fb=None, passes=[(rad_c[..., 3], t_c)], d=d)
    t_f = hip_ops.sample_pdf(t_c, cb["weights"], u_f)
    rad_f = fine.eval_rays(o, d, t_f)
    fb = hip_ops.composite(rad_f, t_f, d)
    return dict(cb=cb, fb=fb, passes=[(rad_c[..., 3], t_c), (rad_f[..., 3], t_f)], d=d)


def dead_tiles(want):
    """(exact, rule) dead tiles of the public path's sigma, both passes: the CPU tool's count.  The padding rays of the last ray
    block have no transmittance (factor 0)."""
    norm = want["d"].norm(p=2, dim=-1).cpu().numpy()
    exact = rule = 0
    for sigma, t in want["passes"]:
        f = RT.factors(sigma.cpu().numpy(), t.cpu().numpy(), norm)
        f = np.pad(f, (((0, (-f.shape[0]) % 8)), (0, 0)))
        RT.check_rule_is_safe(f)
        e, r = RT.dead_tiles(f)
        exact, rule = exact + int(e.sum()), rule + int(r.sum())
    return exact, rule


def counted(render):
    """render() under the profiling hook: (its result, executed flops, skipped tiles, terminated tiles)."""
    from nerfmeshes_amd import hip_ops
    torch.cuda.synchronize()
    hip_ops.mlp_profile_enable(True)
    try:
        hip_ops.mlp_profile_read()
        out = render()
        _, _, flops, skipped, terminated = hip_ops.mlp_profile_read_tiles()
    finally:
        hip_ops.mlp_profile_enable(False)
    return out, flops, skipped, terminated


def check(coarse, fine, want, render, what=""):
    """One counted render against `want`: equal maps, the flop identity, terminated <= exact dead tiles.  Returns the counts."""
    (cb, fb), flops, skipped, terminated = counted(render)
    assert_bundles_equal(cb, want["cb"], what + " coarse")
    if fine is not None:
        assert_bundles_equal(fb, want["fb"], what + " fine")
    samples = sum(int(s.numel()) for s, _ in want["passes"])
    full, density = coarse.flops_per_sample(), coarse.flops_per_sample(True)
    tile = coarse.kernel_variant()[1] * 16
    exact, rule = dead_tiles(want)
    empty = sum(tile_classes(s)[0] for s, _ in want["passes"])
    print(f"{what}: {samples // tile} tiles, {empty} empty, dead {exact} exact / {rule} by the rule | skipped {skipped}, terminated {terminated}")
    assert samples * full - int(round(flops)) == skipped * tile * (full - density) + terminated * tile * full
    assert terminated <= exact
    assert skipped <= empty
    return skipped, terminated, exact, rule, empty


def _render(coarse, fine, o, d):
    from nerfmeshes_amd import hip_ops
    near, far = _bounds()
    u_c, u_f = _u()
    return lambda: hip_ops.render_rays(coarse, fine, o, d, near, far, u_c, u_f if fine is not None else None)


@pytest.fixture(scope="module")
def scene():
    """The benchmark's networks on the scene run and the public path's results (computed once, never modified)."""
    coarse, fine = _pair(S.make_scene_weights(**MLP_KW), MLP_KW)
    rays = 16 * _cus() + 3
    o, d = _rays(rays)
    return dict(coarse=coarse, fine=fine, rays=rays, o=o, d=d, want=public_path(coarse, fine, o, d))


def test_opaque_network_ragged_ray_count():
    """fc_alpha.bias = +1e3: alpha is 1.0f from the first sample on, every ray is dead within depth slot 0 and every tile behind
    slot 0 is dead (3 of 4 coarse, 11 of 12 fine); the last ray block has 5 rays."""
    w = S.make_mlp_weights(2, density_bias=1.0e3, **MLP_KW)
    coarse, fine = _pair(w, MLP_KW)
    o, d = _rays(_ragged())
    want = public_path(coarse, fine, o, d)
    blocks = 2 * _cus() + 1
    exact, rule = dead_tiles(want)
    assert exact == rule == blocks * (3 + 11)
    skipped, terminated, *_ = check(coarse, fine, want, _render(coarse, fine, o, d), "opaque")
    assert 0 < terminated <= exact
    assert float(want["fb"]["acc_map"].min()) > 0.99


def test_scene_run_of_view_2(scene):
    s = scene
    skipped, terminated, exact, rule, empty = check(s["coarse"], s["fine"], s["want"], _render(s["coarse"], s["fine"], s["o"], s["d"]), "scene")
    assert rule > 0 and terminated > 0
    assert float(s["want"]["fb"]["acc_map"].max()) > 0.1


def test_transparent_network_terminates_nothing():
    w = S.make_mlp_weights(2, density_bias=-1.0e3, **MLP_KW)
    coarse, fine = _pair(w, MLP_KW)
    o, d = _rays(_ragged())
    want = public_path(coarse, fine, o, d)
    skipped, terminated, exact, rule, empty = check(coarse, fine, want, _render(coarse, fine, o, d), "transparent")
    assert terminated == 0 and exact == 0
    assert skipped == empty == 16 * (2 * _cus() + 1)


def test_below_the_threshold_nothing_changes(scene):
    """2051 rays are 257 ray blocks, fewer than two per workgroup: block-major order, no table, the skipped count of today."""
    s = scene
    o, d = _rays(2051)
    want = public_path(s["coarse"], s["fine"], o, d)
    skipped, terminated, exact, rule, empty = check(s["coarse"], s["fine"], want, _render(s["coarse"], s["fine"], o, d), "2051 rays")
    assert terminated == 0
    assert skipped == empty


def test_render_view_and_coarse_only(scene):
    from nerfmeshes_amd import hip_ops
    s = scene
    near, far = _bounds()
    u_c, u_f = _u()
    view = hip_ops.make_view(_pose(), SIDE, SIDE, S.LEGO_FOCAL_800)
    _, terminated, *_ = check(s["coarse"], s["fine"], s["want"],
                              lambda: hip_ops.render_view(s["coarse"], s["fine"], view, near, far, u_c, u_f, first=FIRST, count=s["rays"]), "render_view")
    assert terminated > 0
    want_c = dict(s["want"], fb=None, passes=s["want"]["passes"][:1])
    check(s["coarse"], None, want_c, _render(s["coarse"], None, s["o"], s["d"]), "coarse only")


def test_8x128_handle_keeps_its_kernel():
    """The 128-wide skip kernel has no ray termination (its register budget): 4 CUs + 1 ray blocks, two per
    resident workgroup, render as before."""
    w, kw = S.make_smooth_scene_weights("fern_8x128")
    coarse, fine = _pair(w, kw)
    o, d = _rays(8 * (4 * _cus() + 1) - 3)
    want = public_path(coarse, fine, o, d)
    skipped, terminated, exact, rule, empty = check(coarse, fine, want, _render(coarse, fine, o, d), "8x128")
    assert terminated == 0 and skipped == empty > 0


def test_three_renders_of_different_sizes_back_to_back(scene):
    """No synchronisation in between: every launch zeroes the part of the table it uses, no verdict carries over."""
    from nerfmeshes_amd import hip_ops
    s = scene
    near, far = _bounds()
    u_c, u_f = _u()
    w = S.make_mlp_weights(2, density_bias=1.0e3, **MLP_KW)
    opaque_c, opaque_f = _pair(w, MLP_KW)
    sizes = (_ragged(), 8 * 3 * _cus(), 2051)
    rays = [_rays(n) for n in sizes]
    wants = [public_path(opaque_c, opaque_f, *rays[0]), public_path(s["coarse"], s["fine"], *rays[1]), public_path(s["coarse"], s["fine"], *rays[2])]
    torch.cuda.synchronize()
    got = [hip_ops.render_rays(opaque_c, opaque_f, rays[0][0], rays[0][1], near, far, u_c, u_f),     # leaves a table full of dead rays
           hip_ops.render_rays(s["coarse"], s["fine"], rays[1][0], rays[1][1], near, far, u_c, u_f),
           hip_ops.render_rays(s["coarse"], s["fine"], rays[2][0], rays[2][1], near, far, u_c, u_f)]
    torch.cuda.synchronize()
    for i, ((cb, fb), want) in enumerate(zip(got, wants)):
        assert_bundles_equal(cb, want["cb"], f"render {i} coarse")
        assert_bundles_equal(fb, want["fb"], f"render {i} fine")


def test_switched_off_by_the_environment(scene, monkeypatch):
    s = scene
    monkeypatch.setenv("NM_RAY_TERMINATION", "0")
    skipped, terminated, exact, rule, empty = check(s["coarse"], s["fine"], s["want"], _render(s["coarse"], s["fine"], s["o"], s["d"]), "switched off")
    assert terminated == 0 and skipped == empty
