"""The render path's skip / queue / termination kernels over the configurations the public API reaches (MI355X).

test_gpu_render_skip.py, test_gpu_tile_queue.py and test_gpu_ray_termination.py run `mlp_kernel3<..., SKIP>` on essentially one
configuration (8x256, F_xyz 10, skip at layer 4, 64 + 128 samples, scalar bounds, one origin, default options).  Here the same
check -- tests/render_cases.py: `check_render` against the public path, BIT FOR BIT, with the tile counts bounded by what the CPU
tool counts on that path's sigma and t -- runs over

  (a) every instance and trunk layout: both 256-wide instances, 2 to 10 layers, skip layers at other places, the 128-wide ones;
  (b) every render option, with the table (T + 5 rays) and with the queue alone;
  (c) sample geometry: 1, 2, 5, 33 depth slots, linear passes in front of and behind a table pass, the long compositor;
  (d) ray counts around T = 16 CUs, the smallest at which the table is used;
  (e) tiles in the band where the transmittance is denormal or just 0: the only place where the rule's margin changes bits;
  (f) a ray with an infinite origin, and a network whose sigma is NaN or infinite;
  (g) replay from a captured graph with the table.

Every case asserts ON THE PUBLIC PATH'S RESULTS that it has the tile kinds it is about (and acc_map.max() > 0.1: no comparison of
zeros) before it looks at the render path.  Each prints (tiles, empty, skipped, exact, rule, terminated)."""
import numpy as np
import pytest
import torch

from nerfmeshes_amd import synthetic as S
from tests import render_cases as RC
from tests.render_cases import MLP_KW

pytestmark = pytest.mark.gpu


def _kw(num_layers, hidden_size, fx, skip_step):
    return dict(num_layers=num_layers, hidden_size=hidden_size, skip_step=skip_step, num_encoding_fn_xyz=fx, num_encoding_fn_dir=4)


# (a): name -> (network, its skip mask (bit i: layers_xyz[i] takes the encoding again), shift and gain of render_cases.smooth_weights,
# kind).  shift is the 0.6 quantile of the band-limited draw's raw fc_alpha output along the test rays and gain 2000 / its standard
# deviation, both taken from the CPU oracle: about 40 % of the volume is solid, and a ray that enters it is dead within a few samples.
NETWORKS = {
    "8x256_F6_skip4": (_kw(8, 256, 6, 4), 0b10000, -0.02567, 3.5e5, "table"),
    "2x256_F10": (_kw(2, 256, 10, 4), 0, 0.07258, 8.3e4, "table"),                    # one trunk layer, no skip
    "3x256_F6_skip1": (_kw(3, 256, 6, 1), 0b10, -0.01394, 9.6e4, "table"),            # the skip layer feeds fc_feat directly
    "5x256_F10_skip2": (_kw(5, 256, 10, 2), 0b100, 0.01628, 4.7e5, "table"),          # 4 is num_layers - 1: only layer 2
    "10x256_F6_skip3": (_kw(10, 256, 6, 3), 0b1001000, -0.002525, 6.6e5, "table"),    # skips at 3 and 6
    "4x128_F10_skip2": (_kw(4, 128, 10, 2), 0b100, 0.05775, 6.1e4, "skip"),           # skip kernel, no table
    "8x128_F6_skip4": (_kw(8, 128, 6, 4), 0b10000, 0.0206, 2.9e5, "plain"),           # no skip kernel for this shape
}


@pytest.fixture(scope="module")
def scene_pair():
    return RC.pair(S.make_scene_weights(**MLP_KW), MLP_KW)


@pytest.fixture(scope="module")
def opaque_pair():
    """Sigma 1e3 at every sample: alpha rounds to 1.0f, every ray is dead within its first depth slot."""
    return RC.pair(RC.constant_sigma(MLP_KW, 1.0e3), MLP_KW)


def _acc_max(want):
    acc = (want["fb"] if want["fb"] is not None else want["cb"])["acc_map"]
    return float(acc[~torch.isnan(acc)].max())


def _pass_tiles(rays, samples):
    return -(-rays // 8) * (samples // 16) if samples % 16 == 0 else -(-rays * samples // 128)


def _render_rays(coarse, fine, o, d, near, far, u_c, u_f, **cfg):
    from nerfmeshes_amd import hip_ops
    return lambda: hip_ops.render_rays(coarse, fine, o, d, near, far, u_c, u_f, **cfg)


# ---- (a) instances and depths ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(NETWORKS))
def test_instances_and_trunk_layouts(name):
    kw, mask, shift, gain, kind = NETWORKS[name]
    assert RC.skip_mask(kw) == mask
    coarse, fine = RC.pair(RC.smooth_weights(kw, shift, gain), kw)
    rays = RC.table_rays() + 5
    o, d = RC.scene_rays(rays)
    near, far = RC.bounds()
    u_c, u_f = RC.u_pair(64, 128)
    want = RC.public_path(coarse, fine, o, d, near, far, u_c, u_f)
    tiles, empty, full, mixed, exact, rule = RC.tile_counts(want)
    print(f"{name}: (empty, full, mixed) = ({empty}, {full}, {mixed})")
    assert tiles == _pass_tiles(rays, 64) + _pass_tiles(rays, 192)
    assert min(empty, full, mixed) > 0 and rule > 0           # every kind of tile, and tiles behind dead rays
    assert _acc_max(want) > 0.1
    got = RC.check_render(coarse, fine, want, _render_rays(coarse, fine, o, d, near, far, u_c, u_f), name, skip_kernel=kind != "plain")
    if kind == "table":
        assert got["terminated"] > 0
    else:
        assert got["terminated"] == 0


# ---- (b) render options ----------------------------------------------------------------------------------------------------------
OPTIONS = {
    "white_background": dict(white_background=True),
    "lindisp": dict(lindisp=True),
    "training": dict(training=True),
    "threshold_0": dict(attenuation_threshold=0.0),
    "threshold_1e-2": dict(attenuation_threshold=1e-2),
    "per_ray_bounds": dict(per_ray_bounds=True),
    "per_ray_origins": dict(per_ray_origins=True),
    "all_together": dict(white_background=True, lindisp=True, training=True, attenuation_threshold=1e-2, per_ray_bounds=True,
                         per_ray_origins=True),
}


def _ray_count(size):
    return RC.table_rays() + 5 if size == "table" else RC.queue_rays()


def _per_ray_inputs(rays, per_ray_bounds, per_ray_origins):
    o, d = RC.scene_rays(rays)
    near, far = RC.bounds()
    g = torch.Generator().manual_seed(rays)
    if per_ray_bounds:                                    # (R,) tensors, a jitter of +- 0.1 as in test_render_sweep_vs_oracle
        near = (RC.NEAR + 0.1 * torch.rand(rays, generator=g)).to(RC.dev())
        far = (RC.FAR - 0.1 * torch.rand(rays, generator=g)).to(RC.dev())
    if per_ray_origins:
        o = (o.cpu() + 0.05 * torch.randn(rays, 3, generator=g)).to(RC.dev()).contiguous()
    return o, d, near, far


@pytest.mark.parametrize("size", ["table", "queue"])
@pytest.mark.parametrize("option", list(OPTIONS))
def test_render_options(scene_pair, option, size):
    coarse, fine = scene_pair
    cfg = dict(OPTIONS[option])
    rays = _ray_count(size)
    o, d, near, far = _per_ray_inputs(rays, cfg.pop("per_ray_bounds", False), cfg.pop("per_ray_origins", False))
    u_c, u_f = RC.u_pair(64, 128)
    want = RC.public_path(coarse, fine, o, d, near, far, u_c, u_f, **cfg)
    tiles, empty, full, mixed, exact, rule = RC.tile_counts(want)
    assert tiles == 16 * -(-rays // 8) and _pass_tiles(rays, 64) > RC.cus()
    assert empty > 0 and mixed > 0 and (rule > 0 or size == "queue")
    assert _acc_max(want) > 0.1
    got = RC.check_render(coarse, fine, want, _render_rays(coarse, fine, o, d, near, far, u_c, u_f, **cfg), f"{option}, {size}")
    if size == "table":
        assert got["terminated"] > 0
    else:
        assert got["terminated"] == 0


@pytest.mark.parametrize("size", ["table", "queue"])
@pytest.mark.parametrize("option", ["alone", "all_together"])
def test_render_view_ndc(scene_pair, option, size):
    """NDC rays (ndc_near = 1.0, bounds 0 .. 1) generated in the kernels from a forward-facing pose, over a ragged pixel range,
    against render_rays' reference on the materialised `view_rays`.  (No lindisp: near is 0.)"""
    from nerfmeshes_amd import hip_ops
    coarse, fine = scene_pair
    rays = _ray_count(size)
    first = 250 * RC.SIDE + 3             # rows of that view on which the scene network has empty, solid and dead tiles
    c2w = np.concatenate((np.eye(3, dtype=np.float32), np.array([[0.1], [-0.05], [0.2]], dtype=np.float32)), 1)
    view = hip_ops.make_view(c2w, RC.SIDE, RC.SIDE, S.LEGO_FOCAL_800, ndc_near=1.0)
    o, d = hip_ops.view_rays(view, first, rays, device=RC.dev())
    near, far = RC.bounds(0.0, 1.0)
    cfg = {}
    if option == "all_together":
        cfg = dict(white_background=True, training=True, attenuation_threshold=1e-2)
        g = torch.Generator().manual_seed(rays)
        near = (0.02 * torch.rand(rays, generator=g)).to(RC.dev())
        far = (1.0 - 0.02 * torch.rand(rays, generator=g)).to(RC.dev())
    u_c, u_f = RC.u_pair(64, 128)
    want = RC.public_path(coarse, fine, o, d, near, far, u_c, u_f, **cfg)
    tiles, empty, full, mixed, exact, rule = RC.tile_counts(want)
    assert empty > 0 and mixed > 0 and (rule > 0 or size == "queue")
    assert _acc_max(want) > 0.1
    got = RC.check_render(coarse, fine, want,
                          lambda: hip_ops.render_view(coarse, fine, view, near, far, u_c, u_f, first=first, count=rays, **cfg),
                          f"render_view ndc {option}, {size}")
    if size == "table":
        assert got["terminated"] > 0
    else:
        assert got["terminated"] == 0


# ---- (c) sample geometry ---------------------------------------------------------------------------------------------------------
GEOMETRY = [(16, 0), (16, 16), (32, 48), (8, 8), (60, 100), (64, 464), (48, 470)]


def _geometry(pair_, nc, nf, what):
    coarse, fine = pair_ if nf else (pair_[0], None)
    rays = RC.table_rays() + 5
    o, d = RC.scene_rays(rays)
    near, far = RC.bounds()
    u_c, u_f = RC.u_pair(nc, nf)
    want = RC.public_path(coarse, fine, o, d, near, far, u_c, u_f)
    counts = RC.tile_counts(want)
    passes = [nc] + ([nc + nf] if nf else [])
    assert counts[0] == sum(_pass_tiles(rays, s) for s in passes)
    assert _acc_max(want) > 0.1
    # dead tiles can only be found in a ray-tile pass of at least two depth slots
    closed = sum(-(-rays // 8) * (s // 16 - 1) for s in passes if s % 16 == 0)
    return want, counts, closed, lambda: RC.check_render(coarse, fine, want, _render_rays(coarse, fine, o, d, near, far, u_c, u_f), what)


@pytest.mark.parametrize("nc,nf", GEOMETRY)
def test_sample_geometry_scene(scene_pair, nc, nf):
    want, (tiles, empty, full, mixed, exact, rule), closed, check = _geometry(scene_pair, nc, nf, f"scene {nc}+{nf}")
    assert empty > 0 and mixed > 0
    # dead tiles on the scene need a table pass of more than two depth slots (in two slots a whole block of rays would have to die
    # within the first half of its depth range; the opaque twin below has those); one slot can have none
    assert (rule > 0) == ((nc, nf) in ((32, 48), (60, 100), (64, 464), (48, 470))) and (closed > 0 or exact == 0)
    got = check()
    if closed == 0:
        assert got["terminated"] == 0


@pytest.mark.parametrize("nc,nf", GEOMETRY)
def test_sample_geometry_opaque(opaque_pair, nc, nf):
    """Every ray is dead within depth slot 0, so every ray tile behind slot 0 is dead: blocks * (slots - 1) per ray-tile pass."""
    want, (tiles, empty, full, mixed, exact, rule), closed, check = _geometry(opaque_pair, nc, nf, f"opaque {nc}+{nf}")
    assert empty == 0 and exact == rule == closed
    assert float(want["cb"]["acc_map"].min()) > 0.99
    got = check()
    assert (got["terminated"] > 0) == (closed > 0)


# ---- (d) around the threshold ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("network", ["scene", "opaque"])
@pytest.mark.parametrize("offset", [-8, -3, 0, 8])
def test_ray_counts_around_the_table_threshold(scene_pair, opaque_pair, network, offset):
    """T - 8 rays are one ray block short of two per workgroup: no table.  T - 3 rays are 2 CUs blocks, the last one ragged."""
    coarse, fine = scene_pair if network == "scene" else opaque_pair
    rays = RC.table_rays() + offset
    blocks = -(-rays // 8)
    assert blocks == 2 * RC.cus() + (-1 if offset == -8 else 1 if offset == 8 else 0)
    o, d = RC.scene_rays(rays)
    near, far = RC.bounds()
    u_c, u_f = RC.u_pair(64, 128)
    want = RC.public_path(coarse, fine, o, d, near, far, u_c, u_f)
    tiles, empty, full, mixed, exact, rule = RC.tile_counts(want)
    assert tiles == 16 * blocks and _acc_max(want) > 0.1
    if network == "scene":
        assert min(empty, full, mixed) > 0 and rule > 0
    else:
        assert exact == rule == blocks * (3 + 11)
    got = RC.check_render(coarse, fine, want, _render_rays(coarse, fine, o, d, near, far, u_c, u_f), f"{network}, T{offset:+d} rays")
    if offset == -8:
        assert got["terminated"] == 0 and got["skipped"] == got["empty"]
    elif network == "opaque":
        assert got["terminated"] > 0


# ---- (e) the rule's margin -------------------------------------------------------------------------------------------------------
def test_tiles_in_the_denormal_band():
    """Sigma 109 along rays whose depth range grows from 2 to 6 over 520 ray blocks: the transmittance falls by 2^-80 to 2^-240
    per depth slot, so the slot in which a block dies moves through every position relative to 2^-126 (denormal), 2^-150 (exactly 0
    in the compositor) and 2^-160 (the kernel's rule).  On the coarse pass the CPU twin (test_render_matrix_inputs.py) counts 2080
    tiles, 1332 exactly dead, 1298 by the rule, 34 dead but not by the rule, 78 with a denormal front on all 8 rays.  A rule that is
    too eager zeroes a tile whose denormal weights the public path keeps: bit equality of `weights` sees it."""
    from oracle import nerf_oracle as O
    from tests.helpers import BUNDLE_KEYS
    from tests.test_gpu_parity import _close, _depth_close
    blocks, sigma = 520, 109.0
    assert blocks >= 2 * RC.cus()                             # the table is in use
    coarse, fine = RC.pair(RC.constant_sigma(MLP_KW, sigma), MLP_KW)
    near, far, _ = RC.margin_inputs(blocks, sigma)
    angle = np.linspace(0.0, 2.0 * np.pi, blocks, endpoint=False)
    unit = np.stack((np.cos(angle), np.full_like(angle, 0.3), np.sin(angle)), 1)
    unit = np.repeat(unit / np.linalg.norm(unit, axis=1, keepdims=True), 8, 0)     # fp64, rounded once: |d| is 1 to an ulp
    g = torch.Generator().manual_seed(blocks)
    d = torch.from_numpy(unit.astype(np.float32)).to(RC.dev())
    o = (torch.from_numpy((-4.0 * unit).astype(np.float32)) + 0.05 * torch.randn(blocks * 8, 3, generator=g)).to(RC.dev())
    near, far = near.to(RC.dev()), far.to(RC.dev())
    u_c, u_f = RC.u_pair(64, 128)
    want = RC.public_path(coarse, fine, o, d, near, far, u_c, u_f)
    for i, name in enumerate(("coarse", "fine")):
        assert bool((want["passes"][i][0] == sigma).all())
        tiles, exact, rule, not_by_rule, denormal = RC.margin_counts(RC.pass_factors(want, i))       # asserts check_rule_is_safe
        print(f"{name}: {tiles} tiles, {exact} exactly dead, {rule} by the rule, {not_by_rule} dead but not by the rule, {denormal} with a denormal front")
        assert tiles == blocks * (4, 12)[i]
        assert rule > 0 and exact > rule and not_by_rule == exact - rule and denormal > 0
    w = want["cb"]["weights"]
    assert int(((w > 0) & (w < float(RC.TINY))).sum()) > 0   # denormal weights are part of the comparison
    # the reference, anchored once: the oracle's compositor on the same radiance (test_composite_vs_oracle's budget for 64 samples)
    ref = O.composite(want["rad_c"].cpu(), want["passes"][0][1].cpu(), d.cpu(), O.RenderSpec())
    tol = 2e-6
    for k in BUNDLE_KEYS:
        got = want["cb"][k].cpu()
        if k == "mask_weights":
            assert (got != ref[k]).float().mean() < 1e-4
        elif k == "disp_map":
            _close(got, ref[k], 1e-6, rtol=10 * tol, what=k)
        elif k == "depth_map":
            _depth_close(got, ref[k], want["cb"]["acc_map"].cpu(), ref["acc_map"], tol, tol, k)
        else:
            _close(got, ref[k], tol, rtol=tol, what=k)
    got = RC.check_render(coarse, fine, want, _render_rays(coarse, fine, o, d, near, far, u_c, u_f), "margin")
    assert 0 < got["terminated"] <= got["exact"]


# ---- (f) NaN ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("network", ["transparent", "opaque"])
def test_a_ray_with_an_infinite_origin(opaque_pair, network):
    """One ray with an infinite origin coordinate: its encoding is NaN (sin / cos of inf) and so is every sum of layer1 and of
    the skip layer.  It does NOT reach sigma or the colour, on either path: the kernels' ReLU is fmaxf(x, 0), which returns 0 for a
    NaN (torch.relu would keep it), so from layers_xyz[0] on the ray's hidden state is finite, its sigma is fc_alpha.bias exactly
    (fc_alpha.weight is 0 here) and all six maps are finite.  What is asserted is equality with the public path on that, in a
    queue launch and in a table launch; a NaN sigma that does arrive is test_nan_and_infinite_sigma below."""
    if network == "opaque":
        (coarse, fine), rays, b = opaque_pair, RC.table_rays() + 5, 1.0e3
    else:
        (coarse, fine), rays, b = RC.pair(RC.constant_sigma(MLP_KW, -1.0e3), MLP_KW), RC.queue_rays(), -1.0e3
    bad = rays // 2 + 3
    o, d = RC.scene_rays(rays)
    o = o.expand(rays, 3).clone()
    o[bad, 1] = float("inf")
    near, far = RC.bounds()
    u_c, u_f = RC.u_pair(64, 128)
    want = RC.public_path(coarse, fine, o, d, near, far, u_c, u_f)
    for (sig, _), bundle in zip(want["passes"], (want["cb"], want["fb"])):
        assert bool((sig == b).all())                                       # the inf ray included
        assert all(bool(torch.isfinite(v).all()) for v in bundle.values())
    tiles, empty, full, mixed, exact, rule = RC.tile_counts(want)
    blocks = -(-rays // 8)
    assert tiles == 16 * blocks
    if network == "opaque":
        assert empty == 0 and exact == rule == blocks * (3 + 11)
        assert _acc_max(want) > 0.1
    else:
        assert empty == tiles and exact == 0
    got = RC.check_render(coarse, fine, want, _render_rays(coarse, fine, o, d, near, far, u_c, u_f), f"inf origin, {network}")
    if network == "opaque":
        assert got["terminated"] > 0
    else:
        assert got["terminated"] == 0 and got["skipped"] == tiles


def test_nan_and_infinite_sigma():
    """A NaN sigma that does reach the head: fc_alpha.weight[1] = +inf makes sigma NaN wherever hidden unit 1 is exactly 0 (the
    ReLU clipped it: 0 * inf; about 70 % of the samples) and +inf wherever it is positive.  The kernel's two promises: a NaN sigma has density to the vote
    (the tile is not skipped: its NaN must reach the compositor's input as the public path's does) and is no density to the
    compositor or to the termination bound (fmaxf); an infinite sigma kills its ray at once.  In the fine pass two samples of a
    ray may coincide: inf * 0 is a NaN alpha there, on both paths alike -- NaN exactly where the public path has it."""
    w = S.make_mlp_weights(2, **MLP_KW)
    w["fc_alpha.weight"][0, 1] = np.inf
    coarse, fine = RC.pair(w, MLP_KW)
    rays = RC.table_rays() + 5
    o, d = RC.scene_rays(rays)
    near, far = RC.bounds()
    u_c, u_f = RC.u_pair(64, 128)
    want = RC.public_path(coarse, fine, o, d, near, far, u_c, u_f)
    for sig, _ in want["passes"]:
        nan, inf = int(torch.isnan(sig).sum()), int(torch.isinf(sig).sum())
        print(f"sigma: {nan} NaN, {inf} +inf of {sig.numel()}")
        assert nan > sig.numel() // 100 and inf > sig.numel() // 100 and nan + inf == sig.numel()
    assert bool(torch.isfinite(want["cb"]["weights"]).all())                # coarse samples never coincide: the pdf is finite
    tiles, empty, full, mixed, exact, rule = RC.tile_counts(want)
    assert empty == 0 and rule > 0
    assert _acc_max(want) > 0.1
    got = RC.check_render(coarse, fine, want, _render_rays(coarse, fine, o, d, near, far, u_c, u_f), "NaN / inf sigma",
                          equal=RC.assert_bundles_equal_where_finite)
    assert got["skipped"] == 0 and got["terminated"] > 0


# ---- (g) graph replay with the table ---------------------------------------------------------------------------------------------
def test_render_rays_with_the_table_replays_from_a_hip_graph(scene_pair):
    """test_gpu_graph.py's pattern at T + 8 rays: the table's memset and the slot-major launch are part of the captured graph."""
    from nerfmeshes_amd import hip_ops
    from tests.test_gpu_ray_termination import counted
    coarse, fine = scene_pair
    u_c, u_f = RC.u_pair(64, 128)
    near, far = RC.bounds()
    o, d = hip_ops.ray_bundle(RC.pose(), RC.SIDE, RC.SIDE, S.LEGO_FOCAL_800, device=RC.dev())
    o = o[None].contiguous()
    chunk = RC.table_rays() + 8
    static_d = d[:chunk].clone()

    def render(dirs):
        return hip_ops.render_rays(coarse, fine, o, dirs, near, far, u_c, u_f)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up on the capture stream: function attributes, workspace
        render(static_d)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _, captured = render(static_d)
    firsts = (RC.FIRST - 60 * RC.SIDE, RC.FIRST + 50 * RC.SIDE, RC.FIRST)
    for first in firsts:
        static_d.copy_(d[first:first + chunk])
        graph.replay()
        torch.cuda.synchronize()
        _, eager = render(d[first:first + chunk].contiguous())
        torch.cuda.synchronize()
        for k in eager:
            assert torch.equal(captured[k], eager[k]), (first, k)
    assert float(captured["acc_map"].max()) > 0.1
    _, _, _, terminated = counted(lambda: render(d[firsts[-1]:firsts[-1] + chunk].contiguous()))
    print("graph replay: terminated on an eager call of the same rays:", terminated)
    assert terminated > 0
