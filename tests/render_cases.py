"""Shared helpers of the render path's configuration matrix (tests/test_gpu_render_matrix.py, tests/test_render_matrix_inputs.py;
DESIGN.md 3.9).  Nothing here touches the GPU at import.

They generalise what test_gpu_render_skip.py, test_gpu_tile_queue.py and test_gpu_ray_termination.py do for one configuration: the
reference of a render call is the public path on the same handles, which neither skips, queues nor terminates,

    coarse_intervals -> eval_rays -> composite -> sample_pdf -> eval_rays -> composite

with every option `render_rays` takes, and `check_render` holds one counted render against it: equal bits, the tile counts within
what the CPU tool (tests/tools/ray_termination_count.py) counts on that path's sigma and t, and the flop identity."""
import os
import sys

import numpy as np
import torch

from nerfmeshes_amd import synthetic as S
from tests.test_gpu_render_skip import FAR, FIRST, MLP_KW, NEAR, SIDE, assert_bundles_equal, tile_classes

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
from ray_termination_count import check_rule_is_safe, dead_tiles, factors, rule_table, transmittance  # noqa: E402

__all__ = ["FAR", "FIRST", "MLP_KW", "NEAR", "SIDE", "assert_bundles_equal", "tile_classes", "check_rule_is_safe", "dead_tiles",
           "factors", "rule_table", "transmittance"]

BENCH_VIEWS, BENCH_VIEW = 4, 2          # the view test_gpu_ray_termination.py renders: rays into the object
TINY = np.finfo(np.float32).tiny        # the smallest normal fp32


def dev():
    return torch.device("cuda")


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def table_rays():
    """T: the smallest ray count at which a 256-wide render call uses the ray-termination table (two 8-ray blocks per workgroup)."""
    return 16 * cus()


def queue_rays():
    """A ragged count whose 64-sample coarse pass has more tiles than workgroups (the queue is drawn from) and no table."""
    return 8 * (cus() // 4) + 5


def pose():
    return S.orbit_poses(BENCH_VIEWS)[BENCH_VIEW]


def scene_rays(count, first=FIRST):
    """`count` consecutive pixels of the middle rows of the benchmark's view 2: (origin (1, 3), dirs (count, 3))."""
    from nerfmeshes_amd import hip_ops
    o, d = hip_ops.ray_bundle(pose(), SIDE, SIDE, S.LEGO_FOCAL_800, first, count, device=dev())
    return o[None].contiguous(), d


def bounds(near=NEAR, far=FAR):
    return torch.tensor([near], device=dev()), torch.tensor([far], device=dev())


def u_pair(nc, nf):
    return torch.linspace(0.0, 1.0, nc).to(dev()), (torch.linspace(0.0, 1.0, nf).to(dev()) if nf else None)


def pair(w, kw):
    from nerfmeshes_amd import hip_ops
    return hip_ops.HipMLP(w, kw, dev()), hip_ops.HipMLP(w, kw, dev())


# ---- networks --------------------------------------------------------------------------------------------------------------------
def constant_sigma(kw, b, seed=2):
    """Seeded weights whose raw sigma is exactly `b` at every sample (fc_alpha.weight = 0, fc_alpha.bias = b: the head's sum of
    zero products is +0) while the colour still varies."""
    w = S.make_mlp_weights(seed, **kw)
    w["fc_alpha.weight"] = np.zeros_like(w["fc_alpha.weight"])
    w["fc_alpha.bias"] = np.full_like(w["fc_alpha.bias"], b)
    return w


def smooth_weights(kw, shift, gain, seed=2):
    """The construction of synthetic.make_smooth_scene_weights for any network shape: the seeded draw, band-limited, with
    sigma = gain * (raw - shift).  A smooth field has coherent regions without density, solid ones and surfaces in between, so
    empty, mixed, full and dead tiles all occur along rays into it."""
    w = S.band_limit(S.make_mlp_weights(seed, **kw), S.SCENE_DECAY, **kw)
    g = np.float32(gain)
    w["fc_alpha.weight"] = w["fc_alpha.weight"] * g
    w["fc_alpha.bias"] = ((w["fc_alpha.bias"] - np.float32(shift)) * g).astype(np.float32)
    return w


def skip_mask(kw):
    """Bit i: layers_xyz[i] takes cat(hidden, xyz_enc) (models.py:37)."""
    L, step = kw["num_layers"], kw["skip_step"]
    return sum(1 << i for i in range(L - 1) if i % step == 0 and i > 0 and i != L - 1)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def public_path(coarse, fine, o, d, near, far, u_c, u_f, lindisp=False, white_background=False, training=False,
                attenuation_threshold=1e-5):
    """Both bundles from the public entry points with render_rays' options, and per pass (sigma, t) for the tile counts.
    o: (1, 3) or (rays, 3); near / far: (1,) or (rays,)."""
    from nerfmeshes_amd import hip_ops
    opts = dict(attenuation_threshold=attenuation_threshold, white_background=white_background, training=training)
    t_c = hip_ops.coarse_intervals(u_c, near, far, d.shape[0], lindisp=lindisp)
    rad_c = coarse.eval_rays(o, d, t_c)
    cb = hip_ops.composite(rad_c, t_c, d, **opts)
    if fine is None:
        return dict(cb=cb, fb=None, passes=[(rad_c[..., 3], t_c)], d=d, rad_c=rad_c)
    t_f = hip_ops.sample_pdf(t_c, cb["weights"], u_f)
    rad_f = fine.eval_rays(o, d, t_f)
    fb = hip_ops.composite(rad_f, t_f, d, **opts)
    return dict(cb=cb, fb=fb, passes=[(rad_c[..., 3], t_c), (rad_f[..., 3], t_f)], d=d, rad_c=rad_c)


def pass_factors(want, i):
    """The compositor's transmittance factors of pass i of a public path (rays padded to whole blocks of 8: a padding ray has no
    transmittance), or None where the pass runs in linear order (samples % 16 != 0: no ray tiles, no table)."""
    sigma, t = want["passes"][i]
    if sigma.shape[1] % 16:
        return None
    f = factors(sigma.cpu().numpy(), t.cpu().numpy(), want["d"].norm(p=2, dim=-1).cpu().numpy())
    return np.pad(f, ((0, (-f.shape[0]) % 8), (0, 0)))


def tile_counts(want):
    """(tiles, empty, full, mixed, exact, rule) of a public path, both passes: `tile_classes` of its sigma and the CPU tool's dead
    tiles (exact: transmittance 0.0f at the tile's first sample on all 8 rays; rule: what the kernel's bound can find).  A pass in
    linear order has no dead tiles.  Asserts on the way that the rule is safe on these inputs."""
    classes = np.sum([tile_classes(s) for s, _ in want["passes"]], 0)
    exact = rule = 0
    for i in range(len(want["passes"])):
        f = pass_factors(want, i)
        if f is None:
            continue
        r, e = check_rule_is_safe(f)
        exact, rule = exact + e, rule + r
    return int(classes.sum()), int(classes[0]), int(classes[1]), int(classes[2]), exact, rule


def denormal_front_tiles(f):
    """Tiles whose 8 rays all have a denormal, non-zero transmittance at their first sample: bool (ray blocks, depth slots)."""
    front = transmittance(f)[:, ::16]
    return ((front > 0.0) & (front < TINY)).reshape(f.shape[0] // 8, 8, -1).all(1)


def margin_inputs(blocks=520, sigma=109.0, nc=64):
    """The inputs of the margin case (e) on the CPU: per-ray near / far (span constant within a block of 8 rays, linear from 2 to 6
    over the blocks) and the coarse pass's factors for a constant sigma along unit directions."""
    from oracle import nerf_oracle as O
    span = torch.linspace(2.0, 6.0, blocks).repeat_interleave(8)
    near = torch.full((blocks * 8,), 2.0)
    far = near + span
    t = O.coarse_intervals(near, far, nc, blocks * 8).numpy()
    f = factors(np.full_like(t, sigma), t, np.ones(blocks * 8, dtype=np.float32))
    return near, far, f


def margin_counts(f):
    """(tiles, exact, rule, exact and not rule, denormal-front tiles) of one pass's factors; asserts that the rule is safe."""
    check_rule_is_safe(f)
    exact, rule = dead_tiles(f)
    return exact.size, int(exact.sum()), int(rule.sum()), int((exact & ~rule).sum()), int(denormal_front_tiles(f).sum())


# ---- one render against it -------------------------------------------------------------------------------------------------------
def assert_bundles_equal_where_finite(got, want, what):
    """NaN exactly where `want` has it, equal bits elsewhere."""
    assert sorted(got) == sorted(want)
    for k in want:
        nan = torch.isnan(want[k])
        assert torch.equal(torch.isnan(got[k]), nan), (what, k, "NaN in other places")
        assert torch.equal(got[k][~nan], want[k][~nan]), (what, k)


def check_render(coarse, fine, want, render, what="", equal=assert_bundles_equal, skip_kernel=True):
    """One render under the profiling hook against the public path `want`: all six maps of both bundles equal bit for bit, skipped
    <= empty tiles and terminated <= exactly dead tiles, the flop identity of test_gpu_ray_termination.check, and skipped == empty
    whenever nothing was terminated (skip_kernel=False: a shape without the skipping kernel, nothing skipped or terminated).
    Returns dict(tiles, empty, skipped, exact, rule, terminated)."""
    from tests.test_gpu_ray_termination import counted
    (cb, fb), flops, skipped, terminated = counted(render)
    tiles, empty, _, _, exact, rule = tile_counts(want)
    print(f"{what}: (tiles, empty, skipped, exact, rule, terminated) = ({tiles}, {empty}, {skipped}, {exact}, {rule}, {terminated})")
    equal(cb, want["cb"], what + " coarse")
    if fine is not None:
        equal(fb, want["fb"], what + " fine")
    else:
        assert fb is None
    samples = sum(int(s.numel()) for s, _ in want["passes"])
    full, density = coarse.flops_per_sample(), coarse.flops_per_sample(True)
    tile = coarse.kernel_variant()[1] * 16
    assert samples * full - int(round(flops)) == skipped * tile * (full - density) + terminated * tile * full
    assert 0 <= terminated <= exact
    assert 0 <= skipped <= empty
    if not skip_kernel:
        assert skipped == 0 and terminated == 0
    elif terminated == 0:
        assert skipped == empty
    return dict(tiles=tiles, empty=empty, skipped=skipped, exact=exact, rule=rule, terminated=terminated)
