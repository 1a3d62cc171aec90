"""GPU parity: the HIP path (through the C ABI) vs the CPU oracle and the golden vectors of the
unmodified reference, stage by stage and end to end.  Tolerances (fp32 path):
  * MLP outputs: rgb 2e-5 abs, sigma 2e-5 relative to the sigma scale (summation order of a
    K<=319 fp32 dot differs between MFMA k-order and the CPU BLAS blocking);
  * per-ray maps: 2e-5 abs;  resampled depths: 2e-6 abs;
  * PSNR vs the reference on identical rays: |dPSNR| <= 1e-4 dB (BASELINE.json north_star).
"""
import numpy as np
import pytest
import torch

from nerfmeshes_amd import synthetic as S
from oracle import nerf_oracle as O, parity
from tests.helpers import (gen_weights, well_conditioned_rays, BUNDLE_KEYS, RENDER_CASES, golden_hparams, golden_weights, load_golden, mlp_kwargs,
                           specs_from_hparams)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from nerfmeshes_amd import hip_ops
    return hip_ops


def _desc(spec: O.MLPSpec):
    return dict(num_layers=spec.num_layers, hidden_size=spec.hidden_size, skip_step=spec.skip_step,
                num_encoding_fn_xyz=spec.num_encoding_fn_xyz, num_encoding_fn_dir=spec.num_encoding_fn_dir)


def _close(got, ref, atol, rtol=0.0, what=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    err = np.abs(got - ref)
    lim = atol + rtol * np.abs(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.all(err <= lim), f"{what}: max err {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)} " \
                               f"(ref {ref.flat[err.argmax()]:.6g}, got {got.flat[err.argmax()]:.6g}), " \
                               f"{(err > lim).sum()} / {err.size} out of tolerance"


def _depth_close(got, ref, acc_got, acc_ref, atol, rtol, what):
    """depth_map in eval mode is zeroed where acc_map < 1 (modules.py:108-109).  For saturated rays
    acc_map is 1.0 up to the last ulp of a 64..192-term fp32 sum, so WHICH side of 1.0 it lands on
    depends on the summation order (it differs between AVX2 and AVX-512 builds of torch itself).  The
    two sides must agree wherever acc_map is not within 2 ulp of 1.0; elsewhere either branch is
    accepted and the un-zeroed values must still agree."""
    got, ref, acc_got, acc_ref = (np.asarray(x, dtype=np.float32) for x in (got, ref, acc_got, acc_ref))
    same = (got == 0) == (ref == 0)
    near_one = (np.abs(acc_got - 1.0) <= 2.5e-7) & (np.abs(acc_ref - 1.0) <= 2.5e-7)
    assert np.all(same | near_one), f"{what}: depth zeroing disagrees away from acc == 1"
    _close(got[same], ref[same], atol, rtol, what=what)


def _rows_close(got, ref, atol, max_bad_per_row, max_bad_rows_frac, what):
    """(rays, samples) arrays whose sample axis follows the resampled depths: SamplePDF has a genuine
    discontinuity at u == 1.0 (modules.py:243-246: when the last pdf entry is < 1e-5 the sample lands
    on bins[-1] or bins[-2] depending on whether the fp32 cdf tops out at 1.0 or 1.0000001), which
    shifts at most a couple of far-end samples per ray.  Everything else must match."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = np.asarray(ref)
    bad = np.abs(got - ref) > atol
    per_row = bad.sum(-1)
    assert per_row.max() <= max_bad_per_row, f"{what}: {per_row.max()} entries off in one ray"
    assert (per_row > 0).mean() <= max_bad_rows_frac, f"{what}: {(per_row > 0).mean():.3f} of rays differ"


def _fine_samples_without_last(sorted_all, coarse_t):
    """Recover the resampled depths from sort(cat(t_coarse, samples)) by multiset difference with the
    (bit-exact) coarse depths, and drop the largest one -- the u == 1.0 sample, whose position the
    reference itself only defines up to the rounding of the last cdf entries (modules.py:234-246)."""
    out = []
    for row, tc in zip(np.asarray(sorted_all), np.asarray(coarse_t)):
        row = list(row)
        for v in tc:
            row.remove(v)
        out.append(sorted(row)[:-1])
    return np.asarray(out, dtype=np.float32)


def _last_fine_sample(sorted_all, coarse_t):
    """The largest resampled depth (the u == 1.0 sample) of every ray, by the same multiset difference."""
    out = []
    for row, tc in zip(np.asarray(sorted_all), np.asarray(coarse_t)):
        row = list(row)
        for v in tc:
            row.remove(v)
        out.append(max(row))
    return np.asarray(out, dtype=np.float64)


MLP_CONFIGS = [
    dict(),                                                        # 8x256, F=10/4 (lego)
    dict(hidden_size=128),                                         # nerf-colmap-fern.yml
    dict(hidden_size=64, num_layers=4, num_encoding_fn_xyz=6),     # tiny (BASELINE config 1 sizes)
    dict(hidden_size=128, num_layers=6, skip_step=2, num_encoding_fn_xyz=6),   # several skip layers
    dict(hidden_size=64, num_layers=9, skip_step=4, num_encoding_fn_xyz=10),
]


@pytest.mark.parametrize("kw", MLP_CONFIGS)
@pytest.mark.parametrize("n", [1, 16, 777, 5000])
def test_mlp_sample_points_vs_oracle(ops, kw, n):
    spec = O.MLPSpec(**kw)
    w = S.make_mlp_weights(17, density_gain=40.0, density_bias=1.0, **kw)
    mlp = ops.HipMLP(w, _desc(spec), "cuda")
    g = torch.Generator().manual_seed(n)
    pts = (torch.rand(n, 3, generator=g) * 2 - 1) * 4.0
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    ref = O.mlp_forward(w, spec, pts, dirs)
    got = mlp.sample_points(pts.cuda(), dirs.cuda())
    scale = float(ref[:, 3].abs().max()) + 1.0
    _close(got[:, :3], ref[:, :3], 2e-5, what="rgb")
    _close(got[:, 3], ref[:, 3], 2e-5 * scale, what="sigma")


FLAT_CONFIGS = [
    dict(use_viewdirs=False),                                                       # 8x256, trunk -> fc_out
    dict(use_viewdirs=False, hidden_size=128, num_layers=6, skip_step=2, num_encoding_fn_xyz=6),
    dict(use_viewdirs=False, hidden_size=64, num_layers=4, num_encoding_fn_xyz=6, num_encoding_fn_dir=2),   # 2-slot dataflow
]


@pytest.mark.parametrize("kw", FLAT_CONFIGS)
@pytest.mark.parametrize("n", [1, 777, 5000])
def test_mlp_without_view_directions_vs_oracle(ops, kw, n):
    """FlexibleNeRFModel(use_viewdirs=False) (models.py:52-55, 77-79): the trunk ends in fc_out (4 rows); the kernels' mode 2
    evaluates its colour rows next to the density row.  Full output, density-only output, the ray-batch entry point and the
    grid entry point against the oracle; no direction encoding is read (any num_encoding_fn_dir is accepted)."""
    spec = O.MLPSpec(**kw)
    w = S.make_mlp_weights(23, density_gain=40.0, density_bias=1.0, **kw)
    desc = dict(_desc(spec), use_viewdirs=False)
    mlp = ops.HipMLP(w, desc, "cuda")
    assert mlp.flops_per_sample() == mlp.flops_per_sample(density_only=True) + 2 * 3 * spec.hidden_size
    g = torch.Generator().manual_seed(n)
    pts = (torch.rand(n, 3, generator=g) * 2 - 1) * 4.0
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    ref = O.mlp_forward(w, spec, pts, dirs)
    got = mlp.sample_points(pts.cuda(), dirs.cuda())
    scale = float(ref[:, 3].abs().max()) + 1.0
    _close(got[:, :3], ref[:, :3], 2e-5, what="rgb")
    _close(got[:, 3], ref[:, 3], 2e-5 * scale, what="sigma")
    # rays: o + d t in the prologue
    rays, samples = max(1, n // 7), 7
    o = (torch.rand(rays, 3, generator=g) - 0.5) * 2.0
    d = torch.nn.functional.normalize(torch.randn(rays, 3, generator=g), dim=-1)
    t = torch.sort(torch.rand(rays, samples, generator=g) * 3.0, dim=-1).values
    ray_pts = o[:, None, :] + d[:, None, :] * t[..., None]
    ref_r = O.mlp_forward(w, spec, ray_pts.reshape(-1, 3), d[:, None, :].expand(rays, samples, 3).reshape(-1, 3))
    got_r = mlp.eval_rays(o.cuda(), d.cuda(), t.cuda()).reshape(-1, 4)
    _close(got_r[:, :3], ref_r[:, :3], 2e-5, what="rgb (rays)")
    _close(got_r[:, 3], ref_r[:, 3], 2e-5 * (float(ref_r[:, 3].abs().max()) + 1.0), what="sigma (rays)")
    if n == 777:
        ax = torch.linspace(-1.2, 1.2, 9)
        full = mlp.grid_query(ax, ax, ax, density_only=False)
        dens = mlp.grid_query(ax, ax, ax, density_only=True)
        assert torch.equal(full[:, 3], dens), "density-only and full evaluation share the trunk bit for bit"
        grid = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1).reshape(-1, 3)
        ref_g = O.mlp_forward(w, spec, grid, grid)
        _close(full[:, :3], ref_g[:, :3], 2e-5, what="rgb (grid)")
        _close(dens, ref_g[:, 3], 2e-5 * (float(ref_g[:, 3].abs().max()) + 1.0), what="sigma (grid)")


def test_mlp_without_view_directions_vs_reference_golden(ops):
    """The kernels' mode 2 against outputs of the UNMODIFIED reference's FlexibleNeRFModel(use_viewdirs=False)
    (tests/golden/mlp_flat_points.npz, three shapes incl. a 64-wide network on the 2-slot dataflow)."""
    g = load_golden("mlp_flat_points")
    pts = torch.from_numpy(g["points"]).cuda()
    for tag in ("a", "b", "c"):
        kw = {k: int(g[f"{k}_{tag}"]) for k in ("num_layers", "hidden_size", "skip_step", "num_encoding_fn_xyz", "num_encoding_fn_dir")}
        kw["use_viewdirs"] = False
        w = S.make_mlp_weights(int(g["seed"]), density_gain=float(g["gain"]), density_bias=float(g["bias"]), **kw)
        got = ops.HipMLP(w, kw, "cuda").sample_points(pts, pts)
        ref = g["radiance_" + tag]
        _close(got[:, :3], ref[:, :3], 2e-5, what=f"rgb ({tag})")
        _close(got[:, 3], ref[:, 3], 2e-5 * (float(np.abs(ref[:, 3]).max()) + 1.0), what=f"sigma ({tag})")


def test_model_without_view_directions_follows_parameter_updates_and_trains(ops):
    """The nn.Module mirror: forward under no_grad runs the HIP path, an in-place parameter edit is picked up by the
    on-device re-pack (nm_mlp_refresh with fc_out's rows), and with autograd on the same call is differentiable (round 4:
    the taping kernel's mode 2 + the FLAT delta kernel; gradients against fp64 autograd in tests/test_gpu_train.py)."""
    from nerfmeshes_amd.nerf import FlexibleNeRFModel
    torch.manual_seed(4)
    kw = dict(num_layers=4, hidden_size=128, skip_step=4, num_encoding_fn_xyz=6, num_encoding_fn_dir=4, use_viewdirs=False)
    net = FlexibleNeRFModel(**kw).cuda()
    spec = O.MLPSpec(**kw)
    pts = (torch.rand(999, 3) - 0.5) * 3.0
    with torch.no_grad():
        a = net(pts.cuda())
        w = {k: v.detach().cpu() for k, v in net.state_dict().items()}
        _close(a, O.mlp_forward(w, spec, pts, pts), 3e-5, what="fc_out network")
        net.fc_out.weight.mul_(1.7)
        net.fc_out.bias.add_(0.25)
        net.layers_xyz[1].weight.mul_(0.9)
        b = net(pts.cuda())
        w = {k: v.detach().cpu() for k, v in net.state_dict().items()}
        _close(b, O.mlp_forward(w, spec, pts, pts), 3e-5, what="fc_out network after the update")
        assert not torch.equal(a, b)
    out = net(pts.cuda())
    assert out.requires_grad and torch.equal(out.detach(), b), "the taping kernel must not change the output"
    out.square().sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    assert float(net.fc_out.weight.grad.abs().max()) > 0 and float(net.layer1.weight.grad.abs().max()) > 0


def test_mlp_points_golden(ops):
    g = load_golden("mlp_8x256_points")
    w = gen_weights(g["seed"], g["gain"], g["bias"])
    mlp = ops.HipMLP(w, _desc(O.MLPSpec()), "cuda")
    got = mlp.sample_points(torch.from_numpy(g["points"]).cuda(), torch.from_numpy(g["directions"]).cuda())
    _close(got[:, :3], g["radiance"][:, :3], 2e-5, what="rgb")
    _close(got[:, 3], g["radiance"][:, 3], 5e-3, what="sigma (scale ~1e2)")


def test_grid_query_golden(ops):
    g = load_golden("grid_8x256_res20")
    w = gen_weights(g["seed"], g["gain"], g["bias"])
    mlp = ops.HipMLP(w, _desc(O.MLPSpec()), "cuda")
    res, limit = int(g["res"]), float(g["limit"])
    ax = torch.linspace(-limit, limit, res)       # mesh_nerf.py:37 builds the tiles on the host
    full = mlp.grid_query(ax, ax, ax, density_only=False).reshape(res, res, res, 4)
    dens = mlp.grid_query(ax, ax, ax, density_only=True).reshape(res, res, res)
    _close(full[..., :3], g["radiance"][..., :3], 2e-5, what="grid rgb")
    _close(full[..., 3], g["radiance"][..., 3], 5e-3, what="grid sigma")
    assert torch.equal(full[..., 3], dens), "density-only path must reproduce the full path's sigma bit for bit"
    # ragged sub-range of the flattened grid
    part = mlp.grid_query(ax, ax, ax, first=1234, count=999, density_only=True)
    assert torch.equal(part, dens.reshape(-1)[1234:1234 + 999])


def test_ray_bundle_golden(ops):
    g = load_golden("rays")
    for i in range(2):
        h, w, f = g[f"hwf{i}"]
        o, d = ops.ray_bundle(g[f"pose{i}"], int(h), int(w), float(f))
        np.testing.assert_array_equal(o.cpu().numpy(), g[f"origin{i}"])
        _close(d.reshape(int(h), int(w), 3), g[f"dirs{i}"], 1.2e-7, what="dirs")
    o, d = ops.ray_bundle(S.orbit_poses(4)[1], 800, 800, S.LEGO_FOCAL_800)
    _close(d[torch.from_numpy(g["lego_idx"]).cuda()], g["lego_dirs"], 1.2e-7, what="lego dirs")
    # ragged pixel range
    o2, d2 = ops.ray_bundle(S.orbit_poses(4)[1], 800, 800, S.LEGO_FOCAL_800, first=799 * 800 + 3, count=797)
    assert torch.equal(d2, d[799 * 800 + 3:])


@pytest.mark.parametrize("lindisp", [False, True])
@pytest.mark.parametrize("per_ray", [False, True])
def test_coarse_intervals_bit_exact(ops, lindisp, per_ray):
    rays, count = 37, 64
    near = torch.rand(rays) + 0.5 if per_ray else torch.tensor(2.0)
    far = near + 3.0 if per_ray else torch.tensor(6.0)
    ref = O.coarse_intervals(near, far, count, rays, lindisp)
    got = ops.coarse_intervals(torch.linspace(0.0, 1.0, count).cuda(), near.cuda(), far.cuda(), rays, lindisp)
    assert torch.equal(got.cpu(), ref.contiguous())


# 513 / 700 / 1500: beyond one 512-sample pass -- the segmented kernel (the reference takes any count: modules.py:67-121)
# 100 / 300: composite_kernel<2> and lanes of composite_kernel<8> without a sample
@pytest.mark.parametrize("samples", [32, 64, 100, 192, 200, 300, 512, 513, 700, 1500])
@pytest.mark.parametrize("white", [False, True])
def test_composite_vs_oracle(ops, samples, white):
    g = torch.Generator().manual_seed(samples)
    rays = 301
    t = torch.sort(torch.rand(rays, samples, generator=g) * 4 + 2, dim=-1).values
    rad = torch.rand(rays, samples, 4, generator=g)
    rad[..., 3] = (torch.randn(rays, samples, generator=g) * 20.0) * (torch.rand(rays, 1, generator=g) * 1.5)
    rad[:5, :, 3] = -1.0            # empty rays: acc = 0 -> disp NaN -> 0
    rad[5:10, :, 3] = 1e4           # saturating rays
    dirs = torch.randn(rays, 3, generator=g)
    rs = O.RenderSpec(white_background=white)
    ref = O.composite(rad, t, dirs, rs)
    got = ops.composite(rad.cuda(), t.cuda(), dirs.cuda(), white_background=white)
    # the per-ray sums run over `samples` fp32 terms in another order than torch's: the budget of the shipped counts (<= 256),
    # growing with the count beyond
    tol = 2e-6 * max(1.0, samples / 256.0)
    for k in BUNDLE_KEYS:
        if k == "mask_weights":
            assert (got[k].cpu() != ref[k]).float().mean() < 1e-4
        elif k == "disp_map":
            _close(got[k], ref[k], 1e-6, rtol=10 * tol, what=k)
        elif k == "depth_map":
            # eval mode zeroes depth where acc < 1 (modules.py:108); acc within 1 ulp of 1.0 may take
            # the other branch under a different summation order -> compare where the branch agrees
            _depth_close(got[k].cpu(), ref[k], got["acc_map"].cpu(), ref["acc_map"], tol, tol, k)
        else:
            _close(got[k], ref[k], tol, rtol=tol, what=k)


# (300, 400), (64, 900): past the former 256 / 512 limits (a ray's tables are sized per launch now)
@pytest.mark.parametrize("coarse,fine", [(64, 128), (64, 64), (32, 16), (200, 56), (300, 400), (64, 900)])
def test_sample_pdf_vs_oracle(ops, coarse, fine):
    """Conditioning: sample = bins_b + (u - cdf_b) / (cdf_a - cdf_b) * binwidth, so a 1-ulp difference in
    the fp32 cdf (torch.sum's blocking vs a wavefront reduction for the pdf normaliser) moves a sample by
    ~6e-8 / pdf_bin * binwidth.  Rows [71:] keep every pdf entry >~ 1e-3 (error <= 1e-3 of a bin); rows [:71]
    sit at / below the 1e-5 denominator clamp (error up to ~1e-2 of a bin, the reference's own
    sensitivity).  The u == 1.0 sample is excluded, see _fine_samples_without_last."""
    g = torch.Generator().manual_seed(coarse + fine)
    rays = 203
    t = O.coarse_intervals(2.0, 6.0, coarse, rays).contiguous()
    w = torch.rand(rays, coarse, generator=g) ** 8           # peaky: many pdf entries under the 1e-5 clamp
    w[:7] = 0.0                                              # flat pdf (all 1e-5)
    w[7:39, :] = 0.0
    w[7:39, 10] = 50.0                                       # one dominant bin, the rest clamp
    w[39:71, 40 * coarse // 64:] = 0.0                       # empty far part
    w[71:] += 0.02 * w[71:].sum(-1, keepdim=True) / coarse + 1e-3
    ref = O.sample_pdf_intervals(t, w, fine)
    got = ops.sample_pdf(t.cuda(), w.cuda(), torch.linspace(0.0, 1.0, fine).cuda()).cpu()
    assert torch.all(got[:, 1:] >= got[:, :-1]), "output must be sorted"
    assert torch.equal(got[:, -1], t[:, -1]) and torch.equal(got[:, 0], t[:, 0])
    a, b = _fine_samples_without_last(got, t), _fine_samples_without_last(ref, t)
    binw = 4.0 / (coarse - 1)
    # (the pdf entries of rows [71:] shrink with the bin count -- ~1 / coarse --, and with them the conditioning: the budget of the
    # shipped counts up to 128 bins, proportionally more beyond)
    _close(a[71:], b[71:], 1e-3 * binw * max(1.0, coarse / 128.0), what="fine depths (well conditioned)")
    _close(a[:71], b[:71], 2e-2 * binw, what="fine depths (clamped bins)")
    # ... and the excluded u == 1.0 sample is not free either: it can only land where the cdf is within rounding of 1,
    # i.e. between the bin edge in front of the first cdf entry >= 1 - 4 ulp (fp64 cdf) and bins[-1]; when no earlier
    # entry is that close it IS bins[-1] or bins[-2] (modules.py:243-246).  Holds for the oracle's sample too.
    bins = (0.5 * (t[:, 1:] + t[:, :-1])).double().numpy()
    wd = w[:, 1:-1].double().numpy() + 1e-5
    cdf = np.concatenate([np.zeros((rays, 1)), np.cumsum(wd / wd.sum(-1, keepdims=True), -1)], -1)
    first = (cdf >= 1.0 - 4 * 6e-8).argmax(-1)
    lower = bins[np.arange(rays), np.maximum(first - 1, 0)]
    for name, arr in (("hip", got), ("oracle", ref)):
        last = _last_fine_sample(arr, t)
        assert np.all(last >= lower - 1e-6) and np.all(last <= bins[:, -1] + 1e-6), f"{name}: u == 1 sample outside the cdf == 1 plateau"
        tight = first >= bins.shape[1] - 1                      # plateau = the last bin only
        on_edge = np.minimum(np.abs(last - bins[:, -1]), np.abs(last - bins[:, -2])) <= 1e-6
        assert np.all(on_edge[tight & (wd[:, -1] / wd.sum(-1) < 1e-5)]), f"{name}: u == 1 sample not on bins[-1] / bins[-2]"


def _render_case(ops, case, precision="f32"):
    g = load_golden(case)
    hp = golden_hparams(g)
    sc, sf, rs = specs_from_hparams(hp)
    wc, wf = golden_weights(g, hp)
    coarse = ops.HipMLP(wc, _desc(sc), "cuda", precision=precision)
    fine = ops.HipMLP(wf, _desc(sf), "cuda", precision=precision) if wf is not None else None
    near, far = g["bounds"]
    cb, fb = ops.render_rays(coarse, fine, torch.from_numpy(g["origins"]).cuda(), torch.from_numpy(g["directions"]).cuda(),
                             torch.tensor([near]), torch.tensor([far]), torch.linspace(0, 1, rs.num_coarse),
                             torch.linspace(0, 1, rs.num_fine) if fine is not None else None,
                             lindisp=rs.lindisp, white_background=rs.white_background)
    return g, hp, (sc, sf, rs), (wc, wf), (coarse, fine), cb, fb


# the opt-in bf16x3 precision is held to the SAME tolerances on every render fixture: since round 5 it is instantiated for all
# three shipped widths (256, the fern configs' 128, config 1's 64)


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("case", [c for c in RENDER_CASES if c != "render_lego_rough"])
def test_render_golden(ops, case, precision):
    """End to end through nm_render_rays against the unmodified reference's outputs."""
    g, hp, _, _, _, cb, fb = _render_case(ops, case, precision)
    good = well_conditioned_rays(g)
    assert good.mean() > 0.9
    for prefix, b in (("coarse.", cb), ("fine.", fb)):
        if b is None:
            continue
        what = f"{case} {prefix}"
        sel = good if prefix == "fine." else np.ones_like(good)
        gb = {k: b[k].cpu().numpy() for k in BUNDLE_KEYS}
        _close(gb["rgb_map"][sel], g[prefix + "rgb_map"][sel], 1e-4, what=what + "rgb_map")
        _close(gb["rgb_map"], g[prefix + "rgb_map"], 1e-1, what=what + "rgb_map (all rays, loose)")
        _close(gb["acc_map"][sel], g[prefix + "acc_map"][sel], 1e-4, what=what + "acc_map")
        # disparity = acc / depth integrates t: it inherits the resampled depths' conditioning near
        # steep density (a 1e-2-bin slip of one sample next to a sigma~200 surface moves it by ~1 %)
        _close(gb["disp_map"][sel], g[prefix + "disp_map"][sel], 1e-5, rtol=(1e-4 if prefix == "coarse." else 2e-2),
               what=what + "disp_map")
        _depth_close(gb["depth_map"][sel], g[prefix + "depth_map"][sel], gb["acc_map"][sel], g[prefix + "acc_map"][sel],
                     1e-4 if prefix == "coarse." else 5e-3, 0.0, what + "depth_map")
        if prefix == "coarse.":
            _close(gb["weights"], g[prefix + "weights"], 2e-4, what=what + "weights")
            assert (gb["mask_weights"] != g[prefix + "mask_weights"]).mean() < 2e-3
        else:
            _rows_close(gb["weights"][sel], g[prefix + "weights"][sel], 2e-4, 8, 0.5, what + "weights")
            _rows_close(gb["mask_weights"][sel], g[prefix + "mask_weights"][sel], 0.5, 8, 0.5, what + "mask_weights")
    # PSNR parity (north_star: within 1e-4 dB of the reference on identical rays), the same helper bench.py prints:
    # both renders scored against a seeded noisy photograph of the reference render (~34 dB), with the reference's
    # float-batch_count loss, on ALL rays of the fixture -- nothing filtered
    final = fb if fb is not None else cb
    pre = "fine." if fb is not None else "coarse."
    par = parity.psnr_parity(final["rgb_map"].cpu(), g[pre + "rgb_map"], chunk=2048)
    print(f"{case}: {par}")
    # (the reference's float batch_count, rays / 2048 < 1 on these small fixtures, inflates the loss: PSNR 34 dB - 10 log10(2048 / rays))
    assert 10.0 < par["psnr_ref_db"] < 40.0, par
    # The 1e-4 dB bar is a whole-image quantity (one resampling-sensitive ray weighs 1/N): it is asserted as such on
    # the 8192-ray fixture below (test_psnr_parity_view8k) and on 32 768 rays in bench.py; a fixture of N rays is
    # held to the image-equivalent bar 1e-4 * 32768 / N, still on every ray it contains.
    assert par["abs_dpsnr_db"] <= 1e-4 * max(1.0, 32768 / par["rays"]), (case, par)


def test_psnr_parity_view8k(ops):
    """north_star: 'within 1e-4 PSNR on identical rays'.  8192 strided rays of a bench view rendered by the
    UNMODIFIED reference (tests/golden/render_lego_view_8k.npz) vs nm_render_rays, scored by the helper bench.py uses,
    on ALL rays -- no conditioning filter."""
    g = load_golden("render_lego_view_8k")
    kw = dict(num_layers=8, hidden_size=256, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
    w = S.make_scene_weights(int(g["seed"]), **kw)
    mlp = ops.HipMLP(w, kw, "cuda")
    o, d = ops.ray_bundle(g["pose"], 800, 800, S.LEGO_FOCAL_800)
    d = d[torch.from_numpy(g["ray_index"]).cuda()].contiguous()
    cb, fb = ops.render_rays(mlp, mlp, o[None], d, torch.tensor([2.0]), torch.tensor([6.0]), torch.linspace(0, 1, 64),
                             torch.linspace(0, 1, 128))
    for pre, b in (("coarse.", cb), ("fine.", fb)):
        par = parity.psnr_parity(b["rgb_map"].cpu(), g[pre + "rgb_map"], chunk=2048)
        print(pre, par)
        assert 25.0 < par["psnr_ref_db"] < 40.0
        assert par["abs_dpsnr_db"] <= 1e-4, (pre, par)
        assert par["rays_over_1e-4"] <= 0.002 * par["rays"], par       # reported, and bounded: a handful of rays
    assert float((cb["rgb_map"].cpu() - torch.from_numpy(g["coarse.rgb_map"])).abs().max()) < 1e-4
    # every ray above 1e-4 must be one of the DECLARED ill-conditioned classes (oracle/parity.py::explain_outliers):
    # the conditioning argument may not hide an unexplained difference
    spec, rs = O.MLPSpec(**kw), O.RenderSpec()
    rc, rf = O.render(w, w, spec, spec, rs, o[None].cpu(), d.cpu(), 2.0, 6.0)
    t_c = ops.coarse_intervals(torch.linspace(0, 1, 64).cuda(), torch.tensor([2.0]), torch.tensor([6.0]), d.shape[0])
    stage = ops.composite(mlp.eval_rays(o[None], d, t_c), t_c, d)
    t_f = ops.sample_pdf(t_c, stage["weights"], torch.linspace(0, 1, 128).cuda())
    on_ref = ops.composite(mlp.eval_rays(o[None], d, rf["t"].cuda().contiguous()), rf["t"].cuda().contiguous(), d)["rgb_map"]
    err = (fb["rgb_map"].cpu() - torch.from_numpy(g["fine.rgb_map"])).abs().max(-1).values
    why = parity.explain_outliers(err, rc, rf, t_f, on_ref)
    print(why)
    assert why["unexplained"] == 0, why


@pytest.mark.parametrize("name,scene,coarse_n,fine_n", [("render_fern_view_8k", "fern_8x128", 64, 128),
                                                         ("render_tiny_view_8k", "tiny_4x64", 32, 0)])
def test_psnr_parity_view8k_narrow_networks(ops, name, scene, coarse_n, fine_n):
    """The strict bar -- |dPSNR| <= 1e-4 dB, UNSCALED, on all 8192 rays -- for the narrower shipped networks as well: 8x128
    (config/nerf-colmap-fern.yml:115,152; coarse + fine, 64 + 128) and 4x64 (BASELINE configs[0]; 32 coarse samples, no fine
    network), each against 8192 rays rendered by the UNMODIFIED reference (make_golden.py --view8k-narrow)."""
    g = load_golden(name)
    w, kw = S.make_smooth_scene_weights(scene)
    mlp = ops.HipMLP(w, kw, "cuda")
    o, d = ops.ray_bundle(g["pose"], 800, 800, S.LEGO_FOCAL_800)
    d = d[torch.from_numpy(g["ray_index"]).cuda()].contiguous()
    cb, fb = ops.render_rays(mlp, mlp if fine_n else None, o[None], d, torch.tensor([2.0]), torch.tensor([6.0]),
                             torch.linspace(0, 1, coarse_n), torch.linspace(0, 1, fine_n) if fine_n else None)
    for pre, b in (("coarse.", cb), ("fine.", fb)):
        if b is None:
            continue
        par = parity.psnr_parity(b["rgb_map"].cpu(), g[pre + "rgb_map"], chunk=2048)
        print(name, pre, par)
        assert 25.0 < par["psnr_ref_db"] < 40.0
        assert par["abs_dpsnr_db"] <= 1e-4, (name, pre, par)
        assert par["rays_over_1e-4"] <= 0.002 * par["rays"], par
    assert float((cb["rgb_map"].cpu() - torch.from_numpy(g["coarse.rgb_map"])).abs().max()) < 1e-4
    if fb is not None:      # every ray above 1e-4 belongs to a declared ill-conditioned class, as for the lego fixture
        spec, rs = O.MLPSpec(**kw), O.RenderSpec(num_coarse=coarse_n, num_fine=fine_n)
        rc, rf = O.render(w, w, spec, spec, rs, o[None].cpu(), d.cpu(), 2.0, 6.0)
        t_c = ops.coarse_intervals(torch.linspace(0, 1, coarse_n).cuda(), torch.tensor([2.0]), torch.tensor([6.0]), d.shape[0])
        stage = ops.composite(mlp.eval_rays(o[None], d, t_c), t_c, d)
        t_f = ops.sample_pdf(t_c, stage["weights"], torch.linspace(0, 1, fine_n).cuda())
        on_ref = ops.composite(mlp.eval_rays(o[None], d, rf["t"].cuda().contiguous()), rf["t"].cuda().contiguous(), d)["rgb_map"]
        err = (fb["rgb_map"].cpu() - torch.from_numpy(g["fine.rgb_map"])).abs().max(-1).values
        why = parity.explain_outliers(err, rc, rf, t_f, on_ref)
        print(why)
        assert why["unexplained"] == 0, why


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_render_rough_scene_at_the_reference_noise_floor(ops, precision):
    """The rough scene (thresholded high-frequency noise density): the reference differs from itself by
    up to ~3e-2 on individual rays when its fp32 sums are re-ordered (test_reference_self_noise), because
    resampled depths in nearly empty bins are ill-conditioned.  Required here: (a) coarse pass tight,
    (b) the fine pass tight on >= 90 % of the rays and inside the noise floor on the rest,
    (c) given the reference's OWN fine depths, MLP + compositing agree to round-off on every ray."""
    g, hp, (sc, sf, rs), (wc, wf), (coarse, fine), cb, fb = _render_case(ops, "render_lego_rough", precision)
    _close(cb["rgb_map"], g["coarse.rgb_map"], 2e-5, what="coarse rgb")
    _close(cb["weights"], g["coarse.weights"], 2e-5, what="coarse weights")
    err = (fb["rgb_map"].cpu() - torch.from_numpy(g["fine.rgb_map"])).abs().max(-1).values
    assert float((err <= 1e-4).float().mean()) >= 0.9 and float(err.max()) < 5e-2, (err.max(), (err > 1e-4).sum())
    o, d = torch.from_numpy(g["origins"]), torch.from_numpy(g["directions"])
    _, ref = O.render(wc, wf, sc, sf, rs, o, d, float(g["bounds"][0]), float(g["bounds"][1]))
    t_ref = ref["t"].cuda().contiguous()
    rad = fine.eval_rays(o.cuda(), d.cuda(), t_ref)
    _close(rad[..., :3], ref["radiance"][..., :3], 2e-5, what="fine rgb samples on reference depths")
    _close(rad[..., 3], ref["radiance"][..., 3], 1e-3, what="fine sigma (scale ~2e2) on reference depths")
    comp = ops.composite(rad, t_ref, d.cuda())
    _close(comp["rgb_map"], g["fine.rgb_map"], 5e-5, what="fine rgb_map on reference depths")
    _close(comp["acc_map"], g["fine.acc_map"], 5e-5, what="fine acc_map on reference depths")


def test_full_size_view_properties(ops):
    """BASELINE.json configs[1] at full size (800x800 = 640 000 rays, 64+128 samples, 8x256): properties that
    do not need the (12-minute) CPU reference -- chunking invariance (rays are independent: any chunking, and
    therefore any ray sharding across GPUs, must give bit-identical pixels), determinism, and the compositing
    invariants acc = sum(weights) in [0, 1], rgb in [0, 1], depths sorted inside the bounds."""
    kw = dict(num_layers=8, hidden_size=256, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
    w = S.make_scene_weights(**kw)
    mlp = ops.HipMLP(w, kw, "cuda")
    o, d = ops.ray_bundle(S.orbit_poses(4)[2], 800, 800, S.LEGO_FOCAL_800)
    near, far = torch.tensor([2.0]), torch.tensor([6.0])
    uc, uf = torch.linspace(0, 1, 64), torch.linspace(0, 1, 128)

    def render(chunk):
        rgb, acc, wsum = [], [], []
        for s in range(0, d.shape[0], chunk):
            _, fb = ops.render_rays(mlp, mlp, o[None], d[s:s + chunk], near, far, uc, uf)
            rgb.append(fb["rgb_map"].clone()); acc.append(fb["acc_map"].clone()); wsum.append(fb["weights"].sum(-1))
        return torch.cat(rgb), torch.cat(acc), torch.cat(wsum)

    rgb_a, acc_a, wsum_a = render(640000)         # one call
    rgb_b, acc_b, _ = render(65536)               # bench chunking (ragged tail of 50 176 rays)
    rgb_c, _, _ = render(640000)                  # again
    assert torch.equal(rgb_a, rgb_b) and torch.equal(acc_a, acc_b), "chunking changed the pixels"
    assert torch.equal(rgb_a, rgb_c), "non-deterministic"
    # the reference's chunk size on a slice (313 chunks would be slow in Python; 20 chunks suffice)
    sl = slice(123456, 123456 + 20 * 2048)
    parts = [ops.render_rays(mlp, mlp, o[None], d[sl][s:s + 2048], near, far, uc, uf)[1]["rgb_map"].clone()
             for s in range(0, 20 * 2048, 2048)]
    assert torch.equal(torch.cat(parts), rgb_a[sl])
    assert float(rgb_a.min()) >= 0.0 and float(rgb_a.max()) <= 1.0 + 1e-5
    assert float(acc_a.min()) >= 0.0 and float(acc_a.max()) <= 1.0 + 1e-5
    assert float((acc_a - wsum_a).abs().max()) < 1e-5
    assert 0.2 < float(acc_a.mean()) < 0.8, "the synthetic scene should be neither empty nor opaque"


@pytest.mark.parametrize("res", [128])
def test_mesh_topology_end_to_end_vs_cpu_grid(ops, res):
    """`mesh_nerf` end to end against the CPU path (/root/reference/src/mesh_nerf.py:73-79; SURVEY section 7 "hard parts":
    topology parity on an identical grid is bitwise -- tests/test_gpu_mc.py -- and is measured SEPARATELY here end to end):
    the HIP density grid (nm_mlp_grid_query) -> numpy-exact iso level on the GPU -> nm_mc_* against the oracle's CPU grid
    -> numpy iso level -> C marching cubes.  Reported: sign flips at the iso level, the cubes whose corner pattern (hence
    tiling) differs, |dV|, |dF|; asserted: the stated budget, isolated cubes only (oracle/parity.py::mesh_topology)."""
    from nerfmeshes_amd.mesh_nerf import extract_iso_level
    from oracle import mc_oracle
    import contextlib, io
    kw = dict(num_layers=8, hidden_size=256, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
    w = S.make_scene_weights(**kw)
    mlp = ops.HipMLP(w, kw, "cuda")
    ax = torch.linspace(-1.2, 1.2, res)
    grid = mlp.grid_query(ax, ax, ax, density_only=True).view(res, res, res)

    class _A:
        iso_level = 32.0
    with contextlib.redirect_stdout(io.StringIO()):
        iso_hip = float(extract_iso_level(grid, _A))
    mesh_hip = [t.cpu().numpy() for t in ops.marching_cubes(grid, iso_hip)]
    torch.set_num_threads(min(32, torch.get_num_threads()))
    with torch.no_grad():
        ref = O.extract_radiance(w, O.MLPSpec(**kw), 1.2, res)[..., 3]
    iso_ref = float(O.iso_level(ref, 32.0))
    mesh_ref = mc_oracle.marching_cubes(np.ascontiguousarray(ref), iso_ref)
    rep = parity.mesh_topology(grid.cpu().numpy(), ref, iso_hip, iso_ref, mesh_hip, mesh_ref)
    print("mesh topology end to end:", rep)
    assert rep["cubes_cut_by_the_surface"] > 1000 and rep["faces_ref"] > 2000, "the scene must have a surface in the cube"
    assert rep["max_abs_dsigma_over_scale"] <= 2e-5
    # the adaptive level is max - std here: it inherits the grid's own round-off at the largest voxel (sigma scale ~ 6e2)
    assert abs(iso_hip - iso_ref) <= 2e-5 * (float(np.abs(ref).max()) + 1.0)
    assert rep["within_budget"], rep


def test_ndc_rays_kernel_vs_reference_golden(ops):
    """(f)-4: ndc_rays (nerf_helpers.py:280-307) as one HIP kernel, op for op as the reference's torch expressions
    (python-float constants rounded to fp32 once, scalar / tensor as reciprocal * scalar) -> the golden of the
    unmodified reference (rays.npz), bit for bit."""
    from nerfmeshes_amd.nerf import ndc_rays
    g = load_golden("rays")
    for i in range(2):
        h, w, f = (float(v) for v in g[f"hwf{i}"])
        o = torch.from_numpy(g[f"origin{i}"]).cuda()
        d = torch.from_numpy(g[f"dirs{i}"]).cuda()
        no, nd = ndc_rays(int(h), int(w), f, 1.0, o.expand(int(h), int(w), 3) * 0.3, d)
        assert no.shape == d.shape and nd.shape == d.shape
        np.testing.assert_array_equal(no.cpu().numpy(), g[f"ndc_o{i}"])
        np.testing.assert_array_equal(nd.cpu().numpy(), g[f"ndc_d{i}"])
        # shared (1,1,3) origin, as DataBundle.ndc passes it (data_helpers.py:165)
        so, sd = ndc_rays(int(h), int(w), f, 1.0, (o * 0.3)[None, None, :], d)
        assert torch.equal(so, no) and torch.equal(sd, nd)
        ro, rd = O.ndc_rays(int(h), int(w), f, 1.0, (o.cpu() * 0.3)[None, None, :], d.cpu())
        assert torch.equal(so.cpu(), ro) and torch.equal(sd.cpu(), rd)


@pytest.mark.parametrize("ndc", [False, True])
def test_render_view_in_kernel_ray_generation(ops, ndc):
    """(f)-4: nm_render_view generates the rays of a camera view inside the MLP / compositing kernels (12 floats in, no
    ray buffers).  The rays it generates are get_ray_bundle's [+ ndc_rays'] bit for bit (nm_view_rays vs nm_ray_bundle /
    the reference golden), and the pixels equal nm_render_rays on the materialised rays bit for bit -- plain and NDC
    (per-ray origins), on a ragged pixel range."""
    g = load_golden("rays")
    h, w, f = (float(v) for v in g["hwf0"])
    h, w = int(h), int(w)
    pose = g["pose0"]
    view = ops.make_view(pose, h, w, f, ndc_near=1.0 if ndc else None)
    vo, vd = ops.view_rays(view)
    o, d = ops.ray_bundle(pose, h, w, f)
    if not ndc:
        assert torch.equal(vd, d) and torch.equal(vo, o[None].expand_as(vd))
        _close(vd.reshape(h, w, 3), g["dirs0"], 1.2e-7, what="generated dirs vs reference")
    else:
        from nerfmeshes_amd.nerf import ndc_rays
        no, nd = ndc_rays(h, w, f, 1.0, o[None, :], d)
        assert torch.equal(vo, no) and torch.equal(vd, nd)
    kw = dict(num_layers=4, hidden_size=64, skip_step=2, num_encoding_fn_xyz=6, num_encoding_fn_dir=4)
    wts = S.make_mlp_weights(31, density_gain=20.0, density_bias=0.5, **kw)
    mlp = ops.HipMLP(wts, kw, "cuda")
    near, far = (torch.tensor([0.0]), torch.tensor([1.0])) if ndc else (torch.tensor([2.0]), torch.tensor([6.0]))
    uc, uf = torch.linspace(0, 1, 32), torch.linspace(0, 1, 24)
    first, count = 37, h * w - 50
    cb, fb = ops.render_view(mlp, mlp, view, near, far, uc, uf, first=first, count=count)
    cr, fr = ops.render_rays(mlp, mlp, vo[first:first + count].contiguous() if ndc else o[None],
                             vd[first:first + count].contiguous(), near, far, uc, uf)
    for k in BUNDLE_KEYS:
        assert torch.equal(cb[k], cr[k]) and torch.equal(fb[k], fr[k]), k
    assert float(fb["acc_map"].max()) > 0.05, "the scene must not be empty"
    # full-size headline geometry: one 65 536-ray chunk of an 800x800 view, 8x256, 64+128
    if not ndc:
        kw8 = dict(num_layers=8, hidden_size=256, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
        big = ops.HipMLP(S.make_scene_weights(**kw8), kw8, "cuda")
        pose8 = S.orbit_poses(4)[1]
        v8 = ops.make_view(pose8, 800, 800, S.LEGO_FOCAL_800)
        o8, d8 = ops.ray_bundle(pose8, 800, 800, S.LEGO_FOCAL_800)
        n2, f2 = torch.tensor([2.0]), torch.tensor([6.0])
        u64, u128 = torch.linspace(0, 1, 64), torch.linspace(0, 1, 128)
        _, a = ops.render_view(big, big, v8, n2, f2, u64, u128, first=300000, count=65536)
        _, b = ops.render_rays(big, big, o8[None], d8[300000:365536], n2, f2, u64, u128)
        assert torch.equal(a["rgb_map"], b["rgb_map"]) and torch.equal(a["depth_map"], b["depth_map"])


@pytest.mark.parametrize("nf,include", [(10, True), (4, True), (6, False), (0, True)])
def test_positional_encoding_module(ops, nf, include):
    """R3a: PositionalEncoding.forward on its own (modules.py:26-34) -> nm_positional_encoding vs the oracle."""
    from nerfmeshes_amd.nerf import PositionalEncoding
    enc = PositionalEncoding(nf, include_input=include).cuda()
    g = torch.Generator().manual_seed(nf)
    x = (torch.rand(5, 77, 3, generator=g) * 2 - 1) * 3.0
    got = enc(x.cuda()).cpu()
    ref = O.positional_encoding(x, nf, include)
    assert got.shape == ref.shape == (5, 77, enc.output_size())
    _close(got, ref, 1e-6, what="positional encoding")     # sin/cos of arguments up to 2^9 * 3: <= 2 ulp of libm


@pytest.mark.parametrize("rays", [1, 17, 2049])
@pytest.mark.parametrize("nc,nf,kw,precision", [
    (8, 8, dict(hidden_size=128, num_layers=4, num_encoding_fn_xyz=6), "f32"),     # tiny.yaml's literal sizes (4x128, 8+8)
    (16, 0, dict(hidden_size=64, num_layers=4, num_encoding_fn_xyz=6), "f32"),      # coarse only
    (64, 128, dict(), "f32"),                                                        # lego
    (64, 128, dict(), "bf16x3"),                                                     # ... in the opt-in precision, same bars
])
def test_render_sweep_vs_oracle(ops, rays, nc, nf, kw, precision):
    """Ragged ray counts (1 ray, not a multiple of the 128-sample workgroup tile, one more than the reference's
    2048-ray chunk) x sample counts, per-ray origins and bounds given as (R,) tensors."""
    spec = O.MLPSpec(**kw)
    full = dict(num_layers=spec.num_layers, hidden_size=spec.hidden_size, skip_step=spec.skip_step,
                num_encoding_fn_xyz=spec.num_encoding_fn_xyz, num_encoding_fn_dir=spec.num_encoding_fn_dir)
    w = (S.make_scene_weights(**full) if not kw else
         S.make_mlp_weights(23, density_gain=60.0, density_bias=0.5, **full))
    mlp = ops.HipMLP(w, full, "cuda", precision=precision)
    g = torch.Generator().manual_seed(rays * 7 + nc)
    o = torch.tensor([[0.3, -0.2, 4.0]]) + 0.05 * torch.randn(rays, 3, generator=g)
    d = torch.nn.functional.normalize(torch.tensor([[0.0, 0.05, -1.0]]) + 0.2 * torch.randn(rays, 3, generator=g), dim=-1)
    near = 2.0 + 0.1 * torch.rand(rays, generator=g)
    far = 6.0 - 0.1 * torch.rand(rays, generator=g)
    if rays == 1:
        near, far = near.reshape(()), far.reshape(())          # 0-dim bounds, as unpacking a (2,) tensor gives
    rs = O.RenderSpec(num_coarse=nc, num_fine=nf)
    c, f = O.render(w, w if nf else None, spec, spec if nf else None, rs, o, d, near, far)
    cb, fb = ops.render_rays(mlp, mlp if nf else None, o.cuda(), d.cuda(), near, far, torch.linspace(0, 1, nc),
                             torch.linspace(0, 1, nf) if nf else None)
    # the band-limited scene scales fc_alpha by 1e5: sigma carries ~1e-2 of absolute fp32 noise
    _close(cb["rgb_map"], c["rgb_map"], 2e-4, what="coarse rgb")
    _close(cb["weights"], c["weights"], 5e-4, what="coarse weights")
    if nf:
        acc = c["acc_map"].numpy()
        good = ~((acc > 0) & (acc < 5e-3))
        err = (fb["rgb_map"].cpu() - f["rgb_map"]).abs().max(-1).values.numpy()
        # off-path random rays graze the gain-1e5 surface: a resampled depth slipping across it moves single rays
        # (same noise floor as the reference against itself, test_reference_self_noise)
        assert (err[good] <= 2e-3).mean() >= 0.995 and err.max() < 5e-2 and np.median(err) < 1e-5, \
            (err.max(), np.median(err), (err > 2e-3).sum())


# ---- opt-in bf16x3 precision (mlp_device_b3.h): fp32-class accuracy, its own parity budget ---------------------------
def _b3_pair(ops):
    kw = dict(num_layers=8, hidden_size=256, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
    w = S.make_scene_weights(**kw)
    return kw, w, ops.HipMLP(w, kw, "cuda"), ops.HipMLP(w, kw, "cuda", precision="bf16x3")


def test_bf16x3_sample_points_error_class(ops):
    """Six bf16 products of three-way operand splits, fp32 accumulation: the error against an fp64 evaluation of the
    network must stay in the class of the fp32 path's own (<= 2x), on the sigma-gain-1e5 scene (cancellation-prone)."""
    kw, w, f32, b3 = _b3_pair(ops)
    g = torch.Generator().manual_seed(3)
    pts = (torch.rand(20000, 3, generator=g) * 2 - 1) * 2.0
    dirs = torch.nn.functional.normalize(torch.randn(20000, 3, generator=g), dim=-1)
    w64 = {k: torch.as_tensor(v).double() for k, v in w.items()}
    ref = O.mlp_forward(w64, O.MLPSpec(**kw), pts.double(), dirs.double(), keep_graph=True)
    scale = float(ref[:, 3].abs().max()) + 1.0
    err = {}
    for name, m in (("f32", f32), ("b3", b3)):
        got = m.sample_points(pts.cuda(), dirs.cuda()).cpu().double()
        err[name] = (float((got[:, :3] - ref[:, :3]).abs().max()), float((got[:, 3] - ref[:, 3]).abs().max()) / scale)
    assert err["b3"][0] <= max(2 * err["f32"][0], 2e-7) and err["b3"][1] <= max(2 * err["f32"][1], 3e-6), err
    # density-only path == the full path's sigma, bit for bit (same kernel, colour branch skipped)
    ax = torch.linspace(-1.2, 1.2, 24)
    full = b3.grid_query(ax, ax, ax, density_only=False)
    assert torch.equal(full[:, 3], b3.grid_query(ax, ax, ax, density_only=True))


def test_bf16x3_render_parity_and_mesh_topology(ops):
    """The mode's parity budget: 1e-4 dB on the 8192-ray reference fixture (all rays); density grid within 2e-5 of the
    fp32 path's (relative to the sigma scale); mesh topology equal up to isolated cubes."""
    kw, w, f32, b3 = _b3_pair(ops)
    g = load_golden("render_lego_view_8k")
    o, d = ops.ray_bundle(g["pose"], 800, 800, S.LEGO_FOCAL_800)
    d = d[torch.from_numpy(g["ray_index"]).cuda()].contiguous()
    _, fb = ops.render_rays(b3, b3, o[None], d, torch.tensor([2.0]), torch.tensor([6.0]), torch.linspace(0, 1, 64),
                            torch.linspace(0, 1, 128))
    par = parity.psnr_parity(fb["rgb_map"].cpu(), g["fine.rgb_map"], chunk=2048)
    print("bf16x3:", par)
    assert par["abs_dpsnr_db"] <= 1e-4 and par["rays_over_1e-4"] <= 0.005 * par["rays"], par
    res = 128
    ax = torch.linspace(-1.2, 1.2, res)
    g32 = f32.grid_query(ax, ax, ax, density_only=True).view(res, res, res)
    g3 = b3.grid_query(ax, ax, ax, density_only=True).view(res, res, res)
    assert float((g32 - g3).abs().max()) <= 2e-5 * (float(g32.abs().max()) + 1.0)
    # Mesh topology is a discontinuous function of the grid: a voxel within ~3e-6 * |sigma|max of the iso level, or an
    # MC33 face / interior test near its decision boundary, may resolve differently -- exactly as between the fp32 path
    # and the CPU reference, whose sigma differ by the same amount.  Budget of the mode: isolated cubes only.
    flips = int(((g32 > 32.0) != (g3 > 32.0)).sum())
    a, b = ops.marching_cubes(g32, 32.0), ops.marching_cubes(g3, 32.0)
    dv, df = abs(a[0].shape[0] - b[0].shape[0]), abs(a[1].shape[0] - b[1].shape[0])
    differing = int((a[1] != b[1]).any(-1).sum()) if a[1].shape == b[1].shape else None
    print(f"bf16x3 mesh at {res}^3: sign flips at iso {flips}, |dV| {dv}, |dF| {df}, differing faces {differing} of {a[1].shape[0]}")
    assert flips <= 1e-5 * res ** 3 and dv <= 1e-3 * a[0].shape[0] and df <= 1e-3 * a[1].shape[0]


def test_bf16x3_is_inference_only_and_follows_the_module(ops):
    from nerfmeshes_amd import train_ops as T
    from nerfmeshes_amd.nerf import FlexibleNeRFModel
    kw, w, f32, b3 = _b3_pair(ops)
    t = torch.rand(4, 8).sort(-1).values.cuda() + 2.0
    with pytest.raises(Exception):
        T.forward_train(b3, torch.zeros(1, 3).cuda(), torch.ones(4, 3).cuda(), t)
    with pytest.raises(Exception):          # the mode exists for the shipped shapes only: a generic-family width says so
        ops.HipMLP(S.make_mlp_weights(1, hidden_size=96), dict(kw, hidden_size=96), "cuda", precision="bf16x3")
    pts, dirs = torch.rand(5000, 3).cuda() * 2 - 1, torch.nn.functional.normalize(torch.randn(5000, 3), dim=-1).cuda()
    for hidden, layers, fx in ((128, 8, 10), (128, 6, 6), (64, 4, 6), (64, 8, 10)):     # round 5: the narrower shipped shapes
        kn = dict(kw, hidden_size=hidden, num_layers=layers, num_encoding_fn_xyz=fx, skip_step=min(4, layers - 1))
        wn = S.make_mlp_weights(3, density_gain=30.0, **kn)
        a, b = ops.HipMLP(wn, kn, "cuda").sample_points(pts, dirs), ops.HipMLP(wn, kn, "cuda", precision="bf16x3").sample_points(pts, dirs)
        assert not torch.equal(a, b), "bf16x3 is a different arithmetic"
        assert float((a[:, :3] - b[:, :3]).abs().max()) <= 2e-6 and float((a[:, 3] - b[:, 3]).abs().max()) <= 2e-5 * (float(a[:, 3].abs().max()) + 1.0)
    net = FlexibleNeRFModel(**kw).cuda().eval()
    net.precision = "bf16x3"
    with torch.no_grad():
        out = net(torch.rand(100, 3).cuda(), torch.rand(100, 3).cuda())
        assert net.hip().precision == "bf16x3" and out.shape == (100, 4)
    assert net.hip().precision == "f32"        # with autograd on, a forward always runs the (differentiable) fp32 kernels
