"""Inputs, references and tolerances of the training path's ray operators (nerfmeshes_amd/csrc/ray_ops.hip), shared by
tests/test_ray_ops_inputs.py (no GPU) and tests/test_gpu_ray_ops.py.  Nothing here touches the GPU.

Compositing (`composite_kernel<PER, LONG>` in training mode and `composite_backward_kernel<1|2|3|4|8, false>` / `<8, true>`, the
long kernel): 61 rays per case -- the last block of four waves has one live wave --, directions of any norm,
ray 0 with the zero direction, and five ray families of twelve rays each:

    random    sigma = 3 randn (what test_gpu_train.py uses)
    surface   sigma about -1 in front of a random sample, 10**U(0, 4) * U(0, 1) from there on: empty space, a wall with
              alpha == 1.0f and 1 - alpha + 1e-10 == 1e-10f, occluded samples behind it
    opaque    sigma = 1e4 everywhere
    empty     sigma + noise <= 0 everywhere: every gradient is exactly 0
    dups      depths rounded to one decimal: many intervals of length 0

The reference of a gradient is fp64 autograd over the oracle's compositor; the error of ray r is

    err_r = max |got_r - g64_r| / max |g64_r|        over the ray's (samples, 4) gradient rows,

and the tolerance comes from the oracle's own fp32 autograd alone (GRAD_TOL_* below).  A ray whose fp64 gradient is identically 0
must come back as exactly 0.

Inverse-CDF resampling: `pdf_exact_inputs` is a fixture in which every intermediate of SamplePDF is exactly representable, so that any
correct implementation agrees with the oracle bit for bit (see its docstring)."""
import functools

import numpy as np
import torch

from oracle import nerf_oracle as O

RAYS = 61
FAMILIES = ("random", "surface", "opaque", "empty", "dups")
FAMILY_RAYS = 12                      # ray 0 is the zero-direction ray, family f owns rays 1 + 12 f .. 12 + 12 f
GRAD_KEYS = ("rgb_map", "acc_map", "depth_map", "weights")

# every instantiation at its first, a middle and its last count; 257 .. 448: lanes of the PER = 8 kernel without a sample;
# 513 / 1024 / 1025: the long kernel just past one segment, at exactly two, and one sample into a third
SAMPLE_COUNTS = (1, 2, 7, 64, 65, 100, 128, 129, 200, 256, 257, 300, 448, 512, 513, 1024, 1025, 1100)
# one count per instantiation for the cases with ONE upstream gradient (the other three absent, not zero tensors)
SOLO_COUNTS = (7, 100, 192, 250, 300, 700)
INDEPENDENCE_COUNTS = (300, 1025)

# err_r <= max(GRAD_TOL_OWN * e32_r, GRAD_TOL_FAMILY * q95): e32_r is err_r of the oracle's fp32 autograd, q95 its 95th percentile
# (torch.quantile, linear) over the rays of the same family and case whose fp64 gradient is not identically 0.  The kernel's
# arithmetic restated on the CPU (`restated_backward`: fp32 elementwise, fp64 product and suffix scans) must stay within
# RESTATEMENT_BOUND x max(e32_r, q95), asserted without a GPU (it reaches 3.1 on these inputs); 16 leaves 2.5 x over that bound for
# expf on the GPU differing from the host's.  In absolute terms the floor is about 3e-6 per ray.
# measured on the MI355X, worst err_r / max(e32_r, q95) per family over all 42 cases (tests/test_gpu_ray_ops.py prints them):
#   random 8.08 (s7 acc_map only; 4.98 at s1025 with all four gradients), surface 2.30, opaque 1.00, dups 2.77, empty and the
#   zero-direction ray exactly 0.  With acc_map alone the gradient of a ray that ends opaque is 1e-10 of its terms: e32_r is
#   1 .. 1e3 there, for the oracle as for the kernels, and the comparison says little on those rays.
GRAD_TOL_OWN = 4.0
GRAD_TOL_FAMILY = 16.0
RESTATEMENT_BOUND = 6.5


def per_of(samples):
    """The kernel instantiation a sample count reaches (ray_ops.hip: NM_LAUNCH_COMPOSITE)."""
    if samples > 512:
        return "long"
    per = (samples + 63) // 64
    return f"per{per if per <= 4 else 8}"


def family_of(ray):
    return "zero_dir" if ray == 0 else FAMILIES[(ray - 1) // FAMILY_RAYS]


def family_rays(name):
    f = FAMILIES.index(name)
    return range(1 + FAMILY_RAYS * f, 1 + FAMILY_RAYS * (f + 1))


def _cases():
    """(samples, white background, noise present, upstream gradients).  White background and noise rotate over their four
    combinations, so that each instantiation sees both values of each."""
    out = []
    for i, s in enumerate(SAMPLE_COUNTS):
        out.append((s, bool(i & 1), not (i & 2), GRAD_KEYS))
    for i, s in enumerate(SOLO_COUNTS):
        for j, k in enumerate(GRAD_KEYS):
            out.append((s, bool((i + j) & 1), bool((i + j) & 2), (k,)))
    return out


CASES = _cases()
ALL_GRAD_CASES = [c for c in CASES if len(c[3]) == 4]


def case_id(case):
    samples, white, noise, keys = case
    return "-".join([f"s{samples}", per_of(samples), "white" if white else "black", "noise" if noise else "nonoise",
                     "all" if len(keys) == 4 else keys[0] + "_only"])


def inputs(samples, with_noise, seed=None):
    """(radiance (61, S, 4), t (61, S), dirs (61, 3), noise (61, S) or None, upstream gradients), all fp32 on the CPU."""
    g = torch.Generator().manual_seed(1000 + samples if seed is None else seed)
    rays = RAYS
    t = torch.sort(2.0 + 4.0 * torch.rand(rays, samples, generator=g), dim=-1).values
    dirs = torch.randn(rays, 3, generator=g) * (0.5 + 1.5 * torch.rand(rays, 1, generator=g))      # norms of anything but 1
    dirs[0] = 0.0
    noise = torch.randn(rays, samples, generator=g)
    sigma = 3.0 * torch.randn(rays, samples, generator=g)
    r = family_rays("surface")
    first = torch.randint(0, samples, (len(r), 1), generator=g)
    wall = 10.0 ** (4.0 * torch.rand(len(r), samples, generator=g)) * torch.rand(len(r), samples, generator=g)
    front = -1.0 + 0.1 * torch.randn(len(r), samples, generator=g)
    sigma[r.start:r.stop] = torch.where(torch.arange(samples)[None, :] < first, front, wall)
    if with_noise:       # the wall stays a wall and the space in front of it empty whatever the noise draws
        sigma[r.start:r.stop] -= torch.where(torch.arange(samples)[None, :] < first, noise[r.start:r.stop].abs(), torch.zeros(()))
    r = family_rays("opaque")
    sigma[r.start:r.stop] = 1e4
    r = family_rays("empty")
    sigma[r.start:r.stop] = -torch.rand(len(r), samples, generator=g) - (noise[r.start:r.stop].abs() if with_noise else 0.0)
    r = family_rays("dups")
    t[r.start:r.stop] = torch.round(t[r.start:r.stop] * 10.0) / 10.0
    rad = torch.cat((torch.rand(rays, samples, 3, generator=g), sigma[..., None]), -1).contiguous()
    G = dict(rgb_map=torch.randn(rays, 3, generator=g), acc_map=torch.randn(rays, generator=g),
             depth_map=torch.randn(rays, generator=g), weights=torch.randn(rays, samples, generator=g))
    return rad, t.contiguous(), dirs, (noise if with_noise else None), G


def render_spec(samples, white):
    return O.RenderSpec(num_coarse=samples, num_fine=0, white_background=white, training=True)


def oracle_backward(rad, t, dirs, noise, G, keys, white, dtype):
    """Gradient with respect to the radiance of sum_k (bundle[k] * G[k]).sum() over `keys`, by torch autograd over the oracle."""
    r = rad.detach().to(dtype).clone().requires_grad_(True)
    b = O.composite(r, t.to(dtype), dirs.to(dtype), render_spec(t.shape[1], white), noise=None if noise is None else noise.to(dtype))
    sum((b[k] * G[k].to(dtype)).sum() for k in keys).backward()
    return r.grad


def restated_backward(rad, t, dirs, noise, G, keys, white, total_minus_prefix=False, one_minus_alpha=False):
    """The arithmetic of composite_backward_kernel (one pass and long) on the CPU, written plainly: every
    elementwise step in fp32, the transmittance an exclusive fp64 product rounded per element, the sum of dL/dw_j * w_j over the
    samples behind a sample accumulated in fp64 from the far end.  The host's expf stands in for the GPU's.

    The two options restate what the kernels did before these tests existed, and tests/test_ray_ops_inputs.py shows on which rays
    each misses the tolerance:
      total_minus_prefix   the long kernel walked near to far and took the sum behind a sample as total - prefix;
      one_minus_alpha      d alpha / d (sigma * dist) as 1 - alpha, alpha itself being 1 - exp(..): the subtraction has lost
                           exp's low bits (an error of 6e-8 / (1 - alpha) of the entry, all of it from alpha == 1.0f on)."""
    f32 = torch.float32
    norm = dirs.norm(p=2, dim=-1)
    dist = torch.cat((t[:, 1:] - t[:, :-1], torch.full_like(t[:, :1], 1e10)), -1) * norm[:, None]
    raw = rad[..., 3] + (noise if noise is not None else torch.zeros((), dtype=f32))
    e = torch.exp(-torch.relu(raw) * dist)
    alpha = 1.0 - e
    keep = (1.0 - alpha) + torch.tensor(1e-10, dtype=f32)
    prod = torch.cumprod(keep.double(), -1)
    T = torch.cat((torch.ones_like(prod[:, :1]), prod[:, :-1]), -1).to(f32)
    zero = torch.zeros(rad.shape[0], dtype=f32)
    g_rgb = G["rgb_map"] if "rgb_map" in keys else torch.zeros(rad.shape[0], 3, dtype=f32)
    gr, gg, gb = g_rgb[:, 0:1], g_rgb[:, 1:2], g_rgb[:, 2:3]
    gacc = (G["acc_map"] if "acc_map" in keys else zero)[:, None] - (((gr + gg) + gb) if white else 0.0)
    gdepth = (G["depth_map"] if "depth_map" in keys else zero)[:, None]
    dw = ((gr * rad[..., 0] + gg * rad[..., 1]) + gb * rad[..., 2]) + gacc + gdepth * t
    if "weights" in keys:
        dw = dw + G["weights"]
    w = alpha * T
    own = (dw * w).double()
    if total_minus_prefix:
        suffix = (own.sum(-1, keepdim=True) - torch.cumsum(own, -1)).to(f32)
    else:
        behind = torch.cumsum(own.flip(-1), -1).flip(-1)
        suffix = torch.cat((behind[:, 1:], torch.zeros_like(behind[:, :1])), -1).to(f32)
    dalpha = dw * T - suffix / keep
    dsigma = torch.where(raw > 0.0, dalpha * dist * ((1.0 - alpha) if one_minus_alpha else e), torch.zeros((), dtype=f32))
    assert dsigma.dtype == f32 and w.dtype == f32
    return torch.stack((w * gr, w * gg, w * gb, dsigma), -1)


def ray_errors(got, g64):
    """err_r of every ray (0 where got_r and g64_r are both identically 0, inf where only g64_r is)."""
    got, g64 = got.detach().double().cpu().flatten(1), g64.double().flatten(1)
    num = (got - g64).abs().amax(1)
    den = g64.abs().amax(1)
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), num))


@functools.lru_cache(maxsize=None)
def reference(case):
    """Everything a test of one case needs that does not depend on the code under test: the inputs, the fp64 gradient, the error of
    the oracle's fp32 gradient per ray, the family scale q95 per ray and the rays that must come back as exactly 0."""
    samples, white, with_noise, keys = case
    rad, t, dirs, noise, G = inputs(samples, with_noise)
    g64 = oracle_backward(rad, t, dirs, noise, G, keys, white, torch.float64)
    g32 = oracle_backward(rad, t, dirs, noise, G, keys, white, torch.float32)
    e32 = ray_errors(g32, g64)
    zero = g64.flatten(1).abs().amax(1) == 0
    q95 = torch.zeros(RAYS, dtype=torch.float64)
    for name in FAMILIES:
        r = family_rays(name)
        live = e32[r.start:r.stop][~zero[r.start:r.stop]]
        if live.numel():
            q95[r.start:r.stop] = torch.quantile(live, 0.95)
    return dict(rad=rad, t=t, dirs=dirs, noise=noise, G=G, g64=g64, e32=e32, q95=q95, zero=zero,
                forward32=O.composite(rad, t, dirs, render_spec(samples, white), noise=noise))


def grad_ratios(got, ref):
    """err_r / max(e32_r, q95) per ray: what the measured figures beside GRAD_TOL_FAMILY are (nan on the exactly-zero rays)."""
    err = ray_errors(got, ref["g64"])
    scale = torch.maximum(ref["e32"], ref["q95"])
    return torch.where(ref["zero"], torch.full_like(err, float("nan")), err / scale)


def check_gradient(got, ref, what):
    """The per-ray assertion of this module's docstring.  Returns the worst err_r / max(e32_r, q95) per family."""
    got = got.detach().cpu()
    assert got.shape == ref["g64"].shape and got.dtype == torch.float32, what
    for r in torch.nonzero(ref["zero"]).flatten().tolist():
        assert not bool(got[r].any()), f"{what}: ray {r} ({family_of(r)}) has the gradient 0 in fp64 and must be exactly 0, got max |g| = {float(got[r].abs().max()):.3e}"
    err = ray_errors(got, ref["g64"])
    lim = torch.maximum(GRAD_TOL_OWN * ref["e32"], GRAD_TOL_FAMILY * ref["q95"])
    live = ~ref["zero"]
    bad = [(r, family_of(r), float(err[r]), float(lim[r])) for r in torch.nonzero(live & ~(err <= lim)).flatten().tolist()]
    assert not bad, f"{what}: (ray, family, err_r, limit) {bad}"
    return worst_by_family(grad_ratios(got, ref))


def worst_by_family(ratios):
    out = {}
    for name in FAMILIES:
        r = family_rays(name)
        v = ratios[r.start:r.stop]
        v = v[~torch.isnan(v)]
        out[name] = float(v.max()) if v.numel() else 0.0
    return out


# ---- inverse-CDF resampling, exact -------------------------------------------------------------------------------------------------
PDF_EXACT_COARSE = (3, 4, 6, 10, 18, 34, 66, 130, 258)       # coarse - 2 = 1 .. 256 pdf entries: 1 to 4 chunks of the 64-wide cdf scan
PDF_EXACT_RAYS = 7                                            # two blocks, the second with three live waves
PDF_INTERIOR_WEIGHT = np.float32(0.25) - np.float32(1e-5)     # + 1e-5f == 0.25f (asserted in test_ray_ops_inputs.py)
PDF_THIN_WEIGHT = np.float32(2.0 ** -16) - np.float32(1e-5)               # + 1e-5f == 2^-16
PDF_REDUCED_WEIGHT = np.float32(np.float32(0.25) - np.float32(2.0 ** -16)) - np.float32(1e-5)      # + 1e-5f == 1 / 4 - 2^-16
PDF_THIN_M = (8, 16, 32, 64, 128, 256)
PDF_MULTISET_SHAPES = ((64, 128), (65, 1), (67, 200), (3, 5))


def pdf_exact_inputs(coarse, per_ray=True):
    """(t, weights, u) of SamplePDF (modules.py:197-248) in which every intermediate is exactly representable in fp32 AND the
    same number in any precision and any summation order:

      * t = 2 + k / 64, so the bins 0.5 (t[k + 1] + t[k]) are odd multiples of 1 / 128;
      * the coarse - 2 = n interior weights are all w with w + 1e-5f == 0.25f and n is a power of two: their sum is n / 4, every
        pdf entry exactly 1 / n and the cdf k / n;  the two end weights are NaN -- they must not be read;
      * u = k / (8 n): (u - cdf[below]) / (1 / n) is a multiple of 1 / 8 below 1, times the bin width 1 / 64 exact.

    Each ray's u holds k = 0, k = 8 (exactly cdf[1]; which side of the tie is taken shows only in `pdf_thin_bin_inputs`), the
    largest k below 8 n and 8 n itself (u == 1.0: both indices clamp to the last bin and the zero denominator becomes 1); the rest are random.
    per_ray=False: one u row shared by all rays (the render path's entry point)."""
    n = coarse - 2
    fine = 4 * n + 3
    g = torch.Generator().manual_seed(coarse)
    t = (2.0 + torch.arange(coarse, dtype=torch.float32) / 64.0).expand(PDF_EXACT_RAYS, coarse).contiguous()
    w = torch.full((PDF_EXACT_RAYS, coarse), float(PDF_INTERIOR_WEIGHT), dtype=torch.float32)
    w[:, 0] = float("nan")
    w[:, -1] = float("nan")
    k = torch.randint(0, 8 * n + 1, (PDF_EXACT_RAYS if per_ray else 1, fine), generator=g)
    forced = torch.tensor([0, 8, 8 * n - 1, 8 * n])
    for row in k:
        row[torch.randperm(fine, generator=g)[:4]] = forced
    u = (k.to(torch.float32) / float(8 * n)).contiguous()
    assert bool((u.double() * (8 * n) == k.double()).all())
    return t, w, (u if per_ray else u[0].contiguous())


def pdf_thin_bin_inputs(m, per_ray=True):
    """The exact fixture with a bin thinner than SamplePDF's 1e-5 denominator clamp, where the tie rule decides by a whole bin.
    (In `pdf_exact_inputs` the inverse cdf is continuous: u == cdf[j] gives bins[j] as the end of one bin and as the start of the
    next, so `cdf[mid] < u` for `<=` changes no bit there.)

    coarse = m + 3 with m = 8 .. 256 a power of two: m + 1 pdf numerators (w + 1e-5f, each sum exact) of 1 / 4, except entry j
    with 2^-16 and entry j + 1 with 1 / 4 - 2^-16, j = min(m / 2, 63): the sum is m / 4, the pdf 1 / m except 2^-14 / m (below
    1e-5) and 1 / m - 2^-14 / m, every cdf entry a multiple of 2^-14 / m, and from entry j + 2 on a multiple of 1 / m again; with
    j = 63 the thin bin is the last entry of the first 64-wide chunk of the kernel's cdf scan and what follows rides on the carry.
    u = k / (8 m) outside [cdf[j], cdf[j + 2]), plus cdf[j] (the thin bin's start: frac 0 over the clamped denominator) and
    cdf[j + 1] = (j + 2^-14) / m: with right=True the sample is bins[j + 1], with `<` it is bins[j] + 2^-14 / m / 64."""
    coarse, fine, j = m + 3, 4 * m + 3, min(m // 2, 63)
    g = torch.Generator().manual_seed(7 * m)
    t = (2.0 + torch.arange(coarse, dtype=torch.float32) / 64.0).expand(PDF_EXACT_RAYS, coarse).contiguous()
    w = torch.full((PDF_EXACT_RAYS, coarse), float(PDF_INTERIOR_WEIGHT), dtype=torch.float32)
    w[:, 0] = float("nan")
    w[:, -1] = float("nan")
    w[:, 1 + j] = float(PDF_THIN_WEIGHT)
    w[:, 2 + j] = float(PDF_REDUCED_WEIGHT)
    rows = PDF_EXACT_RAYS if per_ray else 1
    k = torch.randint(0, 8 * m + 1, (rows, fine), generator=g)
    inside = (k > 8 * j) & (k < 8 * (j + 1))
    k = torch.where(inside, k + 8, k)                       # moved one bin on: off the thin and the reduced bin
    u = k.to(torch.float32) / float(8 * m)
    forced = torch.tensor([0.0, 8.0 / (8 * m), 1.0, j / m, (j + 2.0 ** -14) / m], dtype=torch.float64).to(torch.float32)
    assert float(forced[4].double() * m) == j + 2.0 ** -14
    for row in u:
        row[torch.randperm(fine, generator=g)[:5]] = forced
    return t, w, (u.contiguous() if per_ray else u[0].contiguous())


def pdf_restated_fp64(t, w, u, side="right"):
    """SamplePDF's formula in fp64 numpy, written plainly (searchsorted side='right'; 'left' is the kernel's search with `<` for
    `<=`); the numerators w + 1e-5 as fp32 forms them, everything after in fp64, rounded to fp32 at the very end."""
    w = (np.asarray(w, dtype=np.float32) + np.float32(1e-5)).astype(np.float32)
    t, w, u = (np.asarray(x, dtype=np.float64) for x in (t, w, u))
    u = np.broadcast_to(u, (t.shape[0], u.shape[-1]))
    out = np.empty((t.shape[0], t.shape[1] + u.shape[1]), dtype=np.float64)
    for r in range(t.shape[0]):
        bins = 0.5 * (t[r, 1:] + t[r, :-1])
        p = w[r, 1:-1]
        cdf = np.concatenate(([0.0], np.cumsum(p / p.sum())))
        idx = np.searchsorted(cdf, u[r], side=side)
        below, above = np.maximum(idx - 1, 0), np.minimum(idx, len(cdf) - 1)
        denom = cdf[above] - cdf[below]
        denom = np.where(denom < 1e-5, 1.0, denom)
        new = bins[below] + (u[r] - cdf[below]) / denom * (bins[above] - bins[below])
        out[r] = np.sort(np.concatenate((t[r], new)))
    assert side != "right" or np.array_equal(out, out.astype(np.float32).astype(np.float64)), "the fixture is not exactly representable in fp32"
    return torch.from_numpy(out.astype(np.float32))


def pdf_ordinary_inputs(coarse, fine, rays=9):
    """Peaky weights on jittered depths, u in [0, 1): what training feeds sample_pdf_kernel."""
    g = torch.Generator().manual_seed(100 * coarse + fine)
    t = O.perturb_intervals(O.coarse_intervals(2.0, 6.0, coarse, rays).contiguous(), torch.rand(rays, coarse, generator=g)).contiguous()
    return t, torch.rand(rays, coarse, generator=g) ** 4, torch.rand(rays, fine, generator=g)


def check_pdf_multiset(out, t, what):
    """`out` is sorted, holds every coarse depth bit-exactly with its multiplicity, and its other entries lie within
    [bins[0], bins[-1]].  Returns those other entries per ray."""
    out, t = np.asarray(out.cpu()), np.asarray(t)
    assert out.shape[0] == t.shape[0] and out.dtype == np.float32, what
    assert np.all(out[:, 1:] >= out[:, :-1]), f"{what}: not sorted"
    rest = []
    for r, (row, tc) in enumerate(zip(out, t)):
        left = list(row)
        for v in tc:
            assert v in left, f"{what}: ray {r} lost the coarse depth {v!r}"
            left.remove(v)
        bins = np.float32(0.5) * (tc[1:] + tc[:-1])
        assert all(bins[0] <= v <= bins[-1] for v in left), f"{what}: ray {r} has a sample outside [{bins[0]!r}, {bins[-1]!r}]"
        rest.append(left)
    return rest


def perturb_inputs(samples, rays=5):
    """Non-uniform depths and draws that contain exact zeros."""
    g = torch.Generator().manual_seed(samples)
    t = torch.sort(2.0 + 4.0 * torch.rand(rays, samples, generator=g), dim=-1).values.contiguous()
    rnd = torch.rand(rays, samples, generator=g)
    rnd[:, 0] = 0.0
    rnd[rays // 2] = 0.0
    return t, rnd
