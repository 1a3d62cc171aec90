"""What tests/test_gpu_ray_ops.py rests on, checked without a GPU (tests/composite_cases.py).

The GPU tests of the training path's ray operators are worth something only while their inputs really reach every kernel
instantiation and every regime (walls with alpha == 1.0f, occluded samples, empty rays, intervals of length 0), while the tolerance of
the compositing backward really is a small multiple of the kernel's own arithmetic, and while the resampling fixture really is exact.
All of that depends on constants and seeds only, so it is asserted here: a change of either cannot make the GPU tests vacuous
unnoticed."""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import composite_cases as CC


def test_case_ids_name_every_backward_instantiation():
    ids = [CC.case_id(c) for c in CC.CASES]
    assert len(set(ids)) == len(ids)
    for per in ("per1", "per2", "per3", "per4", "per8", "long"):
        assert any(f"-{per}-" in i and i.endswith("-all") for i in ids), per
        for k in CC.GRAD_KEYS:
            assert any(f"-{per}-" in i and i.endswith(f"-{k}_only") for i in ids), (per, k)
        mine = [c for c in CC.CASES if CC.per_of(c[0]) == per]
        assert {c[1] for c in mine} == {False, True} and {c[2] for c in mine} == {False, True}, f"{per}: white background / noise"
    assert [CC.per_of(s) for s in (1, 64, 65, 128, 129, 192, 193, 256, 257, 512, 513)] == \
        ["per1", "per1", "per2", "per2", "per3", "per3", "per4", "per4", "per8", "per8", "long"]
    assert tuple(c[0] for c in CC.ALL_GRAD_CASES) == CC.SAMPLE_COUNTS
    assert {CC.per_of(s) for s in CC.SOLO_COUNTS} == {"per1", "per2", "per3", "per4", "per8", "long"}
    assert CC.RAYS % 4 == 1 and CC.RAYS == 1 + len(CC.FAMILIES) * CC.FAMILY_RAYS


@pytest.mark.parametrize("samples", [7, 100, 300, 1025])
@pytest.mark.parametrize("with_noise", [False, True], ids=["nonoise", "noise"])
def test_ray_families_are_what_they_claim(samples, with_noise):
    rad, t, dirs, noise, G = CC.inputs(samples, with_noise)
    assert rad.shape == (61, samples, 4) and all(x.dtype == torch.float32 for x in (rad, t, dirs))
    assert (noise is not None) == with_noise
    assert not bool(dirs[0].any()) and bool((dirs[1:].norm(dim=-1) > 0).all())
    assert float((dirs.norm(dim=-1) - 1.0).abs()[1:].min()) > 1e-3, "a unit direction hides the norm"
    raw = rad[..., 3] + (noise if with_noise else 0.0)
    norm = dirs.norm(p=2, dim=-1)
    dist = torch.cat((t[:, 1:] - t[:, :-1], torch.full_like(t[:, :1], 1e10)), -1) * norm[:, None]
    alpha = 1.0 - torch.exp(-torch.relu(raw) * dist)
    keep = (1.0 - alpha) + torch.tensor(1e-10)
    trans = O.exclusive_cumprod(keep)
    r = CC.family_rays("empty")
    assert bool((raw[r.start:r.stop] <= 0).all())
    r = CC.family_rays("opaque")
    # (sigma = 1e4 over an interval shorter than 1.7e-3 leaves alpha just below 1: random depths have some, a quarter at 1025 samples)
    assert float((alpha[r.start:r.stop] == 1.0).float().mean()) > 0.5 and float((keep[r.start:r.stop] == torch.tensor(1e-10)).float().mean()) > 0.5
    assert bool((alpha[r.start:r.stop, -1] == 1.0).all())
    r = CC.family_rays("surface")
    a, k, tr = alpha[r.start:r.stop], keep[r.start:r.stop], trans[r.start:r.stop]
    assert bool((a == 1.0).any()) and bool((k == torch.tensor(1e-10)).any()), "no wall"
    assert bool(((tr < 1e-8) & (a > 0)).any()), "no occluded sample with density behind a wall"
    assert bool((a[:, 0] == 0).any()), "no empty space in front of a wall"
    r = CC.family_rays("dups")
    d = t[r.start:r.stop, 1:] - t[r.start:r.stop, :-1]
    assert bool((d >= 0).all()) and (samples < 64 or int((d == 0).sum()) > samples), "the rounded depths must collide"
    r = CC.family_rays("random")
    assert 0.2 < float((raw[r.start:r.stop] > 0).float().mean()) < 0.8
    # training mode: rays with acc < 1 keep their depth in the reference the GPU forward is held against
    fwd = O.composite(rad, t, dirs, CC.render_spec(samples, False), noise=noise)
    assert bool(((fwd["acc_map"] < 0.999) & (fwd["depth_map"] > 0)).any())


def _restatement_ratios(case):
    samples, white, with_noise, keys = case
    ref = CC.reference(case)
    got = CC.restated_backward(ref["rad"], ref["t"], ref["dirs"], ref["noise"], ref["G"], keys, white)
    return ref, got, CC.grad_ratios(got, ref)


@pytest.mark.parametrize("case", CC.CASES, ids=CC.case_id)
def test_restated_backward_stays_within_its_bound(case):
    """The kernel's arithmetic on the CPU against fp64 autograd, per ray: within RESTATEMENT_BOUND (6.5) x max(e32_r, q95) on every
    case, exactly 0 where the fp64 gradient is (the empty rays, the zero-direction ray), and within the GPU test's tolerance -- which
    is 2.5 x wider -- with room to spare.  The fp32 oracle itself must pass the GPU test's assertion too."""
    ref, got, ratios = _restatement_ratios(case)
    r = CC.family_rays("empty")
    assert bool(ref["zero"][0]) and bool(ref["zero"][r.start:r.stop].all())
    assert int((~ref["zero"]).sum()) >= 3 * CC.FAMILY_RAYS, "too few rays with a gradient"
    assert not bool(got[ref["zero"]].any())
    worst = CC.worst_by_family(ratios)
    print(CC.case_id(case), {k: round(v, 3) for k, v in worst.items()}, "q95", {n: float(ref["q95"][CC.family_rays(n).start]) for n in CC.FAMILIES})
    assert max(worst.values()) <= CC.RESTATEMENT_BOUND, worst
    CC.check_gradient(got, ref, "restatement")
    CC.check_gradient(CC.oracle_backward(ref["rad"], ref["t"], ref["dirs"], ref["noise"], ref["G"], case[3], case[1], torch.float32), ref, "fp32 oracle")


def _case(samples, keys):
    return next(c for c in CC.CASES if c[0] == samples and c[3] == keys)


@pytest.mark.parametrize("samples,key,family", [(7, "depth_map", "random"), (7, "weights", "dups"), (250, "weights", "surface"),
                                                (700, "weights", "surface")])
def test_one_minus_alpha_in_the_sigma_gradient_misses_the_tolerance(samples, key, family):
    """Why the backward kernels keep exp's result: with 1 - alpha in its place the gradient of a nearly opaque sample is off by
    6e-8 / (1 - alpha) of itself -- 8 to 31 x max(e32_r, q95) on short rays with one upstream gradient -- and a sample with
    alpha == 1.0f gets the gradient 0 where fp64 and the oracle's fp32 autograd agree on a non-zero one (err_r = 1)."""
    case = _case(samples, (key,))
    ref = CC.reference(case)
    got = CC.restated_backward(ref["rad"], ref["t"], ref["dirs"], ref["noise"], ref["G"], case[3], case[1], one_minus_alpha=True)
    worst = CC.worst_by_family(CC.grad_ratios(got, ref))
    print(CC.case_id(case), worst)
    assert worst[family] > CC.RESTATEMENT_BOUND
    if family == "surface":
        with pytest.raises(AssertionError, match="surface"):
            CC.check_gradient(got, ref, "1 - alpha")


@pytest.mark.parametrize("key", ["acc_map", "depth_map"])
def test_total_minus_prefix_misses_the_tolerance_behind_a_surface(key):
    """Why the long kernel walks its segments from the far end: behind a wall the sum of dL/dw_j * w_j over the samples still to
    come is 1e-10 of the total or less, and total - prefix is the rounding error of the total."""
    case = _case(700, (key,))
    ref = CC.reference(case)
    got = CC.restated_backward(ref["rad"], ref["t"], ref["dirs"], ref["noise"], ref["G"], case[3], case[1], total_minus_prefix=True)
    with pytest.raises(AssertionError, match="opaque"):
        CC.check_gradient(got, ref, "total - prefix")


@pytest.mark.parametrize("samples", [100, 700])
def test_check_gradient_sees_one_wrong_sample(samples):
    """One sample of one well-lit ray off by 1e-4 of that ray's largest gradient entry, an empty ray with one entry of 1e-30, and
    the suffix sum taken one sample too far: each is refused.  (The whole-tensor metric with its 5e-5 passes the first two.)"""
    case = _case(samples, CC.GRAD_KEYS if samples == 100 else ("rgb_map",))
    ref, got, _ = _restatement_ratios(case)
    CC.check_gradient(got, ref, "unchanged")
    ray = CC.family_rays("random").start
    seam = min(samples - 1, 64)
    wrong = got.clone()
    wrong[ray, seam, 3] += 1e-4 * float(ref["g64"][ray].abs().max())
    with pytest.raises(AssertionError, match="random"):
        CC.check_gradient(wrong, ref, "one sample")
    whole = float((wrong.double() - ref["g64"]).abs().max() / ref["g64"].abs().max())
    assert whole < 5e-5, "the whole-tensor metric of test_composite_forward_backward_vs_autograd would have passed this"
    wrong = got.clone()
    wrong[CC.family_rays("empty").start, 0, 3] = 1e-30
    with pytest.raises(AssertionError, match="exactly 0"):
        CC.check_gradient(wrong, ref, "empty ray")


def test_interior_weight_of_the_exact_fixture():
    w, eps = CC.PDF_INTERIOR_WEIGHT, np.float32(1e-5)
    assert w.dtype == np.float32 and np.float32(w + eps) == np.float32(0.25)
    assert (torch.tensor(float(w), dtype=torch.float32) + 1e-5).item() == 0.25


@pytest.mark.parametrize("per_ray", [True, False], ids=["u_per_ray", "u_shared"])
@pytest.mark.parametrize("coarse", CC.PDF_EXACT_COARSE)
def test_exact_fixture_oracle_equals_fp64_restatement(coarse, per_ray):
    """The oracle's fp32 SamplePDF equals the formula in fp64 bit for bit on the fixture: nothing in it rounds, so there is nothing
    for a correct kernel to differ in.  The forced draws are there, ties and the upper clamp included."""
    t, w, u = CC.pdf_exact_inputs(coarse, per_ray)
    n = coarse - 2
    fine = 4 * n + 3
    assert n & (n - 1) == 0 and u.shape[-1] == fine and bool(torch.isnan(w[:, 0]).all()) and bool(torch.isnan(w[:, -1]).all())
    rows = u if per_ray else u[None]
    for row in rows:
        k = (row.double() * 8 * n).round().long().tolist()
        assert {0, 8, 8 * n - 1, 8 * n} <= set(k)
    assert float(rows.max()) == 1.0 and float(rows.min()) == 0.0
    ref = O.sample_pdf_intervals(t, w, fine, u=u if per_ray else u.expand(t.shape[0], fine))
    assert ref.dtype == torch.float32 and bool(torch.isfinite(ref).all())
    assert torch.equal(ref, CC.pdf_restated_fp64(t, w, u))
    # the cdf the fixture promises
    cdf = torch.cumsum((w[0, 1:-1] + 1e-5) / (w[0, 1:-1] + 1e-5).sum(), 0)
    assert torch.equal(cdf, torch.arange(1, n + 1, dtype=torch.float32) / n)
    # the tie: u == cdf[1] belongs to the bin that STARTS there (sample == bins[1]), not to the end of the one before
    new = CC.check_pdf_multiset(ref, t, "oracle")
    bins = 0.5 * (t[0, 1:] + t[0, :-1])
    for r, row in enumerate(rows.expand(t.shape[0], fine)):
        ties = int((row == 1.0 / n).sum()) if n > 1 else 0
        assert new[r].count(float(bins[1])) >= ties


@pytest.mark.parametrize("per_ray", [True, False], ids=["u_per_ray", "u_shared"])
@pytest.mark.parametrize("m", CC.PDF_THIN_M)
def test_thin_bin_fixture_is_exact_and_sees_the_tie_rule(m, per_ray):
    """A bin below the 1e-5 denominator clamp: still nothing rounds (oracle == fp64 restatement bit for bit), and searching with
    `<` for `<=` (side='left') moves the sample drawn at the thin bin's end by a bin -- on every ray.  The fixture without a thin
    bin cannot tell the two searches apart: its inverse cdf is continuous."""
    e = np.float32(1e-5)
    assert np.float32(CC.PDF_THIN_WEIGHT + e) == np.float32(2.0 ** -16)
    assert np.float32(CC.PDF_REDUCED_WEIGHT + e) == np.float32(0.25) - np.float32(2.0 ** -16)
    t, w, u = CC.pdf_thin_bin_inputs(m, per_ray)
    fine = u.shape[-1]
    full = u if per_ray else u.expand(t.shape[0], fine)
    ref = O.sample_pdf_intervals(t, w, fine, u=full)
    assert torch.equal(ref, CC.pdf_restated_fp64(t, w, u))
    other = CC.pdf_restated_fp64(t, w, u, side="left")
    assert bool((ref != other).any(1).all()), "the tie is not drawn on every ray"
    j = min(m // 2, 63)
    p = (w[0, 1:-1] + 1e-5) / (w[0, 1:-1] + 1e-5).sum()
    assert float(p[j]) < 1e-5 and float(p.sum()) == 1.0 and float(torch.cumsum(p, 0)[j + 1]) == (j + 1) / m
    t0, w0, u0 = CC.pdf_exact_inputs(m + 2, per_ray)
    assert torch.equal(CC.pdf_restated_fp64(t0, w0, u0), CC.pdf_restated_fp64(t0, w0, u0, side="left"))


@pytest.mark.parametrize("coarse,fine", CC.PDF_MULTISET_SHAPES)
def test_multiset_property_holds_for_the_oracle(coarse, fine):
    t, w, u = CC.pdf_ordinary_inputs(coarse, fine)
    rest = CC.check_pdf_multiset(O.sample_pdf_intervals(t, w, fine, u=u), t, "oracle")
    assert all(len(r) == fine for r in rest)
    broken = O.sample_pdf_intervals(t, w, fine, u=u).clone()
    broken[0, 0] += 1.0                                      # a lost coarse depth / an unsorted row is seen
    with pytest.raises(AssertionError):
        CC.check_pdf_multiset(broken, t, "broken")


@pytest.mark.parametrize("samples", [1, 2, 65])
def test_perturb_inputs(samples):
    t, rnd = CC.perturb_inputs(samples)
    assert t.shape == rnd.shape == (5, samples) and bool((rnd == 0).any()) and bool((rnd < 1).all())
    assert samples < 3 or float((t[:, 2:] - 2 * t[:, 1:-1] + t[:, :-2]).abs().max()) > 1e-3, "uniform depths"
    out = O.perturb_intervals(t, rnd)
    assert torch.equal(out[rnd == 0], torch.cat((t[:, :1], 0.5 * (t[:, 1:] + t[:, :-1])), -1)[rnd == 0])
