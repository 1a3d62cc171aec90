"""The training path's ray operators (nerfmeshes_amd/csrc/ray_ops.hip) on the MI355X: every compositing-backward instantiation and
the long kernel per ray against fp64 autograd over the oracle, the training-mode forward per ray against the oracle, rays independent
of each other bit for bit, the inverse-CDF resampling and the stratified jitter bit for bit against the oracle.

Inputs, references and the tolerance live in tests/composite_cases.py; tests/test_ray_ops_inputs.py checks them without a GPU."""
import pytest
import torch

from oracle import nerf_oracle as O
from tests import composite_cases as CC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from nerfmeshes_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def T():
    from nerfmeshes_amd import train_ops
    return train_ops


def _gpu_backward(T, ref, case, rows=slice(None)):
    """(bundle, gradient with respect to the radiance) of train_ops.composite on the rays `rows` of a case; the upstream gradients
    that the case leaves out are absent (autograd passes None), not zero tensors."""
    samples, white, _, keys = case
    r = ref["rad"][rows].cuda().requires_grad_(True)
    noise = None if ref["noise"] is None else ref["noise"][rows].cuda()
    b = T.composite(r, ref["t"][rows].cuda(), ref["dirs"][rows].cuda(), noise, CC.render_spec(samples, white).attenuation_threshold, white)
    sum((b[k] * ref["G"][k][rows].cuda()).sum() for k in keys).backward()
    return b, r.grad


@pytest.mark.parametrize("case", CC.CASES, ids=CC.case_id)
def test_composite_backward_per_ray_vs_fp64_autograd(T, case):
    ref = CC.reference(case)
    _, grad = _gpu_backward(T, ref, case)
    ratios = CC.grad_ratios(grad, ref)
    print("worst err_r / max(e32_r, q95) per family:", CC.case_id(case), {k: round(v, 3) for k, v in CC.worst_by_family(ratios).items()})
    CC.check_gradient(grad, ref, CC.case_id(case))


@pytest.mark.parametrize("case", CC.ALL_GRAD_CASES, ids=CC.case_id)
def test_composite_training_forward_per_ray_vs_oracle(T, case):
    """weights, rgb_map, acc_map and depth_map of every ray against the fp32 oracle at test_composite_vs_oracle's budget (absolute
    plus relative 2e-6, growing with the count beyond 256); in training mode the depth is not zeroed where acc < 1."""
    samples, white, _, _ = case
    ref = CC.reference(case)
    with torch.no_grad():
        noise = None if ref["noise"] is None else ref["noise"].cuda()
        got = T.composite(ref["rad"].cuda(), ref["t"].cuda(), ref["dirs"].cuda(), noise, 1e-5, white)
    want = ref["forward32"]
    tol = 2e-6 * max(1.0, samples / 256.0)
    for k in ("weights", "rgb_map", "acc_map", "depth_map"):
        g, w = got[k].cpu().reshape(CC.RAYS, -1), want[k].reshape(CC.RAYS, -1)
        assert g.shape == w.shape, k
        over = ((g - w).abs() > tol + tol * w.abs()).any(1)
        assert not bool(over.any()), (k, [(r, CC.family_of(r), float((g[r] - w[r]).abs().max())) for r in torch.nonzero(over).flatten().tolist()])
    assert float((got["mask_weights"].cpu() != want["mask_weights"]).float().mean()) < 1e-4
    r = CC.family_rays("empty")
    for k in ("weights", "acc_map", "depth_map"):
        assert not bool(got[k][0].any()) and not bool(got[k][r.start:r.stop].any()), f"{k}: a ray without density or without direction"


@pytest.mark.parametrize("samples", CC.INDEPENDENCE_COUNTS, ids=lambda s: f"s{s}-{CC.per_of(s)}")
def test_composite_backward_rays_are_independent(T, samples):
    """One wave owns one ray: the gradient of the batch equals, bit for bit, the gradients of its rays computed one at a time (every
    ray in wave 0 of block 0) and of the batch in reverse order (every ray in another wave slot, another block)."""
    case = next(c for c in CC.ALL_GRAD_CASES if c[0] == samples)
    ref = CC.reference(case)
    bundle, whole = _gpu_backward(T, ref, case)
    back = torch.arange(CC.RAYS - 1, -1, -1)
    b_rev, rev = _gpu_backward(T, ref, case, back)
    assert torch.equal(rev.flip(0), whole)
    for k in ("weights", "rgb_map", "acc_map", "depth_map"):
        assert torch.equal(b_rev[k].flip(0), bundle[k]), k
    for r in range(CC.RAYS):
        b_one, one = _gpu_backward(T, ref, case, slice(r, r + 1))
        assert torch.equal(one[0], whole[r]), (r, CC.family_of(r))
        assert torch.equal(b_one["weights"][0], bundle["weights"][r]), (r, CC.family_of(r))


# ---- inverse-CDF resampling ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coarse", CC.PDF_EXACT_COARSE)
def test_sample_pdf_rand_equals_the_oracle_on_the_exact_fixture(T, coarse):
    """Per-ray u (the training branch of sample_pdf_kernel): nothing in the fixture rounds, so the kernel, the oracle and the fp64
    restatement agree bit for bit -- the tie u == cdf[1], u == 0, u == 1.0 and the cdf carry between 64-wide chunks included."""
    t, w, u = CC.pdf_exact_inputs(coarse, per_ray=True)
    want = O.sample_pdf_intervals(t, w, u.shape[1], u=u)
    got = T.sample_pdf_rand(t.cuda(), w.cuda(), u.cuda()).cpu()
    assert torch.equal(got, want), (coarse, int((got != want).sum()), float((got - want).abs().max()))


@pytest.mark.parametrize("coarse", CC.PDF_EXACT_COARSE)
def test_sample_pdf_shared_u_equals_the_oracle_on_the_exact_fixture(ops, coarse):
    """One u row for all rays (the render path's entry point), exactly 1.0 among them: both indices clamp to the last bin and the
    zero denominator becomes 1."""
    t, w, u = CC.pdf_exact_inputs(coarse, per_ray=False)
    assert float(u.max()) == 1.0
    want = O.sample_pdf_intervals(t, w, u.numel(), u=u.expand(t.shape[0], u.numel()))
    got = ops.sample_pdf(t.cuda(), w.cuda(), u.cuda()).cpu()
    assert torch.equal(got, want), (coarse, int((got != want).sum()), float((got - want).abs().max()))


@pytest.mark.parametrize("m", CC.PDF_THIN_M)
def test_sample_pdf_equals_the_oracle_next_to_a_bin_below_the_clamp(ops, T, m):
    """The exact fixture with one bin thinner than the 1e-5 denominator clamp: u at that bin's end belongs to the NEXT bin
    (searchsorted right=True, `cdf[mid] <= u`), a whole bin away from where `<` puts it.  Per-ray and shared u."""
    t, w, u = CC.pdf_thin_bin_inputs(m, per_ray=True)
    want = O.sample_pdf_intervals(t, w, u.shape[1], u=u)
    got = T.sample_pdf_rand(t.cuda(), w.cuda(), u.cuda()).cpu()
    assert torch.equal(got, want), (m, int((got != want).sum()), float((got - want).abs().max()))
    t, w, u = CC.pdf_thin_bin_inputs(m, per_ray=False)
    want = O.sample_pdf_intervals(t, w, u.numel(), u=u.expand(t.shape[0], u.numel()))
    got = ops.sample_pdf(t.cuda(), w.cuda(), u.cuda()).cpu()
    assert torch.equal(got, want), (m, int((got != want).sum()), float((got - want).abs().max()))


@pytest.mark.parametrize("coarse,fine", CC.PDF_MULTISET_SHAPES)
def test_sample_pdf_rand_keeps_every_coarse_depth(T, coarse, fine):
    """Ordinary inputs (peaky weights, jittered depths): the output is sorted, every coarse depth is in it bit-exactly with its
    multiplicity, and the `fine` other entries lie within [bins[0], bins[-1]]."""
    t, w, u = CC.pdf_ordinary_inputs(coarse, fine)
    got = T.sample_pdf_rand(t.cuda(), w.cuda(), u.cuda())
    assert got.shape == (t.shape[0], coarse + fine)
    rest = CC.check_pdf_multiset(got, t, f"({coarse}, {fine})")
    assert all(len(r) == fine for r in rest)


# ---- stratified jitter -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [1, 2, 65])
def test_perturb_intervals_equals_the_oracle(T, samples):
    t, rnd = CC.perturb_inputs(samples)
    assert torch.equal(T.perturb_intervals(t.cuda(), rnd.cuda()).cpu(), O.perturb_intervals(t, rnd))
