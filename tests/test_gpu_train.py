"""Training path on the MI355X against torch autograd over the CPU oracle.

The reference trains through torch autograd (model_nerf.py:88-151); the oracle's functions are the same torch ops,
so `torch.autograd` over them in fp64 is the ground-truth gradient and in fp32 the reference's own noise floor.
Tolerances are relative to each tensor's largest entry (fp32 sums over up to 1e4 samples in a different order)."""
import numpy as np
import pytest
import torch

from tests.helpers import O, S

pytestmark = pytest.mark.gpu

# worst relative error of a gradient entry / projection / norm against the reference's full-size training step
FULL_SIZE_GRAD_TOL = 1e-3   # measured worst: entry 1.6e-4, projection 1.7e-4, norm 5.8e-5 (profiles/r02_raw/train_step_full_errors.json)

SHAPES = [
    dict(num_layers=4, hidden_size=64, skip_step=2, num_encoding_fn_xyz=6, num_encoding_fn_dir=4),
    dict(num_layers=8, hidden_size=256, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4),
    dict(num_layers=3, hidden_size=128, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4),   # no skip layer
]


@pytest.fixture(scope="module")
def ops():
    from nerfmeshes_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def T():
    from nerfmeshes_amd import train_ops
    return train_ops


def _weights(kw, seed=5):
    w = S.make_mlp_weights(seed, density_gain=30.0, density_bias=0.3, **kw)
    return {k: torch.as_tensor(np.asarray(v), dtype=torch.float32) for k, v in w.items()}


def _rays(rays, samples, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.tensor([[0.2, -0.1, 3.5]]) + 0.1 * torch.randn(rays, 3, generator=g)
    d = torch.nn.functional.normalize(torch.tensor([[0.0, 0.1, -1.0]]) + 0.3 * torch.randn(rays, 3, generator=g), dim=-1)
    t = torch.sort(2.0 + 4.0 * torch.rand(rays, samples, generator=g), dim=-1).values
    return o, d, t


def _rel(got, ref):
    ref = ref.detach().to(torch.float64).cpu()
    got = got.detach().to(torch.float64).cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _oracle_grads(w, spec, o, d, t, grad_out, dtype):
    wd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in w.items() if "frequency" not in k}
    pts = O.ray_points(t.to(dtype), d.to(dtype), o.to(dtype)).reshape(-1, 3)
    dirs = d.to(dtype)[:, None, :].expand(-1, t.shape[1], -1).reshape(-1, 3)
    out = O.mlp_forward(wd, spec, pts, dirs, keep_graph=True)
    (out * grad_out.to(dtype).reshape(-1, 4)).sum().backward()
    return out.detach(), {k: v.grad for k, v in wd.items()}


FLAT_SHAPES = [
    dict(num_layers=4, hidden_size=64, skip_step=2, num_encoding_fn_xyz=6, num_encoding_fn_dir=4, use_viewdirs=False),
    dict(num_layers=8, hidden_size=256, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=False),
    dict(num_layers=5, hidden_size=128, skip_step=2, num_encoding_fn_xyz=10, num_encoding_fn_dir=2, use_viewdirs=False),
]


@pytest.mark.parametrize("kw", FLAT_SHAPES, ids=["4x64", "8x256", "5x128"])
@pytest.mark.parametrize("rays,samples", [(37, 9), (128, 16)])
def test_training_a_network_without_view_directions_vs_autograd(ops, T, kw, rays, samples):
    """FlexibleNeRFModel(use_viewdirs=False) (models.py:52-55, 77-79) through the training entry points: the taping kernel's
    mode 2 reproduces the inference output bit for bit and tapes the trunk (the last activation by an explicit store: no
    stage follows that would write it), the FLAT delta kernel starts from fc_out^T applied to the four head deltas; all
    L + 1 weight / bias gradient pairs against fp64 autograd over the oracle, at the view networks' tolerance."""
    spec = O.MLPSpec(**kw)
    w = _weights(kw)
    mlp = ops.HipMLP(w, kw, "cuda")
    o, d, t = _rays(rays, samples, rays)
    grad_out = torch.randn(rays, samples, 4, generator=torch.Generator().manual_seed(1))
    rad, tape = T.forward_train(mlp, o.cuda(), d.cuda(), t.cuda())
    assert torch.equal(rad, mlp.eval_rays(o.cuda(), d.cuda(), t.cuda())), "the taping kernel must not change the output"
    assert tape["feat"] is None and tape["v"] is None and tape["mask_v"] is None, "a trunk-only tape"
    ref32, g32 = _oracle_grads(w, spec, o, d, t, grad_out, torch.float32)
    ref64, g64 = _oracle_grads(w, spec, o, d, t, grad_out, torch.float64)
    assert _rel(rad.reshape(-1, 4), ref64) < max(2e-5, 4 * _rel(ref32, ref64))
    assert float(tape["h"][1:].min()) >= 0.0
    # the last trunk activation is the operand of fc_out's gradient: check it against the oracle's trunk
    pts = O.ray_points(t, d, o).reshape(-1, 3)
    x = O.positional_encoding(pts, kw["num_encoding_fn_xyz"])
    h = torch.nn.functional.linear(x, w["layer1.weight"], w["layer1.bias"])
    for i in range(kw["num_layers"] - 1):
        if spec.is_skip(i):
            h = torch.cat((h, x), -1)
        h = torch.relu(torch.nn.functional.linear(h, w[f"layers_xyz.{i}.weight"], w[f"layers_xyz.{i}.bias"]))
    assert _rel(tape["h"][-1], h) < 2e-5
    got = T.backward(mlp, tape, rad, grad_out.cuda(), o.cuda(), d.cuda(), t.cuda())
    assert set(got) == set(g64) == set(T.param_names(kw["num_layers"], use_viewdirs=False))
    worst = {k: (_rel(got[k], ref), _rel(g32[k], ref)) for k, ref in g64.items()}
    bad = {k: v for k, v in worst.items() if v[0] > max(2e-4, 20 * v[1])}
    assert not bad, f"gradient mismatch (ours, torch-fp32) relative to fp64 autograd: {bad}"


def test_adam_trains_a_network_without_view_directions(ops):
    """End to end through the module surface: NeRF-style training iterations of a use_viewdirs=False FlexibleNeRFModel (the
    differentiable forward used to raise NotImplementedError): the loss falls, and the eval path follows the new weights."""
    from nerfmeshes_amd.nerf import FlexibleNeRFModel
    torch.manual_seed(0)
    net = FlexibleNeRFModel(num_layers=4, hidden_size=128, skip_step=4, num_encoding_fn_xyz=6, use_viewdirs=False).cuda()
    opt = torch.optim.Adam(net.parameters(), lr=2e-3)
    pts = (torch.rand(4096, 3, device="cuda") - 0.5) * 2.0
    target = torch.cat((torch.sigmoid(3.0 * pts), pts.norm(dim=-1, keepdim=True)), -1)
    losses = []
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.mse_loss(net(pts), target)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < 0.5 * losses[0], losses
    with torch.no_grad():
        assert abs(float(torch.nn.functional.mse_loss(net(pts), target)) - losses[-1]) < 0.5 * losses[-1]


@pytest.mark.parametrize("kw", SHAPES, ids=["4x64", "8x256", "3x128"])
def test_refresh_equals_create(ops, T, kw):
    """nm_mlp_refresh (device gather from live tensors) == nm_mlp_create from the same values, bit for bit."""
    a, b = _weights(kw, 5), _weights(kw, 6)
    m_a, m_b = ops.HipMLP(a, kw, "cuda"), ops.HipMLP(b, kw, "cuda")
    p = torch.randn(1000, 3).cuda()
    before = m_a.sample_points(p, p).clone()
    T.refresh(m_a, {k: v.cuda() for k, v in b.items()})
    after = m_a.sample_points(p, p)
    assert not torch.equal(before, after)
    assert torch.equal(after, m_b.sample_points(p, p))


@pytest.mark.parametrize("kw", SHAPES, ids=["4x64", "8x256", "3x128"])
@pytest.mark.parametrize("rays,samples", [(37, 9), (128, 16)])
def test_mlp_tape_and_backward_vs_autograd(ops, T, kw, rays, samples):
    spec = O.MLPSpec(**kw)
    w = _weights(kw)
    mlp = ops.HipMLP(w, kw, "cuda")
    o, d, t = _rays(rays, samples, rays)
    g = torch.Generator().manual_seed(1)
    grad_out = torch.randn(rays, samples, 4, generator=g)

    rad, tape = T.forward_train(mlp, o.cuda(), d.cuda(), t.cuda())
    assert torch.equal(rad, mlp.eval_rays(o.cuda(), d.cuda(), t.cuda())), "the taping kernel must not change the output"
    ref32, g32 = _oracle_grads(w, spec, o, d, t, grad_out, torch.float32)
    ref64, g64 = _oracle_grads(w, spec, o, d, t, grad_out, torch.float64)
    assert _rel(rad.reshape(-1, 4), ref64) < max(2e-5, 4 * _rel(ref32, ref64))   # fp32 sin/cos of x * 2^9

    # the tape rows are the network's activations (checked on the last trunk layer and the view layer)
    n, L = rays * samples, kw["num_layers"]
    assert tape["h"].shape == (L, n, kw["hidden_size"])
    enc_x, enc_d = T.encode_samples(mlp, o.cuda(), d.cuda(), t.cuda())
    pts = O.ray_points(t, d, o).reshape(-1, 3)
    ref_enc = O.positional_encoding(pts, kw["num_encoding_fn_xyz"])
    assert _rel(enc_x, ref_enc) < 1e-6
    h0 = torch.nn.functional.linear(ref_enc, w["layer1.weight"], w["layer1.bias"])
    if tape["h0_taped"]:       # (not written where the backward that will run takes layer1's / layers_xyz[0]'s gradients by linearity)
        assert _rel(tape["h"][0], h0) < 1e-5
    assert float(tape["h"][1:].min()) >= 0.0 and float(tape["feat"].min()) >= 0.0 and float(tape["v"].min()) >= 0.0

    got = T.backward(mlp, tape, rad, grad_out.cuda(), o.cuda(), d.cuda(), t.cuda())
    worst = {}
    for k, ref in g64.items():
        assert got[k].shape == ref.shape, k
        worst[k] = (_rel(got[k], ref), _rel(g32[k], ref))
    bad = {k: v for k, v in worst.items() if v[0] > max(2e-4, 20 * v[1])}
    assert not bad, f"gradient mismatch (ours, torch-fp32) relative to fp64 autograd: {bad}"


@pytest.mark.parametrize("rays,samples,white", [(5, 7, False), (64, 64, False), (33, 192, True), (9, 700, False), (7, 1100, True)])
def test_composite_forward_backward_vs_autograd(ops, T, rays, samples, white):
    g = torch.Generator().manual_seed(samples)
    rad = torch.cat((torch.rand(rays, samples, 3, generator=g), 3.0 * torch.randn(rays, samples, 1, generator=g)), -1)
    _, d, t = _rays(rays, samples, 3)
    noise = torch.randn(rays, samples, generator=g)
    G = dict(rgb_map=torch.randn(rays, 3, generator=g), acc_map=torch.randn(rays, generator=g),
             depth_map=torch.randn(rays, generator=g), weights=torch.randn(rays, samples, generator=g))
    rs = O.RenderSpec(num_coarse=samples, num_fine=0, white_background=white, training=True)

    def loss_of(bundle, dtype):
        return sum((bundle[k] * G[k].to(dtype)).sum() for k in G)

    r64 = rad.double().requires_grad_(True)
    b64 = O.composite(r64, t.double(), d.double(), rs, noise=noise.double())
    loss_of(b64, torch.float64).backward()

    r_gpu = rad.cuda().requires_grad_(True)
    b = T.composite(r_gpu, t.cuda(), d.cuda(), noise.cuda(), rs.attenuation_threshold, white)
    b32 = O.composite(rad, t, d, rs, noise=noise)
    for k in ("rgb_map", "acc_map", "depth_map", "weights"):
        assert _rel(b[k], b32[k]) < 2e-6, k
    sum((b[k] * G[k].cuda()).sum() for k in G).backward()
    assert _rel(r_gpu.grad, r64.grad) < 5e-5
    # rgb_map-only loss (the reference's): the other upstream gradients are absent, not zero tensors
    r2 = rad.cuda().requires_grad_(True)
    (T.composite(r2, t.cuda(), d.cuda(), noise.cuda(), rs.attenuation_threshold, white)["rgb_map"] ** 2).sum().backward()
    r64b = rad.double().requires_grad_(True)
    (O.composite(r64b, t.double(), d.double(), rs, noise=noise.double())["rgb_map"] ** 2).sum().backward()
    assert _rel(r2.grad, r64b.grad) < 5e-5


def test_stochastic_samplers_match_the_oracle_given_the_draws(ops, T):
    g = torch.Generator().manual_seed(9)
    rays, nc, nf = 333, 64, 128
    t = O.coarse_intervals(torch.tensor(2.0), torch.tensor(6.0), nc, rays).contiguous()
    rnd = torch.rand(rays, nc, generator=g)
    tp = T.perturb_intervals(t.cuda(), rnd.cuda())
    ref = O.perturb_intervals(t, rnd)
    assert torch.equal(tp.cpu(), ref)
    weights = torch.rand(rays, nc, generator=g) ** 4
    u = torch.rand(rays, nf, generator=g)
    got = T.sample_pdf_rand(ref.cuda(), weights.cuda(), u.cuda()).cpu()
    want = O.sample_pdf_intervals(ref, weights, nf, u=u)
    assert got.shape == want.shape and bool((got[:, 1:] >= got[:, :-1]).all())
    # same multiset of depths up to the round-off of (u - cdf) / denom in nearly empty bins
    assert float((got - want).abs().max()) < 2e-3 and float((got - want).abs().median()) == 0.0


def _model(cfg_kw, seed=0):
    from nerfmeshes_amd import models
    from nerfmeshes_amd.nerf import CfgNode
    cfg = CfgNode(S.hparams(**cfg_kw))
    torch.manual_seed(seed)
    return models.NeRFModel(cfg).cuda()


def _end_to_end_loss_gradients(num_coarse, num_fine):
    kw = dict(num_layers=4, hidden_size=64, skip_step=2, num_encoding_fn_xyz=6, num_encoding_fn_dir=4)
    model = _model(dict(num_coarse=num_coarse, num_fine=num_fine, train_noise_std=0.0, **kw))
    with torch.no_grad():     # a scene with visible structure: scale sigma
        for net in (model.model_coarse, model.model_fine):
            net.fc_alpha.weight.mul_(40.0)
    model.train()
    rays = 257
    o, d, _ = _rays(rays, 2, 11)
    target = torch.rand(rays, 3, generator=torch.Generator().manual_seed(2))
    bounds = torch.tensor([2.0, 6.0])
    coarse, fine = model((o[:1].cuda(), d.cuda(), bounds))
    loss = torch.nn.functional.mse_loss(coarse.rgb_map, target.cuda()) + torch.nn.functional.mse_loss(fine.rgb_map, target.cuda())
    loss.backward()

    spec = O.MLPSpec(**kw)
    rs = O.RenderSpec(num_coarse=num_coarse, num_fine=num_fine, training=True)
    total, grads = 0.0, {}
    t_c = O.coarse_intervals(2.0, 6.0, num_coarse, rays)
    # the fine depths the model used: the same kernel call on the same coarse weights (the oracle's inverse CDF moves a
    # few depths in thin pdf bins, which is the resampling's conditioning and not what this test is about)
    from nerfmeshes_amd import hip_ops
    t_f = hip_ops.sample_pdf(t_c.cuda(), coarse.weights.detach(), model.sample_pdf.u).cpu()
    assert float((t_f - O.sample_pdf_intervals(t_c, coarse.weights.detach().cpu(), num_fine)).abs().median()) == 0.0
    for name, net, t in (("model_coarse", model.model_coarse, t_c), ("model_fine", model.model_fine, t_f)):
        wd = {k: v.detach().double().cpu().requires_grad_(True) for k, v in net.named_parameters()}
        pts = O.ray_points(t.double(), d.double(), o[:1].double()).reshape(-1, 3)
        dirs = d.double()[:, None, :].expand(-1, t.shape[1], -1).reshape(-1, 3)
        rad = O.mlp_forward(wd, spec, pts, dirs, keep_graph=True).reshape(rays, -1, 4)
        b = O.composite(rad, t.double(), d.double(), rs)
        l = torch.nn.functional.mse_loss(b["rgb_map"], target.double())
        l.backward()
        total += float(l.detach())
        grads[name] = {k: v.grad for k, v in wd.items()}
    assert abs(float(loss.detach()) - total) < 1e-5 * max(1.0, total)
    for name, net in (("model_coarse", model.model_coarse), ("model_fine", model.model_fine)):
        for k, p in net.named_parameters():
            assert p.grad is not None, (name, k)
            assert _rel(p.grad, grads[name][k]) < 5e-4, (name, k, _rel(p.grad, grads[name][k]))


def test_end_to_end_loss_gradients_vs_oracle_autograd():
    """NeRFModel.forward in train() mode, loss as training_step's (coarse + fine MSE), backward: gradients of all
    54 parameter tensors against fp64 autograd through the oracle on the SAME sample depths."""
    _end_to_end_loss_gradients(16, 16)


def test_end_to_end_loss_gradients_with_a_100_sample_fine_pass():
    """The same with 40 + 60 samples: the fine pass composites 100 samples per ray, two per lane (composite_kernel<2> and
    composite_backward_kernel<2>, which no 16 + 16 configuration reaches)."""
    _end_to_end_loss_gradients(40, 60)


@pytest.mark.parametrize("adam", [dict(), dict(fused=True), dict(foreach=False)], ids=["multi-tensor", "fused", "single-tensor"])
def test_adam_steps_reduce_the_loss_and_eval_follows_the_new_weights(adam):
    """A few optimizer steps on one ray batch: the loss falls, and the inference path (nm_render_rays) sees the
    updated parameters (device re-pack) -- it equals a model rebuilt from the new state_dict.  Every implementation of the
    optimizer: torch's fused Adam updates the tensors without moving autograd's version counters, which the re-pack used to key on
    alone (the model then trained on its initial weights for ever; round 5: train_ops.generation())."""
    kw = dict(num_layers=4, hidden_size=64, skip_step=2, num_encoding_fn_xyz=6, num_encoding_fn_dir=4)
    hp = dict(num_coarse=16, num_fine=16, train_noise_std=0.0, **kw)
    model = _model(hp, seed=3)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=5e-3, **adam)
    o, d, _ = _rays(512, 2, 4)
    target = (0.5 + 0.5 * torch.sin(7.0 * d)).cuda()
    batch = (o[:1].cuda(), d.cuda(), torch.tensor([2.0, 6.0]))
    losses = []
    for _ in range(25):
        opt.zero_grad()
        c, f = model(batch)
        loss = torch.nn.functional.mse_loss(c.rgb_map, target) + torch.nn.functional.mse_loss(f.rgb_map, target)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < 0.7 * losses[0], losses
    model.eval()
    with torch.no_grad():
        got = model.query(batch).rgb_map
    fresh = _model(hp, seed=99)
    fresh.load_state_dict(model.state_dict())
    fresh.eval()
    with torch.no_grad():
        want = fresh.query(batch).rgb_map
    assert torch.equal(got, want)


@pytest.mark.parametrize("kw", SHAPES + FLAT_SHAPES[:1], ids=["4x64", "8x256", "3x128", "4x64-flat"])
@pytest.mark.parametrize("rays,samples", [(37, 9), (256, 16)])
def test_the_taping_forward_writes_the_encoding_rows_the_backward_used_to_recompute(ops, T, kw, rays, samples):
    """Round 6: the tuned taping kernels write the PositionalEncoding row of every sample point / view direction (modules.py:26-34,
    reference column order, 64 floats per sample) from the registers they encode into anyway (nm_mlp_tape.d_enc_xyz / d_enc_dir);
    the backward contracts the layer1 / skip / view deltas with those rows instead of running nm_encode_samples_strided.  The rows
    equal that kernel's output bit for bit on every column of the encoding; the gradients are unchanged (the tests above)."""
    import ctypes as C
    from nerfmeshes_amd import _lib
    lib = _lib.load()
    w = _weights(kw)
    mlp = ops.HipMLP(w, kw, "cuda")
    assert lib.nm_mlp_tapes_encodings(mlp.handle) == 1
    o, d, t = _rays(rays, samples, 21)
    o, d, t = o[:1].cuda(), d.cuda(), t.cuda().contiguous()
    _, tape = T.forward_train(mlp, o, d, t)
    torch.cuda.synchronize()
    dx, dd = 6 * kw["num_encoding_fn_xyz"] + 3, 6 * kw["num_encoding_fn_dir"] + 3
    flat = not kw.get("use_viewdirs", True)
    n = rays * samples
    ex = torch.full((n, 64), float("nan"), device="cuda")
    ed = torch.full((n, 64), float("nan"), device="cuda")
    ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    assert lib.nm_encode_samples_strided(mlp.handle, ptr(o), 0, ptr(d), ptr(t), rays, samples, ptr(ex), 64, None if flat else ptr(ed), 64,
                                         None) == 0, lib.nm_last_error()
    torch.cuda.synchronize()
    assert tape["enc_x"].shape == (n, 64) and torch.equal(tape["enc_x"][:, :dx], ex[:, :dx])
    if flat:
        assert tape["enc_d"] is None
    else:
        assert torch.equal(tape["enc_d"][:, :dd], ed[:, :dd])
    # a generic-family handle says so and leaves the job to the separate pass
    g = dict(num_layers=3, hidden_size=100, skip_step=2, num_encoding_fn_xyz=5, num_encoding_fn_dir=2)
    assert lib.nm_mlp_tapes_encodings(ops.HipMLP(_weights(g), g, "cuda").handle) == 0


def _render_after(model, batch, edit):
    """(rgb rendered after `edit`, rgb of a model rebuilt from the edited state_dict, re-packs the edit's render cost)."""
    model.eval()
    with torch.no_grad():
        model.query(batch)                        # the handles exist and hold the un-edited parameters
        before = model.model_fine.refresh_count()
        edit(model)
        got = model.query(batch).rgb_map
        packs = model.model_fine.refresh_count() - before
        fresh = _model(model._test_hp, seed=99)
        fresh.load_state_dict(model.state_dict())
        fresh.eval()
        want = fresh.query(batch).rgb_map
    return got, want, packs


def _scale_data(model):                           # invisible to autograd's version counters and to every optimizer hook
    for p in model.parameters():
        p.data.mul_(1.25)


def _foreach_data(model):
    torch._foreach_add_([p.data for p in model.parameters()], 0.01)


@pytest.mark.parametrize("edit", [_scale_data, _foreach_data], ids=["p.data.mul_", "_foreach_add_ on .data"])
def test_edits_the_host_cannot_see_reach_the_kernels_or_raise(edit, monkeypatch):
    """VERDICT r5 weak 3.  The reference's forward reads the nn.Parameter storages (models.py:60-80), so an edit through `p.data` or
    a torch._foreach_* op on `.data` is simply seen by the next forward.  Here the kernels read a packed copy:
      * default guard ("always"): the copy is rebuilt on the stream in front of every use -- the render equals a model rebuilt
        from the edited state_dict bit for bit;
      * "check": the version-key says "unchanged", the device checksum disagrees -> StaleWeightsError (loud), and after
        .refresh() the render is right;
      * "key" (opt-in, documented hazard): the stale copy renders -- what the default used to do silently."""
    from nerfmeshes_amd import train_ops
    kw = dict(num_layers=4, hidden_size=64, skip_step=2, num_encoding_fn_xyz=6, num_encoding_fn_dir=4)
    hp = dict(num_coarse=16, num_fine=16, train_noise_std=0.0, **kw)
    o, d, _ = _rays(256, 2, 4)
    batch = (o[:1].cuda(), d.cuda(), torch.tensor([2.0, 6.0]))
    monkeypatch.delenv("NERFMESHES_WEIGHTS_GUARD", raising=False)

    model = _model(hp, seed=3)
    model._test_hp = hp
    got, want, packs = _render_after(model, batch, edit)
    assert torch.equal(got, want) and packs == 1

    monkeypatch.setenv("NERFMESHES_WEIGHTS_GUARD", "check")
    model = _model(hp, seed=3)
    model._test_hp = hp
    with pytest.raises(train_ops.StaleWeightsError, match="stale"):
        _render_after(model, batch, edit)
    for net in (model.model_coarse, model.model_fine):
        net.refresh()
    with torch.no_grad():
        again = model.query(batch).rgb_map
        assert model.query(batch).rgb_map.equal(again)            # unchanged parameters: the checksum agrees, nothing raises
    fresh = _model(hp, seed=99)
    fresh.load_state_dict(model.state_dict())
    fresh.eval()
    with torch.no_grad():
        assert torch.equal(again, fresh.query(batch).rgb_map)

    monkeypatch.setenv("NERFMESHES_WEIGHTS_GUARD", "key")
    model = _model(hp, seed=3)
    model._test_hp = hp
    got, want, packs = _render_after(model, batch, edit)
    assert packs == 0 and not torch.equal(got, want), "the key guard re-packs only on what the host can see"


@pytest.mark.parametrize("guard", ["always", "key"])
def test_replaced_parameter_objects_and_submodules_are_seen(guard, monkeypatch):
    """hip() caches the module's Parameter objects (walking the tree costs more than the re-pack it guards): a parameter that is
    re-assigned, a sub-module that is replaced, and a Parameter put straight into `_parameters` must all be picked up."""
    monkeypatch.setenv("NERFMESHES_WEIGHTS_GUARD", guard)
    kw = dict(num_layers=4, hidden_size=64, skip_step=2, num_encoding_fn_xyz=6, num_encoding_fn_dir=4)
    hp = dict(num_coarse=16, num_fine=16, train_noise_std=0.0, **kw)
    model = _model(hp, seed=3).eval()
    o, d, _ = _rays(128, 2, 4)
    batch = (o[:1].cuda(), d.cuda(), torch.tensor([2.0, 6.0]))

    def same_as_rebuilt():
        with torch.no_grad():
            got = model.query(batch).rgb_map
            fresh = _model(hp, seed=99).eval()
            fresh.load_state_dict(model.state_dict())
            return torch.equal(got, fresh.query(batch).rgb_map)

    assert same_as_rebuilt()
    net = model.model_fine
    net.fc_alpha.weight = torch.nn.Parameter(net.fc_alpha.weight.detach() * 1.5)                   # re-assigned (register_parameter)
    assert same_as_rebuilt()
    new = torch.nn.Linear(net.fc_feat.in_features, net.fc_feat.out_features).cuda()
    net.fc_feat = new                                                                              # a replaced sub-module
    assert same_as_rebuilt()
    net.layer1._parameters["bias"] = torch.nn.Parameter(torch.full_like(net.layer1.bias, 0.25))    # behind torch's back
    assert same_as_rebuilt()


def test_gradients_the_backward_does_not_produce_are_refused_not_dropped(ops, T):
    """The HIP backward yields parameter gradients (and the compositing backward the radiance's): a caller who asks for gradients
    with respect to ray origins, directions or depths -- the reference's autograd would deliver them -- gets an error with the
    reason, never a silent zero."""
    from nerfmeshes_amd.nerf.models import FlexibleNeRFModel
    kw = dict(num_layers=4, hidden_size=64, skip_step=2, num_encoding_fn_xyz=6, num_encoding_fn_dir=4)
    net = FlexibleNeRFModel(**kw).cuda().train()
    pts = torch.rand(32, 3, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError, match="require a gradient"):
        net(pts, pts.detach())
    net(pts.detach(), pts.detach()).sum().backward()
    assert all(p.grad is not None for p in net.parameters())
    o, d, t = _rays(8, 16, 1)
    rad = torch.rand(8, 16, 4, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError, match="require a gradient"):
        T.composite(rad, t.cuda().requires_grad_(True), d.cuda())
    T.composite(rad, t.cuda(), d.cuda())["rgb_map"].sum().backward()
    assert rad.grad is not None


def test_copies_and_pickles_of_a_module_get_their_own_handle(tmp_path):
    """copy.deepcopy (how an EMA copy is made), pickle and torch.save of a module that has already rendered: the device handle is
    run-time state of the original -- the copy packs its own on first use and follows ITS parameters."""
    import copy
    import pickle
    kw = dict(num_layers=4, hidden_size=64, skip_step=2, num_encoding_fn_xyz=6, num_encoding_fn_dir=4)
    hp = dict(num_coarse=16, num_fine=16, train_noise_std=0.0, **kw)
    model = _model(hp, seed=3).eval()
    o, d, _ = _rays(128, 2, 4)
    batch = (o[:1].cuda(), d.cuda(), torch.tensor([2.0, 6.0]))
    with torch.no_grad():
        before = model.query(batch).rgb_map.clone()
        ema = copy.deepcopy(model)
        assert ema.model_fine._hip is None and model.model_fine._hip is not None
        assert torch.equal(ema.query(batch).rgb_map, before)
        for p in ema.parameters():
            p.mul_(0.5)
        assert not torch.equal(ema.query(batch).rgb_map, before) and torch.equal(model.query(batch).rgb_map, before)
        assert ema.model_fine._hip is not model.model_fine._hip
        again = pickle.loads(pickle.dumps(model))
        assert torch.equal(again.query(batch).rgb_map, before)
        torch.save(model, tmp_path / "whole_module.pt")
        assert torch.equal(torch.load(tmp_path / "whole_module.pt", weights_only=False).query(batch).rgb_map, before)


def test_the_key_guard_repacks_once_per_visible_change_and_never_otherwise(monkeypatch):
    """Under NERFMESHES_WEIGHTS_GUARD=key a render loop over unchanged parameters re-packs nothing; an in-place op autograd sees,
    an optimizer step (fused Adam moves no version counter: the scoped post-step hook) and load_state_dict each cost exactly one
    re-pack on the next use."""
    from nerfmeshes_amd import train_ops
    monkeypatch.setenv("NERFMESHES_WEIGHTS_GUARD", "key")
    kw = dict(num_layers=4, hidden_size=64, skip_step=2, num_encoding_fn_xyz=6, num_encoding_fn_dir=4)
    hp = dict(num_coarse=16, num_fine=16, train_noise_std=0.0, **kw)
    model = _model(hp, seed=3)
    o, d, _ = _rays(256, 2, 4)
    batch = (o[:1].cuda(), d.cuda(), torch.tensor([2.0, 6.0]))
    model.eval()
    net = model.model_fine
    with torch.no_grad():
        model.query(batch)
        n0 = net.refresh_count()
        for _ in range(5):
            model.query(batch)
        assert net.refresh_count() == n0
        net.fc_alpha.weight.mul_(1.5)
        model.query(batch); model.query(batch)
        assert net.refresh_count() == n0 + 1
        state = {k: v.clone() for k, v in model.state_dict().items()}
        model.load_state_dict(state)
        model.query(batch); model.query(batch)
        assert net.refresh_count() == n0 + 2
    opt = train_ops.make_optimizer("Adam", model.parameters(), 1e-3)
    assert opt.defaults.get("fused")
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    opt.step()
    other = torch.optim.SGD(torch.nn.Linear(2, 2).cuda().parameters(), lr=0.1)      # somebody else's optimizer: not this module's business
    for g in other.param_groups:
        for p in g["params"]:
            p.grad = torch.zeros_like(p)
    other.step()
    with torch.no_grad():
        model.query(batch); model.query(batch)
    assert net.refresh_count() == n0 + 3


@pytest.mark.parametrize("kw", [dict(num_layers=4, hidden_size=64, skip_step=2, num_encoding_fn_xyz=6, num_encoding_fn_dir=4),
                                dict(num_layers=3, hidden_size=100, skip_step=2, num_encoding_fn_xyz=5, num_encoding_fn_dir=2)],
                         ids=["tuned-4x64", "generic-3x100"])
def test_training_iteration_replays_from_a_hipgraph(kw):
    """train_ops.GraphedStep: the whole iteration (forward in train mode, both losses, backward through the HIP kernels, Adam)
    captured once and replayed -- nothing in the library allocates, copies from the host or synchronises once the handles are
    warm.  Deterministic configuration: the parameters after 3 warm-up steps + 4 replays equal those after 7 eager steps bit for
    bit; with perturb + noise every replay draws fresh randoms (torch's generator is part of the graph)."""
    from nerfmeshes_amd import train_ops
    o, d, _ = _rays(512, 2, 4)
    target = (0.5 + 0.5 * torch.sin(7.0 * d)).cuda()
    batch = (o[:1].cuda(), d.cuda(), torch.tensor([2.0, 6.0]))

    def setup(stochastic):
        hp = dict(num_coarse=16, num_fine=16, train_noise_std=0.3 if stochastic else 0.0, train_perturb=stochastic, **kw)
        model = _model(hp, seed=3)
        model.train()
        opt = train_ops.make_optimizer("Adam", model.parameters(), 5e-3, capturable=True)
        assert opt.defaults["fused"] and opt.defaults["capturable"]
        loss_out = torch.zeros((), device="cuda")

        def iteration():
            opt.zero_grad(set_to_none=True)
            c, f = model(batch)
            loss = torch.nn.functional.mse_loss(c.rgb_map, target) + torch.nn.functional.mse_loss(f.rgb_map, target)
            loss.backward()
            opt.step()
            loss_out.copy_(loss.detach())
        return model, iteration, loss_out

    eager, it_e, loss_e = setup(False)
    start = [p.detach().clone() for p in eager.parameters()]
    it_e()
    first = float(loss_e)
    for _ in range(6):
        it_e()
    assert float(loss_e) < 0.9 * first and not any(torch.equal(a, b) for a, b in zip(start, eager.parameters())), "the eager run must have trained"
    graphed, it_g, loss_g = setup(False)
    step = train_ops.GraphedStep(it_g, warmup=3)
    for _ in range(4):
        step()
    torch.cuda.synchronize()
    assert float(loss_g) == float(loss_e)
    for (k, a), b in zip(eager.named_parameters(), graphed.parameters()):
        assert torch.equal(a, b), k
    # the inference path after replays sees the step the graph made last (no Python ran in it: GraphedStep tells the modules)
    graphed.eval(), eager.eval()
    with torch.no_grad():
        assert torch.equal(graphed.query(batch).rgb_map, eager.query(batch).rgb_map)
    _, it_s, loss_s = setup(True)
    step = train_ops.GraphedStep(it_s)
    seen = []
    for _ in range(4):
        step()
        seen.append(float(loss_s))
    assert len(set(seen)) == 4 and all(np.isfinite(seen)), seen


def test_perturb_and_noise_are_seeded_by_torch():
    hp = dict(num_layers=4, hidden_size=64, skip_step=2, num_encoding_fn_xyz=6, num_encoding_fn_dir=4, num_coarse=16,
              num_fine=16, train_perturb=True, train_noise_std=0.2)
    model = _model(hp, seed=1)
    model.train()
    o, d, _ = _rays(100, 2, 8)
    batch = (o[:1].cuda(), d.cuda(), torch.tensor([2.0, 6.0]))
    outs = []
    for seed in (7, 7, 8):
        torch.manual_seed(seed)
        with torch.no_grad():
            outs.append(model(batch)[1].rgb_map.clone())
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])


def test_training_step_api_and_driver(tmp_path):
    """training_step / configure_optimizers / DataBundle through the driver loop (nerfmeshes_amd.train_nerf): a
    4x64 student fitted for 80 iterations to renders of the seeded scene: the training loss falls by > 40 %, the
    held-out view does not get worse (the 8x256 student of the default command line goes from 8 dB to 19 dB in 300
    iterations, profiles/r01_train_bench.json), and the checkpoint loads back through the reference's entry point."""
    from nerfmeshes_amd import models, train_synthetic as train_nerf
    ckpt = tmp_path / "default" / "version_0" / "checkpoints" / "last.ckpt"
    losses, before, after = train_nerf.main(["--iters", "80", "--views", "4", "--size", "48", "--hidden-size", "64",
                                             "--num-layers", "4", "--rays", "1024", "--lr", "2e-3", "--save", str(ckpt)])
    assert len(losses) == 80 and all(np.isfinite(losses))
    assert np.mean(losses[-10:]) < 0.6 * np.mean(losses[:5]), (losses[:5], losses[-10:])
    assert np.isfinite(before) and np.isfinite(after) and after > before - 0.5, (before, after)
    model = models.NeRFModel.load_from_checkpoint(str(ckpt)).cuda().eval()
    o, d, _ = _rays(64, 2, 5)
    with torch.no_grad():
        out = model.query((o[:1].cuda(), d.cuda(), torch.tensor([2.0, 6.0])))
    assert out.rgb_map.shape == (64, 3) and bool(torch.isfinite(out.rgb_map).all())


def test_full_size_gradients_equal_the_sum_over_sub_batches():
    """BASELINE's training shape (2048 rays, 8x256, 64 + 128 samples) is too large for the CPU oracle's autograd in a
    test, so the backward is checked at full size through a size-independent property: rays are independent, so the
    gradient of a summed loss over 2048 rays (393 216 fine samples: three tiles per persistent workgroup, 128-way split-K
    weight-gradient GEMMs) equals the accumulated gradients of sixteen 128-ray sub-batches (the size the oracle
    tests cover).  (A finite-difference check is ill-posed here: the last sample's 1e10 interval makes the loss a
    step function of that sample's sigma -- fp64 autograd over the oracle shows the same.)"""
    model = _model(dict(train_noise_std=0.0), seed=4)
    with torch.no_grad():
        for net in (model.model_coarse, model.model_fine):
            net.fc_alpha.weight.mul_(30.0)
    model.train()
    rays = 2048
    o, d, _ = _rays(rays, 2, 21)
    origin, dirs, bounds = o[:1].cuda(), d.cuda(), torch.tensor([2.0, 6.0])
    target = torch.rand(rays, 3, generator=torch.Generator().manual_seed(6)).cuda()

    def summed_loss(sl):
        coarse, fine = model((origin, dirs[sl], bounds))
        return ((coarse.rgb_map - target[sl]) ** 2).sum() + ((fine.rgb_map - target[sl]) ** 2).sum()

    full = summed_loss(slice(0, rays))
    full.backward()
    whole = {k: p.grad.clone() for k, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    pieces = 0.0
    for s0 in range(0, rays, 128):
        part = summed_loss(slice(s0, s0 + 128))
        part.backward()                                   # .grad accumulates over the sub-batches
        pieces += float(part.detach())
    assert abs(float(full.detach()) - pieces) < 1e-4 * pieces
    for k, p in model.named_parameters():
        ref = p.grad
        assert float(ref.abs().max()) > 0.0, k
        err = float((whole[k] - ref).abs().max() / ref.abs().max())
        assert err < 5e-4, (k, err)


def test_training_step_against_the_reference_golden():
    """NeRFModel.training_step on the MI355X against the UNMODIFIED reference's training_step (fixture
    tests/golden/train_step.npz: loss, logged values, gradient of all 32 tensors; two chunks, the second ragged)."""
    from tests.helpers import golden_hparams, load_golden
    from nerfmeshes_amd import models
    g = load_golden("train_step")
    model = models.NeRFModel(golden_hparams(g))
    state = model.state_dict()
    for k in g.files:
        if k.startswith("param."):
            state[k[len("param."):]] = torch.from_numpy(g[k])
    model.load_state_dict(state)
    model = model.cuda().train()
    batch = dict(ray_origins=torch.from_numpy(g["origin"])[None, None], ray_directions=torch.from_numpy(g["directions"])[None],
                 ray_targets=torch.from_numpy(g["targets"])[None], ray_bounds=torch.tensor([[2.0, 6.0]]))
    out = model.training_step(batch, 0)
    out["loss"].backward()
    ref_loss = float(g["loss"])
    assert abs(float(out["loss"].detach()) - ref_loss) < 1e-4 * ref_loss
    for key in ("train/loss", "train/coarse_loss", "train/coarse_psnr", "train/fine_loss", "train/fine_psnr", "train/lr"):
        assert key in out["log"], key
        ref = float(g["log." + key])
        assert abs(float(out["log"][key]) - ref) < 2e-4 * max(1.0, abs(ref)), (key, float(out["log"][key]), ref)
    for name, p in model.named_parameters():
        ref = torch.from_numpy(g["grad." + name])
        assert p.grad is not None and p.grad.shape == ref.shape, name
        assert _rel(p.grad, ref) < 2e-3, (name, _rel(p.grad, ref))


def test_full_size_training_step_against_the_reference_golden():
    """NeRFModel.training_step at BASELINE's training shape -- 2048 rays, 8x256 coarse + fine, 64 + 128 samples: 524 288
    MLP evaluations, three 128-sample tiles per persistent workgroup, split-over-samples weight-gradient GEMMs -- against
    the UNMODIFIED reference's training_step + loss.backward() at that size (fixture tests/golden/train_step_full.npz:
    loss, logged values, digests of all 48 gradient tensors; tests/helpers.py::grad_digest).  The same fixture pins the
    oracle's autograd on the CPU to 1e-5 (tests/test_oracle_golden.py)."""
    import os
    from tests.helpers import check_grad_digests, gen_weights, golden_hparams, load_golden, mlp_kwargs
    from nerfmeshes_amd import models
    g = load_golden("train_step_full")
    hp = golden_hparams(g)
    model = models.NeRFModel(hp)
    w = gen_weights(int(g["seed"]), 0, 0, **mlp_kwargs(hp, "coarse"))
    state = model.state_dict()
    for prefix in ("model_coarse.", "model_fine."):
        for k, v in w.items():
            assert state[prefix + k].shape == v.shape, k
            state[prefix + k] = torch.from_numpy(np.array(v))
    model.load_state_dict(state)
    model = model.cuda().train()
    batch = dict(ray_origins=torch.from_numpy(g["origin"])[None, None], ray_directions=torch.from_numpy(g["directions"])[None],
                 ray_targets=torch.from_numpy(g["targets"])[None], ray_bounds=torch.tensor([[2.0, 6.0]]))
    out = model.training_step(batch, 0)
    out["loss"].backward()
    ref_loss = float(g["loss"])
    assert abs(float(out["loss"].detach()) - ref_loss) < 1e-4 * ref_loss, (float(out["loss"].detach()), ref_loss)
    for key in ("train/loss", "train/coarse_loss", "train/coarse_psnr", "train/fine_loss", "train/fine_psnr"):
        ref = float(g["log." + key])
        assert abs(float(out["log"][key]) - ref) < 2e-4 * max(1.0, abs(ref)), (key, float(out["log"][key]), ref)
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert all(v is not None for v in grads.values())
    dump = os.environ.get("NM_TEST_DUMP_DIR")
    check_grad_digests(g, grads, tol=FULL_SIZE_GRAD_TOL, dump=os.path.join(dump, "train_step_full_errors.json") if dump else None)


@pytest.mark.parametrize("out_f,stride,in_f", [(256, 256, 256), (256, 64, 63), (128, 256, 256), (128, 128, 128),
                                               (128, 64, 27), (64, 128, 128)])
@pytest.mark.parametrize("n", [16, 1040, 40000])
def test_weight_grad_kernel_vs_fp64(n, out_f, stride, in_f):
    """nm_weight_grad (hand-written split-over-samples fp32 MFMA GEMM + bias column sums, order-fixed reduction) vs
    delta^T @ act in fp64, for every supported block shape; deterministic (two runs bit-identical); writes into a
    column window of a wider matrix (the skip / view layers' cat(...) weights)."""
    from nerfmeshes_amd import hip_ops, train_ops as T
    kw = dict(num_layers=4, hidden_size=128, skip_step=2, num_encoding_fn_xyz=6, num_encoding_fn_dir=4)
    mlp = hip_ops.HipMLP({k: torch.as_tensor(v) for k, v in S.make_mlp_weights(3, **kw).items()}, kw, "cuda")
    g = torch.Generator().manual_seed(n + out_f)
    delta = torch.randn(n, out_f, generator=g) * (torch.rand(n, 1, generator=g) < 0.7)
    act = torch.relu(torch.randn(n, stride, generator=g))
    act[:, in_f:] = 0.0
    dc, ac = delta.cuda().contiguous(), act.cuda().contiguous()
    wide = torch.full((out_f, in_f + 10), 7.0, device="cuda")
    dw, db = T._weight_grad(mlp, dc, ac, in_f)
    dw2, db2 = T._weight_grad(mlp, dc, ac, in_f, out=wide, col0=10)
    ref = (delta.double().t() @ act.double()[:, :in_f])
    scale = float(ref.abs().max()) + 1e-30
    assert float((dw.double().cpu() - ref).abs().max()) <= 2e-6 * scale * max(1.0, (n / 1000) ** 0.5)
    assert float((db.double().cpu() - delta.double().sum(0)).abs().max()) <= 2e-6 * float(delta.abs().sum(0).max() + 1)
    assert torch.equal(wide[:, 10:], dw) and torch.equal(db2, db), "not deterministic / column window wrong"
    assert bool((wide[:, :10] == 7.0).all()), "wrote outside its column window"


@pytest.mark.parametrize("k", [64, 128, 256])
@pytest.mark.parametrize("n", [1, 37, 4096, 131072 + 5])
def test_head_grad_kernel_vs_fp64(n, k):
    """nm_head_grad (fc_alpha / fc_rgb weight gradients: dlast^T @ act for the shared (n, 4) delta + its column sums)
    vs fp64, ragged row counts included; two runs bit-identical (order-fixed reduction, no atomics)."""
    from nerfmeshes_amd import hip_ops, train_ops as T
    kw = dict(num_layers=4, hidden_size=128, skip_step=2, num_encoding_fn_xyz=6, num_encoding_fn_dir=4)
    mlp = hip_ops.HipMLP({k_: torch.as_tensor(v) for k_, v in S.make_mlp_weights(3, **kw).items()}, kw, "cuda")
    g = torch.Generator().manual_seed(n + k)
    dlast = torch.randn(n, 4, generator=g)
    act = torch.relu(torch.randn(n, k, generator=g))
    dc, ac = dlast.cuda().contiguous(), act.cuda().contiguous()
    dw, db = T._head_grad(mlp, dc, ac, bias=True)
    dw2, db2 = T._head_grad(mlp, dc, ac, bias=True)
    dw3, none = T._head_grad(mlp, dc, ac)
    ref = dlast.double().t() @ act.double()
    scale = float(ref.abs().max()) + 1e-30
    assert dw.shape == (4, k) and db.shape == (4,) and none is None
    assert float((dw.double().cpu() - ref).abs().max()) <= 2e-6 * scale * max(1.0, (n / 1000) ** 0.5)
    assert float((db.double().cpu() - dlast.double().sum(0)).abs().max()) <= 2e-6 * float(dlast.abs().sum(0).max() + 1)
    assert torch.equal(dw, dw2) and torch.equal(db, db2) and torch.equal(dw, dw3), "not deterministic"


GENERAL_DW_SHAPES = [
    # out, delta stride, in, act stride: everything the tuned kernel does not serve
    (64, 64, 64, 64), (64, 64, 39, 40), (32, 32, 64, 64), (100, 100, 100, 100), (50, 50, 100, 100), (50, 50, 27, 28),
    (100, 100, 63, 63), (5, 5, 2, 2), (2, 2, 5, 5), (1, 1, 1, 1), (96, 96, 96, 96), (144, 144, 144, 144), (320, 320, 320, 320),
    (160, 160, 320, 320), (400, 400, 400, 400), (400, 400, 93, 96), (512, 512, 512, 512), (256, 512, 256, 300),
    (272, 272, 272, 272), (256, 256, 256, 256), (128, 128, 63, 64),
]


@pytest.mark.parametrize("out_f,lda,in_f,ldb", GENERAL_DW_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("n", [1, 583, 4099, 40000])
def test_general_weight_grad_kernel_vs_fp64(n, out_f, lda, in_f, ldb, monkeypatch):
    """nm_weight_grad_ex's general kernel (nerf_dw_g.hip): any widths, any strides, any row count, operands at bases that are
    not 16-byte aligned -- vs delta^T @ act in fp64.  The operand buffers are filled with NaN beyond the widths (nothing may
    depend on padding) and the rows beyond n of the last chunk come from the buffer descriptor's extent (rows of ANOTHER
    tensor follow in memory: they must not be read).  Deterministic; column window of a wider output."""
    from nerfmeshes_amd import hip_ops, train_ops as T
    monkeypatch.setenv("NM_DW_GENERAL", "1")       # the tuned shapes too go through the general kernel here
    kw = dict(num_layers=4, hidden_size=128, skip_step=2, num_encoding_fn_xyz=6, num_encoding_fn_dir=4)
    mlp = hip_ops.HipMLP({k: torch.as_tensor(v) for k, v in S.make_mlp_weights(3, **kw).items()}, kw, "cuda")
    g = torch.Generator().manual_seed(n + out_f + 7 * in_f)
    delta = torch.randn(n, out_f, generator=g) * (torch.rand(n, 1, generator=g) < 0.7)
    act = torch.relu(torch.randn(n, in_f, generator=g))
    for shift in (0, 1):      # second pass: both operands start 4 bytes off a 16-byte boundary
        # rows n .. n + 40 exist in memory and hold NaN: a kernel that reads past its n rows fails loudly
        da = torch.full(((n + 40) * lda + 8,), float("nan"), device="cuda")
        aa = torch.full(((n + 40) * ldb + 8,), float("nan"), device="cuda")
        dv = da[shift:shift + n * lda].view(n, lda)
        av = aa[shift:shift + n * ldb].view(n, ldb)
        dv[:, :out_f] = delta.cuda()
        av[:, :in_f] = act.cuda()
        dc, ac = dv[:, :out_f], av[:, :in_f]
        wide = torch.full((out_f, in_f + 10), 7.0, device="cuda")
        dw, db = T._weight_grad(mlp, dc, ac, in_f)
        dw2, db2 = T._weight_grad(mlp, dc, ac, in_f, out=wide, col0=10)
        ref = (delta.double().t() @ act.double())
        scale = float(ref.abs().max()) + 1e-30
        assert torch.isfinite(dw).all() and torch.isfinite(db).all(), "read beyond the operands' widths or rows"
        assert float((dw.double().cpu() - ref).abs().max()) <= 2e-6 * scale * max(1.0, (n / 1000) ** 0.5)
        assert float((db.double().cpu() - delta.double().sum(0)).abs().max()) <= 2e-6 * float(delta.abs().sum(0).max() + 1)
        assert torch.equal(wide[:, 10:], dw) and torch.equal(db2, db), "not deterministic / column window wrong"
        assert bool((wide[:, :10] == 7.0).all()), "wrote outside its column window"


@pytest.mark.parametrize("k,ld", [(1, 1), (32, 32), (50, 50), (100, 100), (160, 160), (200, 256), (400, 400), (512, 512), (1000, 1000), (64, 64)])
@pytest.mark.parametrize("n", [1, 37, 4096, 131072 + 5])
def test_general_head_grad_kernel_vs_fp64(n, k, ld, monkeypatch):
    """nm_head_grad_ex's general kernel: any activation width / stride, vs fp64; deterministic."""
    from nerfmeshes_amd import hip_ops, train_ops as T
    monkeypatch.setenv("NM_DW_GENERAL", "1")
    kw = dict(num_layers=4, hidden_size=128, skip_step=2, num_encoding_fn_xyz=6, num_encoding_fn_dir=4)
    mlp = hip_ops.HipMLP({k_: torch.as_tensor(v) for k_, v in S.make_mlp_weights(3, **kw).items()}, kw, "cuda")
    g = torch.Generator().manual_seed(n + k)
    dlast = torch.randn(n, 4, generator=g)
    act = torch.relu(torch.randn(n, k, generator=g))
    buf = torch.full((n, ld), float("nan"), device="cuda")
    buf[:, :k] = act.cuda()
    dc, ac = dlast.cuda().contiguous(), buf[:, :k]
    dw, db = T._head_grad(mlp, dc, ac, bias=True)
    dw2, db2 = T._head_grad(mlp, dc, ac, bias=True)
    ref = dlast.double().t() @ act.double()
    scale = float(ref.abs().max()) + 1e-30
    assert dw.shape == (4, k) and db.shape == (4,)
    assert float((dw.double().cpu() - ref).abs().max()) <= 2e-6 * scale * max(1.0, (n / 1000) ** 0.5)
    assert float((db.double().cpu() - dlast.double().sum(0)).abs().max()) <= 2e-6 * float(dlast.abs().sum(0).max() + 1)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "not deterministic"


@pytest.mark.parametrize("out_f,in_f,jobs,n,general", [(256, 256, 8, 4096, False), (256, 256, 8, 4096, True), (128, 128, 3, 1040, False),
                                                       (100, 100, 5, 583, True), (320, 320, 16, 2000, True), (64, 39, 2, 37, True),
                                                       # more products than the one-product workspace holds sample parts for (8 x 8 output
                                                       # blocks: 4 parts on 256 CUs): issued as sub-batches
                                                       (2048, 2048, 8, 40, True), (1280, 1280, 16, 24, True)])
def test_weight_grad_batch_vs_fp64(out_f, in_f, jobs, n, general, monkeypatch):
    """nm_weight_grad_batch: the same-shape layers of a network in ONE launch + one reduction (a job gets 1 / jobs of the CUs) --
    every job against delta^T @ act in fp64, tuned and general kernel, ragged row counts, a shared output with column windows."""
    from nerfmeshes_amd import hip_ops, train_ops as T
    if general:
        monkeypatch.setenv("NM_DW_GENERAL", "1")
    kw = dict(num_layers=4, hidden_size=128, skip_step=2, num_encoding_fn_xyz=6, num_encoding_fn_dir=4)
    mlp = hip_ops.HipMLP({k: torch.as_tensor(v) for k, v in S.make_mlp_weights(3, **kw).items()}, kw, "cuda")
    g = torch.Generator().manual_seed(n + out_f + jobs)
    ldb = (in_f + 3) & ~3
    deltas = [torch.randn(n, out_f, generator=g) * (torch.rand(n, 1, generator=g) < 0.7) for _ in range(jobs)]
    acts = [torch.relu(torch.randn(n, in_f, generator=g)) for _ in range(jobs)]
    wide = torch.full((out_f, in_f + 7), 5.0, device="cuda")
    todo, outs = [], []
    for j in range(jobs):
        buf = torch.full((n, ldb), float("nan"), device="cuda")
        buf[:, :in_f] = acts[j].cuda()
        out = wide if j == 0 else torch.empty(out_f, in_f, device="cuda")
        db = torch.empty(out_f, device="cuda") if j % 2 == 0 else None
        todo.append((deltas[j].cuda().contiguous(), buf[:, :in_f], in_f, out, 7 if j == 0 else 0, db))
        outs.append((out[:, 7:] if j == 0 else out, db))
    # the workspace is exactly what nm_weight_grad_workspace_bytes_ex asked for, followed by a canary the kernels must not touch
    canaries = []

    def guarded_workspace(mlp_, tag, need):
        ws = torch.empty(need + 4096, dtype=torch.uint8, device="cuda")
        ws[need:] = 0xA5
        canaries.append(ws[need:])
        return ws[:need]

    monkeypatch.setattr(T, "_workspace", guarded_workspace)
    T._weight_grad_batch(mlp, todo)
    first = [(o.clone(), None if b is None else b.clone()) for o, b in outs]
    T._weight_grad_batch(mlp, todo)
    assert canaries and all(bool((c == 0xA5).all()) for c in canaries), "a weight-gradient launch wrote past its workspace"
    for j, ((o, b), (o1, b1)) in enumerate(zip(outs, first)):
        ref = deltas[j].double().t() @ acts[j].double()
        scale = float(ref.abs().max()) + 1e-30
        assert float((o.double().cpu() - ref).abs().max()) <= 2e-6 * scale * max(1.0, (n / 1000) ** 0.5), j
        assert torch.equal(o, o1), "not deterministic"
        if b is not None:
            assert float((b.double().cpu() - deltas[j].double().sum(0)).abs().max()) <= 2e-6 * float(deltas[j].abs().sum(0).max() + 1)
            assert torch.equal(b, b1)
    assert bool((wide[:, :7] == 5.0).all()), "wrote outside its column window"


@pytest.mark.parametrize("kw", SHAPES + FLAT_SHAPES, ids=["4x64", "8x256", "3x128", "4x64-flat", "8x256-flat", "5x128-flat"])
@pytest.mark.parametrize("rays,samples", [(37, 9), (145, 16)])
def test_layer1_gradient_by_linearity_vs_autograd_and_the_full_chain(ops, T, kw, rays, samples, monkeypatch):
    """layer1 has no activation (models.py:62): with NM_BACKWARD_STOP_AT_XYZ0 the delta kernel never applies layers_xyz[0]^T and
    backward() takes grad(layer1) = W0^T [d_h[1]^T enc | sum d_h[1]] (W0 exported from the handle's packed image) and
    grad(layers_xyz[0].weight) = [d_h[1]^T enc | sum d_h[1]] [W1 | b1]^T (its activation rows h[0] = layer1(enc) are never read).  Every gradient
    against fp64 autograd at the training tests' tolerance, and layer1's against the full chain's on the same tape.  (The path is
    taken from n H^2 > 4e9 on: forced here.  Sample counts that the 64-wide networks' fused backward does not serve.)"""
    spec = O.MLPSpec(**kw)
    w = _weights(kw)
    mlp = ops.HipMLP(w, kw, "cuda")
    from nerfmeshes_amd import _lib
    assert _lib.load().nm_mlp_backward_stops_at_xyz0(mlp.handle) == 1
    o, d, t = _rays(rays, samples, rays)
    grad_out = torch.randn(rays, samples, 4, generator=torch.Generator().manual_seed(1))
    rad, tape = T.forward_train(mlp, o.cuda(), d.cuda(), t.cuda())
    assert tape["h0_taped"]                                       # these sample counts are below the threshold of the path
    full = T.backward(mlp, tape, rad, grad_out.cuda(), o.cuda(), d.cuda(), t.cuda())
    monkeypatch.setattr(T, "LINEAR_LAYER1_MIN_WORK", 0)
    rad2, tape2 = T.forward_train(mlp, o.cuda(), d.cuda(), t.cuda())
    assert not tape2["h0_taped"] and torch.equal(rad, rad2)       # the taping forward leaves layer1's output out, nothing else changes
    tape2["h"][0].fill_(float("nan"))                             # ... and nobody reads it
    got = T.backward(mlp, tape2, rad2, grad_out.cuda(), o.cuda(), d.cuda(), t.cuda())
    g32 = _oracle_grads(w, spec, o, d, t, grad_out, torch.float32)[1]
    g64 = _oracle_grads(w, spec, o, d, t, grad_out, torch.float64)[1]
    assert set(got) == set(g64) == set(full)
    worst = {k: (_rel(got[k], ref), _rel(full[k], ref), _rel(g32[k], ref)) for k, ref in g64.items()}
    bad = {k: v for k, v in worst.items() if v[0] > max(2e-4, 20 * v[2])}
    assert not bad, f"gradient mismatch (by linearity, full chain, torch-fp32) relative to fp64 autograd: {bad}"
    for k in got:      # (layers_xyz[0]'s own gradient is taken by the same identity: h[0] = layer1(enc) is linear in the encoding)
        if not k.startswith(("layer1.", "layers_xyz.0.")):
            # every other gradient comes out of the same kernels on the same deltas -- in a batch with one product less, i.e. with
            # another split of the samples over the workgroups: equal up to the summation grouping
            assert _rel(got[k], full[k]) < 2e-6, k
