"""CPU: mesh_nerf --normals (parser default and choices, the --route script rejection) and a float64 restatement of the
contraction nm_mlp_density_grad's last kernel implements -- the deltas at the positional encoding times the encoding's Jacobian
(src/nerf/modules.py:26-34, c-major [x | sin(b_k x_c) | cos(b_k x_c)]) -- against torch autograd through the oracle's
positional_encoding."""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O


def encoding_jacobian_contract(x, g_enc, n_freq, include_input, bands):
    """d x_c = g[c] (include_input) + sum_k b_k (cos(b_k x_c) g_sin[c F + k] - sin(b_k x_c) g_cos[c F + k]) -- the epilogue of
    input_grad_kernel (nerf_input_grad.hip), column by column, in float64."""
    x, g_enc, bands = (np.asarray(a, dtype=np.float64) for a in (x, g_enc, bands))
    out = np.zeros_like(x)
    base = 3 if include_input else 0
    if include_input:
        out += g_enc[:, :3]
    F = n_freq
    for c in range(3):
        for k in range(F):
            arg = bands[k] * x[:, c]
            out[:, c] += bands[k] * (np.cos(arg) * g_enc[:, base + c * F + k] - np.sin(arg) * g_enc[:, base + 3 * F + c * F + k])
    return out


@pytest.mark.parametrize("n_freq,include_input", [(10, True), (6, True), (4, False), (20, True), (31, True), (1, False)])
def test_encoding_jacobian_restatement_matches_autograd(n_freq, include_input):
    g = torch.Generator().manual_seed(n_freq)
    x = (2.4 * torch.rand(257, 3, generator=g, dtype=torch.float64) - 1.2).requires_grad_(True)
    enc = O.positional_encoding(x, n_freq, include_input)
    assert enc.dtype == torch.float64 and enc.shape[1] == 6 * n_freq + (3 if include_input else 0)
    g_enc = torch.randn(enc.shape, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad((enc * g_enc).sum(), x)
    bands = O.frequency_bands(n_freq).to(torch.float64).numpy()
    got = encoding_jacobian_contract(x.detach().numpy(), g_enc.numpy(), n_freq, include_input, bands)
    scale = float(want.abs().max())
    assert float(np.abs(got - want.numpy()).max()) <= 1e-12 * scale


def test_parser_default_and_choices():
    from nerfmeshes_amd import mesh_nerf
    p = mesh_nerf.build_parser()
    assert p.parse_args([]).normals == "grid"
    assert p.parse_args(["--normals", "network"]).normals == "network"
    with pytest.raises(SystemExit):
        p.parse_args(["--normals", "analytic"])


def test_route_script_rejects_network_normals(tmp_path):
    from nerfmeshes_amd import mesh_nerf
    args = mesh_nerf.build_parser().parse_args(["--normals", "network", "--route", "script", "--save-dir", str(tmp_path)])
    with pytest.raises(ValueError, match="route script"):
        mesh_nerf.export_marching_cubes(None, args, None, "cpu")
    assert not any(tmp_path.iterdir()), "rejected before anything runs"
