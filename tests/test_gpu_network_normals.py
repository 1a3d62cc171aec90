"""GPU: d sigma / d x (HipMLP.density_gradient, nm_mlp_density_grad) and mesh_nerf --normals network.  The gradient against
fp64 autograd over the CPU oracle on every kernel family, exactly on an affine network, bit for bit whatever the count, the
offset or the chunking; the bf16x3 rejection and the weights guard; the mesh end to end (geometry untouched, normals
= -g / |g| at the final vertices), a planar surface against the grid's exact normals, the CLI, and 2 / 3 ranks against 1."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nerfmeshes_amd import synthetic as S
from oracle import nerf_oracle as O
from tests.gpu_support import assert_ranks_ok, export_mesh, launch_ranks, scene_model
from tests.gpu_support import ops, scene  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NETS = {"8x256": dict(num_layers=8, hidden_size=256, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4),
        "8x128": dict(num_layers=8, hidden_size=128, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4),
        "4x64": dict(num_layers=4, hidden_size=64, skip_step=2, num_encoding_fn_xyz=6, num_encoding_fn_dir=4),
        "generic": dict(num_layers=4, hidden_size=272, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4),
        "no_viewdirs": dict(num_layers=8, hidden_size=256, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4,
                            use_viewdirs=False),
        "layerwise": dict(num_layers=4, hidden_size=768, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4),
        "20 functions": dict(num_layers=4, hidden_size=128, skip_step=2, num_encoding_fn_xyz=20, num_encoding_fn_dir=4)}


def _points(n, seed):
    g = torch.Generator().manual_seed(seed)
    return 2.4 * torch.rand(n, 3, generator=g) - 1.2


def _oracle_grad(w, kw, pts, dtype):
    spec = O.MLPSpec(**kw)
    wd = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in w.items()}
    x = pts.to(dtype).clone().requires_grad_(True)
    sigma = O.mlp_forward(wd, spec, x, x, keep_graph=True)[:, 3]
    (g,) = torch.autograd.grad(sigma.sum(), x)
    return g


def _relu_margin(w, kw, pts):
    """per point, the smallest |pre-activation| of the trunk's ReLUs in fp64, relative to the largest of its layer: where it is
    within rounding of 0, fp32 arithmetic may legitimately land on the other side of the kink (the gradient is discontinuous
    there)"""
    spec = O.MLPSpec(**kw)
    wd = {k: torch.as_tensor(np.asarray(v)).double() for k, v in w.items()}
    enc = O.positional_encoding(pts.double(), spec.num_encoding_fn_xyz, spec.include_input_xyz)
    h = enc @ wd["layer1.weight"].T + wd["layer1.bias"]
    margins = []
    for i in range(spec.num_layers - 1):
        if spec.is_skip(i):
            h = torch.cat((h, enc), dim=-1)
        z = h @ wd[f"layers_xyz.{i}.weight"].T + wd[f"layers_xyz.{i}.bias"]
        margins.append(z.abs().min(1).values / z.abs().max())
        h = torch.relu(z)
    return torch.stack(margins, 1).min(1).values


@pytest.mark.parametrize("name", list(NETS))
def test_gradient_vs_fp64_autograd(ops, name):
    """HIP's max error relative to max |g64| within 4x the same oracle's in fp32 on the CPU (points with a ReLU
    pre-activation within 1e-6 of its layer's range from the kink left out: at most 1 %)."""
    kw = NETS[name]
    w = S.make_mlp_weights(3, density_gain=30.0, density_bias=0.3, **kw)
    mlp = ops.HipMLP(w, kw, torch.device("cuda"))
    pts = _points(3000, 11)
    got = mlp.density_gradient(pts.cuda()).cpu().double()
    g64 = _oracle_grad(w, kw, pts, torch.float64)
    g32 = _oracle_grad(w, kw, pts, torch.float32).double()
    keep = _relu_margin(w, kw, pts) > 1e-6
    assert int((~keep).sum()) <= 30
    scale = float(g64.abs().max())
    assert scale > 0
    err_hip = float((got - g64)[keep].abs().max()) / scale
    err_32 = float((g32 - g64)[keep].abs().max()) / scale
    assert err_hip <= 4 * err_32, (name, err_hip, err_32)


def _affine_weights(kw, seed=7, gain=20.0):
    """every ReLU stays active on [-1.2, 1.2]^3 and only the raw-input columns of layer1 and the skip layers are non-zero: sigma
    is affine in x.  Signs fixed per coordinate (no cancellation) -> (weights, c = d sigma / d x in fp64)."""
    rng = np.random.default_rng(seed)
    w = S.make_mlp_weights(seed, **kw)
    H, L, dx = kw["hidden_size"], kw["num_layers"], 6 * kw["num_encoding_fn_xyz"] + 3
    spec = O.MLPSpec(**kw)
    sign = np.array([1.0, -1.0, 1.0])
    w1 = np.zeros((H, dx), np.float32)
    w1[:, :3] = (sign * rng.uniform(0.5, 1.0, (H, 3))).astype(np.float32)
    w["layer1.weight"], w["layer1.bias"] = w1, np.full(H, 5.0, np.float32)
    for i in range(L - 1):
        wi = np.zeros((H, H + (dx if spec.is_skip(i) else 0)), np.float32)
        wi[:, :H] = rng.uniform(0.0, 2.0 / H, (H, H)).astype(np.float32)
        if spec.is_skip(i):
            wi[:, H:H + 3] = (0.1 * sign * rng.uniform(0.5, 1.0, (H, 3))).astype(np.float32)
        w[f"layers_xyz.{i}.weight"], w[f"layers_xyz.{i}.bias"] = wi, np.full(H, 1.0, np.float32)
    head = "fc_alpha" if kw.get("use_viewdirs", True) else "fc_out"
    ha = rng.uniform(0.5, 1.0, H) * gain / H
    if head == "fc_alpha":
        w["fc_alpha.weight"] = ha[None, :].astype(np.float32)
    else:
        w["fc_out.weight"][3] = ha.astype(np.float32)
    J = w["layer1.weight"].astype(np.float64)[:, :3]
    for i in range(L - 1):
        wi = w[f"layers_xyz.{i}.weight"].astype(np.float64)
        J = wi[:, :H] @ J + (wi[:, H:H + 3] if spec.is_skip(i) else 0.0)
    c = (w["fc_alpha.weight"][0] if head == "fc_alpha" else w["fc_out.weight"][3]).astype(np.float64) @ J
    return w, c


AFFINE = ["8x256", "4x64", "generic", "no_viewdirs", "layerwise"]


@pytest.mark.parametrize("name", AFFINE)
def test_affine_network_gives_the_weight_product(ops, name):
    kw = NETS[name]
    w, c = _affine_weights(kw)
    pts = _points(2000, 5)
    g64 = _oracle_grad(w, kw, pts, torch.float64).numpy()
    assert np.abs(g64 - c).max() <= 1e-12 * np.abs(c).max(), "the weights make sigma affine on the box"
    got = ops.HipMLP(w, kw, torch.device("cuda")).density_gradient(pts.cuda()).cpu().double().numpy()
    assert (np.abs(got - c) <= 1e-5 * np.abs(c).max()).all(), (name, np.abs(got - c).max() / np.abs(c).max())
    assert (np.sign(got) == np.sign(c)).all()


@pytest.mark.parametrize("name", ["8x256", "no_viewdirs", "generic", "layerwise"])
def test_rows_are_independent_bit_for_bit(ops, name):
    kw = NETS[name]
    mlp = ops.HipMLP(S.make_mlp_weights(4, density_gain=30.0, density_bias=0.3, **kw), kw, torch.device("cuda"))
    n = 150000 if name != "layerwise" else 70000                   # more than one internal chunk (65 536 / 32 768 rows)
    p = _points(n, 9).cuda()
    full = mlp.density_gradient(p)
    assert full.shape == (n, 3) and bool(torch.isfinite(full).all())
    assert mlp.density_gradient(p[:0]).shape == (0, 3)
    for a, b in ((0, 1), (5, 22), (37, 1000), (1, 65600), (n - 17, n), (40000, n)):
        assert torch.equal(mlp.density_gradient(p[a:b]), full[a:b]), (name, a, b)
    assert torch.equal(mlp.density_gradient(p.flip(0)), full.flip(0))


def test_bf16x3_rejected_and_weights_guard(ops):
    kw = NETS["8x256"]
    b3 = ops.HipMLP(S.make_scene_weights(**kw), kw, torch.device("cuda"), precision="bf16x3")
    with pytest.raises(Exception, match="fp32"):
        b3.density_gradient(torch.zeros(64, 3, device="cuda"))
    from nerfmeshes_amd.nerf.models import FlexibleNeRFModel
    torch.manual_seed(0)
    model = FlexibleNeRFModel(**NETS["4x64"]).cuda()
    p = _points(777, 2).cuda()
    with torch.no_grad():
        before = model.hip("f32").density_gradient(p)
        model.layers_xyz[1].weight.data.mul_(1.5)                   # an edit the host cannot see
        model.layer1.weight.data[:, 3:].mul_(-0.5)
        after = model.hip("f32").density_gradient(p)
        fresh = ops.HipMLP(model.state_dict(), model._desc, torch.device("cuda")).density_gradient(p)
    assert not torch.equal(before, after)
    assert torch.equal(after, fresh), "the gradient of the edited weights"


def _run(model, tmp_path, tag, *extra):
    d = tmp_path / tag
    d.mkdir()
    return export_mesh(model, d, *extra), d                      # every caller sets its own --iso-level


@pytest.mark.parametrize("res", [64, 96])
@pytest.mark.parametrize("ss", [0, 2])
def test_end_to_end_on_the_scene(ops, scene, tmp_path, res, ss):
    common = ["--res", str(res), "--iso-level", "32", "--super-sampling", str(ss)]
    (v0, f0, n0, c0), d0 = _run(scene, tmp_path, "grid", *common)
    (v, f, n, c), d1 = _run(scene, tmp_path, "network", *common, "--normals", "network")
    assert torch.equal(v, v0) and torch.equal(f, f0), "geometry and topology are the grid run's"
    g = scene.get_model().hip("f32").density_gradient(v)
    norm = torch.linalg.vector_norm(g, dim=1, keepdim=True)
    ok = (torch.isfinite(norm) & (norm > 0))[:, 0]
    assert bool(ok.any())
    assert torch.equal(n[ok], (-g / norm)[ok]), "normals = -g / |g| at the final vertices, bit for bit"
    assert torch.equal(n[~ok], n0[~ok]), "zero / non-finite gradients keep the grid normal"
    assert float((torch.linalg.vector_norm(n.double(), dim=1) - 1).abs().max()) <= 1e-6
    assert float((n * n0).sum(1).mean()) > 0.5, "both point towards lower density"
    assert not np.array_equal(c, c0), "the appearance rays follow the new normals"


def test_planar_surface_matches_the_grid_normals(ops, tmp_path):
    """On the affine network the surface is a plane: the grid's central differences are exact there, so the network normals
    (-c / |c|, to 1e-5) and the grid normals agree -- the orientation end to end.  The grid normals carry the rounding of the
    fp32 density values they difference (sigma is a large sum minus its bias here): they agree to 1e-4."""
    kw = NETS["8x256"]
    w, c = _affine_weights(kw, seed=3, gain=40.0)
    sigma0 = O.mlp_forward({k: torch.as_tensor(v).double() for k, v in w.items()}, O.MLPSpec(**kw),
                           torch.zeros(1, 3, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.float64), keep_graph=True)[0, 3]
    w["fc_alpha.bias"] = (w["fc_alpha.bias"] - np.float32(float(sigma0))).astype(np.float32)     # sigma(0) = 0: the plane through 0
    model = scene_model("cuda", chunksize=3000, weights=w)
    common = ["--res", "32", "--iso-level", "0", "--no-view-dependence"]
    (v0, f0, n0, _), _ = _run(model, tmp_path, "grid", *common)
    (v, f, n, _), _ = _run(model, tmp_path, "network", *common, "--normals", "network")
    assert v.shape[0] > 100 and torch.equal(v, v0) and torch.equal(f, f0)
    want = torch.from_numpy(-c / np.linalg.norm(c)).cuda()
    assert float((n.double() - want).abs().max()) <= 1e-5
    assert float((n.double() - n0.double()).abs().max()) <= 1e-4


def _obj_lines(path):
    lines = open(path).read().splitlines()
    return ([l for l in lines if l.startswith("v ")], [l for l in lines if l.startswith("f ")],
            [l for l in lines if l.startswith("vn ")])


def test_cli_writes_network_normals(ops, tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_ckpt", os.path.join(ROOT, "scripts", "make_synthetic_checkpoint.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    vdir = mk.write(str(tmp_path / "logs"))
    common = ["--log-checkpoint", vdir, "--res", "48", "--save-dir", str(tmp_path), "--batch-size", "4096",
              "--view-disparity-max-bound", "1.0"]
    r = subprocess.run([sys.executable, "-m", "nerfmeshes_amd.mesh_nerf", *common, "--mesh-name", "grid.obj"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([sys.executable, "-m", "nerfmeshes_amd.mesh_nerf", *common, "--mesh-name", "network.obj", "--normals",
                        "network", "--use-cached-mesh"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "kept their grid normal" in r.stdout
    gv, gf, gn = _obj_lines(tmp_path / "grid.obj")
    nv, nf, nn = _obj_lines(tmp_path / "network.obj")
    # positions and faces byte for byte; the colours on the v lines follow the new appearance rays
    assert [l.split()[:4] for l in gv] == [l.split()[:4] for l in nv] and gf == nf
    assert len(gf) > 100 and len(nn) == len(gn) == len(gv)
    assert gn != nn and gv != nv
    # the vn lines are the network normals at the OBJ's own vertices
    from nerfmeshes_amd import mesh_nerf
    verts = torch.tensor([[float(t) for t in l.split()[1:4]] for l in nv], dtype=torch.float32).cuda()
    cached = torch.load(tmp_path / "mesh_cache.pt", weights_only=False)
    from nerfmeshes_amd import models
    from nerfmeshes_amd.lightning_modules import PathParser
    pp = PathParser()
    pp.parse(None, vdir, None, "model_last.ckpt")
    model = models.NeRFModel.load_from_checkpoint(pp.checkpoint_path).eval().to("cuda")
    assert torch.equal(cached[0].cuda(), verts), "the cache holds the geometry stage's vertices"
    assert cached[2].numpy().tobytes() == np.array([[np.float32(t) for t in l.split()[1:4]] for l in gn], np.float32).tobytes(), \
        "the cache keeps the grid normals"
    with torch.no_grad():
        want, _ = mesh_nerf.network_normals(model.get_model().hip("f32"), verts, cached[2].cuda())
    got = np.array([[np.float32(t) for t in l.split()[1:4]] for l in nn], np.float32)
    assert got.tobytes() == want.cpu().numpy().tobytes()


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_sharing_one_gpu_equal_one_rank(world):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X")
    r = launch_ranks(os.path.join("tests", "tools", "nn_dist_worker.py"), world, timeout=900)
    assert_ranks_ok(r, f"NN_DIST_OK world={world}")
