"""GPU: the super-sampled mesh (mesh_nerf --super-sampling).  Edge keys from the emit pass's scratch, the edge samples and
the refinement kernel bitwise against the numpy restatement (tests/ss_refine.py), HipMLP.sample_density against
grid_query, the whole extract_geometry_with_super_sampling against the dense construction the reference sketched, the CLI,
and 2 / 3 ranks against 1."""
import os

import numpy as np
import pytest
import torch

from nerfmeshes_amd import synthetic as S
from tests import ss_refine
from tests.gpu_support import assert_ranks_ok, launch_ranks
from tests.gpu_support import ops, scene  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _volume(kind, shape, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.standard_normal(shape).astype(np.float32), 0.1
    if kind == "ties":
        return rng.integers(-2, 3, shape).astype(np.float32), 0.0
    g = np.stack(np.meshgrid(*[np.linspace(-1, 1, s) for s in shape], indexing="ij"), -1)
    return (np.sin(3 * g[..., 0]) * np.cos(2 * g[..., 1]) + g[..., 2] ** 2 - 0.3).astype(np.float32), float(np.float32(0.05))


def _fine_values(kind, V, ss, iso, seed):
    rng = np.random.default_rng(seed + 1000)
    if kind == "ties":
        return rng.integers(-2, 3, (V, ss)).astype(np.float32)       # samples exactly on the level as well
    return (iso + rng.standard_normal((V, ss))).astype(np.float32)


def _slabs(n0, parts):
    from nerfmeshes_amd import dist as nd
    layers = n0 - 1
    for r in range(parts):
        lo, hi = nd.split_range(layers, r, parts)
        if hi > lo:
            below, above = int(lo > 0), int(hi < layers)
            yield lo - below, hi + 1 + above, below, above


def _on_edge(v, keys, nums):
    """every edge vertex lies on the edge its key names: the two other coordinates are the voxel's, the edge coordinate in
    [i_a, i_a + 1]"""
    v = v.cpu().numpy().astype(np.float64)
    ijk, axis = ss_refine.decode(keys.cpu().numpy(), nums)
    e = axis != 3
    assert e.sum() > 0.5 * len(v)
    rows = np.nonzero(e)[0]
    a = axis[rows]
    t = v[rows, a] - ijk[rows, a]
    assert (t >= 0).all() and (t <= 1).all()
    for k in range(3):
        other = rows[a != k]
        assert np.array_equal(v[other, k], ijk[other, k].astype(np.float64))
    c = np.nonzero(~e)[0]                                           # centre vertices: inside their cube
    assert ((v[c] >= ijk[c]) & (v[c] <= ijk[c] + 1)).all()


@pytest.mark.parametrize("kind", ["noise", "ties", "smooth"])
def test_keys_name_each_vertex_edge_and_slabs_concatenate(ops, kind):
    shape = (33, 40, 21)
    vol, iso = _volume(kind, shape, 7)
    full = torch.from_numpy(vol).cuda()
    v, f, n, val, keys = ops.marching_cubes(full, iso, return_keys=True)
    assert keys.dtype == torch.int64 and keys.shape == (v.shape[0],)
    _on_edge(v, keys, shape)
    plain = ops.marching_cubes(full, iso)
    assert all(torch.equal(a, b) for a, b in zip(plain, (v, f, n, val))), "return_keys changes nothing else"
    for parts in (2, 3, 8):
        pieces, base = [], 0
        for p_lo, p_hi, below, above in _slabs(shape[0], parts):
            slab = ops.marching_cubes_slab(full[p_lo:p_hi].contiguous(), iso, p_lo, below, above)
            pieces.append(slab.emit(base - slab.ghost_vertices, return_keys=True))
            base += slab.vertices
        got = [torch.cat([p[i] for p in pieces]) for i in range(5)]
        assert torch.equal(got[4], keys), f"{kind} x{parts}: slab keys differ from the whole volume's"
        assert torch.equal(got[0], v)


@pytest.mark.parametrize("ss", [0, 1, 2, 3, 7])
@pytest.mark.parametrize("kind", ["noise", "ties", "smooth"])
def test_refine_kernel_matches_the_restatement_bitwise(ops, kind, ss):
    shape = (26, 31, 19)
    vol, iso = _volume(kind, shape, 11)
    full = torch.from_numpy(vol).cuda()
    v, f, n, val, keys = ops.marching_cubes(full, iso, return_keys=True)
    V = v.shape[0]
    fine = _fine_values(kind, V, ss, iso, ss)
    kh = keys.cpu().numpy()
    want = ss_refine.refine(vol, 0, iso, kh, ss, fine, v.cpu().numpy(), shape)
    got = ops.mc_refine_vertices(full, 0, iso, keys, ss, torch.from_numpy(fine).cuda(), v.clone())
    assert got.cpu().numpy().tobytes() == want.tobytes(), f"{kind} ss={ss}: whole volume"
    if ss == 0:
        assert torch.equal(got, v), "ss = 0 reproduces nm_mc_emit's vertices"
    # slabs: every slab refines its own rows from its own planes
    for parts in (2, 3):
        out, base, row = [], 0, 0
        for p_lo, p_hi, below, above in _slabs(shape[0], parts):
            slab = ops.marching_cubes_slab(full[p_lo:p_hi].contiguous(), iso, p_lo, below, above)
            sv, _, _, _, sk = slab.emit(base - slab.ghost_vertices, return_keys=True)
            base += slab.vertices
            fs = torch.from_numpy(fine[row:row + sv.shape[0]]).cuda()
            row += sv.shape[0]
            out.append(ops.mc_refine_vertices(full[p_lo:p_hi].contiguous(), p_lo, iso, sk, ss, fs, sv))
        assert torch.cat(out).cpu().numpy().tobytes() == want.tobytes(), f"{kind} ss={ss} x{parts}: slabs"
    # the edge samples themselves
    if ss:
        base_ax = [np.linspace(-1.2, 1.2, k).astype(np.float32) for k in shape]
        fine_ax = [ops.fine_axis(1.2, k, ss).numpy() for k in shape]
        pts = ops.mc_edge_points(keys, shape, ss, [torch.from_numpy(a) for a in base_ax], [torch.from_numpy(a) for a in fine_ax])
        wp = ss_refine.edge_points(kh, shape, ss, base_ax, fine_ax)
        e = (kh & 3) != 3
        assert pts.shape == (V, ss, 3) and np.array_equal(pts.cpu().numpy()[e], wp[e])


def test_sphere_accuracy(ops):
    """sigma = 100 sigmoid(s (R - |x|)), iso 50: at ss = 3 the mean | |v| - R | is at most 1/3 of the plain mesh's (the CPU
    restatement gives ~0.03 at this resolution and sharpness); the GPU result is the restatement's bit for bit."""
    n, s, R, lim, ss = 48, 100.0, 0.7, 1.2, 3
    ax = np.linspace(-lim, lim, n, dtype=np.float32)

    def sig(p):
        return (100.0 / (1.0 + np.exp(-s * (R - np.linalg.norm(p.astype(np.float64), axis=-1))))).astype(np.float32)

    vol = sig(np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1))
    full = torch.from_numpy(vol).cuda()
    v, _, _, _, keys = ops.marching_cubes(full, 50.0, return_keys=True)
    fine_ax = ops.fine_axis(lim, n, ss)
    pts = ops.mc_edge_points(keys, (n, n, n), ss, [torch.from_numpy(ax)] * 3, [fine_ax] * 3)
    fine = sig(pts.cpu().numpy())
    got = ops.mc_refine_vertices(full, 0, 50.0, keys, ss, torch.from_numpy(fine).cuda(), v.clone()).cpu().numpy()
    want = ss_refine.refine(vol, 0, 50.0, keys.cpu().numpy(), ss, fine, v.cpu().numpy(), (n, n, n))
    assert got.tobytes() == want.tobytes()
    world = lambda vv: -lim + vv.astype(np.float64) * (2 * lim / (n - 1))          # noqa: E731
    err = lambda vv: float(np.abs(np.linalg.norm(world(vv), axis=1) - R).mean())   # noqa: E731
    assert err(got) <= err(v.cpu().numpy()) / 3, (err(got), err(v.cpu().numpy()))


NETS = [dict(num_layers=8, hidden_size=256, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4),
        dict(num_layers=8, hidden_size=128, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4),
        dict(num_layers=4, hidden_size=64, skip_step=2, num_encoding_fn_xyz=6, num_encoding_fn_dir=4),
        dict(num_layers=4, hidden_size=272, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4),         # generic
        dict(num_layers=8, hidden_size=256, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=False),
        dict(num_layers=4, hidden_size=768, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)]         # layer-wise


@pytest.mark.parametrize("kw", NETS, ids=["8x256", "8x128", "4x64", "generic", "no_viewdirs", "layerwise"])
def test_sample_density_equals_grid_query(ops, kw):
    w = S.make_mlp_weights(3, density_gain=30.0, density_bias=0.3, **kw)
    mlp = ops.HipMLP(w, kw, torch.device("cuda"))
    axes = [torch.linspace(-1.2, 1.2, k) for k in (37, 29, 41)]
    grid = mlp.grid_query(*axes, density_only=True)
    pts = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3).cuda()
    got = mlp.sample_density(pts)
    assert got.shape == grid.shape and torch.equal(got, grid)
    part = mlp.sample_density(pts[1000:1777])                           # any count, any offset
    assert torch.equal(part, grid[1000:1777])


def test_sample_density_rejects_bf16x3(ops):
    kw = dict(num_layers=8, hidden_size=256, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
    mlp = ops.HipMLP(S.make_scene_weights(**kw), kw, torch.device("cuda"), precision="bf16x3")
    with pytest.raises(Exception, match="fp32"):
        mlp.sample_density(torch.zeros(64, 3, device="cuda"))


def _args(res, ss, *extra):
    from nerfmeshes_amd import mesh_nerf
    return mesh_nerf.build_parser().parse_args(["--res", str(res), "--super-sampling", str(ss), "--iso-level", "32", *extra])


@pytest.mark.parametrize("res", [64, 96])
@pytest.mark.parametrize("ss", [1, 2])
def test_end_to_end_equals_the_dense_construction(ops, scene, res, ss):
    from nerfmeshes_amd import mesh_nerf
    args = _args(res, ss)
    with torch.no_grad():
        v0, f0, n0, d0 = mesh_nerf.extract_geometry(scene, "cuda", args)
        v, f, n, d = mesh_nerf.extract_geometry_with_super_sampling(scene, "cuda", args)
        assert v.shape == v0.shape and torch.equal(f, f0) and torch.equal(n, n0) and torch.equal(d, d0)
        iso = mesh_nerf.extract_iso_level(d, args)
        pv, pf, pn, pval, keys = ops.marching_cubes(d, iso, return_keys=True)
        assert torch.equal(pf, f0) and torch.equal(pn, n0)
        # the dense construction: three grids (ss+1)-times denser along one axis each, grid_query(fine, base, base) and rolls
        net = scene.get_model().hip("f32")
        base = [torch.linspace(-args.limit, args.limit, res)] * 3
        fine_ax = ops.fine_axis(args.limit, res, ss)
        rich = [net.grid_query(*[fine_ax if k == a else base[k] for k in range(3)], density_only=True).cpu().numpy()
                for a in range(3)]
        nf = fine_ax.numel()
        rich = [rich[0].reshape(nf, res, res), rich[1].reshape(res, nf, res), rich[2].reshape(res, res, nf)]
        kh = keys.cpu().numpy()
        ijk, axis = ss_refine.decode(kh, (res,) * 3)
        fine = np.zeros((len(kh), ss), np.float32)
        for a in range(3):
            rows = np.nonzero(axis == a)[0]
            for s in range(1, ss + 1):
                idx = [ijk[rows, 0], ijk[rows, 1], ijk[rows, 2]]
                idx[a] = ijk[rows, a] * (ss + 1) + s
                fine[rows, s - 1] = rich[a][tuple(idx)]
        grid_units = ss_refine.refine(d.cpu().numpy(), 0, iso, kh, ss, fine, pv.cpu().numpy(), (res,) * 3)
        want = args.limit * (torch.from_numpy(grid_units).cuda() / (args.res / 2.0) - 1.0)     # the same device op as mesh_nerf's
        assert v.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), f"res {res} ss {ss}: differs from the dense construction"
        _on_edge(torch.from_numpy(grid_units), keys, (res,) * 3)
        moved = (v != v0).any(1).cpu().numpy()
        assert moved.any() and not moved[axis == 3].any(), "only edge vertices move"
        if res == 96 and ss == 2:
            # refinement converges: ss = 3 is closer to ss = 31 than the plain mesh is
            v3 = mesh_nerf.extract_geometry_with_super_sampling(scene, "cuda", _args(res, 3))[0]
            v31 = mesh_nerf.extract_geometry_with_super_sampling(scene, "cuda", _args(res, 31))[0]
            assert float((v3 - v31).norm(dim=1).mean()) < float((v0 - v31).norm(dim=1).mean())


def test_super_sampling_argument_errors(scene):
    from nerfmeshes_amd import mesh_nerf
    with torch.no_grad():
        for bad in (65, 1000):
            with pytest.raises(ValueError, match="super-sampling"):
                mesh_nerf.extract_geometry_with_super_sampling(scene, "cuda", _args(32, bad))
        with pytest.raises(ValueError, match="route script"):
            mesh_nerf.extract_geometry_with_super_sampling(scene, "cuda", _args(32, 2, "--route", "script"))


def _obj(path):
    lines = open(path).read().splitlines()
    return [l for l in lines if l.startswith("v ")], [l for l in lines if l.startswith("f ")]


def test_cli_writes_the_refined_coloured_obj(ops, tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_ckpt", os.path.join(ROOT, "scripts", "make_synthetic_checkpoint.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    vdir = mk.write(str(tmp_path / "logs"))
    from nerfmeshes_amd import mesh_nerf
    common = ["--log-checkpoint", vdir, "--res", "48", "--save-dir", str(tmp_path), "--batch-size", "4096",
              "--view-disparity-max-bound", "1.0"]
    mesh_nerf.main(common + ["--mesh-name", "plain.obj"])
    v, _, _, _ = mesh_nerf.main(common + ["--mesh-name", "ss2.obj", "--super-sampling", "2"])
    pv, pfc = _obj(tmp_path / "plain.obj")
    sv, sfc = _obj(tmp_path / "ss2.obj")
    assert pfc == sfc and len(pfc) > 100 and len(pv) == len(sv)
    assert all(len(l.split()) == 7 for l in sv[:10]), "a coloured OBJ: v x y z r g b"
    # which rows are centre vertices: the keys of the plain mesh of the same grid
    from nerfmeshes_amd import models
    from nerfmeshes_amd.lightning_modules import PathParser
    pp = PathParser()
    cfg, _ = pp.parse(None, vdir, None, "model_last.ckpt")
    model = models.NeRFModel.load_from_checkpoint(pp.checkpoint_path).eval().to("cuda")
    args = mesh_nerf.build_parser().parse_args(common[2:])
    with torch.no_grad():
        d = mesh_nerf.extract_density(model, args, "cuda", 48)
        keys = ops.marching_cubes(d, mesh_nerf.extract_iso_level(d, args), return_keys=True)[4].cpu().numpy()
    diff = np.array([a != b for a, b in zip(pv, sv)])
    assert diff.any() and not diff[(keys & 3) == 3].any(), "v lines differ on edge vertices only"
    with pytest.raises(ValueError, match="route script"):
        mesh_nerf.main(common + ["--mesh-name", "script.obj", "--super-sampling", "2", "--route", "script"])


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_sharing_one_gpu_equal_one_rank(world):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X")
    r = launch_ranks(os.path.join("tests", "tools", "ss_dist_worker.py"), world, timeout=900)
    assert_ranks_ok(r, f"SS_DIST_OK world={world}")
