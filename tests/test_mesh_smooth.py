"""CPU: Taubin smoothing's host side -- the vectorised numpy restatement (tests/mesh_smooth.py) against a plain dict-and-loop
implementation on every mesh of the marching-cubes fixture and on hand-made meshes for the branches the fixture does not take,
its distance from a float umbrella in fp64, what the filter does to a noisy sphere, the sign of the recomputed normals,
mesh_nerf's options (defaults, negatives, the --route script rejection) and the argument checks of the four C entries."""
import ctypes as C

import numpy as np
import pytest

from oracle import mc_oracle
from tests import mesh_smooth as SM
from tests.helpers import load_golden


@pytest.fixture(scope="module")
def meshes():
    g = load_golden("mc_cases")
    out = []
    for i in range(int(g["count"])):
        if f"err_{i}" in g.files:
            continue
        out.append((i, g[f"verts_{i}"].astype(np.float32), g[f"faces_{i}"].astype(np.int32), g[f"normals_{i}"].astype(np.float32)))
    return out


def _loop_neighbours(verts, faces):
    """-> (neighbour sets, faces per edge, degenerate faces), one face at a time"""
    near, on, flat = [set() for _ in verts], {}, 0
    for a, b, c in faces.tolist():
        if a == b or b == c or a == c:
            flat += 1
            continue
        for u, v in ((a, b), (b, c), (c, a)):
            on[min(u, v), max(u, v)] = on.get((min(u, v), max(u, v)), 0) + 1
            near[u].add(v)
            near[v].add(u)
    return near, on, flat


def _loop_smooth(verts, faces, normals, iterations, lam, mu, free_boundary, flip):
    """The contract once more, one vertex at a time with Python sets and Python ints for the sums (no numpy sorting, no vector
    operation)."""
    f32, f64 = np.float32, np.float64
    verts, faces = np.asarray(verts, f32), np.asarray(faces, np.int32)
    near, on, flat = _loop_neighbours(verts, faces)
    pinned = {v for e, n in on.items() if n == 1 for v in e}
    largest = max((abs(float(c)) for x in verts for c in x), default=0.0)
    e = int(np.frexp(f32(largest))[1])
    shift = 40 - e
    x = verts.copy()
    factors = [f32(lam)] + ([f32(mu)] if f32(mu) != 0 else [])
    for f in (factors * iterations if largest > 0 else []):
        q = [[int(np.rint(min(max(float(np.ldexp(f64(c), shift)), -2.0 ** 43), 2.0 ** 43))) for c in row] for row in x]
        new = x.copy()
        for v, ring in enumerate(near):
            if not ring or (v in pinned and not free_boundary):
                continue
            for k in range(3):
                hi, lo = sum(q[u][k] >> 20 for u in ring), sum(q[u][k] & 0xFFFFF for u in ring)
                m = np.ldexp((f64(hi) * f64(2.0 ** 20) + f64(lo)) / f64(len(ring)), -shift)
                new[v, k] = f32(f64(x[v, k]) + f64(f) * (m - f64(x[v, k])))
        x = new
    out_normals = None
    if normals is not None or flip is not None:
        sign, total = f32(1 if flip is None else flip), [[0, 0, 0] for _ in verts]
        for a, b, c in faces.tolist():
            if a == b or b == c or a == c:
                continue
            u, w = x[b] - x[a], x[c] - x[a]
            n = [f32(f32(u[(k + 1) % 3] * w[(k + 2) % 3]) - f32(u[(k + 2) % 3] * w[(k + 1) % 3])) for k in range(3)]
            length = np.sqrt(f32(f32(f32(n[0] * n[0]) + f32(n[1] * n[1])) + f32(n[2] * n[2])))
            if not (np.isfinite(length) and length > 0):
                continue
            for k in range(3):
                qn = int(np.rint(f64(f32(f32(n[k] / length) * sign)) * 2.0 ** 30))
                for v in (a, b, c):
                    total[v][k] += qn
        out_normals = np.zeros((len(verts), 3), f32) if normals is None else np.array(normals, f32)
        for v, t in enumerate(total):
            if t != [0, 0, 0]:
                s = np.array(t, np.int64).astype(f32)
                out_normals[v] = s / np.sqrt(f32(f32(s[0] * s[0]) + f32(s[1] * s[1])) + f32(s[2] * s[2]))
    info = dict(vertices=len(verts), faces=len(faces), edges=len(on), boundary_edges=sum(n == 1 for n in on.values()),
                nonmanifold_edges=sum(n > 2 for n in on.values()), boundary_vertices=len(pinned),
                isolated_vertices=sum(not ring for ring in near), degenerate_faces=flat, exponent=e)
    return x, out_normals, info


def _same(got, want, tag):
    for name, a, b in zip(("verts", "normals"), got[:2], want[:2]):
        if b is None:
            assert a is None, (tag, name)
            continue
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{tag}: {name} differ"
    assert got[2] == want[2], (tag, got[2], want[2])


def _both(v, f, n, tag, **kw):
    got = SM.smooth(v, f, n, **kw)
    _same(got, _loop_smooth(v, f, n, kw.get("iterations", 10), kw.get("lam", 0.5), kw.get("mu", -0.53),
                            kw.get("free_boundary", False), kw.get("flip")), tag)
    return got


def test_restatement_matches_the_loop_on_every_fixture_mesh_and_what_the_fixture_covers(meshes):
    """The fixture's meshes are open pieces of surface in 2 x 2 x 2 to 5 x 5 x 5 volumes: with pinned boundaries 4216 of its
    12 610 vertices can move, in 121 of the 667 meshes; no edge is on more than two faces.  So the duplicate, both-windings,
    non-manifold, degenerate and isolated branches are taken by the hand-made meshes below."""
    assert len(meshes) == 667 and sum(len(v) for _, v, _, _ in meshes) == 12610
    movable = moving_meshes = fans = 0
    for i, v, f, n in meshes:
        pinned = _both(v, f, n, f"mesh {i} pinned", iterations=2, flip=-1)
        free = _both(v, f, None, f"mesh {i} free", iterations=2, free_boundary=True)
        assert free[1] is None and pinned[2] == free[2]
        adj = SM.adjacency(v, f)
        can = int(((adj["degree"] > 0) & ~adj["boundary"]).sum())
        movable += can
        moving_meshes += can > 0
        fans += pinned[2]["nonmanifold_edges"]
        still = ~((adj["degree"] > 0) & ~adj["boundary"])
        assert pinned[0][still].tobytes() == v[still].tobytes(), f"mesh {i}: a pinned vertex leaves as it came"
    assert (movable, moving_meshes, fans) == (4216, 121, 0)


def _sheet(k):
    idx = np.arange(k * k).reshape(k, k)
    gx, gy = np.meshgrid(np.arange(k, dtype=np.float32), np.arange(k, dtype=np.float32), indexing="ij")
    rng = np.random.default_rng(k)
    v = np.stack((gx.ravel(), gy.ravel(), rng.standard_normal(k * k).astype(np.float32)), 1).astype(np.float32)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    return v, np.concatenate((np.stack((a, b, c), 1), np.stack((a, c, d), 1))).astype(np.int32)


def test_hand_made_meshes_take_the_other_branches():
    v, f = _sheet(6)
    plain = _both(v, f, None, "sheet", iterations=3, flip=1)
    assert plain[2]["boundary_vertices"] == 20 and plain[2]["edges"] == 85 and plain[2]["boundary_edges"] == 20
    # a face listed twice / every face twice / once more with the other winding: the same neighbours, the same positions
    for tag, faces in (("one twice", np.concatenate((f, f[7:8]))), ("all twice", np.concatenate((f, f))),
                       ("both windings", np.concatenate((f, f, f[:, [0, 2, 1]])))):
        got = _both(v, faces, None, tag, iterations=3, flip=1)
        if tag == "one twice":                                       # an interior edge of that face is now on three faces
            assert got[2]["nonmanifold_edges"] > 0
            continue
        assert got[2]["boundary_edges"] == 0 and got[2]["edges"] == 85                   # every edge on 2 or 3 faces: nothing pinned,
        free = _both(v, f, None, "free", iterations=3, free_boundary=True, flip=1)       # as the plain sheet with a free boundary
        assert got[0].tobytes() == free[0].tobytes()
    # three faces on one edge (a fan of three wings on the edge 0-1), a degenerate face and an isolated vertex
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0.3], [0.5, 0, 1], [9, 9, 9]], np.float32)
    f = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4], [2, 2, 4]], np.int32)
    n = np.tile(np.float32([0, 0, 1]), (6, 1))
    got = _both(v, f, n, "fan", iterations=4, free_boundary=True, flip=-1)
    assert got[2] == dict(vertices=6, faces=4, edges=7, boundary_edges=6, nonmanifold_edges=1, boundary_vertices=5,
                          isolated_vertices=1, degenerate_faces=1, exponent=4)
    assert got[0][5].tobytes() == v[5].tobytes() and got[1][5].tobytes() == n[5].tobytes(), "the isolated vertex keeps everything"
    assert not np.array_equal(got[0][:5], v[:5])
    pinned = _both(v, f, n, "fan pinned", iterations=4)
    assert pinned[0].tobytes() == v.tobytes(), "every vertex of the fan is on an open edge"
    # nothing to do
    same = _both(v, f, n, "zero iterations", iterations=0)
    assert same[0].tobytes() == v.tobytes()
    zero = _both(np.zeros((4, 3), np.float32), f[:1], None, "all zero", iterations=3, free_boundary=True)
    assert zero[0].tobytes() == np.zeros((4, 3), np.float32).tobytes() and zero[2]["exponent"] == 0


def test_bad_inputs_raise():
    v = np.zeros((4, 3), np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    bad = v.copy()
    bad[2, 1], bad[3, 0] = np.nan, -np.inf
    with pytest.raises(ValueError, match="2 vertices have a non-finite coordinate"):
        SM.smooth(bad, f)
    with pytest.raises(ValueError, match=r"1 faces have a vertex index outside \[0, 4\)"):
        SM.smooth(v, np.array([[0, 1, 4], [0, 1, 2]], np.int32))
    for kw in (dict(iterations=-1), dict(iterations=1001), dict(lam=0.0), dict(lam=1.5), dict(lam=np.nan), dict(mu=0.1),
               dict(mu=-1.5), dict(mu=np.nan), dict(flip=0), dict(flip=2)):
        with pytest.raises(ValueError, match="mesh_smooth"):
            SM.smooth(v, f, **kw)


def _sphere(noise, res=48, seed=0):
    """marching cubes (the oracle's) of a res^3 distance field of a sphere of radius res / 3, with Gaussian noise on the field"""
    g = np.stack(np.meshgrid(*[np.arange(res, dtype=np.float64)] * 3, indexing="ij"), -1)
    centre = (res - 1) / 2.0
    field = res / 3.0 - np.sqrt(((g - centre) ** 2).sum(-1))
    if noise:
        field = field + np.random.default_rng(seed).normal(0.0, noise, field.shape)
    return mc_oracle.marching_cubes(field.astype(np.float32), 0.0)[:3] + (centre,)


@pytest.fixture(scope="module")
def noisy_sphere():
    return _sphere(0.4)


def _float_umbrella(verts, adj, movable, iterations, lam, mu):
    """the same filter with the same neighbour sets in plain fp64, positions kept in fp64 throughout"""
    x = verts.astype(np.float64)
    some = adj["degree"] > 0
    for f in [np.float64(np.float32(lam)), np.float64(np.float32(mu))] * iterations:
        mean = np.zeros_like(x)
        mean[some] = np.add.reduceat(x[adj["dst"]], adj["starts"], axis=0) / adj["degree"][some, None]
        x = np.where(movable[:, None], x + f * (mean - x), x)
    return x


def _ulps(v, f, iterations, free_boundary):
    adj = SM.adjacency(v, f)
    if adj["largest"] == 0:
        return 0.0
    movable = (adj["degree"] > 0) & (free_boundary | ~adj["boundary"])
    got = SM.smooth(v, f, iterations=iterations, free_boundary=free_boundary)[0].astype(np.float64)
    want = _float_umbrella(v, adj, movable, iterations, 0.5, -0.53)
    return float(np.abs(got - want).max() / np.spacing(adj["largest"])) if len(v) else 0.0


def test_distance_from_a_float_umbrella(meshes, noisy_sphere):
    """The restatement (never the kernels) against the same filter in fp64 with the same neighbour sets, in fp32 ulp of the
    largest coordinate.  The restatement rounds the positions to fp32 after every half-step and the means to 2^-40 of the
    coordinate range; the fp64 filter does neither, so the difference is a random walk of half-ulp roundings damped by the
    filter.  Measured: 2.82 ulp over the 667 fixture meshes at 5 iterations (pinned and free boundary), 3.56 ulp on the 48^3
    sphere volumes (noise-free and sigma = 0.4) at 20.  Asserted with a margin of x 2 for inputs not tried."""
    worst = max(_ulps(v, f, 5, free) for _, v, f, _ in meshes for free in (False, True))
    print(f"fixture, 5 iterations: {worst:.3f} ulp")
    v0, f0 = _sphere(0.0)[:2]
    spheres = max(_ulps(v, f, 20, False) for v, f in ((v0, f0), noisy_sphere[:2]))
    print(f"spheres, 20 iterations: {spheres:.3f} ulp")
    assert worst <= 2 * 2.82 and spheres <= 2 * 3.56


def test_the_filter_smooths_a_noisy_sphere_without_shrinking_it(noisy_sphere):
    v, f, _, centre = noisy_sphere
    assert SM.adjacency(v, f)["info"]["boundary_edges"] == 0, "a closed surface: every vertex moves"

    def radii(x):
        return np.sqrt(((x.astype(np.float64) - centre) ** 2).sum(1))

    before, taubin, laplace = radii(v), radii(SM.smooth(v, f, iterations=10)[0]), radii(SM.smooth(v, f, iterations=10, mu=0.0)[0])
    print(f"radial std {before.std():.4f} -> {taubin.std():.4f} (Laplacian {laplace.std():.4f}); mean radius moves by "
          f"{abs(taubin.mean() - before.mean()):.4f} (Laplacian {abs(laplace.mean() - before.mean()):.4f})")
    assert taubin.std() < before.std()
    assert abs(taubin.mean() - before.mean()) < abs(laplace.mean() - before.mean())


def test_the_sign_mesh_nerf_passes_turns_the_normals_outwards():
    """marching cubes winds its triangles against the normals it returns (towards lower density): with mesh_nerf's flip every
    recomputed vertex normal of a noise-free sphere lies on the side of the oracle's."""
    from nerfmeshes_amd import mesh_nerf
    v, f, n, _ = _sphere(0.0)
    assert len(f) > 8000
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    against = (np.cross(b - a, c - a) * n[f[:, 0]]).sum(1) < 0
    assert against.all(), "every face winds against the normals marching cubes returns"
    assert mesh_nerf.SMOOTH_FLIP == -1
    for iterations in (0, 5):
        sv, sn, _ = SM.smooth(v, f, n, iterations=iterations, flip=mesh_nerf.SMOOTH_FLIP)
        assert ((sn * n).sum(1) > 0).all() and np.allclose(np.linalg.norm(sn, axis=1), 1.0, atol=1e-6)
    assert ((SM.vertex_normals(v, f, None, 1) * n).sum(1) < 0).all()


def test_parser_defaults_and_negatives():
    from nerfmeshes_amd import mesh_nerf
    p = mesh_nerf.build_parser()
    d = p.parse_args([])
    assert (d.smooth_iters, d.smooth_lambda, d.smooth_mu, d.smooth_boundary) == (0, 0.5, -0.53, "fixed")
    a = p.parse_args(["--smooth-iters", "7", "--smooth-lambda", "0.3", "--smooth-mu", "-0.31", "--smooth-boundary", "free"])
    assert (a.smooth_iters, a.smooth_lambda, a.smooth_mu, a.smooth_boundary) == (7, 0.3, -0.31, "free")
    for dest in ("smooth_iters", "smooth_lambda", "smooth_mu", "smooth_boundary"):
        assert "(addition)" in next(x.help for x in p._actions if x.dest == dest)
    for bad in (["--smooth-iters", "-1"], ["--smooth-iters", "1.5"], ["--smooth-iters", "two"], ["--smooth-lambda", "half"],
                ["--smooth-boundary", "loose"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


@pytest.mark.parametrize("option", [["--smooth-iters", "3"], ["--smooth-lambda", "0.4"], ["--smooth-mu", "-0.4"],
                                    ["--smooth-boundary", "free"]], ids=lambda o: o[0])
def test_route_script_rejects_the_options(tmp_path, option):
    from nerfmeshes_amd import mesh_nerf
    args = mesh_nerf.build_parser().parse_args([*option, "--route", "script", "--save-dir", str(tmp_path)])
    with pytest.raises(ValueError, match="route script"):
        mesh_nerf.export_marching_cubes(None, args, None, "cpu")
    assert not any(tmp_path.iterdir()), "rejected before anything is written"


@pytest.mark.parametrize("option", [["--smooth-iters", "1001"], ["--smooth-lambda", "0"], ["--smooth-lambda", "1.5"],
                                    ["--smooth-lambda", "nan"], ["--smooth-mu", "0.2"], ["--smooth-mu", "-2"]],
                         ids=lambda o: " ".join(o))
def test_values_out_of_range_are_rejected_before_anything_is_written(tmp_path, option):
    from nerfmeshes_amd import mesh_nerf
    extra = [] if option[0] == "--smooth-iters" else ["--smooth-iters", "2"]
    args = mesh_nerf.build_parser().parse_args([*option, *extra, "--save-dir", str(tmp_path)])
    with pytest.raises(ValueError, match="--smooth-iters must be in"):
        mesh_nerf.export_marching_cubes(None, args, None, "cpu")
    assert not any(tmp_path.iterdir())


def test_argument_errors_without_a_gpu():
    from nerfmeshes_amd import _lib
    lib = _lib.load()
    null, one, two = C.c_void_p(None), C.c_void_p(256), C.c_void_p(512)     # never dereferenced: validation fails first
    counts = (C.c_int64 * 9)(*([-7] * 9))

    def err():
        return (lib.nm_last_error() or b"").decode()

    def build(v=one, nv=20, f=one, nf=10, ws=one, out=counts):
        return lib.nm_mesh_smooth_build(v, nv, f, nf, ws, out, null)

    def run(ws=one, v=one, nv=20, n=5, lam=0.5, mu=-0.53, flags=0, ov=two):
        return lib.nm_mesh_smooth_run(ws, v, nv, n, lam, mu, flags, ov, null)

    def normals(v=one, nv=20, f=one, nf=10, n=null, flip=1, ws=one, on=two):
        return lib.nm_mesh_vertex_normals(v, nv, f, nf, n, flip, ws, on, null)

    for fn in (build, normals):
        for kw in (dict(v=null), dict(f=null), dict(ws=null)):
            assert fn(**kw) == 2 and "bad argument" in err(), (fn.__name__, kw)
        for kw in (dict(nf=-1), dict(nv=-1), dict(nv=1 << 31), dict(nv=(1 << 31) - 64), dict(nf=(1 << 31) - 64)):
            assert fn(**kw) == 2 and "2^31" in err(), (fn.__name__, kw)
        assert fn(nf=3, nv=0) == 2 and "faces without vertices" in err()
    assert build(out=None) == 2 and "bad argument" in err()
    assert list(counts) == [-7] * 9, "nothing is returned by a rejected call"
    for kw in (dict(ws=null), dict(v=null), dict(ov=null)):
        assert run(**kw) == 2 and "bad argument" in err(), kw
    assert run(ov=one) == 2 and "must not be the input" in err()
    for nv in (-1, 1 << 31, (1 << 31) - 64):
        assert run(nv=nv) == 2 and "2^31" in err(), nv
    for n in (-1, 1001, 1 << 30):
        assert run(n=n) == 2 and "iterations" in err(), n
    for lam in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert run(lam=lam) == 2 and "lambda" in err(), lam
    for mu in (1e-6, 0.5, -1.0000001, float("nan"), float("-inf")):
        assert run(mu=mu) == 2 and "mu must be" in err(), mu
    for flags in (2, 3, -1):
        assert run(flags=flags) == 2 and "flags" in err(), flags
    assert normals(on=null) == 2 and "bad argument" in err()
    for flip in (0, 2, -2):
        assert normals(flip=flip) == 2 and "flip" in err(), flip
    # the workspace: 12 bytes per slot of a table of >= 6 F slots, 24 F of neighbour lists, 52 V for the per-vertex arrays
    size = lib.nm_mesh_smooth_workspace_bytes
    assert size(-1, 0) == 0 and size(0, -1) == 0 and size(1 << 31, 0) == 0 and size(0, (1 << 31) - 64) == 0
    assert size((1 << 31) - 64, 0) == 0 and size(0, 0) > 0
    lower = 12 * (1 << 24) + 24 * 1_996_002 + 52 * 1_000_000
    assert lower <= size(1_000_000, 1_996_002) <= lower + 1_000_000 // 8 + 16 * 256
    most = (1 << 31) - 65                                                # the largest accepted sizes: 64-bit offsets, nothing wraps
    assert size(most, most) >= 12 * (1 << 34) + 24 * most + 52 * most
    assert lib.nm_abi_version() == 6


def test_wrapper_checks_its_arguments_before_the_device():
    import torch
    from nerfmeshes_amd import _lib, hip_ops
    v, f = torch.zeros(8, 3), torch.zeros(4, 3, dtype=torch.int32)
    with pytest.raises(_lib.HipLibraryError, match="GPU memory"):
        hip_ops.mesh_smooth(v, f, iterations=1)
    for kw in (dict(iterations=-1), dict(iterations=1001), dict(lam=0.0), dict(lam=2.0), dict(mu=0.5), dict(mu=-1.5),
               dict(lam=float("nan")), dict(flip=0)):
        with pytest.raises(ValueError, match="mesh_smooth"):
            hip_ops.mesh_smooth(v, f, **kw)
