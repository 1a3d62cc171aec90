"""CPU: the super-sampled mesh's refinement rule (tests/ss_refine.py) against the C oracle and exact crossings, and the
argument checks of its C entries (nm_mc_vertex_edges, nm_mc_edge_points, nm_mc_refine_vertices, nm_mlp_sample_density),
which reject bad input before any HIP call."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from oracle import mc_oracle
from tests import ss_refine


def _smooth(shape, seed):
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.linspace(-1, 1, s) for s in shape], indexing="ij"), -1)
    c = rng.uniform(0.5, 3.0, (3,))
    ph = rng.uniform(0, np.pi, (3,))
    vol = np.sin(c[0] * g[..., 0] + ph[0]) * np.cos(c[1] * g[..., 1] + ph[1]) + 0.7 * np.sin(c[2] * g[..., 2] + ph[2])
    return (vol + 0.05 * rng.standard_normal(shape)).astype(np.float32)


@pytest.mark.parametrize("seed,shape", [(0, (9, 11, 13)), (1, (16, 16, 16)), (2, (5, 23, 7)), (3, (20, 12, 17))])
def test_restatement_at_ss0_is_the_oracles_interpolation(seed, shape):
    """ss = 0: the rule reduces to skimage's inverse-|v| interpolation, so every edge vertex comes back bit for bit."""
    vol = _smooth(shape, seed)
    iso = float(np.float32(0.1))
    verts = mc_oracle.marching_cubes(vol, iso)[0]
    rows, keys_for = ss_refine.keys_from_vertices(verts)
    assert len(rows) > 0.5 * len(verts)
    keys = keys_for(shape)
    scrambled = verts[rows].copy()
    ijk, axis = ss_refine.decode(keys, shape)
    scrambled[np.arange(len(rows)), axis] = ijk[np.arange(len(rows)), axis] + 0.25      # forget the along-edge coordinate
    got = ss_refine.refine(vol, 0, iso, keys, 0, np.zeros((len(rows), 0), np.float32), scrambled, shape)
    assert got.tobytes() == verts[rows].tobytes()


@pytest.mark.parametrize("ss", [1, 2, 3, 7, 16])
def test_piecewise_linear_field_gives_the_exact_crossing(ss):
    """A field that is linear between consecutive fine samples crosses the level where inverse-|d| interpolation of the
    bracketing pair says: the refined coordinate is the exact first crossing to 1 fp32 ulp."""
    rng = np.random.default_rng(ss)
    n = 6
    nums = (n, n, n)
    for trial in range(200):
        a = int(rng.integers(0, 3))
        i = [int(rng.integers(0, n - 1)) for _ in range(3)]
        iso = 0.5
        d = rng.choice([-1.0, 1.0], ss + 2) * rng.uniform(0.01, 1.0, ss + 2)
        d[0] = abs(d[0]) * (1 if trial % 2 else -1)
        d[-1] = -abs(d[-1]) * np.sign(d[0])                              # a cut edge: the ends differ in sign
        d = d.astype(np.float32).astype(np.float64)
        vals = (d + iso).astype(np.float32)
        vol = np.full(nums, iso + 1, dtype=np.float32)
        lo = tuple(i)
        hi = list(i)
        hi[a] += 1
        vol[lo], vol[tuple(hi)] = vals[0], vals[-1]
        key = ((i[0] * n + i[1]) * n + i[2]) * 4 + a
        got = ss_refine.refine(vol, 0, iso, np.array([key]), ss, vals[1:-1][None], np.zeros((1, 3), np.float32), nums)[0, a]
        dd = [Fraction(float(v)) - Fraction(iso) for v in vals]
        m = next(k for k in range(ss + 1) if (dd[k] > 0) != (dd[k + 1] > 0))
        exact = i[a] + (m + dd[m] / (dd[m] - dd[m + 1])) / (ss + 1)
        want = np.float32(float(exact))
        assert abs(int(np.float32(got).view(np.int32)) - int(want.view(np.int32))) <= 1, (trial, got, float(exact))


def test_edge_points_restatement_layout():
    nums, ss = (4, 5, 6), 3
    base = [np.linspace(-1, 1, n, dtype=np.float32) for n in nums]
    fine = [np.linspace(-1, 1, (n - 1) * (ss + 1) + 1, dtype=np.float32) for n in nums]
    key = ((2 * 5 + 3) * 6 + 4) * 4 + 1                                # voxel (2, 3, 4), along axis 1
    p = ss_refine.edge_points(np.array([key]), nums, ss, base, fine)[0]
    for s in range(1, ss + 1):
        assert p[s - 1].tolist() == [base[0][2], fine[1][3 * (ss + 1) + s], base[2][4]]


@pytest.fixture(scope="module")
def lib():
    from nerfmeshes_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _err(lib):
    return (lib.nm_last_error() or b"").decode()


def test_new_c_entries_reject_bad_arguments_without_a_gpu(lib):
    null, one = C.c_void_p(None), C.c_void_p(8)          # `one` is never dereferenced: validation fails first
    # nm_mc_vertex_edges(scratch, vertices, ghost_vertices, n0, n1, n2, z_global, keys, stream)
    assert lib.nm_mc_vertex_edges(null, 10, 0, 4, 4, 4, 0, one, null) == 2 and "bad argument" in _err(lib)
    assert lib.nm_mc_vertex_edges(one, 10, 0, 4, 4, 4, 0, null, null) == 2 and "bad argument" in _err(lib)
    assert lib.nm_mc_vertex_edges(one, 10, 0, 1, 4, 4, 0, one, null) == 2 and "2x2x2" in _err(lib)
    assert lib.nm_mc_vertex_edges(one, 10, 11, 4, 4, 4, 0, one, null) == 2
    assert lib.nm_mc_vertex_edges(one, 10, 0, 4, 4, 4, -1, one, null) == 2
    assert lib.nm_mc_vertex_edges(null, 5, 5, 4, 4, 4, 0, null, null) == 0          # no own rows: nothing to do
    # nm_mc_edge_points(keys, V, n0, n1, n2, ss, base0..2, fine0..2, points, stream)
    ep = lambda keys, V, n, ss, pts: lib.nm_mc_edge_points(keys, V, n[0], n[1], n[2], ss, one, one, one, one, one, one, pts, null)
    assert ep(null, 10, (4, 4, 4), 2, one) == 2 and "bad argument" in _err(lib)
    assert ep(one, 10, (4, 4, 4), 2, null) == 2 and "bad argument" in _err(lib)
    for ss in (-1, 65, 1000):
        assert ep(one, 10, (4, 4, 4), ss, one) == 2 and "[0, 64]" in _err(lib)
    assert ep(one, 10, (4, 1, 4), 2, one) == 2 and "2x2x2" in _err(lib)
    assert ep(one, 10, (4, 2 ** 30, 4), 2, one) == 2 and "int32" in _err(lib)       # (n-1)*(ss+1)+1 > 2^31-1
    assert ep(one, -1, (4, 4, 4), 2, one) == 2
    assert lib.nm_mc_edge_points(null, 0, 4, 4, 4, 2, null, null, null, null, null, null, null, null) == 0
    # nm_mc_refine_vertices(volume, n0, n1, n2, z_global, iso, keys, V, ss, fine_sigma, verts, stream)
    rv = lambda vol, n, zg, keys, V, ss, sig, verts: lib.nm_mc_refine_vertices(vol, n[0], n[1], n[2], zg, 0.5, keys, V, ss, sig, verts, null)
    assert rv(null, (4, 4, 4), 0, one, 10, 2, one, one) == 2 and "bad argument" in _err(lib)
    assert rv(one, (4, 4, 4), 0, null, 10, 2, one, one) == 2 and "bad argument" in _err(lib)
    assert rv(one, (4, 4, 4), 0, one, 10, 2, null, one) == 2 and "bad argument" in _err(lib)   # ss > 0 needs the samples
    assert rv(one, (4, 4, 4), 0, one, 10, 2, one, null) == 2 and "bad argument" in _err(lib)
    for ss in (-1, 65):
        assert rv(one, (4, 4, 4), 0, one, 10, ss, one, one) == 2 and "[0, 64]" in _err(lib)
    assert rv(one, (4, 4, 1), 0, one, 10, 2, one, one) == 2 and "2x2x2" in _err(lib)
    assert rv(one, (4, 4, 4), -3, one, 10, 2, one, one) == 2
    assert rv(one, (4, 4, 2 ** 30), 0, one, 10, 2, one, one) == 2 and "int32" in _err(lib)
    # nm_mlp_sample_density(mlp, points, n, sigma, stream)
    assert lib.nm_mlp_sample_density(null, one, 4, one, null) == 2 and "bad argument" in _err(lib)
    assert lib.nm_mlp_sample_density(one, null, 4, one, null) == 2
    assert lib.nm_mlp_sample_density(one, one, 4, null, null) == 2
