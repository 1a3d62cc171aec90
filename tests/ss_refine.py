"""numpy restatement of the super-sampled mesh's edge samples and vertex refinement (DESIGN.md "Super-sampled meshing",
items 2-3): what nm_mc_edge_points / nm_mc_refine_vertices must compute, written for clarity, not speed.

key = global linear index of an edge's lower-corner voxel * 4 + axis (array order; 3 = a centre vertex)."""
import numpy as np

SK_EPS = 2.220446049250313e-16     # skimage's "FLT_EPSILON" (np.spacing(1.0))


def decode(keys, nums):
    keys = np.asarray(keys, dtype=np.int64)
    vox, axis = keys >> 2, keys & 3
    n0, n1, n2 = nums
    return np.stack([vox // (n1 * n2), (vox // n2) % n1, vox % n2], -1), axis


def keys_from_vertices(verts):
    """Keys of the vertices of a plain marching-cubes mesh (grid-index units) that have exactly two integral coordinates --
    the edge vertices whose position is strictly inside their edge -- as (rows, keys) for a grid of any size: the key's
    voxel is returned as (i0, i1, i2) through `keys_for(nums)`."""
    v = np.asarray(verts, dtype=np.float32)
    integral = v == np.floor(v)
    rows = np.nonzero(integral.sum(1) == 2)[0]
    axis = np.argmin(integral[rows], axis=1)
    vox = np.floor(v[rows]).astype(np.int64)

    def keys_for(nums):
        n0, n1, n2 = nums
        return ((vox[:, 0] * n1 + vox[:, 1]) * n2 + vox[:, 2]) * 4 + axis

    return rows, keys_for


def edge_points(keys, nums, ss, base, fine):
    """(V, ss, 3) fp32: sample s = 1..ss of the edge of voxel i along axis a has coordinate a = fine_a[i_a*(ss+1) + s], the
    other two base.  Centre rows: the voxel's base point."""
    ijk, axis = decode(keys, nums)
    base = [np.asarray(b, dtype=np.float32) for b in base]
    fine = [np.asarray(f, dtype=np.float32) for f in fine]
    p = np.stack([base[k][ijk[:, k]] for k in range(3)], -1)
    out = np.repeat(p[:, None, :], ss, axis=1)
    for a in range(3):
        rows = np.nonzero(axis == a)[0]
        for s in range(1, ss + 1):
            out[rows, s - 1, a] = fine[a][ijk[rows, a] * (ss + 1) + s]
    return out


def refine(volume, z_global, iso, keys, ss, fine_sigma, verts, nums):
    """Refined copy of verts (V,3) fp32 (grid-index units).  `volume` holds the global planes [z_global, z_global + n0)
    of a grid of extents `nums`; fine_sigma (V, ss) fp32.  For each edge row: d = (v_lo, f_1..f_ss, v_hi) - iso in fp64,
    m = the first index with (d_m > 0) != (d_m+1 > 0), w1 = 1/(eps + |d_m|), w2 = 1/(eps + |d_m+1|), coordinate a =
    i_a + (m + w2/(w1+w2)) / (ss+1), rounded to fp32 once.  Centre rows (axis 3) are copied."""
    vol = np.asarray(volume, dtype=np.float32)
    out = np.array(verts, dtype=np.float32, copy=True)
    ijk, axis = decode(keys, nums)
    rows = np.nonzero(axis != 3)[0]
    if len(rows) == 0:
        return out
    a = axis[rows]
    lo = ijk[rows].copy()
    lo[:, 0] -= z_global
    hi = lo.copy()
    hi[np.arange(len(rows)), a] += 1
    f = np.asarray(fine_sigma, dtype=np.float32).reshape(len(out), ss)[rows]
    d = np.concatenate([vol[lo[:, 0], lo[:, 1], lo[:, 2]].astype(np.float64)[:, None], f.astype(np.float64),
                        vol[hi[:, 0], hi[:, 1], hi[:, 2]].astype(np.float64)[:, None]], 1) - float(iso)
    pos = d > 0
    change = pos[:, :-1] != pos[:, 1:]
    assert change.any(1).all(), "every edge vertex lies on a cut edge"
    m = np.argmax(change, axis=1)                      # the first sign change from the lower end
    k = np.arange(len(rows))
    w1 = 1.0 / (SK_EPS + np.abs(d[k, m]))
    w2 = 1.0 / (SK_EPS + np.abs(d[k, m + 1]))
    t = (m.astype(np.float64) + w2 / (w1 + w2)) / float(ss + 1)
    out[rows, a] = (ijk[rows, a].astype(np.float64) + t).astype(np.float32)
    return out
