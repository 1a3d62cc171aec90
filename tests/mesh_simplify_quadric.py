"""Quadric placement of mesh simplification restated in numpy (include/nerfmeshes_hip.h, "QUADRIC PLACEMENT"): what
nm_mesh_simplify_quadric_faces / nm_mesh_simplify_emit_quadric must give, bit for bit.  Everything the two placements share --
cells, clusters, faces, numbering, normals, the mean -- is tests/mesh_simplify.py's; the sums are int64 sums, every fp64
operation is a numpy float64 operation (rounded on its own), in the header's order.

  lattice     u = int64(rint(float64(t) * 2^8)) clamped to [-2^9, 2^9]
  corner      per face and corner k, to the cluster of that corner: e1 = (C1 - C0) * 2^8 + (u1 - u0), e2 for the third corner
              (cyclic from k); a component beyond 2^9: FAR, nothing.  nrm = e1 x e2, d = -(nrm . u0); A += nrm nrm^T (six), B += nrm d
  position    n >= 2, 1 <= contributions <= 2^13, tr > 0: (A + tr 2^-6 I) delta = -(A m + b) by the adjugate, x = clamp(m + delta)
"""
import numpy as np

from tests import mesh_simplify as MS

LATTICE = 256
REACH = 512
MAX_CONTRIBUTIONS = 1 << 13
LAMBDA = 2.0 ** -6
COUNT_KEYS = ("quadric_clusters", "crowded_clusters", "singular_clusters", "clamped_clusters", "far_corners")
INFO_KEYS = MS.INFO_KEYS + COUNT_KEYS
SOLVED, CROWDED, SINGULAR, CLAMPED = 1, 2, 4, 8


def grid(verts, cell, origin):
    """the (origin, cell) MS.simplify uses, as float32"""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    if origin is None:
        origin = np.where(np.isfinite(verts), verts, np.inf).min(axis=0) if len(verts) else np.zeros(3)
        origin = np.where(np.isfinite(origin), origin, 0.0)
    return np.asarray(origin, dtype=np.float32).reshape(3), np.float32(cell)


def lattice_of(t):
    """u of t = (x - lo) / cell (float32)"""
    with np.errstate(all="ignore"):
        s = np.asarray(t, dtype=np.float32).astype(np.float64) * np.float64(LATTICE)
        s = np.where(~(s >= -REACH), -np.float64(REACH), np.where(s > REACH, np.float64(REACH), s))
    return np.rint(s).astype(np.int64)


def lattice(verts, origin, cell):
    """-> (C (V,3) int64 cell indices, u (V,3) int64 lattice coordinates local to the cell, q (V,3) int64: MS's 2^30 quanta)"""
    c, _ = MS.cells(verts, origin, cell)
    with np.errstate(all="ignore"):
        lo = origin + c * cell
        t = (verts - lo) / cell
        p = t.astype(np.float64) * MS.QUANTUM
        p = np.where(~(p >= -MS.QMAX), -MS.QMAX, np.where(p > MS.QMAX, MS.QMAX, p))
    return c.astype(np.int64), lattice_of(t), np.rint(p).astype(np.int64)


def kept_clusters(verts, faces, origin, cell):
    """-> (C, u, q of lattice(); cluster (V,) index of every vertex's cluster; first (K,) the clusters' representatives; reps:
    the representatives of the clusters a kept face references, ascending -- the rows MS.simplify returns)"""
    C, u, q = lattice(verts, origin, cell)
    key = C[:, 0] | (C[:, 1] << 21) | (C[:, 2] << 42)
    _, first, cluster = np.unique(key, return_index=True, return_inverse=True)
    cluster = cluster.reshape(-1)
    tri = first[cluster][faces.astype(np.int64)].reshape(-1, 3)
    flat = (tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2])
    live = np.flatnonzero(~flat)
    keep_f = np.zeros(len(faces), dtype=bool)
    keep_f[live[MS.first_of_equal_rows(MS.canonical(tri[live]))]] = True
    return C, u, q, cluster, first, np.unique(tri[keep_f].reshape(-1))


def corner_terms(faces, C, u):
    """-> (terms (F,3,9) int64: the six nrm_i nrm_j and the three nrm_i d of every corner, zeros where far; far (F,3) bool)"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    terms = np.zeros((len(f), 3, 9), dtype=np.int64)
    far = np.zeros((len(f), 3), dtype=bool)
    for k in range(3):
        v0, v1, v2 = f[:, k], f[:, (k + 1) % 3], f[:, (k + 2) % 3]
        e1 = (C[v1] - C[v0]) * LATTICE + (u[v1] - u[v0])
        e2 = (C[v2] - C[v0]) * LATTICE + (u[v2] - u[v0])
        far[:, k] = (np.abs(e1) > REACH).any(axis=1) | (np.abs(e2) > REACH).any(axis=1)
        e1, e2 = np.where(far[:, k, None], 0, e1), np.where(far[:, k, None], 0, e2)
        n = np.stack((e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]), 1)
        d = -(n * u[v0]).sum(axis=1)
        terms[:, k] = np.stack((n[:, 0] * n[:, 0], n[:, 0] * n[:, 1], n[:, 0] * n[:, 2], n[:, 1] * n[:, 1], n[:, 1] * n[:, 2],
                                n[:, 2] * n[:, 2], n[:, 0] * d, n[:, 1] * d, n[:, 2] * d), 1)
    return terms, far


def quadric_sums(faces, cluster, clusters, C, u):
    """-> (sums (clusters, 9) int64: A[6] and B[3], contributions (clusters,) int64, far corners).  int64 wraps as the device's
    adds do; a cluster within the bound never does."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    terms, far = corner_terms(f, C, u)
    where = cluster[f][~far]                                         # the cluster of every corner that contributes
    rows = terms[~far]
    sums = np.zeros((clusters, 9), dtype=np.int64)
    contributions = np.bincount(where, minlength=clusters).astype(np.int64)
    if len(where):
        order = np.argsort(where, kind="stable")
        present, starts = np.unique(where[order], return_index=True)
        sums[present] = np.add.reduceat(rows[order], starts, axis=0)
    return sums, contributions, int(far.sum())


def place(frac, sums, contributions):
    """frac (K,3) float64: the members' mean in units of the cell -> (frac: x / 2^8 where SOLVED, the mean elsewhere; status (K,))"""
    f64 = np.float64
    with np.errstate(all="ignore"):
        a00, a01, a02, a11, a12, a22, b0, b1, b2 = (sums[:, i].astype(f64) for i in range(9))
        tr = (a00 + a11) + a22
        m0, m1, m2 = frac[:, 0] * f64(LATTICE), frac[:, 1] * f64(LATTICE), frac[:, 2] * f64(LATTICE)
        ridge = tr * f64(LAMBDA)
        M00, M11, M22, M01, M02, M12 = a00 + ridge, a11 + ridge, a22 + ridge, a01, a02, a12
        r0 = -(((a00 * m0 + a01 * m1) + a02 * m2) + b0)
        r1 = -(((a01 * m0 + a11 * m1) + a12 * m2) + b1)
        r2 = -(((a02 * m0 + a12 * m1) + a22 * m2) + b2)
        c00 = M11 * M22 - M12 * M12
        c01 = M02 * M12 - M01 * M22
        c02 = M01 * M12 - M02 * M11
        c11 = M00 * M22 - M02 * M02
        c12 = M01 * M02 - M00 * M12
        c22 = M00 * M11 - M01 * M01
        det = (M00 * c00 + M01 * c01) + M02 * c02
        d0 = ((c00 * r0 + c01 * r1) + c02 * r2) / det
        d1 = ((c01 * r0 + c11 * r1) + c12 * r2) / det
        d2 = ((c02 * r0 + c12 * r1) + c22 * r2) / det
        x = np.stack((m0 + d0, m1 + d1, m2 + d2), 1)
        crowded = contributions > MAX_CONTRIBUTIONS
        tried = ~crowded & (contributions > 0) & (tr > 0)
        singular = tried & ~((det > 0) & np.isfinite(d0) & np.isfinite(d1) & np.isfinite(d2))
        solved = tried & ~singular
        clamped = solved & ((x < 0) | (x > LATTICE)).any(axis=1)
        x = np.where(x < 0, f64(0), np.where(x > LATTICE, f64(LATTICE), x))
        out = np.where(solved[:, None], x / f64(LATTICE), frac)
    status = SOLVED * solved + CROWDED * crowded + SINGULAR * singular + CLAMPED * clamped
    return out, status


def simplify(verts, faces, normals=None, cell=1.0, origin=None, placement="quadric"):
    """-> (verts, faces, normals, info), as hip_ops.mesh_simplify(..., placement=placement)"""
    if placement not in ("mean", "quadric"):
        raise ValueError(f"mesh_simplify: placement must be one of ('mean', 'quadric'), got {placement!r}")
    out_verts, out_faces, out_normals, info = MS.simplify(verts, faces, normals, cell=cell, origin=origin)   # raises for bad input
    if placement == "mean":
        return out_verts, out_faces, out_normals, info
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    origin, cell = grid(verts, cell, origin)
    C, u, q, cluster, first, reps = kept_clusters(verts, faces, origin, cell)
    count = np.bincount(cluster, minlength=len(first))
    assert len(reps) == len(out_verts)
    kept = cluster[reps]
    sums, contributions, far = quadric_sums(faces, cluster, len(first), C, u)
    members = count[kept]
    with np.errstate(all="ignore"):
        psum = MS.cluster_sums(q, cluster, len(first))
        mean = psum[kept].astype(np.float64) / (members.astype(np.float64) * MS.QUANTUM)[:, None]
        frac, status = place(mean, sums[kept], contributions[kept])
        status = np.where(members >= 2, status, 0)
        c32, _ = MS.cells(verts[reps], origin, cell)
        lo = origin + c32 * cell
        moved = (lo.astype(np.float64) + np.float64(cell) * frac).astype(np.float32)
    out_verts = np.where(((status & SOLVED) != 0)[:, None], moved, out_verts)
    info = dict(info, quadric_clusters=int(((status & SOLVED) != 0).sum()), crowded_clusters=int(((status & CROWDED) != 0).sum()),
                singular_clusters=int(((status & SINGULAR) != 0).sum()), clamped_clusters=int(((status & CLAMPED) != 0).sum()),
                far_corners=far)
    return np.ascontiguousarray(out_verts).reshape(-1, 3), out_faces, out_normals, info
