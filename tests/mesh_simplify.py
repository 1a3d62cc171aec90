"""Mesh simplification by vertex clustering restated in numpy (the role tests/mesh_components.py plays for its kernels): what
nm_mesh_simplify_cluster / _emit must give, bit for bit.  Every fp32 operation is a numpy float32 operation (rounded on its
own), the sums are int64 sums.

  cell        c = floor((x - origin) / cell) per axis in fp32; a vertex with a non-finite coordinate or a c outside [0, 2^21)
              is bad, a face with an index outside [0, V) is bad: either raises ValueError, as hip_ops.mesh_simplify does
  cluster     all vertices of one cell; representative = its smallest vertex index
  position    one member: that member's rows.  More: lo = origin + c * cell, t = (x - lo) / cell,
              q = int64(rint(float64(t) * 2^30)) clamped to [-2^31, 2^31], S = sum q,
              p = float32(float64(lo) + float64(cell) * (float64(S) / (float64(n) * 2^30)))
  normal      q = int64(rint(float64(component) * 2^30)) of the members whose three components are finite and <= 2 in magnitude;
              s = float32(S); s / sqrt((sx sx + sy sy) + sz sz); S = 0: the representative's own normal
  faces       corners -> representatives; two equal corners: degenerate; same corners in the same cyclic order: duplicates, the
              smallest face index stays; kept faces in input order, corners in their own order
  vertices    clusters on a kept face, by ascending representative: new = cumsum(used) - 1
"""
import numpy as np

CELLS = 1 << 21
QUANTUM = float(1 << 30)
QMAX = float(1 << 31)
NORMAL_MAX = np.float32(2.0)
INFO_KEYS = ("vertices", "faces", "clusters", "vertices_kept", "faces_kept", "degenerate_faces", "duplicate_faces")


def cells(verts, origin, cell):
    """-> (c (V,3) float32 cell indices, bad (V,) bool)"""
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    origin, cell = np.asarray(origin, dtype=np.float32), np.float32(cell)
    with np.errstate(all="ignore"):
        c = np.floor((verts - origin) / cell)
        bad = ~(np.isfinite(verts) & (c >= 0) & (c < CELLS)).all(axis=1)
    return c, bad


def canonical(tri):
    """(N,3) corner triples with the smallest corner rotated to the front (the cyclic order kept)"""
    tri = np.asarray(tri)
    k = np.where((tri[:, 0] <= tri[:, 1]) & (tri[:, 0] <= tri[:, 2]), 0, np.where(tri[:, 1] <= tri[:, 2], 1, 2))
    rows = np.arange(len(tri))
    return np.stack((tri[rows, k], tri[rows, (k + 1) % 3], tri[rows, (k + 2) % 3]), 1)


def first_of_equal_rows(rows):
    """indices of the first row of every set of equal rows: np.unique(rows, axis=0, return_index=True)[1] without its order --
    a stable lexicographic sort keeps equal rows in input order, so the head of each run is the smallest index (np.unique on
    rows sorts a structured view: several seconds on two million faces)"""
    if len(rows) == 0:
        return np.zeros(0, dtype=np.int64)
    order = np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))
    ordered = rows[order]
    head = np.ones(len(rows), dtype=bool)
    head[1:] = (ordered[1:] != ordered[:-1]).any(axis=1)
    return order[head]


def cluster_sums(q, cluster, clusters):
    """(clusters, 3) int64: the sum of q's rows per cluster (every cluster has a member)"""
    order = np.argsort(cluster, kind="stable")
    starts = np.searchsorted(cluster[order], np.arange(clusters))
    return np.add.reduceat(q[order], starts, axis=0) if len(q) else np.zeros((0, 3), dtype=np.int64)


def simplify(verts, faces, normals=None, cell=1.0, origin=None):
    """-> (verts, faces, normals, info), as hip_ops.mesh_simplify (numpy arrays in, numpy arrays out)."""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    if normals is not None:
        normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    nv, nf = len(verts), len(faces)
    cell = np.float32(cell)
    if not (np.isfinite(cell) and cell > 0):
        raise ValueError(f"mesh_simplify: the cell size must be finite and > 0, got {cell}")
    if origin is None:
        origin = np.where(np.isfinite(verts), verts, np.inf).min(axis=0) if nv else np.zeros(3)    # of the finite coordinates
        origin = np.where(np.isfinite(origin), origin, 0.0)
    origin = np.asarray(origin, dtype=np.float32).reshape(3)
    if not np.isfinite(origin).all():
        raise ValueError("mesh_simplify: the origin must be finite")
    c, bad = cells(verts, origin, cell)
    if bad.any():
        raise ValueError(f"mesh simplify: {int(bad.sum())} vertices have a non-finite coordinate or a cell index outside [0, {CELLS})")
    bad_f = ((faces < 0) | (faces >= nv)).any(axis=1)
    if bad_f.any():
        raise ValueError(f"mesh simplify: {int(bad_f.sum())} faces have a vertex index outside [0, {nv})")
    key = c[:, 0].astype(np.int64) | (c[:, 1].astype(np.int64) << 21) | (c[:, 2].astype(np.int64) << 42)
    _, first, cluster = np.unique(key, return_index=True, return_inverse=True)      # first = the smallest index of each key
    cluster = cluster.reshape(-1)
    rep = first[cluster]                                                            # (V,) representative of every vertex
    count = np.bincount(cluster, minlength=len(first))
    # faces
    tri = rep[faces.astype(np.int64)].reshape(-1, 3)
    flat = (tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2])
    live = np.flatnonzero(~flat)
    keep_f = np.zeros(nf, dtype=bool)
    keep_f[live[first_of_equal_rows(canonical(tri[live]))]] = True
    used = np.zeros(nv, dtype=bool)
    used[tri[keep_f].reshape(-1)] = True                                            # bits at representatives only
    new = np.cumsum(used) - 1
    out_faces = new[tri[keep_f]].astype(np.int32).reshape(-1, 3)
    reps = np.flatnonzero(used)
    # positions
    with np.errstate(all="ignore"):
        lo = origin + c * cell
        t = (verts - lo) / cell
        s = t.astype(np.float64) * QUANTUM
        s = np.where(~(s >= -QMAX), -QMAX, np.where(s > QMAX, QMAX, s))
        q = np.rint(s).astype(np.int64)
        psum = cluster_sums(q, cluster, len(first))
        members = count[cluster[reps]]
        mean = psum[cluster[reps]].astype(np.float64) / (members.astype(np.float64) * QUANTUM)[:, None]
        out_verts = (lo[reps].astype(np.float64) + np.float64(cell) * mean).astype(np.float32)
        out_verts = np.where((members == 1)[:, None], verts[reps], out_verts)
        out_normals = None
        if normals is not None:
            ok = (np.isfinite(normals) & (np.abs(normals) <= NORMAL_MAX)).all(axis=1)
            qn = np.where(ok[:, None], np.rint(np.where(ok[:, None], normals, 0).astype(np.float64) * QUANTUM), 0).astype(np.int64)
            nsum = cluster_sums(qn, cluster, len(first))
            big = nsum[cluster[reps]]
            sf = big.astype(np.float32)
            length = np.sqrt((sf[:, 0] * sf[:, 0] + sf[:, 1] * sf[:, 1]) + sf[:, 2] * sf[:, 2])
            own = (members == 1) | ~big.any(axis=1)
            out_normals = np.where(own[:, None], normals[reps], sf / length[:, None]).astype(np.float32)
    info = dict(vertices=nv, faces=nf, clusters=len(first), vertices_kept=len(reps), faces_kept=int(keep_f.sum()),
                degenerate_faces=int(flat.sum()), duplicate_faces=int(len(live) - keep_f.sum()))
    return (np.ascontiguousarray(out_verts).reshape(-1, 3), out_faces,
            None if out_normals is None else np.ascontiguousarray(out_normals).reshape(-1, 3), info)
