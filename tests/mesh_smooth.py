"""Taubin smoothing restated in numpy (the role tests/mesh_simplify.py plays for its kernels): what nm_mesh_smooth_build / _run
and nm_mesh_vertex_normals must give, bit for bit.  Every fp32 / fp64 operation is a numpy operation of that type (rounded on
its own), the sums are int64 sums.

  validity    a vertex with a non-finite coordinate is bad, a face with an index outside [0, V) is bad: either raises
              ValueError, as hip_ops.mesh_smooth does.  A face with two equal corners is degenerate: no edge
  edges       the three undirected edges (min, max) of every other face, each ONCE (np.unique): a neighbour counts once
              however many faces share the edge.  On exactly one face: a boundary edge, its ends boundary vertices (pinned
              unless free_boundary); on more than two: non-manifold, not boundary.  A vertex on no edge is isolated
  half-step   e = frexp's exponent of the largest |coordinate| of the input, shift = 40 - e;
              q = int64(rint(ldexp(float64(x), shift))) clamped to [-2^43, 2^43]; hi = sum q >> 20, lo = sum q & 0xFFFFF over the
              neighbours; m = ldexp((float64(hi) * 2^20 + float64(lo)) / float64(degree), -shift);
              x' = float32(float64(x) + float64(f) * (m - float64(x))); pinned and isolated vertices keep their bits
  iteration   a half-step with lam, then one with mu (none when mu = 0: plain Laplacian smoothing)
  normals     per non-degenerate face the fp32 unit normal of cross(b - a, c - a) times flip, skipped when its length is zero
              or not finite; q = int64(rint(float64(n) * 2^30)) added to the three corners; s = float32(S);
              s / sqrt((sx sx + sy sy) + sz sz); S = 0: the input normal, or zero
"""
import numpy as np

BITS = 40
QMAX = float(1 << 43)
SPLIT = float(1 << 20)
QUANTUM = float(1 << 30)
INFO_KEYS = ("vertices", "faces", "edges", "boundary_edges", "nonmanifold_edges", "boundary_vertices", "isolated_vertices",
             "degenerate_faces", "exponent")


def degenerate(faces):
    return (faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])


def adjacency(verts, faces):
    """-> dict(a, b: the ends of the unique edges (a < b); count: faces per edge; degree (V,); boundary (V,) bool;
    src, dst: both directions of every edge sorted by src; starts: the first entry of every vertex of degree > 0; info)"""
    nv = len(verts)
    bad = ~np.isfinite(verts).all(axis=1)
    if bad.any():
        raise ValueError(f"mesh smooth: {int(bad.sum())} vertices have a non-finite coordinate")
    bad_f = ((faces < 0) | (faces >= nv)).any(axis=1)
    if bad_f.any():
        raise ValueError(f"mesh smooth: {int(bad_f.sum())} faces have a vertex index outside [0, {nv})")
    flat = degenerate(faces)
    live = faces[~flat].astype(np.int64)
    ends = np.concatenate((live[:, [0, 1]], live[:, [1, 2]], live[:, [2, 0]]))
    key, count = np.unique((ends.min(axis=1) << 32) | ends.max(axis=1), return_counts=True)
    a, b = key >> 32, key & 0xFFFFFFFF
    degree = np.bincount(a, minlength=nv) + np.bincount(b, minlength=nv)
    boundary = np.zeros(nv, dtype=bool)
    boundary[a[count == 1]] = True
    boundary[b[count == 1]] = True
    src, dst = np.concatenate((a, b)), np.concatenate((b, a))
    order = np.argsort(src, kind="stable")
    src, dst = src[order], dst[order]
    starts = (np.cumsum(degree) - degree)[degree > 0]
    largest = np.abs(verts).max() if verts.size else np.float32(0)
    info = dict(vertices=nv, faces=len(faces), edges=len(key), boundary_edges=int((count == 1).sum()),
                nonmanifold_edges=int((count > 2).sum()), boundary_vertices=int(boundary.sum()),
                isolated_vertices=int((degree == 0).sum()), degenerate_faces=int(flat.sum()), exponent=int(np.frexp(largest)[1]))
    return dict(a=a, b=b, count=count, degree=degree, boundary=boundary, src=src, dst=dst, starts=starts, largest=largest, info=info)


def half_step(x, adj, movable, shift, f):
    """one half-step with the fp32 factor f -> the new (V,3) float32 positions"""
    with np.errstate(all="ignore"):
        s = np.ldexp(x.astype(np.float64), shift)
        s = np.where(~(s >= -QMAX), -QMAX, np.where(s > QMAX, QMAX, s))
        q = np.rint(s).astype(np.int64)[adj["dst"]]
        some = adj["degree"] > 0
        hi, lo = np.zeros((len(x), 3), np.int64), np.zeros((len(x), 3), np.int64)
        if len(q):
            hi[some] = np.add.reduceat(q >> 20, adj["starts"], axis=0)
            lo[some] = np.add.reduceat(q & 0xFFFFF, adj["starts"], axis=0)
        total = hi.astype(np.float64) * SPLIT + lo.astype(np.float64)
        mean = np.ldexp(total / adj["degree"].astype(np.float64)[:, None], -shift)
        own = x.astype(np.float64)
        moved = (own + np.float64(np.float32(f)) * (mean - own)).astype(np.float32)
    return np.where(movable[:, None], moved, x)


def vertex_normals(verts, faces, normals=None, flip=1):
    """(V,3) float32: the normalised sum of the unit face normals times flip; the input normal (or zero) where the sum is zero"""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    nv = len(verts)
    ok = ~((faces < 0) | (faces >= nv)).any(axis=1) & ~degenerate(faces)
    c = faces[ok].astype(np.int64)
    total = np.zeros((nv, 3), np.int64)
    with np.errstate(all="ignore"):
        u, w = verts[c[:, 1]] - verts[c[:, 0]], verts[c[:, 2]] - verts[c[:, 0]]
        n = np.stack([u[:, (k + 1) % 3] * w[:, (k + 2) % 3] - u[:, (k + 2) % 3] * w[:, (k + 1) % 3] for k in range(3)], axis=1)
        length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        good = np.isfinite(length) & (length > 0)
        unit = (n[good] / length[good, None]) * np.float32(flip)
        q = np.rint(unit.astype(np.float64) * QUANTUM).astype(np.int64)
        for k in range(3):
            order = np.argsort(c[good, k], kind="stable")
            corner = c[good, k][order]
            if len(corner):
                head = np.flatnonzero(np.r_[True, corner[1:] != corner[:-1]])
                total[corner[head]] += np.add.reduceat(q[order], head, axis=0)
        s = total.astype(np.float32)
        length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        own = np.zeros((nv, 3), np.float32) if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        out = np.where(total.any(axis=1)[:, None], s / length[:, None], own).astype(np.float32)
    return np.ascontiguousarray(out).reshape(-1, 3)


def smooth(verts, faces, normals=None, iterations=10, lam=0.5, mu=-0.53, free_boundary=False, flip=None):
    """-> (verts, normals, info), as hip_ops.mesh_smooth (numpy arrays in, numpy arrays out)."""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    iterations, lam, mu = int(iterations), np.float32(lam), np.float32(mu)
    if not 0 <= iterations <= 1000:
        raise ValueError(f"mesh_smooth: iterations must be in [0, 1000], got {iterations}")
    if not 0 < lam <= 1:
        raise ValueError(f"mesh_smooth: lam must be in (0, 1], got {lam}")
    if not -1 <= mu <= 0:
        raise ValueError(f"mesh_smooth: mu must be in [-1, 0], got {mu}")
    if flip not in (None, 1, -1):
        raise ValueError(f"mesh_smooth: flip must be +1 or -1, got {flip}")
    adj = adjacency(verts, faces)
    movable = (adj["degree"] > 0) & (free_boundary | ~adj["boundary"])
    x = verts
    if adj["largest"] > 0:
        shift = BITS - adj["info"]["exponent"]
        for _ in range(iterations):
            x = half_step(x, adj, movable, shift, lam)
            if mu != 0:
                x = half_step(x, adj, movable, shift, mu)
    out_normals = None
    if normals is not None or flip is not None:
        out_normals = vertex_normals(x, faces, normals, 1 if flip is None else flip)
    return np.ascontiguousarray(x).reshape(-1, 3).copy(), out_normals, adj["info"]
