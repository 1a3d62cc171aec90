"""Adaptive levels of mesh simplification restated in numpy (include/nerfmeshes_hip.h, "ADAPTIVE LEVELS"): what
nm_mesh_simplify_adaptive_level / _faces / _emit must give, bit for bit.  Cells, clusters, faces and numbering are
tests/mesh_simplify.py's, lattice, quadric and place tests/mesh_simplify_quadric.py's, each run per level on the grid
(origin, cell * 2^l); the sums are int64 sums, every fp64 operation is a numpy float64 operation (rounded on its own), in the
header's order.

  level     l = 0 .. L: the grid of cell_l = float32(cell) * 2^l (exact), the same origin; c_l = c_0 >> l per axis
  error     of a SOLVED cluster of n >= 2: the maximum over its contributing corners with nrm != 0, with x = frac * 2^8, of
            d2 = ((n0 (x0 - u0_0) + n1 (x1 - u0_1)) + n2 (x2 - u0_2))^2 / ((n0 n0 + n1 n1) + n2 n2)
  accept    l >= 1: one member, or SOLVED and no FAR corner and error <= tol_l^2, tol_l = (E / float64(cell_l)) * 2^8; l = 0: always
  choice    every vertex joins the cluster of the largest l whose cell is acceptable
  output    faces through the final representatives (MS's rules); a chosen cluster's rows are its level's
"""
import math

import numpy as np

from tests import mesh_simplify as MS
from tests import mesh_simplify_quadric as MQ

MAX_LEVELS = 8
LEVEL_KEYS = ("level_vertices", "level_clusters", "refused_error", "refused_crowded", "refused_singular", "refused_far",
              "refused_empty")
ADAPTIVE_KEYS = ("levels",) + LEVEL_KEYS + ("level_kept", "largest_error")
INFO_KEYS = MQ.INFO_KEYS + ADAPTIVE_KEYS


def level_cell(cell, level):
    """the cell edge of a level, float32: the multiplication by a power of two is exact"""
    return np.float32(cell) * np.float32(2.0 ** level)


def tolerance2(max_error, cell_l):
    """tol_l^2 in squared lattice units of the level's cell: three fp64 operations"""
    with np.errstate(all="ignore"):
        in_cells = np.float64(max_error) / np.float64(cell_l)
        tol = in_cells * np.float64(MQ.LATTICE)
        return tol * tol


def corner_planes(faces, C, u):
    """-> (nrm (F,3,3) int64: e1 x e2 of every corner, zeros where far; far (F,3) bool): MQ.corner_terms' geometry"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nrm = np.zeros((len(f), 3, 3), dtype=np.int64)
    far = np.zeros((len(f), 3), dtype=bool)
    for k in range(3):
        v0, v1, v2 = f[:, k], f[:, (k + 1) % 3], f[:, (k + 2) % 3]
        e1 = (C[v1] - C[v0]) * MQ.LATTICE + (u[v1] - u[v0])
        e2 = (C[v2] - C[v0]) * MQ.LATTICE + (u[v2] - u[v0])
        far[:, k] = (np.abs(e1) > MQ.REACH).any(axis=1) | (np.abs(e2) > MQ.REACH).any(axis=1)
        e1, e2 = np.where(far[:, k, None], 0, e1), np.where(far[:, k, None], 0, e2)
        nrm[:, k] = np.stack((e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                              e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]), 1)
    return nrm, far


def corner_d2(nrm, u0, x):
    """d2 of corners: nrm (N,3) int64 (not zero), u0 (N,3) int64, x (N,3) float64 -> (N,) float64, in the header's order"""
    n = nrm.astype(np.float64)
    w = u0.astype(np.float64)
    with np.errstate(all="ignore"):
        p0, p1, p2 = n[:, 0] * (x[:, 0] - w[:, 0]), n[:, 1] * (x[:, 1] - w[:, 1]), n[:, 2] * (x[:, 2] - w[:, 2])
        s = (p0 + p1) + p2
        den = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        return (s * s) / den


def level_clusters(verts, faces, normals, origin, cell_l):
    """Everything of ONE level, per cluster k of its K clusters (by ascending packed cell): a dict of
    cluster (V,) the cluster of every vertex; first (K,) representatives; count (K,); status (K,) MQ's, 0 for one member;
    frac (K,3) float64 the placed point in units of the cell (the mean where not SOLVED); error (K,) float64 the largest d2
    (0 where not SOLVED); far (K,) bool: a corner of the cluster was far; far_corners; pos (K,3) float32, nrm (K,3) float32 or None:
    the rows the cluster emits"""
    C, u, q = MQ.lattice(verts, origin, cell_l)
    key = C[:, 0] | (C[:, 1] << 21) | (C[:, 2] << 42)
    _, first, cluster = np.unique(key, return_index=True, return_inverse=True)
    cluster = cluster.reshape(-1)
    K = len(first)
    count = np.bincount(cluster, minlength=K)
    sums, contributions, far_corners = MQ.quadric_sums(faces, cluster, K, C, u)
    f = faces.astype(np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        psum = MS.cluster_sums(q, cluster, K)
        mean = psum.astype(np.float64) / (count.astype(np.float64) * MS.QUANTUM)[:, None]
        frac, status = MQ.place(mean, sums, contributions)
        status = np.where(count >= 2, status, 0)
        solved = (status & MQ.SOLVED) != 0
        # the error and the far marks, corner by corner
        nrm, far = corner_planes(f, C, u)
        where = cluster[f]                                           # (F,3): the cluster of every corner
        far_mark = np.zeros(K, dtype=bool)
        far_mark[where[far]] = True
        use = ~far & nrm.any(axis=2) & solved[where]
        d2 = corner_d2(nrm[use], u[f][use], frac[where[use]] * np.float64(MQ.LATTICE))
        error = np.zeros(K, dtype=np.float64)
        if len(d2):                                                  # the maximum per cluster: sorted runs (ufunc.at is slow)
            rows = where[use]
            order = np.argsort(rows, kind="stable")
            present, starts = np.unique(rows[order], return_index=True)
            error[present] = np.maximum.reduceat(d2[order], starts)
        # the rows
        c32, _ = MS.cells(verts[first], origin, cell_l)
        lo = origin + c32 * cell_l
        pos = (lo.astype(np.float64) + np.float64(cell_l) * frac).astype(np.float32)
        pos = np.where((count == 1)[:, None], verts[first], pos)
        nrm_rows = None
        if normals is not None:
            ok = (np.isfinite(normals) & (np.abs(normals) <= MS.NORMAL_MAX)).all(axis=1)
            qn = np.where(ok[:, None], np.rint(np.where(ok[:, None], normals, 0).astype(np.float64) * MS.QUANTUM), 0).astype(np.int64)
            big = MS.cluster_sums(qn, cluster, K)
            sf = big.astype(np.float32)
            length = np.sqrt((sf[:, 0] * sf[:, 0] + sf[:, 1] * sf[:, 1]) + sf[:, 2] * sf[:, 2])
            own = (count == 1) | ~big.any(axis=1)
            nrm_rows = np.where(own[:, None], normals[first], sf / length[:, None]).astype(np.float32)
    return dict(cluster=cluster, first=first, count=count, status=status, frac=frac, error=error, far=far_mark,
                far_corners=far_corners, pos=pos, nrm=nrm_rows, C=C, u=u)


def acceptable(data, tol2, level):
    """(K,) bool: the header's `accept`"""
    if level == 0:
        return np.ones(len(data["first"]), dtype=bool)
    solved = (data["status"] & MQ.SOLVED) != 0
    return (data["count"] == 1) | (solved & ~data["far"] & (data["error"] <= tol2))


def simplify(verts, faces, normals=None, cell=1.0, origin=None, placement="quadric", levels=0, max_error=None, details=False,
             cache=None):
    """-> (verts, faces, normals, info), as hip_ops.mesh_simplify(..., placement=placement, levels=levels, max_error=max_error);
    details: a fifth value, dict(level (V,), rep (V,), reps, data: level_clusters per level, tol2 per level).
    cache: a dict the caller keeps for ONE mesh and origin: a level's clusters depend on neither `levels` nor `max_error`, so
    the calls of a test matrix share them, keyed by the level's cell size (without details)"""
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 0 <= levels <= MAX_LEVELS:
        raise ValueError(f"mesh_simplify: levels must be an integer in [0, {MAX_LEVELS}], got {levels!r}")
    if levels == 0:
        return MQ.simplify(verts, faces, normals, cell=cell, origin=origin, placement=placement)
    if placement != "quadric":
        raise ValueError(f"mesh_simplify: levels = {levels} needs placement='quadric', got {placement!r}")
    if max_error is None:
        raise ValueError("mesh_simplify: max_error is required with levels > 0")
    max_error = float(max_error)
    if not max_error >= 0.0:
        raise ValueError(f"mesh_simplify: max_error must be >= 0, got {max_error}")
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    if normals is not None:
        normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    nv, nf = len(verts), len(faces)
    if not (np.isfinite(np.float32(cell)) and np.float32(cell) > 0) or (origin is not None and not np.isfinite(np.float32(origin)).all()) \
            or MS.cells(verts, MQ.grid(verts, cell, origin)[0], cell)[1].any() or ((faces < 0) | (faces >= nv)).any():
        MS.simplify(verts, faces, normals, cell=cell, origin=origin)  # raises for bad input, in its words
    origin, cell = MQ.grid(verts, cell, origin)
    assert not (details and cache is not None)
    level_of = np.full(nv, -1, dtype=np.int64)
    rep = np.full(nv, -1, dtype=np.int64)
    pos = np.zeros((nv, 3), dtype=np.float32)
    nrm = np.zeros((nv, 3), dtype=np.float32)
    status = np.zeros(nv, dtype=np.int64)
    rows = {name: [0] * (levels + 1) for name in LEVEL_KEYS}
    largest, datas, tols, far_corners = 0.0, {}, {}, 0
    everyone = np.arange(nv)
    for level in range(levels, -1, -1):
        cell_l = level_cell(cell, level)
        data = None if cache is None else cache.get(float(cell_l))
        if data is None:
            data = level_clusters(verts, faces, normals, origin, cell_l)
            if cache is not None:
                cache[float(cell_l)] = data = {k: x for k, x in data.items() if k not in ("C", "u")}
        tol2 = tolerance2(max_error, cell_l)
        datas[level], tols[level] = data, tol2
        ok = acceptable(data, tol2, level)
        cluster, first = data["cluster"], data["first"]
        free = level_of < 0
        take = free & ok[cluster]
        heads = first[cluster] == everyone
        rep[take] = first[cluster][take]
        level_of[take] = level
        chosen = cluster[take & heads]                               # the clusters this level keeps
        pos[first[chosen]] = data["pos"][chosen]
        if normals is not None:
            nrm[first[chosen]] = data["nrm"][chosen]
        status[first[chosen]] = data["status"][chosen]
        refused = cluster[free & ~ok[cluster] & heads]
        st = data["status"][refused]
        solved = (st & MQ.SOLVED) != 0
        rows["level_vertices"][level] = int(take.sum())
        rows["level_clusters"][level] = len(chosen)
        rows["refused_crowded"][level] = int(((st & MQ.CROWDED) != 0).sum())
        rows["refused_empty"][level] = int((st == 0).sum())
        rows["refused_singular"][level] = int(((st & MQ.SINGULAR) != 0).sum())
        rows["refused_far"][level] = int((solved & data["far"][refused]).sum())
        rows["refused_error"][level] = int((solved & ~data["far"][refused]).sum())
        if level == 0:
            far_corners = data["far_corners"]
        else:
            big = chosen[data["count"][chosen] >= 2]
            d2 = float(data["error"][big].max()) if len(big) else 0.0
            largest = max(largest, math.sqrt(d2) / 256.0 * (float(cell) * 2.0 ** level))
    assert (level_of >= 0).all()
    # faces through the final representatives: MS.simplify's rules
    tri = rep[faces.astype(np.int64)].reshape(-1, 3)
    flat = (tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2])
    live = np.flatnonzero(~flat)
    keep_f = np.zeros(nf, dtype=bool)
    keep_f[live[MS.first_of_equal_rows(MS.canonical(tri[live]))]] = True
    used = np.zeros(nv, dtype=bool)
    used[tri[keep_f].reshape(-1)] = True
    new = np.cumsum(used) - 1
    out_faces = new[tri[keep_f]].astype(np.int32).reshape(-1, 3)
    reps = np.flatnonzero(used)
    kept_status = status[reps]
    info = dict(vertices=nv, faces=nf, clusters=int(sum(rows["level_clusters"])), vertices_kept=len(reps),
                faces_kept=int(keep_f.sum()), degenerate_faces=int(flat.sum()), duplicate_faces=int(len(live) - keep_f.sum()),
                quadric_clusters=int(((kept_status & MQ.SOLVED) != 0).sum()), crowded_clusters=int(((kept_status & MQ.CROWDED) != 0).sum()),
                singular_clusters=int(((kept_status & MQ.SINGULAR) != 0).sum()),
                clamped_clusters=int(((kept_status & MQ.CLAMPED) != 0).sum()), far_corners=far_corners, levels=levels)
    info.update((name, tuple(rows[name])) for name in LEVEL_KEYS)
    info["level_kept"] = tuple(int((level_of[reps] == l).sum()) for l in range(levels + 1))
    info["largest_error"] = largest
    out = (np.ascontiguousarray(pos[reps]).reshape(-1, 3), out_faces,
           None if normals is None else np.ascontiguousarray(nrm[reps]).reshape(-1, 3), info)
    return out + (dict(level=level_of, rep=rep, reps=reps, data=datas, tol2=tols),) if details else out
