"""numpy restatement of the exact point-to-mesh distance (nm_points_to_mesh in nerfmeshes_amd/csrc/mesh_metrics.hip; the
arithmetic contract is in include/nerfmeshes_hip.h, "Point to mesh") and of the reductions hip_ops.mesh_surface_distance
builds on it.  Every fp32 operation of the kernel is one numpy fp32 operation in the kernel's order, so the GPU tests compare
bytes.  `ericson` is an independent fp64 closest-point routine (Ericson, Real-Time Collision Detection, 5.1.5), the accuracy
yardstick of the CPU tests only."""
import numpy as np

from tests import mesh_metrics as MM

F32 = np.float32

# |sqrt(d2_fp32) - d_fp64 (Ericson)| relative to the mesh's largest absolute coordinate, 2000 uniform queries in 1.5 x the
# mesh's box, measured on the CPU: uv_sphere(32, 16) 1.38e-7, soup of 500 faces 6.7e-8, the soup scaled by 1e-3 5.1e-8, by
# 1e3 4.2e-8 (the form is scale-free up to rounding).  The bound is 4 x the largest of them.
ERICSON_BOUND = 4 * 1.4e-7
# samples of uv_sphere(32, 16) (2000 draws, MM.sample_points) against the mesh they were drawn from: the largest distance is
# 1.12e-7 (mean 2.6e-8), the winning face is the face drawn in every case, |dot| of the two normals >= 1 - 2.4e-7.
ON_SURFACE_BOUND = 4 * 1.2e-7


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(u, v):
    return np.stack((u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1],
                     u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]), -1)


def _seg(q, e, r):
    t = _dot(q, e) * r
    t = np.fmin(np.fmax(t, F32(0)), F32(1))                          # fmax / fmin: the non-NaN operand
    d = q - t[..., None] * e
    return _dot(d, d)


def pair_dist2(x, verts, faces, dtype=F32):
    """(N, F) squared distances by the contract in `dtype`; NaN for a pair with a NaN segment term and for every pair of a
    face with an index outside [0, V)"""
    one, zero = dtype(1), dtype(0)
    x = np.ascontiguousarray(x, dtype=dtype).reshape(-1, 3)
    verts = np.ascontiguousarray(verts, dtype=dtype).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < len(verts))).all(1)
    safe = np.where(ok[:, None], faces, 0)
    with np.errstate(all="ignore"):
        if len(verts) == 0:
            return np.full((len(x), len(faces)), np.nan, dtype)
        a, b, c = (verts[safe[:, k]] for k in range(3))
        ab, ac, bc, ca = b - a, c - a, c - b, a - c
        n = _cross(ab, ac)
        nn = _dot(n, n)
        rab, rbc, rca, rnn = one / _dot(ab, ab), one / _dot(bc, bc), one / _dot(ca, ca), one / nn
        p = x[:, None, :]
        ap, bp, cp = p - a[None], p - b[None], p - c[None]
        s1, s2, s3 = _seg(ap, ab[None], rab[None]), _seg(bp, bc[None], rbc[None]), _seg(cp, ca[None], rca[None])
        inside = ((_dot(n[None], _cross(ab[None], ap)) >= zero) & (_dot(n[None], _cross(bc[None], bp)) >= zero)
                  & (_dot(n[None], _cross(ca[None], cp)) >= zero) & (nn > zero)[None])
        h = _dot(n[None], ap)
        pl = (h * h) * rnn[None]
        pl = np.where(inside & (pl < np.inf), pl, dtype(np.inf))
        d2 = np.minimum(np.minimum(s1, s2), np.minimum(s3, pl))      # np.minimum hands a NaN on
        d2[:, ~ok] = np.nan
    return d2.astype(dtype)


def points_to_mesh(x, verts, faces, rows=256):
    """-> (dist2 (N,) f32, face (N,) i32, normals (N,3) f32): the smallest d2, the first face that attains it, that face's
    c / |c|; a NaN pair never wins, a row without a winner gets (+inf, -1, NaN)"""
    x = np.ascontiguousarray(x, dtype=F32).reshape(-1, 3)
    verts = np.ascontiguousarray(verts, dtype=F32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    n = len(x)
    dist2, face = np.full(n, np.inf, F32), np.full(n, -1, np.int32)
    if len(faces):
        for lo in range(0, n, rows):
            d2 = pair_dist2(x[lo:lo + rows], verts, faces)
            valid = ~np.isnan(d2)
            best = np.where(valid, d2, np.inf).min(1)
            wins = valid & (d2 == best[:, None])
            any_win = wins.any(1)
            dist2[lo:lo + rows] = np.where(any_win, best, np.inf)
            face[lo:lo + rows] = np.where(any_win, wins.argmax(1), -1)
    normals = np.full((n, 3), np.nan, F32)
    won = face >= 0
    if won.any():
        with np.errstate(all="ignore"):
            c, length = MM._cross(verts, faces[face[won]])[3:]
            normals[won] = c / length[:, None]
    return dist2, face, normals


def metrics(dist2_x, dist2_y, normals_x, face_normals_x, normals_y, face_normals_y, thresholds=()):
    """hip_ops.surface_metrics on host arrays"""
    out, roots = {}, {}
    for side, d2 in (("x_to_y", dist2_x), ("y_to_x", dist2_y)):
        d2 = np.asarray(d2).astype(np.float64)
        roots[side] = np.sqrt(d2)
        out[side] = float(d2.sum()) / len(d2)
    out["chamfer"] = out["x_to_y"] + out["y_to_x"]
    out["accuracy"] = float(roots["x_to_y"].sum()) / len(roots["x_to_y"])
    out["completeness"] = float(roots["y_to_x"].sum()) / len(roots["y_to_x"])
    for side in ("x_to_y", "y_to_x"):
        out["hausdorff_" + side] = float(roots[side].max())
    out["hausdorff"] = max(out["hausdorff_x_to_y"], out["hausdorff_y_to_x"])
    for side, a, b in (("x_to_y", normals_x, face_normals_x), ("y_to_x", normals_y, face_normals_y)):
        a, b = np.asarray(a, F32), np.asarray(b, F32)
        with np.errstate(all="ignore"):
            dot = _dot(a, b)
        ok = np.isfinite(a).all(1) & np.isfinite(b).all(1)
        out["normal_pairs_" + side] = int(ok.sum())
        out["normal_consistency_" + side] = float(np.abs(dot[ok].astype(np.float64)).sum()) / int(ok.sum()) if ok.any() else float("nan")
    out["normal_consistency"] = 0.5 * (out["normal_consistency_x_to_y"] + out["normal_consistency_y_to_x"])
    out["fscore"] = []
    for tau in thresholds:
        tau = float(tau)
        p, r = (int((np.asarray(d2).astype(np.float64) <= tau * tau).sum()) / len(d2) for d2 in (dist2_x, dist2_y))
        out["fscore"].append(dict(threshold=tau, precision=p, recall=r, fscore=2 * p * r / (p + r) if p + r > 0 else 0.0))
    return out


def ericson(x, verts, faces, rows=256):
    """fp64 distance (not squared) of every row of x to the mesh by Ericson's region algorithm; faces whose closest point is
    not a number (degenerate ones can divide 0 by 0) are left out of the minimum"""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    verts = np.asarray(verts, np.float64)
    a, b, c = (verts[np.asarray(faces)[:, k]][None] for k in range(3))
    ab, ac = b - a, c - a
    out = np.empty(len(x))
    dot = lambda u, v: (u * v).sum(-1)                               # noqa: E731
    with np.errstate(all="ignore"):
        for lo in range(0, len(x), rows):
            p = x[lo:lo + rows, None, :]
            ap, bp, cp = p - a, p - b, p - c
            d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
            vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
            denom = 1.0 / (va + vb + vc)
            conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                     (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
            e = lambda t: t[..., None]                               # noqa: E731
            picks = [a + 0 * p, b + 0 * p, a + e(d1 / (d1 - d3)) * ab, c + 0 * p, a + e(d2 / (d2 - d6)) * ac,
                     b + e((d4 - d3) / ((d4 - d3) + (d5 - d6))) * (c - b)]
            closest = a + ab * e(vb * denom) + ac * e(vc * denom)
            for cond, pick in reversed(list(zip(conds, picks))):     # the first condition that holds decides
                closest = np.where(e(cond), pick, closest)
            d = np.sqrt(dot(p - closest, p - closest))
            out[lo:lo + rows] = np.nanmin(d, 1)
    return out


def soup(faces, seed, scale=1.0):
    """`faces` random triangles with their own three vertices each"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-1, 1, (faces, 1, 3))
    verts = (centres + rng.normal(0, 0.3, (faces, 3, 3))) * scale
    return verts.reshape(-1, 3).astype(F32), np.arange(3 * faces, dtype=np.int32).reshape(-1, 3)
