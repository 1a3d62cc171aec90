"""numpy restatement of the mesh-quality kernels (nerfmeshes_amd/csrc/mesh_metrics.hip; the arithmetic contract is in
include/nerfmeshes_hip.h): integer area weights and their prefix sums, the surface sampling rule, the brute-force nearest
neighbour and the fp64 mean.  Every fp32 operation is one numpy fp32 operation in the kernels' order, so the GPU tests
compare bytes."""
import numpy as np

F32 = np.float32


def _cross(verts, faces):
    """(v0, v1, v2, c, |c|) of every face, fp32"""
    verts = np.ascontiguousarray(verts, dtype=F32)
    v0, v1, v2 = (verts[faces[:, k]] for k in range(3))
    e1, e2 = v1 - v0, v2 - v0
    c = np.stack((e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                  e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]), 1)
    with np.errstate(invalid="ignore", over="ignore"):
        length = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    return v0, v1, v2, c, length


def face_weights(verts, faces):
    """-> (areas (F,) f32, cdf (F,) uint64, bad): area = 0.5f |e1 x e2|, 0 when it is not finite or the face has an index
    outside [0, V) (`bad` counts those); weight = trunc(area * 2^(32-e)) with the largest area m = f * 2^e, f in [0.5, 1)."""
    faces = np.asarray(faces).reshape(-1, 3)
    nv = len(verts)
    ok = ((faces >= 0) & (faces < nv)).all(1)
    with np.errstate(invalid="ignore", over="ignore"):
        length = _cross(verts, np.where(ok[:, None], faces, 0))[4]
        areas = F32(0.5) * length
    areas = np.where(ok & (areas < np.inf), areas, F32(0)).astype(F32)
    m = areas.max() if len(areas) else F32(0)
    if m > 0:
        _, e = np.frexp(np.float64(m))
        weights = np.trunc(areas.astype(np.float64) * np.ldexp(1.0, 32 - int(e))).astype(np.uint64)
    else:
        weights = np.zeros(len(areas), np.uint64)
    return areas, np.cumsum(weights, dtype=np.uint64), int((~ok).sum())


def sample_points(u, verts, faces, cdf):
    """-> (points (N,3) f32, face_ids (N,) i32, normals (N,3) f32) for draws u (N,3) in [0, 1)"""
    u = np.ascontiguousarray(u, dtype=F32)
    faces = np.asarray(faces).reshape(-1, 3)
    total = cdf[-1]
    assert total > 0
    t = np.trunc(u[:, 0].astype(np.float64) * np.float64(total)).astype(np.uint64)
    face = np.searchsorted(cdf, t, side="right")                     # the first i with cdf[i] > t
    v0, v1, v2, c, length = _cross(verts, faces[face])
    s = np.sqrt(u[:, 1])
    w0, w1, w2 = F32(1) - s, s * (F32(1) - u[:, 2]), s * u[:, 2]
    points = (w0[:, None] * v0 + w1[:, None] * v1) + w2[:, None] * v2
    return points.astype(F32), face.astype(np.int32), (c / length[:, None]).astype(F32)


def nearest(x, y, rows=256):
    """-> (dist2 (N,) f32, index (N,) i32): min over j of ((dx dx + dy dy) + dz dz), the first j that attains it; a NaN pair
    never wins, a row without a winner gets (+inf, -1)"""
    x, y = np.ascontiguousarray(x, dtype=F32).reshape(-1, 3), np.ascontiguousarray(y, dtype=F32).reshape(-1, 3)
    n, m = len(x), len(y)
    dist2, index = np.full(n, np.inf, F32), np.full(n, -1, np.int32)
    if m == 0:
        return dist2, index
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, n, rows):
            q = x[lo:lo + rows]
            dx, dy, dz = (q[:, None, k] - y[None, :, k] for k in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            valid = ~np.isnan(d2)
            best = np.where(valid, d2, np.inf).min(1)
            wins = valid & (d2 == best[:, None])
            any_win = wins.any(1)
            dist2[lo:lo + rows] = np.where(any_win, best, np.inf)
            index[lo:lo + rows] = np.where(any_win, wins.argmax(1), -1)
    return dist2, index


def mean64(dist2):
    return float(np.asarray(dist2).astype(np.float64).sum() / len(dist2))


def chamfer(x, y):
    dx, dy = nearest(x, y)[0], nearest(y, x)[0]
    return dict(chamfer=mean64(dx) + mean64(dy), x_to_y=mean64(dx), y_to_x=mean64(dy), dist2_x=dx, dist2_y=dy)


def uv_sphere(nu=64, nv=32, radius=1.0):
    """nu x nv quads of a latitude / longitude sphere, each split into two triangles: 2 nu nv faces, of which the 2 nu that
    touch a pole with two corners are degenerate (area exactly 0: two of their corners are the same point)."""
    theta = (np.arange(nv + 1, dtype=np.float64) / nv) * np.pi
    phi = (np.arange(nu, dtype=np.float64) / nu) * 2 * np.pi
    st, ct = np.sin(theta), np.cos(theta)
    st[0] = st[-1] = 0.0                                             # the poles are single points
    verts = np.stack((np.outer(st, np.cos(phi)), np.outer(st, np.sin(phi)), np.outer(ct, np.ones(nu))), -1).reshape(-1, 3)
    faces = []
    for i in range(nv):
        for j in range(nu):
            a, b = i * nu + j, i * nu + (j + 1) % nu
            c, d = a + nu, b + nu
            faces += [(a, c, d), (a, d, b)]
    return (radius * verts).astype(F32), np.asarray(faces, np.int32)
