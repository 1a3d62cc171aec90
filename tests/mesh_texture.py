"""numpy restatement of the texture atlas (nerfmeshes_amd/csrc/mesh_texture.hip; written from the rule in
include/nerfmeshes_hip.h, "Texture atlas of a mesh"): the layout in integers, the samples, the fill, the coordinates and the
bilinear fetch, every fp32 operation rounded on its own in the order the rule gives.  The device must reproduce every array
bit for bit."""
import numpy as np

F32, I64 = np.float32, np.int64
MAX_RES, MAX_SIDE = 255, 16384
QNAN = np.array([0x7FC00000], np.uint32).view(F32)[0]


def layout(num_faces, n, limit=MAX_SIDE):
    """-> dict(width, height, cols, rows, samples_per_face); ValueError where the rule refuses (limit=None: the width's limit
    is not applied)"""
    num_faces, n = int(num_faces), int(n)
    if not 1 <= n <= MAX_RES or not 0 <= num_faces < 2 ** 31 - 64:
        raise ValueError("n or the face count is out of range")
    cw, ch, cells = n + 3, n + 2, (num_faces + 1) // 2
    cols = 1
    while cols * cw < -(-cells // cols) * ch:
        cols += 1
    if limit is not None and cols * cw > limit:
        raise ValueError("the atlas would be wider than 16384 texels")
    rows = -(-cells // cols)
    return dict(width=cols * cw, height=rows * ch, cols=cols, rows=rows, samples_per_face=(n + 1) * (n + 2) // 2)


def lattice(n):
    """-> (i, j) of the T lattice points in index order"""
    j, i = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    keep = i + j <= n
    return i[keep].astype(I64), j[keep].astype(I64)


def index(n, i, j):
    return j * (n + 1) - j * (j - 1) // 2 + i


def cell_owner(n):
    """One cell -> (upper (Ch,Cw) bool, i (Ch,Cw), j (Ch,Cw)): which of the cell's two faces owns local texel (a, b) = (column,
    row), and at which lattice point"""
    b, a = np.meshgrid(np.arange(n + 2, dtype=I64), np.arange(n + 3, dtype=I64), indexing="ij")
    lower = a + b <= n + 1
    return ~lower, np.where(lower, a, n + 2 - a), np.where(lower, b, n + 1 - b)


def cell_origin(num_faces, n):
    """-> (x0 (P,), y0 (P,)) of the P = ceil(F / 2) cells"""
    lay = layout(num_faces, n)
    c = np.arange((num_faces + 1) // 2, dtype=I64)
    return (c % lay["cols"]) * (n + 3), (c // lay["cols"]) * (n + 2)


def texel_owner(num_faces, n):
    """Every texel of the atlas -> (face (H,W) int64, -1 where the slot is empty; i (H,W); j (H,W)): the cell, the face and the
    lattice point by the rule's formulas"""
    lay = layout(num_faces, n)
    y, x = np.meshgrid(np.arange(lay["height"], dtype=I64), np.arange(lay["width"], dtype=I64), indexing="ij")
    a, b = x % (n + 3), y % (n + 2)
    cell = (y // (n + 2)) * lay["cols"] + x // (n + 3)
    lower = a + b <= n + 1
    face = 2 * cell + np.where(lower, 0, 1)
    i, j = np.where(lower, a, n + 2 - a), np.where(lower, b, n + 1 - b)
    return np.where(face < num_faces, face, -1), i, j


def corner_texels(num_faces, n):
    """-> (x (F,3), y (F,3)): the texel of every face corner"""
    lay = layout(num_faces, n)
    f = np.arange(num_faces, dtype=I64)[:, None]
    i, j = np.array([[0, n, 0]], I64), np.array([[0, 0, n]], I64)
    cell, lower = f // 2, (f % 2) == 0
    x = (cell % lay["cols"]) * (n + 3) + np.where(lower, i, n + 2 - i)
    y = (cell // lay["cols"]) * (n + 2) + np.where(lower, j, n + 1 - j)
    return x, y


def face_uv(num_faces, n):
    lay = layout(num_faces, n)
    x, y = corner_texels(num_faces, n)
    u = (2 * x + 1).astype(F32) / F32(2 * lay["width"])
    v = (2 * (lay["height"] - y) - 1).astype(F32) / F32(2 * lay["height"])
    return np.stack((u, v), -1).astype(F32)


def _blend(b, rows):
    return (b[0] * rows[0] + b[1] * rows[1]) + b[2] * rows[2]


def _length(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def samples(verts, faces, normals, n, first=0, count=None, flip=1):
    """-> (positions (count*T,3) fp32, directions (count*T,3) fp32, fallback samples, samples of faces with a bad index)"""
    verts = np.asarray(verts, F32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3).astype(I64)
    count = len(faces) - first if count is None else count
    window = faces[first:first + count]
    i, j = lattice(n)
    per_face, nv = len(i), len(verts)
    fn = F32(n)
    b = [((n - i - j).astype(F32) / fn)[None, :, None], (i.astype(F32) / fn)[None, :, None], (j.astype(F32) / fn)[None, :, None]]
    good = ((window >= 0) & (window < nv)).all(axis=1)
    safe = np.where(good[:, None], window, 0)
    with np.errstate(all="ignore"):
        corners = [verts[safe[:, k]][:, None, :] for k in range(3)] if nv else [np.zeros((count, 1, 3), F32)] * 3
        pos = _blend(b, corners).astype(F32)
        pos = np.where(np.isnan(pos), QNAN, pos)
        direction = np.zeros_like(pos)
        have = np.zeros((count, per_face), bool)
        if normals is not None:
            normals = np.asarray(normals, F32).reshape(-1, 3)
            m = _blend(b, [normals[safe[:, k]][:, None, :] for k in range(3)]).astype(F32)
            length = _length(m)
            have = (length > 0) & np.isfinite(length)
            direction = np.where(have[..., None], -(m / np.where(have, length, F32(1))[..., None]), direction)
        e1, e2 = corners[1] - corners[0], corners[2] - corners[0]
        g = np.stack([e1[..., (a + 1) % 3] * e2[..., (a + 2) % 3] - e1[..., (a + 2) % 3] * e2[..., (a + 1) % 3] for a in range(3)], -1)
        glen = _length(g)
        gok = (glen > 0) & np.isfinite(glen)
        geometric = np.where(gok[..., None], (g / np.where(gok, glen, F32(1))[..., None]) * F32(-flip), np.array([0, 0, -1], F32))
        direction = np.where(have[..., None], direction, np.broadcast_to(geometric, direction.shape))
    pos = np.where(good[:, None, None], pos, F32(0)).astype(F32)
    direction = np.where(good[:, None, None], direction, F32(0)).astype(F32)
    fallback = int((~have & good[:, None]).sum())
    return pos.reshape(-1, 3), direction.reshape(-1, 3), fallback, int((~good).sum()) * per_face


def quantise(c):
    with np.errstate(all="ignore"):
        t = np.minimum(np.maximum(np.where(np.isnan(c), F32(0), c), F32(0)), F32(1)) * F32(255) + F32(0.5)
    return t.astype(np.uint8)


def fill_float(colors, num_faces, n):
    """the atlas before quantisation (H,W,3) fp32; an empty slot is 0"""
    colors = np.asarray(colors, F32).reshape(num_faces, -1, 3)
    face, i, j = texel_owner(num_faces, n)
    used = face >= 0
    out = np.zeros(face.shape + (3,), F32)
    fi, ii, jj = face[used], i[used], j[used]
    inside = ii + jj <= n
    at = lambda a, b: colors[fi, index(n, np.clip(a, 0, n), np.clip(b, 0, n))]          # noqa: E731
    with np.errstate(all="ignore"):
        inner = (at(ii - 1, jj) + at(ii, jj - 1)) - at(ii - 1, jj - 1)
    edge = np.where((ii == 0)[:, None], at(0 * ii, 0 * jj + n), at(0 * ii + n, 0 * jj))
    plain = at(np.where(inside, ii, 0), np.where(inside, jj, 0))
    out[used] = np.where(inside[:, None], plain, np.where(((ii >= 1) & (jj >= 1))[:, None], inner, edge))
    return out


def fill(colors, num_faces, n):
    """colors (F*T,3) fp32 -> the atlas (H,W,3) uint8"""
    face, _, _ = texel_owner(num_faces, n)
    return np.where((face >= 0)[..., None], quantise(fill_float(colors, num_faces, n)), np.uint8(0)).astype(np.uint8)


def bilinear(texture, u, v):
    """the rule's fetch of a (Ht,Wt,3) image of fp32 texel VALUES at fp32 coordinates u, v (any shape) -> (..., 3) fp32"""
    th, tw = texture.shape[:2]
    u, v = np.asarray(u, F32), np.asarray(v, F32)
    with np.errstate(all="ignore"):
        tx = np.minimum(np.maximum(u * F32(tw) - F32(0.5), F32(0)), F32(tw - 1))
        ty = np.minimum(np.maximum((F32(1) - v) * F32(th) - F32(0.5), F32(0)), F32(th - 1))
    tx, ty = np.where(np.isfinite(tx), tx, F32(0)), np.where(np.isfinite(ty), ty, F32(0))     # a NaN: the caller masks it
    flx, fly = np.floor(tx), np.floor(ty)
    ix0, iy0 = flx.astype(I64), fly.astype(I64)
    ix1, iy1 = np.minimum(ix0 + 1, tw - 1), np.minimum(iy0 + 1, th - 1)
    fx, fy = (tx - flx)[..., None], (ty - fly)[..., None]
    c00, c10, c01, c11 = texture[iy0, ix0], texture[iy0, ix1], texture[iy1, ix0], texture[iy1, ix1]
    top = c00 + fx * (c10 - c00)
    bottom = c01 + fx * (c11 - c01)
    return (top + fy * (bottom - top)).astype(F32)


def texel_values(texture_u8):
    return np.asarray(texture_u8, np.uint8).astype(F32) / F32(255)


def pixel_uv(face_id, bary, uv):
    """-> (u, v, ok): the interpolated coordinates per pixel, ok where the face is one of the mesh and both are finite"""
    uv = np.asarray(uv, F32).reshape(-1, 3, 2)
    flat, b = face_id.reshape(-1).astype(I64), np.asarray(bary, F32).reshape(-1, 3)
    ok = (flat >= 0) & (flat < len(uv))
    rows = uv[np.where(ok, flat, 0)] if len(uv) else np.zeros((len(flat), 3, 2), F32)
    with np.errstate(all="ignore"):
        at = (b[:, 0:1] * rows[:, 0] + b[:, 1:2] * rows[:, 1]) + b[:, 2:3] * rows[:, 2]
    ok &= np.isfinite(at).all(axis=1)
    return at[:, 0], at[:, 1], ok


def lookup(face_id, bary, uv, texture_u8, background, values=None):
    """-> (H,W,3) fp32 (or face_id's shape + (3,)).  values: fetch these fp32 texel values instead of the quantised image's"""
    u, v, ok = pixel_uv(face_id, bary, uv)
    values = texel_values(texture_u8) if values is None else np.asarray(values, F32)
    out = bilinear(values, np.where(ok, u, F32(0)), np.where(ok, v, F32(0)))
    out = np.where(ok[:, None], out, np.asarray(background, F32)[None, :]).astype(F32)
    return out.reshape(*face_id.shape, 3)
