"""CPU: the texture atlas as tests/mesh_texture.py restates it (the rule in include/nerfmeshes_hip.h, "Texture atlas of a
mesh") -- the layout's bookkeeping against the native nm_mesh_texture_layout, the gutter's filter identity, the accuracy of a
textured render of an affine colour, the gain over per-vertex colours that the feature is for --, the textured OBJ through
nm_export_obj_textured and load_obj_textured, the argument errors of the C entries (which return before any HIP call) and the
new options of mesh_nerf and mesh_render."""
import ctypes as C

import numpy as np
import pytest

from nerfmeshes_amd import synthetic as S
from tests import mesh_metrics as MM
from tests import mesh_raster as MR
from tests import mesh_texture as MT
from tests.test_mesh_raster import SPHERE_VIEWS, sheet

F32, F64, I64 = np.float32, np.float64, np.int64
EPS = 2.0 ** -24                                                     # half an fp32 ulp of 1: one rounding's relative error
FACES = (1, 2, 3, 7, 8, 1000, 1001)
RES = (1, 2, 5, 8, 255)


@pytest.fixture(scope="module")
def lib():
    from nerfmeshes_amd import _lib
    return _lib.load()


def native_layout(lib, num_faces, n):
    out = (C.c_int64 * 5)()
    rc = lib.nm_mesh_texture_layout(num_faces, n, out)
    return rc, dict(zip(("width", "height", "cols", "rows", "samples_per_face"), (int(x) for x in out)))


@pytest.mark.parametrize("n", RES)
def test_the_two_faces_tile_a_cell_and_lattice_and_texel_are_a_bijection(n):
    upper, i, j = MT.cell_owner(n)
    per_face = (n + 1) * (n + 2) // 2
    assert upper.shape == (n + 2, n + 3) and 2 * per_face + 2 * (n + 2) == upper.size
    li, lj = MT.lattice(n)
    assert len(li) == per_face and (MT.index(n, li, lj) == np.arange(per_face)).all(), "the sample index counts the lattice in order"
    for face in (False, True):
        own = upper == face
        pi, pj = i[own], j[own]
        assert own.sum() == per_face + n + 2 and (pi >= 0).all() and (pj >= 0).all() and (pi + pj <= n + 1).all()
        assert len(set(zip(pi.tolist(), pj.tolist()))) == own.sum(), "every lattice point and gutter point once: a bijection"
        assert ((pi + pj) == n + 1).sum() == n + 2, "each face owns its own gutter diagonal"
        # the corners sit where the coordinates say: vertex 0 at (0, 0), vertex 1 at (n, 0), vertex 2 at (0, n)
        for k, (ci, cj) in enumerate(((0, 0), (n, 0), (0, n))):
            b, a = np.argwhere(own & (i == ci) & (j == cj))[0]
            assert (a, b) == ((n + 2 - ci, n + 1 - cj) if face else (ci, cj)), k


@pytest.mark.parametrize("n", RES)
@pytest.mark.parametrize("num_faces", FACES)
def test_layout(lib, num_faces, n):
    lay = MT.layout(num_faces, n)
    cw, ch, cells = n + 3, n + 2, (num_faces + 1) // 2
    assert lay["width"] == lay["cols"] * cw and lay["height"] == lay["rows"] * ch and lay["height"] <= lay["width"]
    assert lay["rows"] == -(-cells // lay["cols"]) and lay["cols"] * lay["rows"] >= cells > lay["cols"] * (lay["rows"] - 1)
    for fewer in range(1, lay["cols"]):
        assert fewer * cw < -(-cells // fewer) * ch, "cols is the smallest admissible"
    rc, native = native_layout(lib, num_faces, n)
    assert rc == 0 and native == lay, "the native layout agrees integer for integer"
    # every cell has a place of its own inside the image: with the per-cell tiling above, every texel is owned exactly once
    x0, y0 = MT.cell_origin(num_faces, n)
    assert len(x0) == cells and (x0 % cw == 0).all() and (y0 % ch == 0).all()
    assert x0.max() + cw <= lay["width"] and y0.max() + ch <= lay["height"]
    assert len(np.unique(y0 // ch * lay["cols"] + x0 // cw)) == cells
    cx, cy = MT.corner_texels(num_faces, n)
    upper = (np.arange(num_faces) % 2 == 1)[:, None]
    want_a = np.where(upper, n + 2 - np.array([[0, n, 0]]), np.array([[0, n, 0]]))
    want_b = np.where(upper, n + 1 - np.array([[0, 0, n]]), np.array([[0, 0, n]]))
    assert (cx == x0[np.arange(num_faces) // 2][:, None] + want_a).all() and (cy == y0[np.arange(num_faces) // 2][:, None] + want_b).all()
    if lay["width"] * lay["height"] <= 1 << 20:                      # the whole image, texel by texel
        face, i, j = MT.texel_owner(num_faces, n)
        counts = np.bincount(face[face >= 0], minlength=num_faces)
        assert (counts == lay["samples_per_face"] + n + 2).all()
        assert (face < 0).sum() == lay["width"] * lay["height"] - num_faces * (lay["samples_per_face"] + n + 2)
        key = (face * (n + 2) + i) * (n + 2) + j
        assert len(np.unique(key[face >= 0])) == (face >= 0).sum(), "no lattice point of a face twice"
        assert (face[cy, cx] == np.arange(num_faces)[:, None]).all()
        uv = MT.face_uv(num_faces, n)
        assert uv.dtype == F32 and uv.shape == (num_faces, 3, 2) and (uv > 0).all() and (uv < 1).all()
        assert np.abs(uv[..., 0].astype(F64) * lay["width"] - 0.5 - cx).max() < 1e-3
        assert np.abs((1 - uv[..., 1].astype(F64)) * lay["height"] - 0.5 - cy).max() < 1e-3


@pytest.mark.parametrize("n", RES)
def test_the_first_face_count_that_is_too_wide_is_refused(lib, n):
    lo, hi = 1, 2 ** 31 - 65                                         # the widths grow with F: the first refusal by bisection
    assert MT.layout(lo, n)["width"] <= MT.MAX_SIDE and MT.layout(hi, n, limit=None)["width"] > MT.MAX_SIDE
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if MT.layout(mid, n, limit=None)["width"] > MT.MAX_SIDE:
            hi = mid
        else:
            lo = mid
    assert native_layout(lib, lo, n) == (0, MT.layout(lo, n))
    assert native_layout(lib, lo - 1, n)[0] == 0 and MT.layout(lo, n)["width"] <= MT.MAX_SIDE
    rc, _ = native_layout(lib, hi, n)
    assert rc == 2 and b"wider than 16384" in lib.nm_last_error()
    assert native_layout(lib, hi + 1, n)[0] == 2 and native_layout(lib, 2 ** 31 - 65, n)[0] == 2
    with pytest.raises(ValueError):
        MT.layout(hi, n)


def _linear_colours(num_faces, n, rng):
    """per face and channel c(i, j) = alpha + beta i + gamma j with values in [0.2, 0.8] over the chart AND its gutter"""
    i, j = MT.lattice(n)
    beta = rng.uniform(-0.2, 0.2, (num_faces, 1, 3)) / (n + 1)
    gamma = rng.uniform(-0.2, 0.2, (num_faces, 1, 3)) / (n + 1)
    alpha = rng.uniform(0.4, 0.6, (num_faces, 1, 3))
    colours = alpha + beta * i[None, :, None] + gamma * j[None, :, None]
    return alpha[:, 0], beta[:, 0], gamma[:, 0], colours.astype(F32).reshape(-1, 3)


@pytest.mark.parametrize("n", [1, 2, 5, 8])
@pytest.mark.parametrize("num_faces", [1, 2, 3, 8])
def test_a_bilinear_fetch_in_a_chart_is_linear_interpolation_on_the_lattice(num_faces, n):
    """Before quantisation, for a colour linear in the lattice coordinates, both faces of a cell, the hypotenuse included.
    The bound, with eps = 2^-24 per rounding and W >= H the atlas size: the corner coordinates are one rounding each, their
    blend three products and two sums of positive terms <= 1, so |du| <= 4 eps; tx = u W - 0.5 adds two roundings of values
    <= W: |dtx| <= 6 eps W texels, likewise ty.  The colour moves by (|beta| + |gamma|) per texel, and a fetch within |dtx| of a
    texel border may give a neighbouring texel of any value <= 1 a weight <= |dtx|: 6 eps W (|beta| + |gamma| + 1).  The
    stored colour is one rounding, a gutter value two more, and the three lerps three operations each on values <= 2:
    <= 32 eps in all."""
    rng = np.random.default_rng(100 * num_faces + n)
    alpha, beta, gamma, colours = _linear_colours(num_faces, n, rng)
    values = MT.fill_float(colours, num_faces, n)
    lay = MT.layout(num_faces, n)
    # barycentrics on a dyadic grid: exact in fp32 and summing to exactly 1, the corners, edges and hypotenuse included
    p, q = np.meshgrid(np.arange(0, 1025, 16), np.arange(0, 1025, 16), indexing="ij")
    keep = p + q <= 1024
    p, q = p[keep], q[keep]
    extra = rng.integers(0, 1025, (400, 2))
    extra = extra[extra.sum(1) <= 1024]
    p, q = np.concatenate((p, extra[:, 0], np.arange(1025))), np.concatenate((q, extra[:, 1], 1024 - np.arange(1025)))
    bary = np.stack((1024 - p - q, p, q), -1).astype(F32) / F32(1024)
    assert (bary.astype(F64).sum(-1) == 1).all()
    uv = MT.face_uv(num_faces, n)
    worst = 0.0
    for f in range(num_faces):
        face_id = np.full(len(bary), f, np.int32)
        got = MT.lookup(face_id, bary, uv, None, (0, 0, 0), values=values).astype(F64)
        s, t = n * bary[:, 1].astype(F64), n * bary[:, 2].astype(F64)
        want = alpha[f] + beta[f] * s[:, None] + gamma[f] * t[:, None]
        bound = 6 * EPS * lay["width"] * (np.abs(beta[f]) + np.abs(gamma[f]) + 1).max() + 32 * EPS
        worst = max(worst, np.abs(got - want).max() / bound)
        assert np.abs(got - want).max() <= bound, (f, np.abs(got - want).max(), bound)
    print(f"filter identity F={num_faces} n={n}: worst error / bound = {worst:.3f}")


def affine(p):
    """a colour affine in the position and inside [0.2, 0.8] on [-1, 1]^3"""
    p = np.asarray(p, F64)
    return np.stack((0.5 + 0.1 * p[..., 0] + 0.1 * p[..., 1] - 0.1 * p[..., 2], 0.5 - 0.15 * p[..., 0] + 0.1 * p[..., 2],
                     0.45 + 0.05 * p[..., 0] + 0.2 * p[..., 1] + 0.05 * p[..., 2]), -1)


def bake(verts, faces, normals, n, colour):
    """the restated bake of an analytic colour -> (face_uv, atlas uint8)"""
    positions, _, _, _ = MT.samples(verts, faces, normals, n)
    colours = colour(positions).astype(F32)
    return MT.face_uv(len(faces), n), MT.fill(colours, len(faces), n)


@pytest.fixture(scope="module")
def sphere_rasters():
    """the sphere of the raster tests at its three views, rasterised once"""
    verts, faces = MM.uv_sphere(64, 32)
    return verts, faces, [MR.rasterize(verts, faces, S.pose_spherical(*angles), h, w, focal, 0.1) for angles, h, w, focal in SPHERE_VIEWS]


def _accuracy(verts, faces, raster, n, tag):
    """|textured render - analytic colour at the pixel's surface point| over the covered pixels, against 1 / 255 plus the fp32
    terms: each texel is within 0.5 / 255 of the colour at its lattice point (the gutter is exact for an affine colour: its
    three terms are within the rounding of the stored colours), the fetch is a convex combination of four of them, and an affine
    colour's bilinear interpolant is the colour itself; the coordinates carry |dtx| <= 6 eps W texels (the filter identity's
    derivation) plus (sum of the barycentrics - 1 <= 3 eps) W texels, at a colour step of at most `step` per texel; the surface
    point is three products and two sums (5 eps |p|) through a gradient <= 0.4, and the fetch's own arithmetic is <= 32 eps."""
    uv, atlas = bake(verts, faces, None, n, affine)
    face_id, _, bary, _ = raster
    covered = face_id >= 0
    got = MT.lookup(face_id, bary, uv, atlas, (0, 0, 0))[covered].astype(F64)
    point = MR.interpolate(face_id, bary, faces, verts, (0, 0, 0))[covered]
    want = affine(point)
    tri = affine(verts[faces[np.unique(face_id[covered])]])
    step = np.abs(tri - np.roll(tri, 1, axis=1)).max() / n
    width = MT.layout(len(faces), n)["width"]
    bound = 1.0 / 255 + 9 * EPS * width * step + 5 * EPS * 0.4 * np.abs(verts).max() + 32 * EPS
    err = np.abs(got - want).max()
    print(f"{tag}: n = {n}, {covered.sum()} px, largest error {err:.6f} = {err * 255:.4f} / 255, bound {bound:.6f}")
    assert covered.sum() > 500 and err <= bound
    return err


def test_a_textured_render_of_an_affine_colour_is_within_one_grey_level(sphere_rasters):
    verts, faces, pose = sheet()
    _accuracy(verts, faces, MR.rasterize(verts, faces, pose, 48, 48, 60.0, 0.1), 4, "sheet")
    verts, faces, rasters = sphere_rasters
    for (angles, _, _, _), raster in zip(SPHERE_VIEWS, rasters):
        _accuracy(verts, faces, raster, 3, f"sphere {angles}")


def test_a_texture_keeps_what_per_vertex_colours_lose():
    """The point of the feature: a colour 0.5 + 0.5 sin(k . x) whose wavelength is about one triangle edge (a 16 x 8 sphere:
    edges of 0.39 at the equator; |k| = 16: a wavelength of 0.39).  Three colours per face cannot carry it; 45 samples per
    face at n = 8 can.  The ratio of the two MSEs against the analytic colour at each pixel's surface point is printed
    (chosen on the restatement to be >= 4) and 2 is asserted."""
    verts, faces = MM.uv_sphere(16, 8)
    k = np.array([9.0, -7.0, 11.0]) * (16.0 / np.linalg.norm([9.0, -7.0, 11.0]))
    colour = lambda p: np.repeat((0.5 + 0.5 * np.sin(np.asarray(p, F64) @ k))[..., None], 3, -1)  # noqa: E731
    uv, atlas = bake(verts, faces, verts, 8, colour)
    per_vertex = colour(verts).astype(F32)
    mse_texture = mse_vertex = pixels = 0
    for angles, h, w, focal in SPHERE_VIEWS[:2]:
        face_id, _, bary, _ = MR.rasterize(verts, faces, S.pose_spherical(*angles), h, w, focal, 0.1)
        covered = face_id >= 0
        want = colour(MR.interpolate(face_id, bary, faces, verts, (0, 0, 0))[covered])
        textured = MT.lookup(face_id, bary, uv, atlas, (0, 0, 0))[covered].astype(F64)
        blended = MR.interpolate(face_id, bary, faces, per_vertex, (0, 0, 0))[covered].astype(F64)
        mse_texture += ((textured - want) ** 2).sum()
        mse_vertex += ((blended - want) ** 2).sum()
        pixels += covered.sum()
    print(f"MSE over {pixels} px: texture {mse_texture / pixels / 3:.6f}, per vertex {mse_vertex / pixels / 3:.6f}, "
          f"ratio {mse_vertex / mse_texture:.2f}")
    assert pixels > 1000 and mse_vertex >= 2 * mse_texture


def test_samples_restatement_corners_directions_and_counts():
    verts, faces = MM.uv_sphere(16, 8)
    n = 5
    pos, direction, fallback, bad = MT.samples(verts, faces, verts, n)
    per_face = (n + 1) * (n + 2) // 2
    assert pos.dtype == F32 and pos.shape == (len(faces) * per_face, 3) and fallback == 0 and bad == 0
    pos = pos.reshape(len(faces), per_face, 3)
    for k, (i, j) in enumerate(((0, 0), (n, 0), (0, n))):
        got, want = pos[:, MT.index(n, i, j)], verts[faces[:, k]]
        assert (got == want).all(), "a corner sample is the vertex: 1 p + 0 q + 0 r, exactly"
        assert (got.view(np.uint32) == want.view(np.uint32))[want != 0].all(), "bit for bit (a -0 coordinate comes back as +0)"
    assert np.abs(np.linalg.norm(direction.astype(F64), axis=1) - 1).max() < 1e-6
    assert ((direction.astype(F64) * pos.reshape(-1, 3)).sum(1) < 0).all(), "minus the normal: towards the centre"
    # without normals: minus flip times the winding's normal; the 2 x 16 faces at the poles are degenerate -> (0, 0, -1)
    _, geometric, fallback, _ = MT.samples(verts, faces, None, n, flip=1)
    flipped = MT.samples(verts, faces, None, n, flip=-1)[1]
    assert fallback == len(faces) * per_face
    degenerate = np.repeat((np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]]) == 0).all(1), per_face)
    assert degenerate.sum() == 32 * per_face and (geometric[degenerate] == np.array([0, 0, -1], F32)).all()
    assert (geometric[~degenerate] == -flipped[~degenerate]).all() and (flipped[degenerate] == geometric[degenerate]).all()
    outward = (geometric.astype(F64) * pos.reshape(-1, 3)).sum(1)[~degenerate]
    assert (outward < 0).all() or (outward > 0).all(), "one sign over the whole sphere: the winding's"
    # windows concatenate to the whole; a face with a bad index gives zero rows and is counted
    whole = MT.samples(verts, faces, verts, n)
    parts = [MT.samples(verts, faces, verts, n, first, count) for first, count in ((0, 1), (1, len(faces) - 2), (len(faces) - 1, 1))]
    assert np.concatenate([p[0] for p in parts]).tobytes() == whole[0].tobytes()
    assert np.concatenate([p[1] for p in parts]).tobytes() == whole[1].tobytes()
    broken = faces.copy()
    broken[3, 1] = len(verts)
    pos, direction, fallback, bad = MT.samples(verts, broken, verts, n)
    assert bad == per_face and fallback == 0 and not pos[3 * per_face:4 * per_face].any() and not direction[3 * per_face:4 * per_face].any()


def test_fill_restatement_gutter_empty_slots_and_quantisation():
    n, num_faces = 2, 3
    per_face = 6
    colours = np.zeros((num_faces * per_face, 3), F32)
    colours[:, 0] = np.arange(num_faces * per_face) / 32.0
    colours[0, 1], colours[1, 1], colours[2, 1] = np.nan, 2.0, -1.0
    atlas = MT.fill(colours, num_faces, n)
    lay = MT.layout(num_faces, n)
    assert atlas.dtype == np.uint8 and atlas.shape == (lay["height"], lay["width"], 3) == (4, 10, 3)
    face, i, j = MT.texel_owner(num_faces, n)
    assert (atlas[face < 0] == 0).all() and (face[:, 5:] <= 2).all() and (face[:, 5:] == -1).sum() == 10, "face 3 is an empty slot"
    q = lambda c: int(F32(min(max(c, 0.0), 1.0)) * F32(255) + F32(0.5))       # noqa: E731
    assert atlas[0, 0].tolist() == [0, 0, 0] and atlas[0, 1, 1] == 255 and atlas[0, 2, 1] == 0, "NaN -> 0, clamped to [0, 1]"
    assert atlas[1, 1, 0] == q(colours[MT.index(n, 1, 1), 0])
    # the gutter of face 0: (3, 0) = c(2, 0); (0, 3) = c(0, 2); (2, 1) = c(1, 1) + c(2, 0) - c(1, 0)
    c = lambda a, b: colours[MT.index(n, a, b), 0]                             # noqa: E731
    assert atlas[0, 3, 0] == q(c(2, 0)) and atlas[3, 0, 0] == q(c(0, 2)) and atlas[1, 2, 0] == q((c(1, 1) + c(2, 0)) - c(1, 0))
    assert atlas[2, 1, 0] == q((c(0, 2) + c(1, 1)) - c(0, 1))


def test_lookup_restatement_clamps_and_masks():
    texture = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3) * 10
    uv = np.array([[[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]], F32)
    face_id = np.array([0, 0, 0, 0, -1, 1, 0, 0], np.int32)
    bary = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-3, 2, 2], [1, 0, 0], [1, 0, 0], [np.nan, 0, 1], [np.inf, 1, 0]], F32)
    out = MT.lookup(face_id, bary, uv, texture, (9, 8, 7))
    values = MT.texel_values(texture)
    assert out.dtype == F32 and out.shape == (8, 3)
    assert (out[0] == values[1, 0]).all() and (out[1] == values[1, 2]).all() and (out[2] == values[0, 0]).all(), "v points up"
    assert (out[3] == values[0, 2]).all(), "(2, 2) is clamped to the edge"
    assert (out[4:] == np.array([9, 8, 7], F32)).all(), "no face, a face beyond the mesh, coordinates that are not finite"
    centre = MT.lookup(np.zeros(1, np.int32), np.array([[0.0, 0.5, 0.5]], F32), uv, texture, (0, 0, 0))
    assert np.abs(centre[0] - (0.5 * values[1, 1] + 0.5 * values[0, 1])).max() < 1e-6, "(u, v) = (0.5, 0.5): the middle column, between the two rows"


def _small_textured_mesh():
    rng = np.random.default_rng(4)
    v = (rng.standard_normal((40, 3)) * 2).astype(F32)
    v[0] = [1e-30, -0.0, 123456.789]
    c = rng.random((40, 3), dtype=F32)
    n = rng.standard_normal((40, 3)).astype(F32)
    f = rng.integers(0, 40, (61, 3)).astype(np.int32)
    uv = MT.face_uv(len(f), 3)
    atlas = rng.integers(0, 256, (MT.layout(len(f), 3)["height"], MT.layout(len(f), 3)["width"], 3)).astype(np.uint8)
    return v, f, c, n, uv, atlas


def test_the_textured_obj_round_trip(tmp_path, lib):
    from nerfmeshes_amd.nerf.nerf_helpers import export_obj, export_obj_textured, load_obj_attributes, load_obj_textured
    v, f, c, n, uv, atlas = _small_textured_mesh()
    path, plain = str(tmp_path / "t.obj"), str(tmp_path / "plain.obj")
    export_obj_textured(v, f, c, n, uv, atlas, path)
    export_obj(v, f, c, n, plain)
    rv, rf, rc, rn, ruv, image = load_obj_textured(path)
    for got, want in ((rv, v), (rf, f), (rc, c), (rn, n), (ruv, uv)):
        got = got.numpy()
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
    assert image == str(tmp_path / "t.png")
    from PIL import Image
    assert np.asarray(Image.open(image)).tobytes() == atlas.tobytes(), "the PNG keeps the atlas byte for byte"
    lines, base = open(path).read().split("\n"), open(plain).read().split("\n")
    assert lines[0] == "mtllib t.mtl" and [l for l in lines if l.startswith(("v ", "vn "))] == [l for l in base if l.startswith(("v ", "vn "))]
    assert lines[1:1 + 80] == base[:80], "the v and vn lines are nm_export_obj's, byte for byte and in place"
    assert lines[81:81 + 183] == [f"vt {float(a)!r} {float(b)!r}" for a, b in uv.reshape(-1, 2)] and lines[264] == "usemtl material_0"
    want_f = [" ".join(["f"] + [f"{int(a) + 1}/{3 * t + k + 1}/{int(a) + 1}" for k, a in enumerate(row)]) for t, row in enumerate(f)]
    assert lines[265:265 + 61] == want_f and lines[326:] == [""]
    mtl = open(tmp_path / "t.mtl").read().split("\n")
    assert mtl[0] == "newmtl material_0" and "Kd 1 1 1" in mtl and "map_Kd t.png" in mtl
    for a, b in zip(load_obj_attributes(path), load_obj_attributes(plain)):
        assert a.numpy().tobytes() == b.numpy().tobytes(), "load_obj_attributes does not see the texture"
    assert load_obj_textured(plain)[4:] == (None, None)


def test_an_obj_without_a_usable_texture_is_still_read(tmp_path):
    from nerfmeshes_amd.nerf.nerf_helpers import export_obj_textured, load_obj_textured
    v, f, c, n, uv, atlas = _small_textured_mesh()
    path = str(tmp_path / "t.obj")
    export_obj_textured(v, f, c, n, uv, atlas, path)
    text = open(path).read()
    cases = {"no_mtllib.obj": text.replace("mtllib t.mtl\n", ""), "missing_mtl.obj": text.replace("mtllib t.mtl", "mtllib gone.mtl")}
    lines = text.split("\n")
    first_face = next(k for k, l in enumerate(lines) if l.startswith("f "))
    entries = lines[first_face].split()
    entries[2] = entries[2].split("/")[0] + "//" + entries[2].split("/")[2]
    cases["one_corner_without_vt.obj"] = "\n".join(lines[:first_face] + [" ".join(entries)] + lines[first_face + 1:])
    entries[2] = entries[2].split("/")[0] + "/99999/" + entries[2].split("/")[2]
    cases["vt_out_of_range.obj"] = "\n".join(lines[:first_face] + [" ".join(entries)] + lines[first_face + 1:])
    for name, body in cases.items():
        open(tmp_path / name, "w").write(body)
        rv, rf, rc, rn, ruv, image = load_obj_textured(str(tmp_path / name))
        assert ruv is None and image is None, name
        assert rv.numpy().tobytes() == v.tobytes() and rf.numpy().tobytes() == f.tobytes() and rc.numpy().tobytes() == c.tobytes(), name
    (tmp_path / "noimage").mkdir()
    open(tmp_path / "noimage" / "t.obj", "w").write(text)
    open(tmp_path / "noimage" / "t.mtl", "w").write("newmtl material_0\nmap_Kd t.png\n")
    assert load_obj_textured(str(tmp_path / "noimage" / "t.obj"))[4:] == (None, None), "the image itself is missing"
    quad = "mtllib t.mtl\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nf 1/1 2/2 3/3 4/4\nf -4/-4 -3/-3 -2/-2\n"
    open(tmp_path / "quad.obj", "w").write(quad)
    _, qf, _, _, quv, image = load_obj_textured(str(tmp_path / "quad.obj"))
    assert qf.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2]] and image == str(tmp_path / "t.png")
    assert quv.tolist() == [[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]], [[0, 0], [1, 0], [1, 1]]], "the fan carries vt along"


def test_argument_errors_return_2_before_any_hip_call(lib, tmp_path):
    p = C.c_void_p(256)                                              # never dereferenced: every call fails its checks first

    def samples(verts=p, nv=3, faces=p, nf=2, normals=None, n=4, flip=1, first=0, count=2, pos=p, direction=p, counts=p):
        return lib.nm_mesh_texture_samples(verts, nv, faces, nf, normals, n, flip, first, count, pos, direction, counts, None)

    for name in ("verts", "faces", "pos", "direction", "counts"):
        assert samples(**{name: None}) == 2 and b"bad argument" in lib.nm_last_error(), name
    for n in (0, -1, 256):
        assert samples(n=n) == 2 and b"resolution" in lib.nm_last_error()
    assert samples(flip=0) == 2 and b"flip" in lib.nm_last_error() and samples(flip=2) == 2
    for first, count in ((-1, 1), (0, 3), (2, 1), (3, 0), (0, -1)):
        assert samples(first=first, count=count) == 2 and b"window" in lib.nm_last_error(), (first, count)
    assert samples(nv=0) == 2 and samples(nf=-1) == 2 and samples(nv=2 ** 31 - 64) == 2
    assert samples(nf=10 ** 6, count=10 ** 6, n=255) == 2 and b"one window" in lib.nm_last_error()
    fill = lambda colors=p, nf=2, n=4, atlas=p: lib.nm_mesh_texture_fill(colors, nf, n, atlas, None)   # noqa: E731
    assert fill(colors=None) == 2 and fill(atlas=None) == 2 and fill(n=0) == 2 and fill(n=256) == 2 and fill(nf=-1) == 2
    assert fill(nf=2 ** 30, n=8) == 2 and b"wider than 16384" in lib.nm_last_error()
    uv = lambda nf=2, n=4, out=p: lib.nm_mesh_texture_uv(nf, n, out, None)                             # noqa: E731
    assert uv(out=None) == 2 and uv(n=0) == 2 and uv(nf=2 ** 31 - 64) == 2 and uv(nf=2 ** 30, n=8) == 2

    def lookup(ids=p, bary=p, pixels=64, uv=p, nf=2, texture=p, th=4, tw=4, background=p, out=p):
        return lib.nm_mesh_texture_lookup(ids, bary, pixels, uv, nf, texture, th, tw, background, out, None)

    for name in ("ids", "bary", "uv", "texture", "background", "out"):
        assert lookup(**{name: None}) == 2 and b"bad argument" in lib.nm_last_error(), name
    for th, tw in ((0, 4), (4, 0), (16385, 4), (4, 16385), (-1, 4)):
        assert lookup(th=th, tw=tw) == 2 and b"sides" in lib.nm_last_error()
    assert lookup(pixels=-1) == 2 and lookup(pixels=2 ** 28 + 1) == 2 and lookup(nf=-1) == 2
    assert lib.nm_mesh_texture_layout(2, 4, None) == 2 and native_layout(lib, 2, 0)[0] == 2 and native_layout(lib, -1, 4)[0] == 2
    rc, empty = native_layout(lib, 0, 4)
    assert rc == 0 and empty["height"] == 0 and empty["rows"] == 0, "the C entry lays out no face; the Python layer refuses it"

    v = np.zeros((3, 3), F32)
    f = np.array([[0, 1, 2]], np.int32)
    t = np.zeros((3, 2), F32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)                                                           # noqa: E731
    path = str(tmp_path / "x.obj").encode()

    def export(uv=ptr(t), mtllib=b"x.mtl", material=b"m", verts=ptr(v)):
        return lib.nm_export_obj_textured(verts, 3, None, 0, None, 0, ptr(f), 1, uv, mtllib, material, path)

    assert export() == 0
    assert export(uv=None) == 2 and b"texture coordinates" in lib.nm_last_error()
    assert export(verts=None) == 2 and b"null array" in lib.nm_last_error()
    for bad in (None, b"", b"two words.mtl", b"line\nbreak"):
        assert export(mtllib=bad) == 2 and export(material=bad) == 2 and b"names" in lib.nm_last_error()
    assert lib.nm_export_obj_textured(ptr(v), 3, None, 0, None, 0, ptr(f), 1, ptr(t), b"x.mtl", b"m", str(tmp_path / "no" / "x.obj").encode()) == 6


def test_the_python_layer_refuses_what_the_rule_refuses():
    from nerfmeshes_amd import hip_ops
    with pytest.raises(ValueError, match="no atlas"):
        hip_ops.mesh_texture_layout(0, 4)
    with pytest.raises(ValueError, match="wider than 16384"):
        hip_ops.mesh_texture_layout(2 ** 30, 8)
    with pytest.raises(ValueError, match="resolution"):
        hip_ops.mesh_texture_layout(10, 256)
    assert hip_ops.mesh_texture_layout(1001, 8) == MT.layout(1001, 8)


def test_mesh_nerf_takes_texture_res_and_refuses_the_script_route():
    from nerfmeshes_amd import mesh_nerf, mesh_render
    args = mesh_nerf.build_parser().parse_args(["--texture-res", "8"])
    assert args.texture_res == 8 and mesh_nerf.build_parser().parse_args([]).texture_res == 0
    bad = mesh_nerf.build_parser().parse_args(["--texture-res", "4", "--route", "script", "--save-dir", "."])
    with pytest.raises(ValueError, match="--texture-res has no --route script"):
        mesh_nerf.export_marching_cubes(None, bad, None, "cpu")
    big = mesh_nerf.build_parser().parse_args(["--texture-res", "256", "--save-dir", "."])
    with pytest.raises(ValueError, match="--texture-res must be in"):
        mesh_nerf.export_marching_cubes(None, big, None, "cpu")
    p = mesh_render.build_parser()
    assert p.parse_args(["--mesh", "m.obj"]).appearance == "auto" and p.parse_args(["--mesh", "m.obj", "--appearance", "texture"]).appearance == "texture"
    with pytest.raises(SystemExit):
        p.parse_args(["--mesh", "m.obj", "--appearance", "both"])
