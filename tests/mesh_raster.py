"""numpy restatement of the mesh rasteriser (nerfmeshes_amd/csrc/mesh_raster.hip; the rule is written out in
include/nerfmeshes_hip.h, "Rasteriser of a mesh"): the same fp64 / int64 / fp32 operations in the same order, a vectorised
walk over every face's bounding box and the 64-bit minimum per pixel.  The device must reproduce every array bit for bit."""
import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64
COUNT_NAMES = ("drawn", "bad_index", "not_finite", "near", "out_of_range", "culled", "off_screen", "degenerate", "large", "covered",
               "fragments")
RANGE = 2.0 ** 24
LARGE_THRESHOLD = 128                            # hip_ops.RASTER_LARGE_THRESHOLD
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def project(verts, pose, height, width, focal):
    """the vertex stage -> (X int64, Y int64, w fp32, finite, in_range)"""
    pose = np.asarray(pose, F32)[:3, :4]
    rot, t = pose[:, :3].astype(F64), pose[:, 3].astype(F64)
    p = np.asarray(verts, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d = p.astype(F64) - t
        cam = [(rot[0, k] * d[:, 0] + rot[1, k] * d[:, 1]) + rot[2, k] * d[:, 2] for k in range(3)]
        w = (-cam[2]).astype(F32)
        wd = w.astype(F64)
        sx = ((cam[0] / wd) * F64(focal) + F64(width) * 0.5) * 256.0
        sy = (-(cam[1] / wd) * F64(focal) + F64(height) * 0.5) * 256.0
        finite = np.isfinite(p).all(axis=1) & np.isfinite(w)
        in_range = (np.abs(sx) <= RANGE) & (np.abs(sy) <= RANGE)
        x = np.where(in_range, np.rint(np.where(in_range, sx, 0.0)), 0.0).astype(I64)
        y = np.where(in_range, np.rint(np.where(in_range, sy, 0.0)), 0.0).astype(I64)
    return x, y, w, finite, in_range


def rasterize(verts, faces, pose, height, width, focal, near, cull_back=False, large_threshold=LARGE_THRESHOLD):
    """-> (face_id (H,W) int32, depth (H,W) fp32, bary (H,W,3) fp32, counts dict)"""
    height, width = int(height), int(width)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    nv = len(np.asarray(verts).reshape(-1, 3))
    x, y, w, finite, in_range = project(verts, pose, height, width, focal)
    near = F32(near)
    counts = dict.fromkeys(COUNT_NAMES, 0)
    words = np.full((height, width), EMPTY, np.uint64)
    bary = np.zeros((height, width, 3), F32)
    for f, c in enumerate(faces.astype(I64)):
        if ((c < 0) | (c >= nv)).any():
            counts["bad_index"] += 1
            continue
        if not finite[c].all():
            counts["not_finite"] += 1
            continue
        if (w[c] < near).any():
            counts["near"] += 1
            continue
        if not in_range[c].all():
            counts["out_of_range"] += 1
            continue
        px, py = x[c], y[c]
        area = (px[1] - px[0]) * (py[2] - py[0]) - (py[1] - py[0]) * (px[2] - px[0])
        if cull_back and area > 0:
            counts["culled"] += 1
            continue
        ilo, ihi = max((px.min() + 255) >> 8, 0), min(px.max() >> 8, width - 1)
        jlo, jhi = max((py.min() + 255) >> 8, 0), min(py.max() >> 8, height - 1)
        if ilo > ihi or jlo > jhi:
            counts["off_screen"] += 1
            continue
        if area == 0:
            counts["degenerate"] += 1
            continue
        counts["drawn"] += 1
        if (ihi - ilo + 1) * (jhi - jlo + 1) > large_threshold:
            counts["large"] += 1
        sign = -1 if area < 0 else 1
        gx = (256 * np.arange(ilo, ihi + 1, dtype=I64))[None, :]
        gy = (256 * np.arange(jlo, jhi + 1, dtype=I64))[:, None]
        inside, e = True, []
        for k in range(3):                       # edge k runs from corner k + 1 to corner k + 2
            a, b = (k + 1) % 3, (k + 2) % 3
            dx, dy = sign * (px[b] - px[a]), sign * (py[b] - py[a])
            ek = dx * (gy - py[a]) - dy * (gx - px[a])
            inside = inside & ((ek >= 0) if (dy < 0 or (dy == 0 and dx > 0)) else (ek > 0))
            e.append(ek)
        if not inside.any():
            continue
        with np.errstate(all="ignore"):
            t = [(e[k].astype(F64) / F64(sign * area)) * (1.0 / F64(w[c[k]])) for k in range(3)]
            q = (t[0] + t[1]) + t[2]
            depth = (1.0 / q).astype(F32)
            b = np.stack([(t[k] / q).astype(F32) for k in range(3)], -1)
        inside = inside & np.isfinite(depth) & (depth > 0)
        counts["fragments"] += int(inside.sum())
        word = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
        box = words[jlo:jhi + 1, ilo:ihi + 1]
        win = inside & (word < box)
        box[win] = word[win]
        bary[jlo:jhi + 1, ilo:ihi + 1][win] = b[win]
    covered = words != EMPTY
    face_id = np.where(covered, (words & np.uint64(0xFFFFFFFF)).astype(I64), -1).astype(np.int32)
    depth = np.where(covered, (words >> np.uint64(32)).astype(np.uint32), np.uint32(0)).astype(np.uint32).view(F32)
    counts["covered"] = int(covered.sum())
    return face_id, depth, bary, counts


def interpolate(face_id, bary, faces, attributes, background):
    """out = (b0 a0 + b1 a1) + b2 a2 in fp32 per channel; the background row where nothing was drawn"""
    faces = np.asarray(faces, np.int32).reshape(-1, 3).astype(I64)
    attributes = np.asarray(attributes, F32)
    nv, nf = len(attributes), len(faces)
    flat, b = face_id.reshape(-1).astype(I64), np.asarray(bary, F32).reshape(-1, 3)
    ok = (flat >= 0) & (flat < nf)
    corners = faces[np.where(ok, flat, 0)] if nf else np.zeros((len(flat), 3), I64)
    ok &= ((corners >= 0) & (corners < nv)).all(axis=1)
    corners = np.where(ok[:, None], corners, 0)
    rows = [attributes[corners[:, k]] if nv else np.zeros((len(flat), attributes.shape[1]), F32) for k in range(3)]
    out = (b[:, 0:1] * rows[0] + b[:, 1:2] * rows[1]) + b[:, 2:3] * rows[2]
    out = np.where(ok[:, None], out, np.asarray(background, F32)[None, :]).astype(F32)
    return out.reshape(*face_id.shape, attributes.shape[1])


def pixel_rays(pose, height, width, focal):
    """-> (origin, dirs (H,W,3)) in fp64: get_ray_bundle's camera-space ray (x, y, -1) BEFORE it is normalised, turned into the
    world.  Its parameter is the distance along the camera's axis, the rasteriser's depth: a pixel sees origin + depth * dir."""
    pose = np.asarray(pose, F64)[:3, :4]
    i, j = np.meshgrid(np.arange(width, dtype=F64), np.arange(height, dtype=F64), indexing="xy")
    cam = np.stack(((i - width * 0.5) / focal, -(j - height * 0.5) / focal, -np.ones_like(i)), -1)
    return pose[:, 3], cam @ pose[:, :3].T
