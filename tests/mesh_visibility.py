"""numpy restatement of the hidden-face filter (nerfmeshes_amd/csrc/mesh_raster.hip, nm_mesh_visibility_*; the rule is written
out in include/nerfmeshes_hip.h, "Hidden faces of a mesh"): the faces that win a pixel of tests/mesh_raster.py's rasteriser in at
least one view, `rings` rounds of growth over shared vertices, numpy's own renumbering.  Integer work only: the device must
reproduce every array and every count bit for bit."""
import numpy as np

from tests import mesh_raster as MR

F32, F64, I64 = np.float32, np.float64, np.int64


def sphere_poses(count, centre, radius):
    """mesh_render.sphere_views' cameras: (count, 3, 4) fp32 camera-to-world matrices on a Fibonacci lattice around `centre`,
    every camera looking at it.  fp64 on the host, cast to fp32 once."""
    centre = np.asarray(centre, F64).reshape(3)
    poses = np.zeros((int(count), 3, 4), F64)
    for k in range(int(count)):
        z = 1.0 - (2 * k + 1) / F64(count)
        a = k * (np.pi * (3.0 - np.sqrt(5.0)))
        s = np.sqrt(1.0 - z * z)
        d = np.array([s * np.cos(a), s * np.sin(a), z], F64)
        up = np.array([0.0, 1.0, 0.0] if abs(z) > 0.999 else [0.0, 0.0, 1.0], F64)
        right = np.cross(up, d)
        right /= np.sqrt((right * right).sum())
        poses[k, :, 0], poses[k, :, 1], poses[k, :, 2] = right, np.cross(d, right), d
        poses[k, :, 3] = centre + F64(radius) * d
    return poses.astype(F32)


def frame(verts, cull_radius, size):
    """mesh_render.frame_views: -> (centre (3,) fp64, radius, focal, near fp32).  The bounding sphere of the vertices' box fills
    95 % of a size x size image from `cull_radius` bounding radii away, and no face can fail the near test."""
    verts = np.asarray(verts, F32).reshape(-1, 3)
    lo, hi = verts.min(axis=0).astype(F64), verts.max(axis=0).astype(F64)
    centre = (lo + hi) / 2
    rb = 0.5 * np.sqrt(((hi - lo) ** 2).sum())
    radius = F64(cull_radius) * rb
    focal = 0.5 * size * np.sqrt(radius * radius - rb * rb) / rb * 0.95
    return centre, float(radius), float(focal), F32((radius - rb) / 2)


def seen_faces(verts, faces, poses, size, focal, near, seen=None):
    """-> (seen (F,) bool: the winners of at least one pixel of at least one view, OR-ed into `seen` when given; new_faces: per
    view the number of faces it saw first; the rasteriser's counts per view)"""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    seen = np.zeros(len(faces), bool) if seen is None else seen.copy()
    new_faces, counts = [], []
    for pose in poses:
        face_id, _, _, c = MR.rasterize(verts, faces, pose, size, size, focal, near)
        winners = np.unique(face_id[face_id >= 0])
        new_faces.append(int((~seen[winners]).sum()))
        seen[winners] = True
        counts.append(c)
    return seen, new_faces, counts


def grow(faces, nv, seen, rings):
    """-> (keep_f (F,) bool, keep_v (V,) bool, bad_faces): `rings` times every face with valid indices that touches a corner of
    a kept face becomes kept; a vertex is kept iff a kept face uses it"""
    faces = np.asarray(faces, np.int32).reshape(-1, 3).astype(I64)
    valid = ((faces >= 0) & (faces < nv)).all(axis=1)
    if nv == 0:
        return np.zeros(len(faces), bool), np.zeros(0, bool), len(faces)
    safe = np.where(valid[:, None], faces, 0)

    def corners(keep_f):
        marked = np.zeros(nv, bool)
        marked[safe[keep_f].reshape(-1)] = True
        return marked

    keep_f = seen & valid
    for _ in range(int(rings)):
        keep_f = valid & corners(keep_f)[safe].any(axis=1)
    return keep_f, corners(keep_f), int((~valid).sum())


def compact(verts, faces, normals, keep_f, keep_v):
    """numpy's renumbering: new = cumsum(keep_v) - 1; out = new[faces[keep_f]] -> (verts, faces, normals | None, face_index)"""
    verts = np.asarray(verts, F32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    new = np.cumsum(keep_v) - 1
    out_faces = new[faces[keep_f].astype(I64)].astype(np.int32).reshape(-1, 3)
    out_normals = None if normals is None else np.asarray(normals, F32).reshape(-1, 3)[keep_v]
    return verts[keep_v], out_faces, out_normals, np.nonzero(keep_f)[0].astype(np.int32)


def cull_hidden(verts, faces, normals, poses, size, focal, near, rings):
    """hip_ops.mesh_cull_hidden over square views of side `size` -> (verts, faces, normals, face_index, info)"""
    verts = np.asarray(verts, F32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    seen, new_faces, _ = seen_faces(verts, faces, poses, size, focal, near)
    keep_f, keep_v, bad = grow(faces, len(verts), seen, rings)
    info = dict(faces=len(faces), faces_seen=int(seen.sum()), faces_kept=int(keep_f.sum()), vertices=len(verts),
                vertices_kept=int(keep_v.sum()), bad_faces=bad, new_faces=new_faces)
    return compact(verts, faces, normals, keep_f, keep_v) + (info,)
