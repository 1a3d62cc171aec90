"""The oracle of the surface point cloud: the filter of the reference's script (src/mesh_surface_ray.py:115-141) restated in
torch on the CPU -- this project's own words for the same arithmetic in the same order of operations, one pass per window
offset over clamped index tensors -- and a small PLY reader for both formats.  Same role as tests/ss_refine.py: the HIP
kernels (nerfmeshes_amd/csrc/surface_filter.hip) are compared with it bit for bit."""
import numpy as np
import torch


def surface_filter(origins, dirs, depth, step, dist_threshold, prob_threshold, opacity=None, min_opacity=None):
    """origins (H, W, 3) or broadcastable to it, dirs (H, W, 3), depth (H, W) [, opacity (H, W) with min_opacity]
    -> (votes (H, W) int64, keep (H, W) bool, points (N, 3), normals (N, 3)), the kept pixels in row-major order.

    Line by line against the reference: the surface points (:115); the pixel grid and its clamped copy per offset (:118,
    :121-126); the squared distance summed over the last axis and compared with the Python float (:128-129); the vote count
    against `size_samples * prob_threshold` in Python doubles (:120, :133); the depth test (:135-136); boolean-mask indexing
    and the points recomputed from the masked rays (:138-141); the normal is the negated direction (:144).
    With `opacity`, the depth used is `depth` where opacity >= min_opacity and 0 elsewhere (the well-conditioned rule)."""
    height, width = depth.shape
    dirs = dirs.reshape(height, width, 3)
    origins = origins.expand(height, width, 3) if origins.dim() == 3 else origins.reshape(-1, 3).expand(height * width, 3).reshape(height, width, 3)
    if opacity is not None:
        depth = torch.where(opacity >= min_opacity, depth, torch.zeros_like(depth))
    surface = origins + dirs * depth[..., None]
    rows, cols = torch.meshgrid(torch.arange(height), torch.arange(width), indexing="ij")
    side = 2 * step + 1
    neighbours = side ** 2 - 1
    near = []
    for a in range(-step, step + 1):
        for b in range(-step, step + 1):
            r = (rows + a).clamp(0, height - 1)
            c = (cols + b).clamp(0, width - 1)
            shifted = surface[r, c]
            near.append(((shifted - surface) ** 2).sum(-1) < dist_threshold)
    votes = torch.stack(near, -1).sum(-1)
    keep = (votes > neighbours * prob_threshold) & (depth > 0)
    o, d, z = origins[keep], dirs[keep], depth[keep]
    return votes, keep, o + d * z[..., None], -d


def color_bytes(rgb):
    """fp32 colours -> the PLY's uchar: trunc(clamp(rgb * 255, 0, 255)), NaN -> 0 (numpy's own u1 cast truncates alike inside
    [0, 256) and wraps outside)."""
    c = rgb.detach().cpu().numpy() if isinstance(rgb, torch.Tensor) else np.asarray(rgb)
    c = c.astype(np.float32) * np.float32(255)
    return np.nan_to_num(np.clip(c, 0, 255), nan=0.0).astype(np.uint8)


PLY_PROPERTIES = [("x", "float"), ("y", "float"), ("z", "float"), ("nx", "float"), ("ny", "float"), ("nz", "float"),
                  ("red", "uchar"), ("green", "uchar"), ("blue", "uchar")]


def read_ply(path):
    """-> (format, points (N,3) f32, normals (N,3) f32, colours (N,3) u8) of a PLY with exactly PLY_PROPERTIES."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    assert head[0] == "ply" and head[-1] == "end_header"
    fmt = head[1].split()
    assert fmt[0] == "format" and fmt[2] == "1.0"
    elements = [l.split() for l in head if l.startswith("element")]
    assert len(elements) == 1 and elements[0][1] == "vertex"
    n = int(elements[0][2])
    props = [tuple(l.split()[:0:-1]) for l in head if l.startswith("property")]
    assert props == PLY_PROPERTIES, props
    body = data[end:]
    if fmt[1] == "ascii":
        lines = body.decode("ascii").splitlines()
        assert len(lines) == n
        cells = [l.split(" ") for l in lines]
        assert all(len(c) == 9 for c in cells)
        floats = np.array([[np.float32(t) for t in c[:6]] for c in cells], dtype=np.float32).reshape(n, 6)
        colours = np.array([[int(t) for t in c[6:]] for c in cells], dtype=np.int64).reshape(n, 3)
        assert ((colours >= 0) & (colours <= 255)).all()
        return "ascii", floats[:, :3].copy(), floats[:, 3:].copy(), colours.astype(np.uint8)
    assert fmt[1] == "binary_little_endian" and len(body) == 27 * n
    rec = np.frombuffer(body, dtype=np.dtype([("f", "<f4", 6), ("c", "u1", 3)]))
    return "binary", rec["f"][:, :3].copy(), rec["f"][:, 3:].copy(), rec["c"].copy()
