"""Helper functions the three scripts import by name (mirror of /root/reference/src/nerf/nerf_helpers.py)."""
import os

import numpy as np
import torch

from .. import hip_ops


def img2mse(img_src, img_tgt):
    return torch.nn.functional.mse_loss(img_src, img_tgt)


def mse2psnr(mse):
    """nerf_helpers.py:17-23: PSNR = -10 log10(mse), MAX = 1."""
    mse = torch.as_tensor(mse)
    if mse == 0:
        mse = torch.full_like(mse, 1e-5, dtype=torch.float32)
    return -10.0 * torch.log10(mse)


# colours of the depth-residual point clouds (nerf_helpers.py:8-11)
POINT_GROUND_TRUTH = torch.tensor([0., 0., 255.])
POINT_OUT_TRUE = torch.tensor([0., 255., 0.])
POINT_OUT_FALSE_VOID = torch.tensor([0., 0., 0.])
POINT_OUT_FALSE_SURFACE = torch.tensor([255., 0., 0.])


def create_point_cloud(ray_origins, ray_directions, depth, color, mask=None):
    """nerf_helpers.py:56-64: points o + d * depth (of the masked rays), one constant colour, normals = -d."""
    if mask is not None:
        ray_directions, depth = ray_directions[mask], depth[mask]
    vertices = (ray_origins + ray_directions * depth[..., None]).view(-1, 3)
    return vertices, color.to(vertices.device).expand(vertices.shape), -ray_directions.view(-1, 3)


def get_point_clouds(ray_origins, ray_directions, depth_output, depth_target=None, threshold=0.2, empty=0.):
    """nerf_helpers.py:26-53: the rendered depths as a coloured point cloud; with target depths, four clouds
    (target / hits within `threshold` / misses over empty space / misses over the surface) concatenated per field."""
    if depth_target is None:
        return create_point_cloud(ray_origins, ray_directions, depth_output, POINT_GROUND_TRUTH)
    hit = torch.abs(depth_output - depth_target) < threshold
    clouds = [create_point_cloud(ray_origins, ray_directions, depth_target, POINT_GROUND_TRUTH),
              create_point_cloud(ray_origins, ray_directions, depth_output, POINT_OUT_TRUE, hit),
              create_point_cloud(ray_origins, ray_directions, depth_output, POINT_OUT_FALSE_VOID, (depth_target == empty) & ~hit),
              create_point_cloud(ray_origins, ray_directions, depth_output, POINT_OUT_FALSE_SURFACE, (depth_target != empty) & ~hit)]
    return [torch.cat(field, dim=0) for field in zip(*clouds)]


def comp_depth(depth_output, depth_target, empty_value=0.):
    """nerf_helpers.py:67-83: depth MSE overall / over empty pixels / over surface pixels, and the mean signed error."""
    mse = torch.nn.functional.mse_loss
    surface = depth_target > empty_value
    return (mse(depth_output, depth_target), mse(depth_output[~surface], depth_target[~surface]),
            mse(depth_output[surface], depth_target[surface]), (depth_output[surface] - depth_target[surface]).mean())


def batchify(*data, batch_size=1024, device="cpu", progress=True):
    """nerf_helpers.py:114-139: yield aligned slices of every tensor, moved to `device`."""
    size = data[0].shape[0]
    assert all(s is None or s.shape[0] == size for s in data), "Sizes of tensors must match for dimension 0."

    def gen():
        for start in range(0, size, batch_size):
            yield [s[start:start + batch_size].to(device) if s is not None else s for s in data]

    if not progress:
        return gen()
    try:
        from tqdm import tqdm
        return tqdm(gen(), total=(size - 1) // batch_size + 1)
    except ImportError:
        return gen()


def meshgrid_xy(tensor1, tensor2):
    ii, jj = torch.meshgrid(tensor1, tensor2, indexing="ij")
    return ii.transpose(-1, -2), jj.transpose(-1, -2)


def cumprod_exclusive(tensor):
    """nerf_helpers.py:199-223 (kept for API compatibility; the render path does the scan in-kernel)."""
    c = torch.roll(torch.cumprod(tensor, -1), 1, -1)
    c[..., 0] = 1.0
    return c


def get_ray_bundle(height, width, focal_length, tform_cam2world):
    """nerf_helpers.py:226-277 on the GPU: (origin (3,), directions (H, W, 3))."""
    dev = tform_cam2world.device if isinstance(tform_cam2world, torch.Tensor) and tform_cam2world.is_cuda else "cuda"
    origin, dirs = hip_ops.ray_bundle(tform_cam2world, int(height), int(width), float(focal_length), device=dev)
    return origin, dirs.reshape(int(height), int(width), 3)


def ndc_rays(H, W, focal, near, rays_o, rays_d):
    """nerf_helpers.py:280-307 -> nm_ndc_rays (one HIP kernel, op for op as the reference's torch expressions)."""
    return hip_ops.ndc_rays(H, W, focal, near, rays_o, rays_d)


def cast_to_image(tensor):
    """(H, W, 3) float -> (3, H, W) uint8 numpy (nerf_helpers.py:155-181 family)."""
    img = (tensor.detach().cpu().clamp(0.0, 1.0) * 255).to(torch.uint8).numpy()
    return np.moveaxis(img, [-1], [0])


def cast_to_pil_image(tensor):
    return (tensor.detach().cpu().clamp(0.0, 1.0) * 255).to(torch.uint8).numpy()


def cast_to_disparity_image(tensor, white_background=False):
    """(H, W) -> uint8 image, min-max normalised; exact zeros become white if requested."""
    img = (tensor - tensor.min()) / (tensor.max() - tensor.min())
    img = (img.clamp(0.0, 1.0) * 255).byte()
    if white_background:
        img[img == 0] = 255
    return img.detach().cpu().numpy()


def export_point_cloud(it, ray_origins, ray_directions, depth_fine, dep_target):
    """nerf_helpers.py:142-152: rendered (red) and target (blue) depth points of one image -> `<it:04d>.obj`."""
    rendered = (ray_origins + ray_directions * depth_fine[..., None]).view(-1, 3)
    target = (ray_origins + ray_directions * dep_target[..., None]).view(-1, 3)
    red, blue = torch.zeros_like(rendered), torch.zeros_like(target)
    red[:, 0], blue[:, 2] = 1.0, 1.0
    back = -ray_directions.view(-1, 3)
    export_obj(torch.cat((rendered, target), 0), [], torch.cat((red, blue), 0), torch.cat((back, back), 0), f"{it:04d}.obj")


def export_obj(vertices, triangles, diffuse, normals, filename):
    """nerf_helpers.py:86-111 text format: `v x y z [r g b]`, `vn x y z`, `f a//a b//b c//c` (1-based), numbers exactly
    as the reference's `"{}".format(tensor_element)` prints them (repr of the fp32 value widened to a Python float).
    Formatting runs in the native library on all host threads (nm_export_obj): the per-element Python writer needs
    10.6 s for the 480^3 mesh (2.3 M lines, 209 MB) -- 14x the whole GPU extraction."""
    import ctypes as C
    from .. import _lib

    def host(x, dtype):
        if isinstance(x, torch.Tensor):
            x = x.detach().cpu().numpy()
        return np.ascontiguousarray(np.asarray(x), dtype=dtype).reshape(-1, 3)

    v, c, n, t = host(vertices, np.float32), host(diffuse, np.float32), host(normals, np.float32), host(triangles, np.int32)
    print("Writing to obj...")
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    _lib.check(_lib.load().nm_export_obj(ptr(v), len(v), ptr(c), len(c), ptr(n), len(n), ptr(t), len(t),
                                         os.fsencode(filename)), "nm_export_obj")
    print(f"Finished writing to {filename} with {len(v)} vertices")


def load_obj(path):
    """Wavefront OBJ -> (verts (V,3) f32, faces (F,3) i32, 0-based) as host tensors: the reader `export_obj` lacked (the
    reference's loader for `<basedir>/model.obj` is commented out, datasets.py:88-103).  `v x y z [r g b]` lines give the
    vertices (colour columns are dropped); `f` lines take `i`, `i/t`, `i//n` and `i/t/n` entries, negative indices count back
    from the vertices read so far, polygons are fan-triangulated (a, b, c, d -> abc, acd).  Every other line is ignored.
    ValueError with the line number for a face index out of range or a line that cannot be read."""
    verts, faces, forward = [], [], []
    with open(path, "r", errors="replace") as fh:
        for lineno, line in enumerate(fh, 1):
            if line.startswith("v ") or line.startswith("v\t"):
                parts = line.split()
                try:
                    verts.append((float(parts[1]), float(parts[2]), float(parts[3])))
                except (IndexError, ValueError):
                    raise ValueError(f"{path}:{lineno}: a vertex needs three numbers: {line.strip()!r}") from None
            elif line.startswith("f ") or line.startswith("f\t"):
                nv, corners = len(verts), []
                for entry in line.split()[1:]:
                    try:
                        i = int(entry.split("/", 1)[0])
                    except ValueError:
                        raise ValueError(f"{path}:{lineno}: cannot read the face entry {entry!r}") from None
                    if i > 0:                              # absolute: may name a vertex that a later line defines
                        i -= 1
                        if i >= nv:
                            forward.append((lineno, i))
                    else:                                  # relative to the vertices read so far; 0 is no index
                        i = nv + i if i < 0 else -1
                        if i < 0:
                            raise ValueError(f"{path}:{lineno}: face index {entry.split('/', 1)[0]} is out of range "
                                             f"({nv} vertices so far)")
                    corners.append(i)
                if len(corners) < 3:
                    raise ValueError(f"{path}:{lineno}: a face needs at least three vertices: {line.strip()!r}")
                for k in range(1, len(corners) - 1):
                    faces.append((corners[0], corners[k], corners[k + 1]))
    for lineno, i in forward:
        if i >= len(verts):
            raise ValueError(f"{path}:{lineno}: face index {i + 1} is out of range ({len(verts)} vertices)")
    v = np.asarray(verts, dtype=np.float64).astype(np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).astype(np.int32).reshape(-1, 3)
    return torch.from_numpy(v), torch.from_numpy(f)


def load_obj_attributes(path):
    """`load_obj` plus what `export_obj` writes beside the positions -> (verts, faces, colors, normals): colors (V,3) f32
    from `v x y z r g b` lines, None unless EVERY vertex line carries three colour columns; normals (V,3) f32 from the `vn`
    lines, None unless there are exactly as many as vertices (export_obj's `f a//a` pairs normal i with vertex i).  The
    printed numbers read back to the fp32 values that were written."""
    verts, faces = load_obj(path)
    colors, normals = [], []
    with open(path, "r", errors="replace") as fh:
        for lineno, line in enumerate(fh, 1):
            if line.startswith(("v ", "v\t", "vn ", "vn\t")):
                parts = line.split()
                try:
                    if parts[0] == "vn":
                        normals.append((float(parts[1]), float(parts[2]), float(parts[3])))
                    elif len(parts) >= 7:
                        colors.append((float(parts[4]), float(parts[5]), float(parts[6])))
                except (IndexError, ValueError):
                    raise ValueError(f"{path}:{lineno}: cannot read the numbers of {line.strip()!r}") from None
    count = verts.shape[0]
    as_rows = lambda rows: torch.from_numpy(np.asarray(rows, dtype=np.float64).astype(np.float32).reshape(-1, 3))  # noqa: E731
    return (verts, faces, as_rows(colors) if count and len(colors) == count else None,
            as_rows(normals) if count and len(normals) == count else None)


MATERIAL_NAME = "material_0"


def write_mtl(path, image_name, material=MATERIAL_NAME):
    """the one-material library of a textured OBJ: white diffuse, the image as its diffuse map"""
    with open(path, "w") as fh:
        fh.write(f"newmtl {material}\nKa 0 0 0\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {image_name}\n")


def export_obj_textured(vertices, triangles, diffuse, normals, face_uv, atlas, filename):
    """`export_obj` with a texture (addition; nm_export_obj_textured): <stem>.obj with `mtllib <stem>.mtl`, the same `v x y z
    [r g b]` and `vn` lines, 3F `vt u v` lines from face_uv (F,3,2), `usemtl` and `f a/t/a b/t/b c/t/c`; <stem>.mtl naming
    <stem>.png; <stem>.png: the atlas (H,W,3) uint8, row 0 on top."""
    import ctypes as C
    from .. import _lib
    from ..eval_nerf import _imwrite

    def host(x, dtype, width=3):
        if isinstance(x, torch.Tensor):
            x = x.detach().cpu().numpy()
        return np.ascontiguousarray(np.asarray(x), dtype=dtype).reshape(-1, width)

    v, c, n, t = host(vertices, np.float32), host(diffuse, np.float32), host(normals, np.float32), host(triangles, np.int32)
    uv = host(face_uv, np.float32, 2)
    if len(uv) != 3 * len(t):
        raise ValueError(f"export_obj_textured: {len(uv)} texture coordinates for {len(t)} faces")
    image = atlas.detach().cpu().numpy() if isinstance(atlas, torch.Tensor) else np.asarray(atlas)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError(f"export_obj_textured: the atlas must be (H,W,3) uint8, got {image.shape} {image.dtype}")
    stem = os.path.splitext(filename)[0]
    name = os.path.basename(stem)
    print("Writing to obj...")
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    lib = _lib.load()
    rc = lib.nm_export_obj_textured(ptr(v), len(v), ptr(c), len(c), ptr(n), len(n), ptr(t), len(t), ptr(uv),
                                    os.fsencode(name + ".mtl"), MATERIAL_NAME.encode(), os.fsencode(filename))
    if rc == 2:
        raise ValueError((lib.nm_last_error() or b"nm_export_obj_textured: bad argument").decode())
    _lib.check(rc, "nm_export_obj_textured")
    write_mtl(stem + ".mtl", name + ".png")
    _imwrite(stem + ".png", np.ascontiguousarray(image))
    print(f"Finished writing to {filename} with {len(v)} vertices")


def _read_map_kd(obj_path, library):
    """the first `map_Kd` image of the material library named beside the OBJ, as a path, or None"""
    mtl = os.path.join(os.path.dirname(obj_path), library)
    try:
        with open(mtl, "r", errors="replace") as fh:
            for line in fh:
                parts = line.split()
                if parts and parts[0] == "map_Kd" and len(parts) >= 2:
                    image = os.path.join(os.path.dirname(mtl), parts[-1])
                    return image if os.path.isfile(image) and os.access(image, os.R_OK) else None
    except OSError:
        return None
    return None


def load_obj_textured(path):
    """`load_obj_attributes` plus the texture -> (verts, faces, colors, normals, face_uv, image_path): face_uv (F,3,2) f32 from
    the `vt` lines through the `f a/t/n` entries (fan triangulation carries the vt indices along; negative ones count back),
    image_path: the `map_Kd` file of the `mtllib` beside the OBJ.  The last two are None unless EVERY face corner has a vt
    index in range and the library and its image can be read; the first four are load_obj_attributes' own."""
    verts, faces, colors, normals = load_obj_attributes(path)
    coords, corners, library, complete = [], [], None, True
    with open(path, "r", errors="replace") as fh:
        for line in fh:
            if line.startswith(("vt ", "vt\t")):
                parts = line.split()
                try:
                    coords.append((float(parts[1]), float(parts[2])))
                except (IndexError, ValueError):
                    coords.append((float("nan"), float("nan")))
                    complete = False
            elif line.startswith(("f ", "f\t")):
                entry_uv = []
                for entry in line.split()[1:]:
                    fields = entry.split("/")
                    try:
                        t = int(fields[1]) if len(fields) >= 2 and fields[1] else 0
                    except ValueError:
                        t = 0
                    entry_uv.append(t - 1 if t > 0 else (len(coords) + t if t < 0 else -1))
                for k in range(1, len(entry_uv) - 1):
                    corners.append((entry_uv[0], entry_uv[k], entry_uv[k + 1]))
            elif line.startswith(("mtllib ", "mtllib\t")) and library is None:
                library = line.split(None, 1)[1].strip()
    index = np.asarray(corners, dtype=np.int64).reshape(-1, 3)
    image = _read_map_kd(path, library) if library else None
    if (not complete or image is None or len(index) != faces.shape[0] or not len(index) or not len(coords)
            or index.min() < 0 or index.max() >= len(coords)):
        return verts, faces, colors, normals, None, None
    table = np.asarray(coords, dtype=np.float64).astype(np.float32).reshape(-1, 2)
    return verts, faces, colors, normals, torch.from_numpy(np.ascontiguousarray(table[index])), image
