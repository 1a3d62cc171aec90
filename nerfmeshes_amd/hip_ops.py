"""Tensor-level host wrappers over the C ABI (torch is plumbing: device memory + streams).

Every function takes/returns torch CUDA(HIP) fp32 tensors, launches on torch's current stream and
raises if the HIP library is unavailable or an input is on the CPU -- no silent fallback.
"""
import ctypes as C
import math
import struct

import numpy as np
import torch

from . import _lib
from ._lib import BundleOut, MlpDesc, MlpWeights, RenderCfg, check

BUNDLE_FIELDS = ("rgb_map", "depth_map", "weights", "mask_weights", "acc_map", "disp_map")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """torch's current stream on the current device as the `void* stream` of the C ABI (the raw accessor costs 0.3 us, building a
    torch.cuda.Stream object 5 -- 9: every wrapper below pays it once or twice per call)."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev32(t, device=None, name="tensor"):
    """contiguous fp32 tensor on the GPU; host tensors are accepted only where the reference
    hands over host data (ray bounds: eval_nerf.py:65, mesh_nerf.py:179)."""
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t, dtype=torch.float32)
    elif t.is_cuda and t.dtype is torch.float32 and t.is_contiguous() and (device is None or t.device == device):
        return t.detach()                      # the common case: nothing to convert
    if device is not None and t.device != device:
        t = t.to(device)
    if not t.is_cuda:
        raise _lib.HipLibraryError(f"{name} must live in GPU memory (got {t.device}); there is no CPU path")
    return t.detach().to(torch.float32).contiguous()


_small_cache = {}


def _dev32_small(t, device):
    """`_dev32` for the few-element HOST tensors that are the same call after call -- the ray bounds the reference keeps on
    the CPU (eval_nerf.py:65, mesh_nerf.py:179, every training batch): device copies cached by value.  A pageable H2D copy
    per call is a host-blocking hipMemcpy that first drains the stream: at the top of every training iteration / render
    chunk it left the GPU idle for the CPU's launch latency."""
    if isinstance(t, torch.Tensor) and not t.is_cuda and t.numel() <= 4:
        key = (str(device), tuple(float(x) for x in t.reshape(-1).tolist()))
        hit = _small_cache.get(key)
        if hit is None:
            if len(_small_cache) > 256:
                _small_cache.clear()
            hit = _small_cache[key] = t.detach().to(device=device, dtype=torch.float32).contiguous()
        return hit
    return _dev32(t, device)


PRECISIONS = {"f32": 0, "bf16x3": 1}


class HipMLP:
    """Device-resident packed copy of one FlexibleNeRFModel (handle of nm_mlp_create_ex)."""

    def __init__(self, state, desc, device, precision="f32", force_generic=False):
        """state: dict name -> array-like in torch.nn.Linear layout, keyed like
        FlexibleNeRFModel.state_dict(); desc: dict of constructor hyper-parameters.
        precision: "f32" (default: fp32 MFMA, the reference's arithmetic) or the opt-in "bf16x3" (every product emulated
        by six bf16 MFMA products of three-way operand splits, fp32 accumulation: fp32-class error, ~2x the throughput,
        inference only, the shipped 64- / 128- / 256-wide shapes).  force_generic: bind to the generic-shape kernel family even where a tuned
        kernel exists for the shape (NM_KERNEL_GENERIC: a cross-check, same results bit for bit)."""
        lib = _lib.load()
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, got {precision!r}")
        self.precision = precision
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.HipLibraryError("HipMLP needs a GPU device")
        L = int(desc["num_layers"])
        host = {}

        def arr(key):
            v = state[key]
            a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            host[key] = np.ascontiguousarray(a, dtype=np.float32)
            return C.c_void_p(host[key].ctypes.data)

        fx, fd = int(desc["num_encoding_fn_xyz"]), int(desc["num_encoding_fn_dir"])
        for key, n, log in (("encode_xyz.frequency_bands", fx, desc.get("log_sampling_xyz", True)),
                            ("encode_dir.frequency_bands", fd, desc.get("log_sampling_dir", True))):
            if key not in state:
                state = dict(state)
                state[key] = (2.0 ** torch.linspace(0.0, n - 1, n)) if log else torch.linspace(1.0, 2.0 ** (n - 1), n)
        d = MlpDesc(L, int(desc["hidden_size"]), int(desc["skip_step"]), fx, fd,
                    int(bool(desc.get("include_input_xyz", True))), int(bool(desc.get("include_input_dir", True))),
                    int(bool(desc.get("use_viewdirs", True))))
        xs_w = (C.c_void_p * (L - 1))(*[arr(f"layers_xyz.{i}.weight") for i in range(L - 1)])
        xs_b = (C.c_void_p * (L - 1))(*[arr(f"layers_xyz.{i}.bias") for i in range(L - 1)])
        if d.use_viewdirs:
            w = MlpWeights(arr("layer1.weight"), arr("layer1.bias"), xs_w, xs_b,
                           arr("layers_dir.0.weight"), arr("layers_dir.0.bias"),
                           arr("fc_alpha.weight"), arr("fc_alpha.bias"), arr("fc_rgb.weight"), arr("fc_rgb.bias"),
                           arr("fc_feat.weight"), arr("fc_feat.bias"),
                           arr("encode_xyz.frequency_bands"), arr("encode_dir.frequency_bands"))
        else:
            # models.py:77-79: the trunk ends in fc_out (4, H): rows 0..2 are the colour rows, row 3 the density row
            if precision != "f32":
                raise _lib.HipLibraryError("use_viewdirs=False networks run in fp32 only")
            arr("fc_out.weight"), arr("fc_out.bias")
            H = int(desc["hidden_size"])
            ow, ob = host["fc_out.weight"].ctypes.data, host["fc_out.bias"].ctypes.data
            w = MlpWeights(arr("layer1.weight"), arr("layer1.bias"), xs_w, xs_b, C.c_void_p(None), C.c_void_p(None),
                           C.c_void_p(ow + 3 * H * 4), C.c_void_p(ob + 3 * 4), C.c_void_p(ow), C.c_void_p(ob),
                           C.c_void_p(None), C.c_void_p(None),
                           arr("encode_xyz.frequency_bands"), arr("encode_dir.frequency_bands"))
        self._h = C.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        check(lib.nm_mlp_create_ex(C.byref(d), C.byref(w), idx, PRECISIONS[precision] | (0x100 if force_generic else 0),
                                   C.byref(self._h)), "nm_mlp_create_ex")
        self._lib = lib
        self.desc = dict(desc)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.nm_mlp_destroy(h)

    @property
    def handle(self):
        return self._h

    def refresh_count(self):
        return int(_lib.load().nm_mlp_refresh_count(self.handle))

    def kernel_variant(self):
        nw = C.c_int()
        return int(self._lib.nm_mlp_kernel_variant(self._h, C.byref(nw))), nw.value

    def flops_per_sample(self, density_only=False):
        return int(self._lib.nm_mlp_flops_per_sample(self._h, int(density_only)))

    def sample_points(self, points, dirs):
        points, dirs = _dev32(points, self.device, "points"), _dev32(dirs, self.device, "dirs")
        lead = points.shape[:-1]
        points, dirs = points.reshape(-1, 3), dirs.expand(*lead, 3).reshape(-1, 3).contiguous()
        out = torch.empty(points.shape[0], 4, dtype=torch.float32, device=self.device)
        check(self._lib.nm_mlp_sample_points(self._h, _ptr(points), _ptr(dirs), points.shape[0], _ptr(out), _stream()),
              "nm_mlp_sample_points")
        return out.reshape(*lead, 4)

    def sample_density(self, points):
        """Raw sigma (n,) of the points (..., 3) (nm_mlp_sample_density): grid_query(density_only=True)'s value for the same
        fp32 triple, at arbitrary positions (the super-sampled mesh's edge samples).  fp32 handles only."""
        points = _dev32(points, self.device, "points").reshape(-1, 3)
        out = torch.empty(points.shape[0], dtype=torch.float32, device=self.device)
        check(self._lib.nm_mlp_sample_density(self._h, _ptr(points), points.shape[0], _ptr(out), _stream()),
              "nm_mlp_sample_density")
        return out

    def density_gradient(self, points):
        """d sigma / d x (n, 3) of sample_density's raw sigma at the points (..., 3) (nm_mlp_density_grad): the taping forward
        and the delta chain of the training path, then one kernel through the encoding columns and the positional encoding.  A
        point's result depends on that point and the packed weights only (not on the count, its offset or the chunking).  fp32
        handles only."""
        points = _dev32(points, self.device, "points").reshape(-1, 3)
        n = points.shape[0]
        out = torch.empty(n, 3, dtype=torch.float32, device=self.device)
        nbytes = int(self._lib.nm_mlp_density_grad_workspace_bytes(self._h, n))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=self.device)
        check(self._lib.nm_mlp_density_grad(self._h, _ptr(points), n, _ptr(ws), max(nbytes, 0), _ptr(out), _stream()),
              "nm_mlp_density_grad")
        return out

    def eval_rays(self, origins, dirs, t):
        origins, dirs, t = (_dev32(x, self.device) for x in (origins, dirs, t))
        rays, samples = t.shape
        per_ray = int(origins.reshape(-1, 3).shape[0] == rays and rays > 1)
        out = torch.empty(rays, samples, 4, dtype=torch.float32, device=self.device)
        check(self._lib.nm_mlp_eval_rays(self._h, _ptr(origins), per_ray, _ptr(dirs), _ptr(t), rays, samples,
                                         _ptr(out), _stream()), "nm_mlp_eval_rays")
        return out

    def grid_query(self, ax0, ax1, ax2, first=0, count=None, density_only=True, out=None):
        ax = [_dev32(a, self.device) for a in (ax0, ax1, ax2)]
        n0, n1, n2 = (a.numel() for a in ax)
        count = n0 * n1 * n2 - first if count is None else count
        if out is None:
            out = torch.empty((count,) if density_only else (count, 4), dtype=torch.float32, device=self.device)
        check(self._lib.nm_mlp_grid_query(self._h, _ptr(ax[0]), _ptr(ax[1]), _ptr(ax[2]), n0, n1, n2, first, count,
                                          int(density_only), _ptr(out), _stream()), "nm_mlp_grid_query")
        return out


def ray_bundle(c2w, height, width, focal, first=0, count=None, device="cuda"):
    """get_ray_bundle on the GPU: (origin (3,) on `device`, dirs (count,3))."""
    lib = _lib.load()
    count = height * width - first if count is None else count
    pose = np.ascontiguousarray(np.asarray(c2w.detach().cpu() if isinstance(c2w, torch.Tensor) else c2w,
                                           dtype=np.float32)[:3, :4])
    dirs = torch.empty(count, 3, dtype=torch.float32, device=device)
    origin = np.zeros(3, dtype=np.float32)
    check(lib.nm_ray_bundle(pose.ctypes.data_as(_lib.c_float_p), height, width, float(focal), first, count,
                            _ptr(dirs), origin.ctypes.data_as(_lib.c_float_p), _stream()), "nm_ray_bundle")
    return torch.from_numpy(origin).to(device), dirs


def coarse_intervals(u, near, far, rays, lindisp=False):
    lib = _lib.load()
    u = _dev32(u)
    near, far = _dev32_small(near, u.device).reshape(-1), _dev32_small(far, u.device).reshape(-1)
    per_ray = int(near.numel() == rays and rays > 1)
    t = torch.empty(rays, u.numel(), dtype=torch.float32, device=u.device)
    check(lib.nm_coarse_intervals(_ptr(u), _ptr(near), _ptr(far), per_ray, int(lindisp), rays, u.numel(), _ptr(t),
                                  _stream()), "nm_coarse_intervals")
    return t


def _alloc_bundle(rays, samples, device, want=BUNDLE_FIELDS):
    shapes = dict(rgb_map=(rays, 3), depth_map=(rays,), weights=(rays, samples), mask_weights=(rays, samples),
                  acc_map=(rays,), disp_map=(rays,))
    tensors = {k: torch.empty(shapes[k], dtype=torch.float32, device=device) for k in want}
    out = BundleOut(*[_ptr(tensors.get(k)) for k in BUNDLE_FIELDS])
    return tensors, out


def composite(radiance, t, dirs, attenuation_threshold=1e-5, white_background=False, training=False):
    lib = _lib.load()
    radiance, t = _dev32(radiance), _dev32(t)
    dirs = _dev32(dirs, radiance.device)
    rays, samples = t.shape
    tensors, out = _alloc_bundle(rays, samples, radiance.device)
    check(lib.nm_composite(_ptr(radiance), _ptr(t), _ptr(dirs), rays, samples, float(attenuation_threshold),
                           int(white_background), int(training), C.byref(out), _stream()), "nm_composite")
    return tensors


def sample_pdf(t, weights, u):
    lib = _lib.load()
    t, weights = _dev32(t), _dev32(weights)
    u = _dev32(u, t.device)
    rays, coarse = t.shape
    out = torch.empty(rays, coarse + u.numel(), dtype=torch.float32, device=t.device)
    check(lib.nm_sample_pdf(_ptr(t), _ptr(weights), _ptr(u), rays, coarse, u.numel(), _ptr(out), _stream()),
          "nm_sample_pdf")
    return out


_workspaces = {}


def _workspace(nbytes, device):
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def render_rays(coarse, fine, origins, dirs, near, far, u_coarse, u_fine, lindisp=False, white_background=False,
                training=False, attenuation_threshold=1e-5):
    """NeRFModel.forward in one C call.  Returns (coarse dict, fine dict | None)."""
    lib = _lib.load()
    device = coarse.device
    origins, dirs = _dev32(origins, device, "origins").reshape(-1, 3), _dev32(dirs, device, "dirs").reshape(-1, 3)
    rays = dirs.shape[0]
    near, far = _dev32(near, device).reshape(-1), _dev32(far, device).reshape(-1)
    u_coarse = _dev32(u_coarse, device)
    sc = u_coarse.numel()
    nf = 0 if fine is None else int(u_fine.numel())
    u_f = None if fine is None else _dev32(u_fine, device)
    cfg = RenderCfg(sc, nf, int(lindisp), int(white_background), int(training), float(attenuation_threshold))
    ws = _workspace(int(lib.nm_render_workspace_bytes(rays, sc, nf)), device)
    ct, cout = _alloc_bundle(rays, sc, device)
    ft, fout = (None, None) if fine is None else _alloc_bundle(rays, sc + nf, device)
    per_ray_o = int(origins.shape[0] == rays and rays > 1)
    per_ray_b = int(near.numel() == rays and rays > 1)
    if rays == 0:      # an empty shard (more ranks than rays): empty bundles, no launch (zero-size tensors have no address to pass)
        return ct, ft
    check(lib.nm_render_rays(coarse.handle, fine.handle if fine is not None else None, C.byref(cfg), _ptr(origins),
                             per_ray_o, _ptr(dirs), _ptr(near), _ptr(far), per_ray_b, _ptr(u_coarse), _ptr(u_f),
                             rays, _ptr(ws), C.byref(cout), C.byref(fout) if fout is not None else None, _stream()),
          "nm_render_rays")
    return ct, ft


def make_view(c2w, height, width, focal, ndc_near=None):
    """nm_view from a (3|4, 4) camera-to-world matrix; ndc_near != None selects NDC rays (DataBundle.ndc uses 1.0)."""
    pose = np.ascontiguousarray(np.asarray(c2w.detach().cpu() if isinstance(c2w, torch.Tensor) else c2w,
                                           dtype=np.float32)[:3, :4]).reshape(-1)
    return _lib.View((C.c_float * 12)(*pose.tolist()), int(height), int(width), float(focal),
                     int(ndc_near is not None), float(ndc_near if ndc_near is not None else 1.0))


def view_rays(view, first=0, count=None, device="cuda"):
    """The rays nm_render_view generates, materialised: (origins (count,3), dirs (count,3))."""
    count = view.height * view.width - first if count is None else count
    o = torch.empty(count, 3, dtype=torch.float32, device=device)
    d = torch.empty(count, 3, dtype=torch.float32, device=device)
    check(_lib.load().nm_view_rays(C.byref(view), first, count, _ptr(o), _ptr(d), _stream()), "nm_view_rays")
    return o, d


def ndc_rays(height, width, focal, near, origins, dirs):
    """ndc_rays (nerf_helpers.py:280-307) on the GPU (nm_ndc_rays): origins (...,3) broadcastable to dirs (...,3)."""
    dirs = _dev32(dirs, name="rays_d")
    shape = dirs.shape
    d = dirs.reshape(-1, 3)
    origins = _dev32(origins, dirs.device, "rays_o")
    per_ray = origins.numel() != 3
    o = (origins.expand(shape).reshape(-1, 3) if per_ray else origins.reshape(1, 3)).contiguous()
    oo, od = torch.empty_like(d), torch.empty_like(d)
    check(_lib.load().nm_ndc_rays(int(height), int(width), float(focal), float(near), _ptr(o), int(per_ray), _ptr(d),
                                  d.shape[0], _ptr(oo), _ptr(od), _stream()), "nm_ndc_rays")
    return oo.reshape(shape), od.reshape(shape)


def positional_encoding(x, bands, include_input=True):
    """PositionalEncoding.forward (modules.py:26-34) on the GPU (nm_positional_encoding)."""
    x = _dev32(x, name="x")
    lead, dim = x.shape[:-1], x.shape[-1]
    b = np.ascontiguousarray(np.asarray(bands.detach().cpu() if isinstance(bands, torch.Tensor) else bands,
                                        dtype=np.float32))
    flat = x.reshape(-1, dim)
    out = torch.empty(flat.shape[0], 2 * dim * b.size + (dim if include_input else 0), dtype=torch.float32, device=x.device)
    check(_lib.load().nm_positional_encoding(_ptr(flat), flat.shape[0], dim, b.ctypes.data_as(_lib.c_float_p), b.size,
                                             int(bool(include_input)), _ptr(out), _stream()), "nm_positional_encoding")
    return out.reshape(*lead, out.shape[-1])


def render_view(coarse, fine, view, near, far, u_coarse, u_fine, first=0, count=None, lindisp=False,
                white_background=False, training=False, attenuation_threshold=1e-5):
    """NeRFModel.forward on rays generated in the kernels from the camera pose (nm_render_view): pixels
    [first, first+count) of `view` (hip_ops.make_view).  Returns (coarse dict, fine dict | None)."""
    lib = _lib.load()
    device = coarse.device
    count = view.height * view.width - first if count is None else count
    near, far = _dev32(near, device).reshape(-1), _dev32(far, device).reshape(-1)
    u_coarse = _dev32(u_coarse, device)
    sc = u_coarse.numel()
    nf = 0 if fine is None else int(u_fine.numel())
    u_f = None if fine is None else _dev32(u_fine, device)
    cfg = RenderCfg(sc, nf, int(lindisp), int(white_background), int(training), float(attenuation_threshold))
    ws = _workspace(int(lib.nm_render_workspace_bytes(count, sc, nf)), device)
    ct, cout = _alloc_bundle(count, sc, device)
    ft, fout = (None, None) if fine is None else _alloc_bundle(count, sc + nf, device)
    per_ray_b = int(near.numel() == count and count > 1)
    check(lib.nm_render_view(coarse.handle, fine.handle if fine is not None else None, C.byref(cfg), C.byref(view),
                             first, count, _ptr(near), _ptr(far), per_ray_b, _ptr(u_coarse), _ptr(u_f), _ptr(ws),
                             C.byref(cout), C.byref(fout) if fout is not None else None, _stream()), "nm_render_view")
    return ct, ft


def mlp_profile_enable(on=True):
    check(_lib.load().nm_mlp_profile_enable(int(on)), "nm_mlp_profile_enable")


def mlp_profile_read():
    """(launches, total kernel ms, total EXECUTED flops) of the fused-MLP launches since the last read: the algorithmic count
    minus what the render path's skipped tiles (workgroup tiles without density: no fc_feat, view layer, fc_rgb) did not run."""
    n, ms, fl = C.c_int64(), C.c_double(), C.c_double()
    check(_lib.load().nm_mlp_profile_read(C.byref(n), C.byref(ms), C.byref(fl)), "nm_mlp_profile_read")
    return n.value, ms.value, fl.value


def mlp_profile_read_tiles():
    """mlp_profile_read() and the two tile counts of the stretch: (launches, kernel ms, executed flops, skipped tiles,
    terminated tiles).  A skipped tile (no sample with density) ran the trunk and the density head only; a terminated one
    (every ray of it behind transmittance 0: the render calls' ray termination) ran nothing."""
    n, ms, fl, sk, dead = C.c_int64(), C.c_double(), C.c_double(), C.c_int64(), C.c_int64()
    check(_lib.load().nm_mlp_profile_read_tiles(C.byref(n), C.byref(ms), C.byref(fl), C.byref(sk), C.byref(dead)),
          "nm_mlp_profile_read_tiles")
    return n.value, ms.value, fl.value, sk.value, dead.value


def mlp_profile_read_skipped(model, samples):
    """mlp_profile_read() for a profiled stretch in which networks of `model`'s shape evaluated `samples` samples in full:
    (launches, kernel ms, executed flops, skipped tiles).  The library counts skipped tiles per launch and reports them as the
    flops they did not execute; a tile is `waves * 16` samples, and both counts are integers far below 2**53, so the division
    is exact.  The stretch must bracket exactly those evaluations (render calls of one network shape, say): any other
    profiled fused-MLP launch in it -- a density-only query, another shape -- makes the counts disagree, which raises."""
    n, ms, fl = mlp_profile_read()
    full, density = model.flops_per_sample(), model.flops_per_sample(True)
    per_tile = model.kernel_variant()[1] * 16 * (full - density)
    missing = int(samples) * full - int(round(fl))
    if missing < 0 or missing % per_tile:
        raise _lib.HipLibraryError(f"profiled flops {fl!r} do not match {samples} full evaluations minus whole skipped tiles")
    return n, ms, fl, missing // per_tile


TIE_ORDERS = {"stable": 0, "reference": 1}
BUFF_REFERENCE_MAX_VOXELS = 8192      # nm_buff_intersect_ex(NM_TIES_REFERENCE): sort keys of every voxel per ray in LDS


def buff_intersect(voxels, origins, dirs, near, far, samples, ids="stable"):
    """TreeSampling.batch_ray_voxel_intersect on the GPU (nm_buff_intersect_ex):
    (z (R,S) f32, voxel ids (R,S) i64, ray_mask (R,) bool).  ids="stable" (default): every id is the voxel its
    sample lies in; ids="reference": ties ordered as the reference's three unstable torch.sort calls order them on
    the CPU (libstdc++ introsort, evaluated wave-parallel in the kernel) -- the reference's ids bit for bit; what
    TreeSampling uses while training (tie_order="auto"), ~3x the stable order's time."""
    if ids not in TIE_ORDERS:
        raise ValueError(f"ids must be one of {sorted(TIE_ORDERS)}, got {ids!r}")
    lib = _lib.load()
    voxels = _dev32(voxels, name="voxels")
    dev = voxels.device
    origins, dirs = _dev32(origins, dev, "origins").reshape(-1, 3), _dev32(dirs, dev, "dirs").reshape(-1, 3)
    rays = dirs.shape[0]
    key = ("linspace", str(dev), int(samples))                    # tree.py:318; one H2D per (device, count), not per call
    u = _small_cache.get(key)
    if u is None:
        u = _small_cache[key] = torch.linspace(0, 1.0, samples).to(dev)
    z = torch.empty(rays, samples, dtype=torch.float32, device=dev)
    idx = torch.empty(rays, samples, dtype=torch.int64, device=dev)
    mask = torch.empty(rays, dtype=torch.uint8, device=dev)
    check(lib.nm_buff_intersect_ex(_ptr(voxels), voxels.shape[0], _ptr(origins),
                                   int(origins.shape[0] == rays and rays > 1), _ptr(dirs), float(near), float(far), _ptr(u),
                                   rays, samples, TIE_ORDERS[ids], _ptr(z), _ptr(idx), _ptr(mask), _stream()),
          "nm_buff_intersect_ex")
    return z, idx, mask.bool()


def buff_intersect_random(voxels, origins, dirs, near, far, u_pick, u_pos):
    """TreeSampling.batch_ray_voxel_intersect with `tree.use_random_sampling` (tree.py:280-297) on the GPU
    (nm_buff_intersect_random), as a function of the draws: u_pick (R,S) float64 -- what torch.multinomial consumes,
    one double per sample -- and u_pos (R,S) float32 (torch.rand_like).  Returns (z (R,S) f32 sorted, voxel ids (R,S)
    i64, ray_mask (R,) bool); rows of rays that cross no voxel are zero-filled (the caller overwrites them)."""
    lib = _lib.load()
    voxels = _dev32(voxels, name="voxels")
    dev = voxels.device
    origins, dirs = _dev32(origins, dev, "origins").reshape(-1, 3), _dev32(dirs, dev, "dirs").reshape(-1, 3)
    rays = dirs.shape[0]
    if not (isinstance(u_pick, torch.Tensor) and u_pick.is_cuda):
        raise _lib.HipLibraryError("u_pick must live in GPU memory; there is no CPU path")
    u_pick = u_pick.detach().to(device=dev, dtype=torch.float64).contiguous()
    u_pos = _dev32(u_pos, dev, "u_pos")
    if u_pick.dim() != 2 or u_pick.shape[0] != rays or tuple(u_pos.shape) != tuple(u_pick.shape):
        raise ValueError(f"u_pick / u_pos must both be (rays, samples) = ({rays}, S); got {tuple(u_pick.shape)}, {tuple(u_pos.shape)}")
    samples = u_pick.shape[1]
    z = torch.empty(rays, samples, dtype=torch.float32, device=dev)
    idx = torch.empty(rays, samples, dtype=torch.int64, device=dev)
    mask = torch.empty(rays, dtype=torch.uint8, device=dev)
    check(lib.nm_buff_intersect_random(_ptr(voxels), voxels.shape[0], _ptr(origins),
                                       int(origins.shape[0] == rays and rays > 1), _ptr(dirs), float(near), float(far),
                                       _ptr(u_pick), _ptr(u_pos), rays, samples, _ptr(z), _ptr(idx), _ptr(mask), _stream()),
          "nm_buff_intersect_random")
    return z, idx, mask.bool()


def tree_integrate(memm, counter, indices, weights, mask_weights):
    """TreeSampling.ray_batch_integration's arithmetic (nm_tree_integrate): updates `memm` (N,) in place from the
    (K,S) voxel ids / weights / visibility masks of the rays that hit the tree."""
    lib = _lib.load()
    memm = memm if (memm.is_cuda and memm.dtype == torch.float32 and memm.is_contiguous()) else None
    if memm is None:
        raise _lib.HipLibraryError("tree_integrate: memm must be a contiguous fp32 GPU tensor (updated in place)")
    dev = memm.device
    idx = indices.to(device=dev, dtype=torch.int64).contiguous()
    w, mw = _dev32(weights, dev, "weights"), _dev32(mask_weights, dev, "mask_weights")
    if not (idx.numel() == w.numel() == mw.numel()):
        raise ValueError("tree_integrate: indices / weights / mask_weights differ in size")
    ws = torch.empty(int(lib.nm_tree_workspace_bytes(memm.numel())), dtype=torch.uint8, device=dev)
    check(lib.nm_tree_integrate(_ptr(idx), _ptr(w), _ptr(mw), idx.numel(), memm.numel(), int(counter), _ptr(memm),
                                _ptr(ws), _stream()), "nm_tree_integrate")
    return memm


def np_stats(x):
    """numpy's fp32 statistics of a GPU tensor, bit for bit (nm_np_stats): dict(sum, mean, var, std, min, max) of python
    floats holding the fp32 values `x.cpu().numpy().sum() / .mean() / .var() / .std() / .min() / .max()` would give."""
    lib = _lib.load()
    x = _dev32(x, name="x").reshape(-1)
    if x.numel() == 0:
        raise ValueError("np_stats of an empty tensor")
    ws = torch.empty(int(lib.nm_np_stats_workspace_bytes(x.numel())), dtype=torch.uint8, device=x.device)
    out = np.zeros(6, dtype=np.float32)
    check(lib.nm_np_stats(_ptr(x), x.numel(), _ptr(ws), out.ctypes.data_as(_lib.c_float_p), _stream()), "nm_np_stats")
    return dict(zip(("sum", "mean", "var", "std", "min", "max"), (np.float32(v) for v in out)))


def np_stats_sharded(x_local, first, n_total, own_lo, own_hi, gather):
    """`np_stats` of an array of `n_total` elements that is spread over several ranks, numpy's fp32 result bit for bit
    (nm_np_chunk_sums / nm_np_finish).  `x_local` holds the global elements [first, first + x_local.numel()); this rank is
    responsible for the 8192-element chunks that START in [own_lo, own_hi) (their elements must be among the ones it
    holds: slabs carry a halo).  `gather(t)`: all-gather of a tensor with a ragged first dimension in rank order (identity
    on one rank); it is called once per pass (2 collectives in all).  Every rank returns the same dict."""
    lib = _lib.load()
    x = _dev32(x_local, name="x").reshape(-1)
    dev = x.device
    chunk = 8192
    chunks = int(lib.nm_np_chunk_count(int(n_total)))
    c_lo, c_hi = -(-int(own_lo) // chunk), min(-(-int(own_hi) // chunk), chunks)
    m = max(c_hi - c_lo, 0)
    out = np.zeros(6, dtype=np.float32)
    d_out = torch.empty(8, dtype=torch.float32, device=dev)
    mine = torch.empty(3, m + 1, dtype=torch.float32, device=dev)
    result = {}
    for second in (0, 1):
        if m:
            check(lib.nm_np_chunk_sums(_ptr(x), int(first), x.numel(), int(n_total), c_lo, c_hi, second,
                                       float(result.get("mean", 0.0)), _ptr(mine[0]), _ptr(mine[1]), _ptr(mine[2]), _stream()),
                  "nm_np_chunk_sums")
        # one gather per pass: the (sum, min, max) rows of a rank's chunks travel as one (m, 3) block
        nrows = 1 if second else 3
        packed = gather(mine[:nrows, :m].t().contiguous())
        if packed.shape[0] != chunks:
            raise RuntimeError(f"np_stats_sharded: the ranks cover {packed.shape[0]} of {chunks} chunks")
        rows = [packed[:, r].contiguous() for r in range(nrows)]
        check(lib.nm_np_finish(_ptr(rows[0]), _ptr(rows[1]) if not second else None, _ptr(rows[2]) if not second else None,
                               chunks, int(n_total), second, _ptr(d_out), out.ctypes.data_as(_lib.c_float_p), _stream()),
              "nm_np_finish")
        if not second:
            result.update(sum=np.float32(out[0]), mean=np.float32(out[1]), min=np.float32(out[4]), max=np.float32(out[5]))
        else:
            result.update(var=np.float32(out[2]), std=np.float32(out[3]))
    return result


def _mc_outputs(nv, nf, dev):
    """The four output arrays of a marching-cubes call as ONE allocation (256-byte aligned pieces): the host work between
    the count and the emit pass -- during which the GPU waits -- is two allocations and some integer arithmetic; the typed
    views are made after the kernels are launched.  Returns (buffer, device pointers, views())."""
    al = lambda b: (b + 255) & ~255
    sizes = (nv * 12, nf * 12, nv * 12, nv * 4)
    offs, total = [], 0
    for b in sizes:
        offs.append(total)
        total += al(b)
    out = torch.empty(max(total, 256), dtype=torch.uint8, device=dev)
    base = out.data_ptr()
    ptrs = tuple(C.c_void_p(base + o) for o in offs)

    def views():
        piece = lambda k, dt: out[offs[k]:offs[k] + sizes[k]].view(dt)
        return (piece(0, torch.float32).view(nv, 3), piece(1, torch.int32).view(nf, 3), piece(2, torch.float32).view(nv, 3),
                piece(3, torch.float32))

    return out, ptrs, views


def marching_cubes(volume, level, return_keys=False):
    """skimage.measure.marching_cubes(volume, level) on the GPU (nm_mc_count + nm_mc_emit).
    volume: (n0,n1,n2) fp32 CUDA tensor.  Returns (verts (V,3) f32, faces (F,3) i32, normals (V,3) f32,
    values (V,) f32) as CUDA tensors; raises ValueError / RuntimeError exactly where skimage does.
    return_keys: also return the (V,) int64 edge keys of the vertices (nm_mc_vertex_edges; see mc_edge_points)."""
    lib = _lib.load()
    if not isinstance(volume, torch.Tensor) or volume.dim() != 3:
        raise ValueError("Input volume should be a 3D tensor.")
    if min(volume.shape) < 2:
        raise ValueError("Input array must be at least 2x2x2.")
    vol = _dev32(volume, name="volume")
    level = float(level)
    n0, n1, n2 = vol.shape
    dev = vol.device
    ws = torch.empty(int(lib.nm_mc_workspace_bytes(n0, n1, n2)), dtype=torch.uint8, device=dev)
    nv, nf = C.c_int64(), C.c_int64()
    p_vol, p_ws, stream = _ptr(vol), _ptr(ws), _stream()       # the GPU idles between the two calls: nothing is looked up twice
    check(lib.nm_mc_count(p_vol, n0, n1, n2, level, p_ws, C.byref(nv), C.byref(nf), stream), "nm_mc_count")
    if nv.value == 0:
        # skimage checks the level against the data range first (ValueError) and only then finds no surface
        # (RuntimeError).  A level outside [min, max] cannot produce a vertex, so the 442 MB min/max pass is only
        # paid on this error path instead of on every call.
        lo, hi = (float(v) for v in torch.aminmax(vol))
        if level < lo or level > hi:
            raise ValueError("Surface level must be within volume data range.")
        raise RuntimeError("No surface found at the given iso value.")
    out, (p_verts, p_faces, p_normals, p_values), views = _mc_outputs(nv.value, nf.value, dev)
    scratch = torch.empty(int(lib.nm_mc_vertex_scratch_bytes(nv.value, nf.value)) + 256, dtype=torch.uint8, device=dev)
    check(lib.nm_mc_emit(p_vol, n0, n1, n2, level, p_ws, _ptr(scratch), nv.value, nf.value, p_verts, p_faces, p_normals,
                         p_values, stream), "nm_mc_emit")
    verts, faces, normals, values = views()
    if return_keys:
        keys = torch.empty(nv.value, dtype=torch.int64, device=dev)
        check(lib.nm_mc_vertex_edges(_ptr(scratch), nv.value, 0, n0, n1, n2, 0, _ptr(keys), stream), "nm_mc_vertex_edges")
        return verts, faces, normals, values, keys
    return verts, faces, normals, values


def marching_cubes_slab(volume, level, z_global, ghost_below, ghost_above):
    """Marching cubes of ONE axis-0 slab of a larger grid (nm_mc_count_slab / nm_mc_emit_slab).  `volume` holds the global
    planes [z_global, z_global + n0); its first cube layer is a ghost of the slab below (`ghost_below`), its last one a ghost
    of the slab above (`ghost_above`).  Returns an object with `.vertices` (the slab's own vertex count), `.faces`,
    `.ghost_vertices`, and `.emit(index_base)` -> (verts, faces, normals, values) with face entries = local id + index_base
    (`.emit(index_base, return_keys=True)` appends the (V,) int64 edge keys of the slab's own vertices, global voxel indices).
    Concatenating the ranks' arrays in rank order, with index_base = (own vertex counts of all lower ranks) - ghost_vertices,
    gives the mesh of the whole grid bit for bit (dist.marching_cubes_sharded does that)."""
    lib = _lib.load()
    if not isinstance(volume, torch.Tensor) or volume.dim() != 3:
        raise ValueError("Input volume should be a 3D tensor.")
    vol = _dev32(volume, name="volume")
    level = float(level)
    n0, n1, n2 = vol.shape
    dev = vol.device
    ws = torch.empty(int(lib.nm_mc_workspace_bytes(n0, n1, n2)), dtype=torch.uint8, device=dev)
    nv, nf, gv, gf = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    check(lib.nm_mc_count_slab(_ptr(vol), n0, n1, n2, level, int(z_global), int(bool(ghost_below)), int(bool(ghost_above)),
                               _ptr(ws), C.byref(nv), C.byref(nf), C.byref(gv), C.byref(gf), _stream()), "nm_mc_count_slab")

    class Slab:
        vertices, faces = nv.value - gv.value, nf.value - gf.value
        ghost_vertices, ghost_faces = gv.value, gf.value

        @staticmethod
        def emit(index_base, return_keys=False):
            verts = torch.empty(Slab.vertices, 3, dtype=torch.float32, device=dev)
            normals = torch.empty(Slab.vertices, 3, dtype=torch.float32, device=dev)
            values = torch.empty(Slab.vertices, dtype=torch.float32, device=dev)
            faces = torch.empty(Slab.faces, 3, dtype=torch.int32, device=dev)
            keys = torch.empty(Slab.vertices, dtype=torch.int64, device=dev)
            if nv.value:
                scratch = torch.empty(int(lib.nm_mc_vertex_scratch_bytes(nv.value, nf.value)) + 256, dtype=torch.uint8, device=dev)
                check(lib.nm_mc_emit_slab(_ptr(vol), n0, n1, n2, level, int(z_global), int(bool(ghost_below)), int(bool(ghost_above)),
                                          _ptr(ws), _ptr(scratch), nv.value, nf.value, gv.value, gf.value, int(index_base),
                                          _ptr(verts), _ptr(faces), _ptr(normals), _ptr(values), _stream()), "nm_mc_emit_slab")
                if return_keys:
                    check(lib.nm_mc_vertex_edges(_ptr(scratch), nv.value, gv.value, n0, n1, n2, int(z_global), _ptr(keys), _stream()),
                          "nm_mc_vertex_edges")
            if return_keys:
                return verts, faces, normals, values, keys
            return verts, faces, normals, values

    return Slab


SS_MAX = 64


def fine_axis(limit, n, ss):
    """The fine axis of super-sampling ss over a base axis of n points: linspace(-limit, limit, (n-1)*(ss+1)+1) in fp32 on the
    host, as mesh_nerf._axes builds the base axes; base point i is fine point i*(ss+1) (up to fp32 rounding of linspace)."""
    return torch.linspace(-limit, limit, (n - 1) * (ss + 1) + 1)


def check_super_sampling(nums, ss):
    """ValueError unless 1 <= ss <= 64 and every fine axis fits int32."""
    if not 1 <= int(ss) <= SS_MAX:
        raise ValueError(f"--super-sampling must be in [1, {SS_MAX}] (0 = off), got {ss}")
    if any((n - 1) * (ss + 1) + 1 > 2 ** 31 - 1 for n in nums):
        raise ValueError(f"--super-sampling {ss}: a fine axis of the grid {tuple(nums)} does not fit int32")


def mc_edge_points(keys, nums, ss, base, fine):
    """(V, ss, 3) fp32: the ss interior samples of every vertex's edge (nm_mc_edge_points).  keys: (V,) int64 of a global
    (n0,n1,n2) grid; base / fine: the three base / fine axes (any device; copied to the keys' device)."""
    lib = _lib.load()
    dev = keys.device
    n0, n1, n2 = (int(n) for n in nums)
    V = int(keys.numel())
    base = [_dev32(a, dev) for a in base]
    fine = [_dev32(a, dev) for a in fine]
    if [a.numel() for a in base] != [n0, n1, n2] or [a.numel() for a in fine] != [(n - 1) * (ss + 1) + 1 for n in (n0, n1, n2)]:
        raise ValueError("mc_edge_points: axis lengths do not match the grid and the super-sampling")
    points = torch.empty(V, ss, 3, dtype=torch.float32, device=dev)
    keys = keys.contiguous()
    check(lib.nm_mc_edge_points(_ptr(keys), V, n0, n1, n2, int(ss), *[_ptr(a) for a in base], *[_ptr(a) for a in fine],
                                _ptr(points), _stream()), "nm_mc_edge_points")
    return points


def mc_refine_vertices(volume, z_global, level, keys, ss, fine_sigma, verts):
    """Moves every edge vertex of `verts` (V,3) fp32 (grid-index units, in place) along its edge to the first sign change of
    (volume, fine_sigma (V, ss), volume) against `level` (nm_mc_refine_vertices).  `volume` holds the global planes
    [z_global, z_global + n0).  ss = 0 reproduces marching_cubes' own vertices.  Returns verts."""
    lib = _lib.load()
    vol = _dev32(volume, name="volume")
    n0, n1, n2 = vol.shape
    if verts.dtype != torch.float32 or not verts.is_contiguous() or verts.device != vol.device:
        raise ValueError("mc_refine_vertices: verts must be a contiguous fp32 tensor on the volume's device")
    V = int(keys.numel())
    if verts.shape != (V, 3) or (ss and tuple(fine_sigma.shape[:1]) != (V,)):
        raise ValueError("mc_refine_vertices: keys, fine_sigma and verts disagree on the vertex count")
    sig = _dev32(fine_sigma, vol.device).reshape(V, ss) if ss else None
    keys = keys.contiguous()
    check(lib.nm_mc_refine_vertices(_ptr(vol), n0, n1, n2, int(z_global), float(level), _ptr(keys), V, int(ss), _ptr(sig),
                                    _ptr(verts), _stream()), "nm_mc_refine_vertices")
    return verts


KEEP_LARGEST_MAX = 1024


def _mesh_faces(faces, num_vertices):
    """(F,3) contiguous int32 faces on the GPU + the two sizes, checked."""
    if not isinstance(faces, torch.Tensor) or not faces.is_cuda:
        raise _lib.HipLibraryError("faces must live in GPU memory; there is no CPU path")
    if faces.dtype is not torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces must be an (F,3) int32 tensor, got {tuple(faces.shape)} {faces.dtype}")
    nv, nf = int(num_vertices), int(faces.shape[0])
    if nv < 0 or (nf and not nv):
        raise ValueError(f"a mesh of {nf} faces over {nv} vertices")
    return faces.detach().contiguous(), nv, nf


def _mesh_inputs(what, verts, faces, normals=None, values=None, keys=None):
    """The opening of the wrapper `what`: the checked faces (_mesh_faces) and, on their device, contiguous, the (V,3) f32 vertices
    and whichever of normals (V,3) f32, values (V,) f32 and keys (V,) i64 came, all of the same V.
    -> (verts, faces, normals, values, keys, nv, nf, device)"""
    faces, nv, nf = _mesh_faces(faces, verts.shape[0])
    dev = faces.device
    verts = _dev32(verts, dev, "verts")
    normals = _dev32(normals, dev, "normals") if normals is not None else None
    values = _dev32(values, dev, "values") if values is not None else None
    if keys is not None:
        if keys.dtype is not torch.int64 or keys.device != dev:
            raise ValueError("keys must be an int64 tensor on the faces' device")
        keys = keys.contiguous()
    if verts.shape != (nv, 3) or (normals is not None and normals.shape != (nv, 3)) or \
            (values is not None and values.shape != (nv,)) or (keys is not None and keys.shape != (nv,)):
        raise ValueError(f"{what}: the per-vertex arrays disagree on the vertex count")
    return verts, faces, normals, values, keys, nv, nf, dev


def _mesh_subset_outputs(kv, kf, dev, normals=None, values=None, keys=None):
    """What a _compact / _emit entry fills: kv vertices, kf faces and a row array for each per-vertex input that came.
    -> (verts, faces, normals, values, keys)"""
    return (torch.empty(kv, 3, dtype=torch.float32, device=dev), torch.empty(kf, 3, dtype=torch.int32, device=dev),
            torch.empty(kv, 3, dtype=torch.float32, device=dev) if normals is not None else None,
            torch.empty(kv, dtype=torch.float32, device=dev) if values is not None else None,
            torch.empty(kv, dtype=torch.int64, device=dev) if keys is not None else None)


def _mesh_check(lib, rc, what):
    """status of a nm_mesh_* entry: 2 (an argument the entry refuses) is the caller's ValueError, in the entry's own words"""
    if rc == 2:
        raise ValueError((lib.nm_last_error() or f"{what}: bad argument".encode()).decode())
    check(rc, what)


def _mesh_workspace(nbytes, what, nv, nf, device):
    """the workspace of a mesh entry; its *_workspace_bytes gives 0 for sizes the entry refuses"""
    if nbytes == 0:
        raise ValueError(f"{what}: {nv} vertices / {nf} faces are beyond the supported sizes")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _mesh_components(lib, faces, nv, nf):
    dev = faces.device
    labels = torch.empty(nv, dtype=torch.int32, device=dev)
    counts = torch.empty(nv, dtype=torch.int32, device=dev)
    ws = _mesh_workspace(int(lib.nm_mesh_components_workspace_bytes(nv, nf)), "mesh components", nv, nf, dev)
    check(lib.nm_mesh_components(_ptr(faces), nf, nv, _ptr(labels), _ptr(counts), _ptr(ws), _stream()), "nm_mesh_components")
    return labels, counts, ws


def mesh_components(faces, num_vertices):
    """Connected components of an indexed triangle mesh (nm_mesh_components; semantics in include/nerfmeshes_hip.h).
    faces: (F,3) int32 CUDA tensor with entries in [0, num_vertices) -> (labels (V,) int32: every vertex's component, named by
    its smallest vertex index; face_counts (V,) int32: the component's number of triangles at that index, 0 elsewhere).
    Raises ValueError for a face index out of range (the one read-back of this call)."""
    lib = _lib.load()
    faces, nv, nf = _mesh_faces(faces, num_vertices)
    labels, counts, ws = _mesh_components(lib, faces, nv, nf)
    bad = int(ws[:8].view(torch.int64).item())
    if bad:
        raise ValueError(f"mesh components: {bad} faces have a vertex index outside [0, {nv})")
    return labels, counts


def mesh_filter_components(verts, faces, normals, values=None, keys=None, min_faces=0, keep_largest=0):
    """Drops whole components of a mesh (nm_mesh_components + _select + _compact): those with fewer than `min_faces` triangles,
    and, with keep_largest = K > 0, all but the K with most triangles of the rest (ties to the smaller label; fewer than K:
    all of them).  verts (V,3) f32, faces (F,3) i32, normals (V,3) f32, values (V,) f32 or None, keys (V,) i64 or None, all on
    the GPU -> (verts, faces, normals, values, keys, info): the kept rows in their original order, faces renumbered
    (numpy: new = cumsum(keep_v) - 1; new[faces[keep_f]]), None where None came in; info = dict(components, components_kept,
    faces, faces_kept, vertices, vertices_kept).  Nothing left gives empty (0,3) arrays."""
    lib = _lib.load()
    min_faces, keep_largest = int(min_faces), int(keep_largest)
    if min_faces < 0 or keep_largest < 0:
        raise ValueError("min_faces and keep_largest must be >= 0")
    if keep_largest > KEEP_LARGEST_MAX:
        raise ValueError(f"keep_largest is at most {KEEP_LARGEST_MAX}, got {keep_largest}")
    verts, faces, normals, values, keys, nv, nf, dev = _mesh_inputs("mesh_filter_components", verts, faces, normals, values, keys)
    labels, counts, ws = _mesh_components(lib, faces, nv, nf)
    kv, kf, comps, kept = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    rc = lib.nm_mesh_components_select(_ptr(faces), nf, nv, _ptr(labels), _ptr(counts), min_faces, keep_largest, _ptr(ws),
                                       C.byref(kv), C.byref(kf), C.byref(comps), C.byref(kept), _stream())
    _mesh_check(lib, rc, "nm_mesh_components_select")
    out_verts, out_faces, out_normals, out_values, out_keys = _mesh_subset_outputs(kv.value, kf.value, dev, normals, values, keys)
    if kv.value:
        check(lib.nm_mesh_components_compact(_ptr(ws), _ptr(faces), nf, nv, _ptr(verts), _ptr(normals), _ptr(values), _ptr(keys),
                                             kv.value, kf.value, _ptr(out_verts), _ptr(out_faces), _ptr(out_normals),
                                             _ptr(out_values), _ptr(out_keys), _stream()), "nm_mesh_components_compact")
    info = dict(components=comps.value, components_kept=kept.value, faces=nf, faces_kept=kf.value, vertices=nv,
                vertices_kept=kv.value)
    return out_verts, out_faces, out_normals, out_values, out_keys, info


SIMPLIFY_CELLS = 1 << 21                 # cells per axis of the clustering grid (nm_mesh_simplify_cluster)
SIMPLIFY_AGGREGATE = False               # wave aggregation of equal clusters before the atomics: the same bytes, another speed
                                         # (tests/tools/time_mesh_simplify.py measures both)


SIMPLIFY_QUADRIC_AGGREGATE = True        # the same for the face pass of placement="quadric": nine 64-bit adds per corner land in
                                         # rows that wave-mates share, and aggregation takes that pass from 2.4 -- 2.6 ms to
                                         # 1.0 -- 1.4 (tests/tools/time_mesh_simplify_quadric.py)
SIMPLIFY_PLACEMENTS = ("mean", "quadric")
SIMPLIFY_QUADRIC_COUNTS = ("quadric_clusters", "crowded_clusters", "singular_clusters", "clamped_clusters", "far_corners")


SIMPLIFY_MAX_LEVELS = 8                  # NM_MESH_SIMPLIFY_MAX_LEVELS
SIMPLIFY_LEVEL_FIELDS = ("level_vertices", "level_clusters", "refused_error", "refused_crowded", "refused_singular",
                         "refused_far", "refused_empty")         # NM_MESH_SIMPLIFY_LEVEL_* order; then the largest d2's bits
SIMPLIFY_ADAPTIVE_KEYS = ("levels",) + SIMPLIFY_LEVEL_FIELDS + ("level_kept", "largest_error")


def _simplify_adaptive(lib, verts, faces, normals, nv, nf, dev, cell, origin, aggregate, levels, max_error):
    """mesh_simplify with levels > 0: nm_mesh_simplify_adaptive_level for level = levels .. 0, then _faces (the counts; the
    first read-back) and _emit (the second)."""
    ws = _mesh_workspace(int(lib.nm_mesh_simplify_workspace_bytes(nv, nf)), "mesh simplify", nv, nf, dev)
    quadrics = _mesh_workspace(int(lib.nm_mesh_simplify_quadric_workspace_bytes(nv, nf)), "mesh simplify", nv, nf, dev)
    staged = _mesh_workspace(int(lib.nm_mesh_simplify_adaptive_workspace_bytes(nv, nf)), "mesh simplify", nv, nf, dev)
    flags = (1 if (SIMPLIFY_AGGREGATE if aggregate is None else aggregate) else 0) | \
            (2 if (SIMPLIFY_QUADRIC_AGGREGATE if aggregate is None else aggregate) else 0)
    for level in range(levels, -1, -1):
        rc = lib.nm_mesh_simplify_adaptive_level(_ptr(verts), nv, _ptr(faces), nf, _ptr(normals), *origin, cell, level, levels,
                                                 max_error, flags, _ptr(ws), _ptr(quadrics), _ptr(staged), _stream())
        _mesh_check(lib, rc, "nm_mesh_simplify_adaptive_level")
    fields = len(SIMPLIFY_LEVEL_FIELDS) + 1
    counts = (C.c_int64 * (7 + (SIMPLIFY_MAX_LEVELS + 1) * fields))()
    rc = lib.nm_mesh_simplify_adaptive_faces(_ptr(faces), nf, nv, levels, _ptr(ws), _ptr(staged), counts, _stream())
    _mesh_check(lib, rc, "nm_mesh_simplify_adaptive_faces")
    clusters, kv, kf, degenerate, duplicate, bad_v, bad_f = (int(x) for x in counts[:7])
    if bad_v:
        raise ValueError(f"mesh simplify: {bad_v} vertices have a non-finite coordinate or a cell index outside [0, {SIMPLIFY_CELLS})")
    if bad_f:
        raise ValueError(f"mesh simplify: {bad_f} faces have a vertex index outside [0, {nv})")
    out_verts, out_faces, out_normals, _, _ = _mesh_subset_outputs(kv, kf, dev, normals)
    tally = (C.c_int64 * (len(SIMPLIFY_QUADRIC_COUNTS) + SIMPLIFY_MAX_LEVELS + 1))()
    rc = lib.nm_mesh_simplify_adaptive_emit(_ptr(ws), _ptr(staged), _ptr(faces), nf, nv, levels, int(normals is not None), kv, kf,
                                            _ptr(out_verts), _ptr(out_faces), _ptr(out_normals), tally, _stream())
    _mesh_check(lib, rc, "nm_mesh_simplify_adaptive_emit")
    info = dict(vertices=nv, faces=nf, clusters=clusters, vertices_kept=kv, faces_kept=kf, degenerate_faces=degenerate,
                duplicate_faces=duplicate)
    info.update(zip(SIMPLIFY_QUADRIC_COUNTS, (int(x) for x in tally)))
    rows = [[int(x) for x in counts[7 + l * fields:7 + (l + 1) * fields]] for l in range(levels + 1)]
    info["levels"] = levels
    for k, name in enumerate(SIMPLIFY_LEVEL_FIELDS):
        info[name] = tuple(row[k] for row in rows)
    info["level_kept"] = tuple(int(x) for x in tally[len(SIMPLIFY_QUADRIC_COUNTS):len(SIMPLIFY_QUADRIC_COUNTS) + levels + 1])
    # the largest error of a chosen cluster in the units of `cell`: sqrt(d2) lattice units of 1 / 2^8 of that level's cell
    largest = 0.0
    for l in range(1, levels + 1):
        d2 = struct.unpack("<d", struct.pack("<q", rows[l][-1]))[0]
        largest = max(largest, math.sqrt(d2) / 256.0 * (cell * 2.0 ** l))
    info["largest_error"] = largest
    return out_verts, out_faces, out_normals, info


def mesh_simplify(verts, faces, normals=None, cell=None, origin=None, aggregate=None, placement="mean", levels=0, max_error=None):
    """Vertex clustering on the device (nm_mesh_simplify_cluster + _emit; semantics in include/nerfmeshes_hip.h): the vertices in
    one cell of the grid (origin, cell) become one vertex -- the exact mean of its members, a single member unchanged bit for bit
    --, degenerate and duplicate faces go (opposite windings are not duplicates), and so do the clusters no face is left on.
    verts (V,3) f32, faces (F,3) i32, normals (V,3) f32 or None, all on the GPU; cell: the cell edge (> 0, finite); origin: three
    floats, None = the per-axis minimum of the vertices.  -> (verts, faces, normals, info): kept faces in input order, vertices
    by ascending smallest member index, normals None where None came in; info = dict(vertices, faces, clusters, vertices_kept,
    faces_kept, degenerate_faces, duplicate_faces).  Nothing left gives empty (0,3) arrays.  Raises ValueError for a vertex with
    a non-finite coordinate or beyond 2^21 cells from the origin and for a face index out of range (the one read-back).
    placement="quadric" (nm_mesh_simplify_quadric_faces + _emit_quadric) puts a cluster of two or more members at the point of
    its cell nearest to the planes of the faces around it, from exact integer quadrics, instead of at the mean -- the same
    faces, numbering and normals -- and adds to info the kept clusters placed so (quadric_clusters, the clamped_clusters among
    them moved back into their cell), those left at the mean (crowded_clusters: more than 2^13 face corners; singular_clusters)
    and far_corners, the face corners with an edge longer than two cells, which contribute nothing.
    levels = L > 0 (at most 8; placement="quadric" only) with max_error = E >= 0 in the units of `cell` (inf allowed) is adaptive
    clustering (nm_mesh_simplify_adaptive_*): the same clustering on the nested grids of cell * 2^l, l = 0 .. L, every vertex in
    the coarsest cell whose quadric vertex lies within E of every triangle plane around it, level 0 always allowed.  info gains
    levels, per level (tuples of L + 1) level_vertices, level_clusters, the clusters refused there by reason (refused_error,
    refused_crowded, refused_singular, refused_far, refused_empty) and level_kept, and largest_error, the largest plane distance
    of a chosen cluster of a level >= 1 in the units of `cell`; the quadric counts are of the kept clusters at their level.
    levels = 0 is the call without the two arguments, whatever max_error is."""
    if placement not in SIMPLIFY_PLACEMENTS:
        raise ValueError(f"mesh_simplify: placement must be one of {SIMPLIFY_PLACEMENTS}, got {placement!r}")
    if cell is None:
        raise ValueError("mesh_simplify: the cell size is required")
    cell = float(np.float32(cell))
    if not (np.isfinite(cell) and cell > 0):
        raise ValueError(f"mesh_simplify: the cell size must be finite and > 0, got {cell}")
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 0 <= levels <= SIMPLIFY_MAX_LEVELS:
        raise ValueError(f"mesh_simplify: levels must be an integer in [0, {SIMPLIFY_MAX_LEVELS}], got {levels!r}")
    levels = int(levels)
    if levels:
        if placement != "quadric":
            raise ValueError(f"mesh_simplify: levels = {levels} needs placement='quadric', got {placement!r}")
        if max_error is None:
            raise ValueError("mesh_simplify: max_error is required with levels > 0")
        max_error = float(max_error)
        if not max_error >= 0.0:
            raise ValueError(f"mesh_simplify: max_error must be >= 0, got {max_error}")
        if cell * 2.0 ** levels > float(np.finfo(np.float32).max):
            raise ValueError(f"mesh_simplify: the coarsest cell size {cell} * 2^{levels} must be finite")
    lib = _lib.load()
    verts, faces, normals, _, _, nv, nf, dev = _mesh_inputs("mesh_simplify", verts, faces, normals)
    if origin is None:
        # the minimum of the finite coordinates: a NaN or infinite vertex is reported below with its count, not as a bad origin
        low = torch.where(torch.isfinite(verts), verts, torch.full_like(verts, float("inf"))).min(dim=0).values if nv else None
        origin = [x if np.isfinite(x) else 0.0 for x in low.tolist()] if nv else (0.0, 0.0, 0.0)
    origin = [float(np.float32(x)) for x in (origin.tolist() if isinstance(origin, (torch.Tensor, np.ndarray)) else origin)]
    if len(origin) != 3 or not all(np.isfinite(x) for x in origin):
        raise ValueError(f"mesh_simplify: the origin must be three finite numbers, got {origin}")
    if levels:
        return _simplify_adaptive(lib, verts, faces, normals, nv, nf, dev, cell, origin, aggregate, levels, max_error)
    ws = _mesh_workspace(int(lib.nm_mesh_simplify_workspace_bytes(nv, nf)), "mesh simplify", nv, nf, dev)
    counts = (C.c_int64 * 7)()
    flags = 1 if (SIMPLIFY_AGGREGATE if aggregate is None else aggregate) else 0
    rc = lib.nm_mesh_simplify_cluster(_ptr(verts), nv, _ptr(faces), nf, _ptr(normals), *origin, cell, flags, _ptr(ws), counts,
                                      _stream())
    _mesh_check(lib, rc, "nm_mesh_simplify_cluster")
    clusters, kv, kf, degenerate, duplicate, bad_v, bad_f = (int(x) for x in counts)
    if bad_v:
        raise ValueError(f"mesh simplify: {bad_v} vertices have a non-finite coordinate or a cell index outside [0, {SIMPLIFY_CELLS})")
    if bad_f:
        raise ValueError(f"mesh simplify: {bad_f} faces have a vertex index outside [0, {nv})")
    out_verts, out_faces, out_normals, _, _ = _mesh_subset_outputs(kv, kf, dev, normals)
    info = dict(vertices=nv, faces=nf, clusters=clusters, vertices_kept=kv, faces_kept=kf, degenerate_faces=degenerate,
                duplicate_faces=duplicate)
    if placement == "quadric":
        quadrics = _mesh_workspace(int(lib.nm_mesh_simplify_quadric_workspace_bytes(nv, nf)), "mesh simplify", nv, nf, dev)
        face_flags = 1 if (SIMPLIFY_QUADRIC_AGGREGATE if aggregate is None else aggregate) else 0
        rc = lib.nm_mesh_simplify_quadric_faces(_ptr(ws), _ptr(verts), nv, _ptr(faces), nf, *origin, cell, face_flags,
                                                _ptr(quadrics), _stream())
        _mesh_check(lib, rc, "nm_mesh_simplify_quadric_faces")
        tally = (C.c_int64 * len(SIMPLIFY_QUADRIC_COUNTS))()
        rc = lib.nm_mesh_simplify_emit_quadric(_ptr(ws), _ptr(quadrics), _ptr(verts), nv, _ptr(faces), nf, _ptr(normals), *origin,
                                               cell, kv, kf, _ptr(out_verts), _ptr(out_faces), _ptr(out_normals), tally, _stream())
        _mesh_check(lib, rc, "nm_mesh_simplify_emit_quadric")
        info.update(zip(SIMPLIFY_QUADRIC_COUNTS, (int(x) for x in tally)))
    elif kv:
        check(lib.nm_mesh_simplify_emit(_ptr(ws), _ptr(verts), nv, _ptr(faces), nf, _ptr(normals), *origin, cell, kv, kf,
                                        _ptr(out_verts), _ptr(out_faces), _ptr(out_normals), _stream()), "nm_mesh_simplify_emit")
    return out_verts, out_faces, out_normals, info


SMOOTH_MAX_ITERATIONS = 1000
SMOOTH_FREE_BOUNDARY = 1                 # NM_MESH_SMOOTH_FREE_BOUNDARY


def mesh_smooth(verts, faces, normals=None, iterations=10, lam=0.5, mu=-0.53, free_boundary=False, flip=None):
    """Taubin's lambda | mu smoothing on the device (nm_mesh_smooth_build + _run + nm_mesh_vertex_normals; semantics in
    include/nerfmeshes_hip.h): `iterations` times a uniform umbrella half-step with factor lam in (0, 1], then one with mu in
    [-1, 0] (mu = 0: plain Laplacian smoothing).  Boundary vertices -- the ends of an edge on exactly one face -- stay where
    they are unless free_boundary; a vertex on no edge never moves.  verts (V,3) f32, faces (F,3) i32, normals (V,3) f32 or
    None, all on the GPU.  -> (verts, normals, info): the same numbering; normals are the area-independent sum of the unit
    face normals of the RESULT times flip (+1: the winding's own side; -1: the other, which is the side marching cubes'
    normals point to), a vertex without one keeping its input normal (or zero) -- None where None came in and no flip was
    asked for (flip=None, which is +1 where normals came); info = dict(vertices, faces, edges, boundary_edges,
    nonmanifold_edges, boundary_vertices, isolated_vertices, degenerate_faces, exponent).  Raises ValueError for a vertex
    with a non-finite coordinate and for a face index out of range (the one read-back)."""
    lib = _lib.load()
    iterations = int(iterations)
    lam, mu = float(np.float32(lam)), float(np.float32(mu))
    if not 0 <= iterations <= SMOOTH_MAX_ITERATIONS:
        raise ValueError(f"mesh_smooth: iterations must be in [0, {SMOOTH_MAX_ITERATIONS}], got {iterations}")
    if not 0.0 < lam <= 1.0:
        raise ValueError(f"mesh_smooth: lam must be in (0, 1], got {lam}")
    if not -1.0 <= mu <= 0.0:
        raise ValueError(f"mesh_smooth: mu must be in [-1, 0], got {mu}")
    if flip not in (None, 1, -1):
        raise ValueError(f"mesh_smooth: flip must be +1 or -1, got {flip}")
    verts, faces, normals, _, _, nv, nf, dev = _mesh_inputs("mesh_smooth", verts, faces, normals)
    ws = _mesh_workspace(int(lib.nm_mesh_smooth_workspace_bytes(nv, nf)), "mesh smooth", nv, nf, dev)
    counts = (C.c_int64 * 9)()
    _mesh_check(lib, lib.nm_mesh_smooth_build(_ptr(verts), nv, _ptr(faces), nf, _ptr(ws), counts, _stream()), "nm_mesh_smooth_build")
    edges, boundary_edges, nonmanifold, boundary_vertices, isolated, degenerate, bad_v, bad_f, exponent = (int(x) for x in counts)
    if bad_v:
        raise ValueError(f"mesh smooth: {bad_v} vertices have a non-finite coordinate")
    if bad_f:
        raise ValueError(f"mesh smooth: {bad_f} faces have a vertex index outside [0, {nv})")
    out_verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    flags = SMOOTH_FREE_BOUNDARY if free_boundary else 0
    _mesh_check(lib, lib.nm_mesh_smooth_run(_ptr(ws), _ptr(verts), nv, iterations, lam, mu, flags, _ptr(out_verts), _stream()),
                "nm_mesh_smooth_run")
    out_normals = None
    if normals is not None or flip is not None:
        out_normals = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        _mesh_check(lib, lib.nm_mesh_vertex_normals(_ptr(out_verts), nv, _ptr(faces), nf, _ptr(normals), 1 if flip is None else flip,
                                                    _ptr(ws), _ptr(out_normals), _stream()), "nm_mesh_vertex_normals")
    info = dict(vertices=nv, faces=nf, edges=edges, boundary_edges=boundary_edges, nonmanifold_edges=nonmanifold,
                boundary_vertices=boundary_vertices, isolated_vertices=isolated, degenerate_faces=degenerate, exponent=exponent)
    return out_verts, out_normals, info


RASTER_CULL_BACK = 1                     # NM_MESH_RASTER_CULL_BACK
RASTER_LARGE_THRESHOLD = 128             # pixel centres in a face's clipped bounding box above which a whole wave draws it: the
                                         # same bytes, another speed (tests/tools/time_mesh_render.py measures it)
RASTER_COUNTS = ("drawn", "bad_index", "not_finite", "near", "out_of_range", "culled", "off_screen", "degenerate", "large",
                 "covered", "fragments")  # the NM_MESH_RASTER_* indices
INTERPOLATE_MAX_CHANNELS = 16


def mesh_rasterize(verts, faces, view, near, cull_back=False, large_threshold=None):
    """Which face of a mesh a pinhole camera sees at every pixel (nm_mesh_rasterize; the rule in include/nerfmeshes_hip.h).
    verts (V,3) f32, faces (F,3) i32 on the GPU, view: a non-NDC hip_ops.make_view, near > 0: a face with a corner nearer is
    not drawn (there is no clipping).  -> (face_id (H,W) int32, -1 where nothing was drawn; depth (H,W) f32: the distance
    along the camera's axis, 0 where nothing was drawn; bary (H,W,3) f32; counts: dict of RASTER_COUNTS -- the read-back of
    this call).  Both windings are drawn unless cull_back, which drops the faces that wind clockwise on the screen."""
    lib = _lib.load()
    faces, nv, nf = _mesh_faces(faces, verts.shape[0])
    dev = faces.device
    verts = _dev32(verts, dev, "verts")
    if verts.shape != (nv, 3):
        raise ValueError(f"mesh_rasterize: verts must be (V,3), got {tuple(verts.shape)}")
    height, width = int(view.height), int(view.width)
    threshold = RASTER_LARGE_THRESHOLD if large_threshold is None else int(large_threshold)
    ws = _mesh_workspace(int(lib.nm_mesh_raster_workspace_bytes(nv, nf, height, width)), "mesh raster", nv, nf, dev)
    face_id = torch.empty(height, width, dtype=torch.int32, device=dev)
    depth = torch.empty(height, width, dtype=torch.float32, device=dev)
    bary = torch.empty(height, width, 3, dtype=torch.float32, device=dev)
    counts = torch.empty(len(RASTER_COUNTS), dtype=torch.int64, device=dev)
    rc = lib.nm_mesh_rasterize(C.byref(view), _ptr(verts), nv, _ptr(faces), nf, float(near), RASTER_CULL_BACK if cull_back else 0,
                               threshold, _ptr(ws), _ptr(face_id), _ptr(depth), _ptr(bary), _ptr(counts), _stream())
    _mesh_check(lib, rc, "nm_mesh_rasterize")
    return face_id, depth, bary, dict(zip(RASTER_COUNTS, (int(x) for x in counts.tolist())))


def mesh_interpolate(raster, faces, attributes, background):
    """Per-vertex attributes at every pixel of a mesh_rasterize result (nm_mesh_interpolate): raster = (face_id, depth, bary,
    ...) as returned, faces the (F,3) i32 faces it was drawn from, attributes (V,C) f32 with C in [1, 16], background: C
    floats for the pixels nothing was drawn at.  -> (H,W,C) f32: (b0 a0 + b1 a1) + b2 a2 in fp32."""
    lib = _lib.load()
    face_id, bary = raster[0], raster[2]
    attributes = _dev32(attributes, face_id.device, "attributes")
    if attributes.dim() != 2:
        raise ValueError(f"mesh_interpolate: attributes must be (V,C), got {tuple(attributes.shape)}")
    faces, nv, nf = _mesh_faces(faces, attributes.shape[0])
    channels = int(attributes.shape[1])
    background = _dev32(torch.as_tensor(background, dtype=torch.float32).reshape(-1), face_id.device, "background")
    if background.numel() != channels:
        raise ValueError(f"mesh_interpolate: {background.numel()} background values for {channels} channels")
    out = torch.empty(*face_id.shape, channels, dtype=torch.float32, device=face_id.device)
    rc = lib.nm_mesh_interpolate(_ptr(face_id), _ptr(bary), face_id.numel(), _ptr(faces), nf, _ptr(attributes), nv, channels,
                                 _ptr(background), _ptr(out), _stream())
    _mesh_check(lib, rc, "nm_mesh_interpolate")
    return out


VISIBILITY_MAX_RINGS = 1024              # NM_MESH_VISIBILITY_MAX_RINGS


def mesh_cull_hidden(verts, faces, normals, views, near, rings=1, large_threshold=None):
    """Drops the faces no camera of `views` sees (nm_mesh_visibility_views + _select + _compact; the rule in
    include/nerfmeshes_hip.h): a face stays when it wins a pixel of the rasteriser in at least one view -- both windings drawn,
    a face with a corner nearer than `near` not at all --, or is within `rings` rounds of sharing a vertex with one that does.
    verts (V,3) f32, faces (F,3) i32, normals (V,3) f32 or None on the GPU; views: non-NDC hip_ops.make_view results.
    -> (verts, faces, normals, face_index, info): the kept rows in their original order, faces renumbered (numpy: new =
    cumsum(keep_v) - 1; new[faces[keep_f]]), normals None where None came in, face_index (faces_kept,) int32: the kept faces'
    original indices; info = dict(faces, faces_seen, faces_kept, vertices, vertices_kept, bad_faces, new_faces: per view the
    faces it saw first).  Nothing left gives empty (0,3) arrays.  One read-back of the counts, one of new_faces."""
    lib = _lib.load()
    rings = int(rings)
    if not 0 <= rings <= VISIBILITY_MAX_RINGS:
        raise ValueError(f"mesh_cull_hidden: rings must be in [0, {VISIBILITY_MAX_RINGS}], got {rings}")
    verts, faces, normals, _, _, nv, nf, dev = _mesh_inputs("mesh_cull_hidden", verts, faces, normals)
    views = list(views)
    array = (_lib.View * max(len(views), 1))(*views)
    height, width = (max(int(v.height) for v in views), max(int(v.width) for v in views)) if views else (1, 1)
    threshold = RASTER_LARGE_THRESHOLD if large_threshold is None else int(large_threshold)
    ws = _mesh_workspace(int(lib.nm_mesh_visibility_workspace_bytes(nv, nf, height, width)), "mesh visibility", nv, nf, dev)
    new_faces = torch.empty(len(views), dtype=torch.int64, device=dev)
    rc = lib.nm_mesh_visibility_views(array, len(views), _ptr(verts), nv, _ptr(faces), nf, float(near), threshold, 1, _ptr(ws),
                                      _ptr(new_faces), None, _stream())
    _mesh_check(lib, rc, "nm_mesh_visibility_views")
    kv, kf, seen, bad = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    rc = lib.nm_mesh_visibility_select(_ptr(faces), nf, nv, rings, _ptr(ws), C.byref(kv), C.byref(kf), C.byref(seen), C.byref(bad),
                                       _stream())
    _mesh_check(lib, rc, "nm_mesh_visibility_select")
    out_verts, out_faces, out_normals, _, _ = _mesh_subset_outputs(kv.value, kf.value, dev, normals)
    face_index = torch.empty(kf.value, dtype=torch.int32, device=dev)
    if kv.value:
        check(lib.nm_mesh_visibility_compact(_ptr(ws), _ptr(faces), nf, nv, _ptr(verts), _ptr(normals), kv.value, kf.value,
                                             _ptr(out_verts), _ptr(out_faces), _ptr(out_normals), _ptr(face_index), _stream()),
              "nm_mesh_visibility_compact")
    info = dict(faces=nf, faces_seen=seen.value, faces_kept=kf.value, vertices=nv, vertices_kept=kv.value, bad_faces=bad.value,
                new_faces=[int(x) for x in new_faces.tolist()])
    return out_verts, out_faces, out_normals, face_index, info


TEXTURE_MAX_RES = 255                    # NM_MESH_TEXTURE_MAX_RES
TEXTURE_MAX_SIDE = 16384                 # NM_MESH_TEXTURE_MAX_SIDE


def mesh_texture_layout(num_faces, n):
    """The atlas of `num_faces` per-face charts at `n` lattice intervals per triangle side (nm_mesh_texture_layout: host code,
    the rule in include/nerfmeshes_hip.h) -> dict(width, height, cols, rows, samples_per_face).  ValueError for no face, n
    outside [1, 255] and an atlas wider than 16384 texels."""
    lib = _lib.load()
    num_faces, n = int(num_faces), int(n)
    if num_faces <= 0:
        raise ValueError(f"mesh texture: a mesh of {num_faces} faces has no atlas")
    out = (C.c_int64 * 5)()
    _mesh_check(lib, lib.nm_mesh_texture_layout(num_faces, n, out), "nm_mesh_texture_layout")
    return dict(zip(("width", "height", "cols", "rows", "samples_per_face"), (int(x) for x in out)))


def mesh_texture_samples(verts, faces, normals, n, first=0, count=None, flip=1):
    """The surface samples behind the texels of faces [first, first + count) (nm_mesh_texture_samples): verts (V,3) f32, faces
    (F,3) i32, normals (V,3) f32 or None, all on the GPU.  -> (positions (count*T, 3), directions (count*T, 3): minus the
    interpolated unit normal, or minus flip times the face's geometric normal where there is none, fallback: how many samples
    took that, bad: how many samples belong to faces with an index outside [0, V) -- their rows are zeros)."""
    lib = _lib.load()
    faces, nv, nf = _mesh_faces(faces, verts.shape[0])
    dev = faces.device
    verts = _dev32(verts, dev, "verts")
    normals = _dev32(normals, dev, "normals") if normals is not None else None
    if verts.shape != (nv, 3) or (normals is not None and normals.shape != (nv, 3)):
        raise ValueError("mesh_texture_samples: verts and normals must be (V,3)")
    n, first = int(n), int(first)
    if not 1 <= n <= TEXTURE_MAX_RES:
        raise ValueError(f"mesh texture: the resolution n must be in [1, {TEXTURE_MAX_RES}], got {n}")
    count = nf - first if count is None else int(count)
    if first < 0 or count < 0 or first + count > nf:
        raise ValueError(f"mesh_texture_samples: the window [{first}, {first + count}) is not inside [0, {nf}]")
    rows = count * ((n + 1) * (n + 2) // 2)
    positions = torch.empty(rows, 3, dtype=torch.float32, device=dev)
    directions = torch.empty(rows, 3, dtype=torch.float32, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    rc = lib.nm_mesh_texture_samples(_ptr(verts), nv, _ptr(faces), nf, _ptr(normals), n, int(flip), first, count, _ptr(positions),
                                     _ptr(directions), _ptr(counts), _stream())
    _mesh_check(lib, rc, "nm_mesh_texture_samples")
    fallback, bad = (int(x) for x in counts.tolist())
    return positions, directions, fallback, bad


def mesh_texture_fill(colors, num_faces, n):
    """colors (F*T, 3) f32 on the GPU, in sample-row order -> the atlas (H, W, 3) uint8 (nm_mesh_texture_fill): every texel
    copies its lattice point, extrapolates its chart's gutter or is 0, and is quantised."""
    lib = _lib.load()
    layout = mesh_texture_layout(num_faces, n)
    colors = _dev32(colors, name="colors")
    if colors.shape != (int(num_faces) * layout["samples_per_face"], 3):
        raise ValueError(f"mesh_texture_fill: colors must be ({int(num_faces) * layout['samples_per_face']}, 3), got {tuple(colors.shape)}")
    atlas = torch.empty(layout["height"], layout["width"], 3, dtype=torch.uint8, device=colors.device)
    _mesh_check(lib, lib.nm_mesh_texture_fill(_ptr(colors), int(num_faces), int(n), _ptr(atlas), _stream()), "nm_mesh_texture_fill")
    return atlas


def mesh_texture_uv(num_faces, n, device="cuda"):
    """-> (F,3,2) f32: the texture coordinates of every face corner in the atlas of mesh_texture_layout (nm_mesh_texture_uv)"""
    lib = _lib.load()
    mesh_texture_layout(num_faces, n)
    uv = torch.empty(int(num_faces), 3, 2, dtype=torch.float32, device=device)
    _mesh_check(lib, lib.nm_mesh_texture_uv(int(num_faces), int(n), _ptr(uv), _stream()), "nm_mesh_texture_uv")
    return uv


def mesh_texture_lookup(raster, face_uv, texture, background):
    """The bilinear, clamp-to-edge fetch of a texture at every pixel of a mesh_rasterize result (nm_mesh_texture_lookup): raster =
    (face_id, depth, bary, ...), face_uv (F,3,2) f32: ANY texture coordinates, v pointing up, texture (Ht,Wt,3) uint8: ANY
    image, both on the GPU; background: three floats for the pixels nothing was drawn at or whose coordinates are not finite.
    -> (H,W,3) f32."""
    lib = _lib.load()
    face_id, bary = raster[0], raster[2]
    dev = face_id.device
    face_uv = _dev32(face_uv, dev, "face_uv")
    if face_uv.dim() != 3 or face_uv.shape[1:] != (3, 2):
        raise ValueError(f"mesh_texture_lookup: face_uv must be (F,3,2), got {tuple(face_uv.shape)}")
    if not isinstance(texture, torch.Tensor) or not texture.is_cuda:
        raise _lib.HipLibraryError("texture must live in GPU memory; there is no CPU path")
    if texture.dtype is not torch.uint8 or texture.dim() != 3 or texture.shape[2] != 3:
        raise ValueError(f"mesh_texture_lookup: texture must be (Ht,Wt,3) uint8, got {tuple(texture.shape)} {texture.dtype}")
    texture = texture.detach().to(dev).contiguous()
    background = _dev32(torch.as_tensor(background, dtype=torch.float32).reshape(-1), dev, "background")
    if background.numel() != 3:
        raise ValueError(f"mesh_texture_lookup: {background.numel()} background values for 3 channels")
    out = torch.empty(*face_id.shape, 3, dtype=torch.float32, device=dev)
    rc = lib.nm_mesh_texture_lookup(_ptr(face_id), _ptr(bary), face_id.numel(), _ptr(face_uv), int(face_uv.shape[0]), _ptr(texture),
                                    int(texture.shape[0]), int(texture.shape[1]), _ptr(background), _ptr(out), _stream())
    _mesh_check(lib, rc, "nm_mesh_texture_lookup")
    return out


SSIM_WINDOW = 11                         # NM_IMAGE_SSIM_WINDOW
SSIM_MAX_CHANNELS = 4                    # NM_IMAGE_SSIM_MAX_CHANNELS


def image_ssim(a, b, want_map=False, height=None):
    """The structural similarity of two images (nm_image_ssim; the rule in include/nerfmeshes_hip.h, "Image SSIM"): a, b (H,W,C)
    -- or (H*W,C) with `height=` -- fp32 on the GPU, data range 1.  -> dict(ssim: the mean over the valid windows and the
    channels, NaN when a window was not finite; per_channel: C floats; nonfinite: how many S were not finite; sums: the (C,2)
    int64 the library wrote, as numpy; map: (H-10,W-10,C) fp64 on the GPU, or None).  One host read, of the sums.  ValueError for
    what the library refuses: a side below 11 or above 16384, channels outside [1, 4]."""
    lib = _lib.load()
    a = _dev32(a, name="a")
    b = _dev32(b, a.device, "b")
    if a.shape != b.shape:
        raise ValueError(f"image_ssim: the images must have one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    if height is not None:
        if a.dim() != 2 or int(height) <= 0 or a.shape[0] % int(height):
            raise ValueError(f"image_ssim: height={height} needs (H*W,C) images, got {tuple(a.shape)}")
        shape = (int(height), a.shape[0] // int(height), a.shape[1])
    elif a.dim() == 3:
        shape = tuple(a.shape)
    else:
        raise ValueError(f"image_ssim: the images must be (H,W,C), or (H*W,C) with height=, got {tuple(a.shape)}")
    h, w, c = shape
    if h > 2 ** 31 - 1 or w > 2 ** 31 - 1 or c > 2 ** 31 - 1:
        raise ValueError(f"image_ssim: {shape} is beyond the supported sizes")
    ok = h >= SSIM_WINDOW and w >= SSIM_WINDOW and 1 <= c <= SSIM_MAX_CHANNELS    # nothing is allocated for what is refused
    out = torch.empty(h - 10, w - 10, c, dtype=torch.float64, device=a.device) if want_map and ok else None
    sums = torch.empty(max(c, 1), 2, dtype=torch.int64, device=a.device)
    _mesh_check(lib, lib.nm_image_ssim(_ptr(a), _ptr(b), h, w, c, _ptr(out), _ptr(sums), _stream()), "nm_image_ssim")
    host = sums.cpu().numpy()
    windows = (h - 10) * (w - 10) * 2 ** 32
    per_channel = [int(s) / windows for s in host[:, 0]]
    nonfinite = int(host[:, 1].sum())
    total = 0.0
    for v in per_channel:
        total = total + v
    return dict(ssim=float("nan") if nonfinite else total / c, per_channel=per_channel, nonfinite=nonfinite, sums=host, map=out)


TSDF_MAX_VIEWS = 1024                    # NM_TSDF_MAX_VIEWS
TSDF_COUNTS = ("observed", "interior", "outside")     # NM_TSDF_OBSERVED, _INTERIOR, _OUTSIDE


def tsdf_integrate(views, depth, opacity, axes, trunc, near, min_opacity=0.5, first=0, count=None, want_observations=False):
    """Depth maps fused into a truncated signed distance field on voxels [first, first + count) of a grid (nm_tsdf_integrate; the
    rule in include/nerfmeshes_hip.h, "TSDF fusion").  views: V non-NDC hip_ops.make_view results of one size; depth (V,H,W) fp32
    on the GPU, measured along the camera's axis; opacity (V,H,W) or None; axes: the three fp32 axes of the grid, as
    HipMLP.grid_query takes them.  -> dict(field (count,) fp32: inside-positive, in [-1, 1]; observations (count,) int32 or None;
    counts (3,) int64 ON THE DEVICE in the order of TSDF_COUNTS -- no host read here).  ValueError for what the library refuses."""
    lib = _lib.load()
    views = list(views)
    depth = _dev32(depth, name="depth")
    dev = depth.device
    if not views or depth.dim() != 3 or depth.shape[0] != len(views):
        raise ValueError(f"tsdf_integrate: depth must be (V,H,W) with one image per view, got {tuple(depth.shape)} for {len(views)} views")
    if tuple(depth.shape[1:]) != (int(views[0].height), int(views[0].width)):
        raise ValueError(f"tsdf_integrate: depth images of {tuple(depth.shape[1:])} for views of "
                         f"({int(views[0].height)}, {int(views[0].width)})")
    if opacity is not None:
        opacity = _dev32(opacity, dev, "opacity")
        if opacity.shape != depth.shape:
            raise ValueError(f"tsdf_integrate: opacity {tuple(opacity.shape)} must have depth's shape {tuple(depth.shape)}")
    ax = [_dev32(a, dev, "axis").reshape(-1) for a in axes]
    if len(ax) != 3 or any(a.numel() == 0 or a.numel() > 2 ** 31 - 1 for a in ax):
        raise ValueError("tsdf_integrate: axes must be three non-empty arrays")
    n0, n1, n2 = (a.numel() for a in ax)
    first = int(first)
    count = n0 * n1 * n2 - first if count is None else int(count)
    v, h, w = (int(s) for s in depth.shape)
    nbytes = int(lib.nm_tsdf_workspace_bytes(v, h, w))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)      # 0: a size the entry refuses, in its own words below
    array = (_lib.View * len(views))(*views)
    ok = 0 <= first and 0 <= count <= n0 * n1 * n2 - first                # nothing is allocated for what is refused
    field = torch.empty(count if ok else 0, dtype=torch.float32, device=dev)
    obs = torch.empty(count, dtype=torch.int32, device=dev) if want_observations and ok else None
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    # a zero-size tensor has no address: the entry takes none for count == 0
    _mesh_check(lib, lib.nm_tsdf_integrate(array, v, _ptr(depth), _ptr(opacity), _ptr(ax[0]), _ptr(ax[1]), _ptr(ax[2]), n0, n1, n2,
                                           first, count, float(trunc), float(near), float(min_opacity), _ptr(ws),
                                           _ptr(field) if field.numel() else None, _ptr(obs) if obs is not None and obs.numel() else None,
                                           _ptr(counts), _stream()), "nm_tsdf_integrate")
    return dict(field=field, observations=obs, counts=counts)


def _mesh_arrays(verts, faces, what):
    """(V,3) fp32 vertices and (F,3) int32 faces of one mesh on the GPU (host arrays are copied over), checked."""
    verts = _dev32(verts if isinstance(verts, torch.Tensor) and verts.is_cuda else torch.as_tensor(verts).cuda(), name="verts")
    if not isinstance(faces, torch.Tensor):
        faces = torch.as_tensor(faces)
    if faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: faces must be an integer tensor, got {faces.dtype}")
    faces = faces.to(device=verts.device, dtype=torch.int32)
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{what}: verts must be (V,3) and faces (F,3), got {tuple(verts.shape)} and {tuple(faces.shape)}")
    faces, nv, nf = _mesh_faces(faces, verts.shape[0])
    return verts, faces, nv, nf


def _mesh_face_weights(lib, verts, faces, nv, nf, what):
    """areas, cdf and the total weight of a checked mesh; the header read-back is the one synchronisation."""
    dev = verts.device
    areas = torch.empty(nf, dtype=torch.float32, device=dev)
    cdf = torch.empty(nf, dtype=torch.int64, device=dev)             # uint64 on the device; every prefix is below 2^63
    hdr = torch.empty(int(lib.nm_mesh_face_weights_workspace_bytes()), dtype=torch.uint8, device=dev)
    rc = lib.nm_mesh_face_weights(_ptr(verts), nv, _ptr(faces), nf, _ptr(areas), _ptr(cdf), _ptr(hdr), _stream())
    _mesh_check(lib, rc, "nm_mesh_face_weights")
    bad, total = (int(v) for v in hdr[:16].view(torch.int64).tolist())
    if bad:
        raise ValueError(f"{what}: {bad} faces have a vertex index outside [0, {nv})")
    return areas, cdf, total


def mesh_face_weights(verts, faces):
    """Area-proportional sampling weights of a triangle mesh (nm_mesh_face_weights; arithmetic in include/nerfmeshes_hip.h).
    verts (V,3) f32, faces (F,3) i32 -> (areas (F,) f32, cdf (F,) int64: the inclusive prefix sums of the integer weights
    trunc(area * 2^(32-e)), exact).  Raises ValueError for a face index out of range (the one read-back of this call)."""
    lib = _lib.load()
    verts, faces, nv, nf = _mesh_arrays(verts, faces, "mesh_face_weights")
    areas, cdf, _ = _mesh_face_weights(lib, verts, faces, nv, nf, "mesh_face_weights")
    return areas, cdf


def mesh_sample_points(verts, faces, n=None, u=None, generator=None, return_normals=False):
    """Points distributed uniformly over the surface of a triangle mesh (nm_mesh_face_weights + nm_mesh_sample_points):
    draw row (u0, u1, u2) picks the face whose cdf interval holds trunc(u0 * total) and the barycentric weights
    (1 - sqrt(u1), sqrt(u1) (1 - u2), sqrt(u1) u2), pytorch3d's.  `u` (N,3) in [0, 1) defaults to
    torch.rand(n, 3, device=..., generator=generator).  -> (points (N,3) f32, face_ids (N,) i32[, normals (N,3): the face's
    unit normal]).  ValueError when nothing can be sampled (no face, or only degenerate ones) or a face index is out of range."""
    lib = _lib.load()
    verts, faces, nv, nf = _mesh_arrays(verts, faces, "mesh_sample_points")
    dev = verts.device
    if u is None:
        if n is None:
            raise ValueError("mesh_sample_points: give the number of points n or the draws u")
        u = torch.rand(int(n), 3, device=dev, generator=generator)
    u = _dev32(u, dev, "u")
    if u.dim() != 2 or u.shape[1] != 3 or (n is not None and u.shape[0] != int(n)):
        raise ValueError(f"mesh_sample_points: u must be (n,3) draws, got {tuple(u.shape)}")
    _, cdf, total = _mesh_face_weights(lib, verts, faces, nv, nf, "mesh_sample_points")
    if total == 0:
        raise ValueError(f"mesh_sample_points: a mesh of {nf} faces with no area cannot be sampled")
    count = int(u.shape[0])
    points = torch.empty(count, 3, dtype=torch.float32, device=dev)
    face_ids = torch.empty(count, dtype=torch.int32, device=dev)
    normals = torch.empty(count, 3, dtype=torch.float32, device=dev) if return_normals else None
    rc = lib.nm_mesh_sample_points(_ptr(u), count, _ptr(verts), nv, _ptr(faces), nf, _ptr(cdf), _ptr(points), _ptr(face_ids),
                                   _ptr(normals), _stream())
    _mesh_check(lib, rc, "nm_mesh_sample_points")
    return (points, face_ids, normals) if return_normals else (points, face_ids)


def _points(t, device, name):
    t = _dev32(t, device, name)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} must be an (N,3) point cloud, got {tuple(t.shape)}")
    return t


def points_nearest(x, y):
    """Exact nearest neighbour of every row of x (N,3) among the rows of y (M,3) (nm_points_nearest: brute force, no N x M
    intermediate) -> (dist2 (N,) f32: the squared distance ((dx dx + dy dy) + dz dz), index (N,) i32: the smallest j that
    attains it).  NaN pairs never win; a row without a winner (a NaN query, M = 0) gets (+inf, -1)."""
    lib = _lib.load()
    x = _points(x, None, "x")
    dev = x.device
    y = _points(y, dev, "y")
    n, m = int(x.shape[0]), int(y.shape[0])
    nbytes = int(lib.nm_points_nearest_workspace_bytes(n, m))
    if nbytes == 0:
        raise ValueError(f"points_nearest: {n} x {m} points are beyond the supported sizes")
    dist2 = torch.empty(n, dtype=torch.float32, device=dev)
    index = torch.empty(n, dtype=torch.int32, device=dev)
    ws = _workspace(nbytes, dev)
    check(lib.nm_points_nearest(_ptr(x), n, _ptr(y), m, _ptr(dist2), _ptr(index), _ptr(ws), _stream()), "nm_points_nearest")
    return dist2, index


def _nearest_dist2_sharded(x, y):
    """dist2 of `points_nearest(x, y)`, the queries split over the ranks of torch.distributed: every rank searches its
    dist.split_range slice against the whole of y and one dist.all_gather_rows assembles the (N,) array on every rank."""
    from . import dist as nd
    if nd.world()[1] == 1:
        return points_nearest(x, y)[0]
    lo, hi, counts = nd.own_range(int(x.shape[0]))
    return nd.all_gather_rows(points_nearest(x[lo:hi], y)[0].contiguous(), counts)


def chamfer_distance(x, y):
    """Chamfer distance of two point clouds x (N,3), y (M,3) with pytorch3d's `chamfer_distance` defaults (squared L2,
    point_reduction="mean"): chamfer = mean_i min_j |x_i - y_j|^2 + mean_j min_i |y_j - x_i|^2.  -> dict: chamfer, x_to_y,
    y_to_x (Python floats; the means are fp64 sums of the gathered (N,) / (M,) arrays only), dist2_x (N,), dist2_y (M,)
    (device tensors).  Under torch.distributed every rank searches a slice of the queries and then reduces the same gathered
    arrays: any number of ranks gives the single-rank result bit for bit."""
    x = _points(x, None, "x")
    y = _points(y, x.device, "y")
    if x.shape[0] == 0 or y.shape[0] == 0:
        raise ValueError(f"chamfer_distance: empty point cloud ({x.shape[0]} and {y.shape[0]} points)")
    dist2_x = _nearest_dist2_sharded(x, y)
    dist2_y = _nearest_dist2_sharded(y, x)
    x_to_y = float(dist2_x.double().sum().item()) / dist2_x.shape[0]
    y_to_x = float(dist2_y.double().sum().item()) / dist2_y.shape[0]
    return dict(chamfer=x_to_y + y_to_x, x_to_y=x_to_y, y_to_x=y_to_x, dist2_x=dist2_x, dist2_y=dist2_y)


def points_to_mesh(x, verts, faces, return_normals=False):
    """Exact distance of every row of x (N,3) to the TRIANGLES of a mesh (nm_points_to_mesh: brute force over all N * F pairs;
    the arithmetic is in include/nerfmeshes_hip.h, "Point to mesh") -> (dist2 (N,) f32: the smallest squared distance to a
    face, face (N,) i32: the smallest face index that attains it[, normals (N,3): that face's unit normal, NaN for a face
    without area]).  NaN pairs never win; a row without a winner (a NaN query, F = 0) gets (+inf, -1, NaN).  Raises ValueError
    for a face index out of range (the one read-back of this call)."""
    lib = _lib.load()
    x = _points(x, None, "x")
    dev = x.device
    verts, faces, nv, nf = _mesh_arrays(verts.to(dev) if isinstance(verts, torch.Tensor) else verts, faces, "points_to_mesh")
    n = int(x.shape[0])
    _mesh_face_weights(lib, verts, faces, nv, nf, "points_to_mesh")
    nbytes = int(lib.nm_points_to_mesh_workspace_bytes(n, nf))
    if nbytes == 0:
        raise ValueError(f"points_to_mesh: {n} points x {nf} faces are beyond the supported sizes")
    dist2 = torch.empty(n, dtype=torch.float32, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    normals = torch.empty(n, 3, dtype=torch.float32, device=dev) if return_normals else None
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)          # 112 bytes per face: not kept beyond the call
    _mesh_check(lib, lib.nm_points_to_mesh(_ptr(x), n, _ptr(verts), nv, _ptr(faces), nf, _ptr(dist2), _ptr(face), _ptr(normals),
                                           _ptr(ws), _stream()), "nm_points_to_mesh")
    return (dist2, face, normals) if return_normals else (dist2, face)


def _points_to_mesh_sharded(x, verts, faces):
    """`points_to_mesh(x, verts, faces, return_normals=True)`, the queries split over the ranks of torch.distributed as
    `_nearest_dist2_sharded` splits them: one dist.all_gather_rows per array assembles it on every rank."""
    from . import dist as nd
    if nd.world()[1] == 1:
        return points_to_mesh(x, verts, faces, return_normals=True)
    lo, hi, counts = nd.own_range(int(x.shape[0]))
    return tuple(nd.all_gather_rows(t.contiguous(), counts) for t in points_to_mesh(x[lo:hi], verts, faces, return_normals=True))


def surface_metrics(dist2_x, dist2_y, normals_x, face_normals_x, normals_y, face_normals_y, thresholds=()):
    """The numbers of `mesh_surface_distance` from its gathered arrays (x: mesh -> target, y: target -> mesh): fp64 sums,
    integer counts, Python numbers.  The normal agreement of a row is |dot| of the sample's normal and the winning face's,
    the dot in fp32 as (x x' + y y') + z z', over the rows where both are finite."""
    out = {}
    roots = {}
    for side, d2 in (("x_to_y", dist2_x), ("y_to_x", dist2_y)):
        d2 = d2.double()
        roots[side] = d2.sqrt()
        out[side] = float(d2.sum().item()) / d2.shape[0]
    out["chamfer"] = out["x_to_y"] + out["y_to_x"]
    out["accuracy"] = float(roots["x_to_y"].sum().item()) / roots["x_to_y"].shape[0]
    out["completeness"] = float(roots["y_to_x"].sum().item()) / roots["y_to_x"].shape[0]
    for side in ("x_to_y", "y_to_x"):
        out["hausdorff_" + side] = float(roots[side].max().item())
    out["hausdorff"] = max(out["hausdorff_x_to_y"], out["hausdorff_y_to_x"])
    for side, a, b in (("x_to_y", normals_x, face_normals_x), ("y_to_x", normals_y, face_normals_y)):
        dot = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
        ok = torch.isfinite(a).all(1) & torch.isfinite(b).all(1)
        pairs = int(ok.sum().item())
        total = float(torch.where(ok, dot.double().abs(), torch.zeros((), dtype=torch.float64, device=dot.device)).sum().item())
        out["normal_pairs_" + side] = pairs
        out["normal_consistency_" + side] = total / pairs if pairs else float("nan")
    out["normal_consistency"] = 0.5 * (out["normal_consistency_x_to_y"] + out["normal_consistency_y_to_x"])
    out["fscore"] = []
    for tau in thresholds:
        tau = float(tau)
        p, r = (int((d2.double() <= tau * tau).sum().item()) / d2.shape[0] for d2 in (dist2_x, dist2_y))
        out["fscore"].append(dict(threshold=tau, precision=p, recall=r, fscore=2 * p * r / (p + r) if p + r > 0 else 0.0))
    return out


def mesh_surface_distance(verts_a, faces_a, verts_b, faces_b, n, generator=None, thresholds=()):
    """Surface distance of two triangle meshes without a noise floor of its own: `n` points with their face normals are
    sampled on each mesh (mesh_sample_points from `generator`, mesh A first: the draws `mesh_chamfer.compare_meshes` makes) and
    every cloud is measured against the other mesh's TRIANGLES (points_to_mesh).  -> dict: x_to_y, y_to_x, chamfer (means of
    squared distances), accuracy, completeness (means of distances, A -> B and B -> A), hausdorff_x_to_y, hausdorff_y_to_x,
    hausdorff (maxima), normal_consistency_x_to_y, normal_consistency_y_to_x, normal_consistency and normal_pairs_* (mean
    |cos| between the sample's and the winning face's normal over the rows where both are finite; NaN without any), fscore: a
    list of dict(threshold, precision, recall, fscore) per threshold (dist2 <= tau^2 in fp64; 0 when P + R = 0), and the
    device arrays dist2_x, dist2_y, face_x, face_y.  Under torch.distributed every rank measures a slice of the queries and
    then reduces the same gathered arrays: any number of ranks gives the single-rank result bit for bit."""
    n = int(n)
    if n < 1:
        raise ValueError(f"mesh_surface_distance: the number of samples must be >= 1, got {n}")
    thresholds = tuple(float(t) for t in thresholds)
    if any(not (0.0 < t < float("inf")) for t in thresholds):
        raise ValueError(f"mesh_surface_distance: thresholds must be finite and > 0, got {thresholds}")
    verts_a, faces_a, _, _ = _mesh_arrays(verts_a, faces_a, "mesh_surface_distance")
    verts_b, faces_b, _, _ = _mesh_arrays(verts_b, faces_b, "mesh_surface_distance")
    points_a, _, normals_a = mesh_sample_points(verts_a, faces_a, n=n, generator=generator, return_normals=True)
    points_b, _, normals_b = mesh_sample_points(verts_b, faces_b, n=n, generator=generator, return_normals=True)
    dist2_x, face_x, fn_x = _points_to_mesh_sharded(points_a, verts_b, faces_b)
    dist2_y, face_y, fn_y = _points_to_mesh_sharded(points_b, verts_a, faces_a)
    out = surface_metrics(dist2_x, dist2_y, normals_a, fn_x, normals_b, fn_y, thresholds)
    out.update(dist2_x=dist2_x, dist2_y=dist2_y, face_x=face_x, face_y=face_y)
    return out


SURFACE_STEP_MAX = 8


def surface_min_votes(step, prob_threshold):
    """The smallest vote count the reference's `count > ((2 step + 1)^2 - 1) * prob_threshold` (mesh_surface_ray.py:120,133)
    accepts, the product taken in Python doubles as there (24 * 0.6 = 14.399999999999999 -> 15; 24 * 0.5 = 12.0 -> 13)."""
    import math
    return int(math.floor(((2 * int(step) + 1) ** 2 - 1) * prob_threshold)) + 1


def surface_filter(origins, dirs, depth, height, width, step=2, dist_threshold=0.002, min_votes=15, opacity=None,
                   min_opacity=None):
    """The reference's neighbourhood vote over the surface points of one height x width image of rays (nm_surface_filter;
    semantics in include/nerfmeshes_hip.h).  origins (1|H*W, 3), dirs (H*W, 3), depth (H*W), opacity (H*W) with min_opacity
    or None -> dict: votes (H, W) int32, keep (H, W) bool, count (1,) int64 ON THE DEVICE (reading it is the caller's
    synchronisation), and the state `surface_gather` needs."""
    lib = _lib.load()
    height, width = int(height), int(width)
    if height <= 0 or width <= 0:
        raise ValueError(f"surface_filter: image of {height} x {width} pixels")
    if (opacity is None) != (min_opacity is None):
        raise ValueError("surface_filter: opacity and min_opacity come together")
    dirs = _dev32(dirs, name="dirs").reshape(-1, 3)
    dev = dirs.device
    n = height * width
    origins = _dev32(origins, dev, "origins").reshape(-1, 3)
    depth = _dev32(depth, dev, "depth").reshape(-1)
    opacity = _dev32(opacity, dev, "opacity").reshape(-1) if opacity is not None else None
    if dirs.shape[0] != n or depth.numel() != n or origins.shape[0] not in (1, n) or (opacity is not None and opacity.numel() != n):
        raise ValueError(f"surface_filter: the inputs do not describe {height} x {width} rays")
    per_ray_o = int(origins.shape[0] == n and n > 1)
    votes = torch.empty(height, width, dtype=torch.int32, device=dev)
    keep = torch.empty(height, width, dtype=torch.uint8, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(int(lib.nm_surface_filter_workspace_bytes(height, width)), dtype=torch.uint8, device=dev)
    mo = float(min_opacity) if min_opacity is not None else 0.0
    check(lib.nm_surface_filter(_ptr(origins), per_ray_o, _ptr(dirs), _ptr(depth), _ptr(opacity), mo, height, width, int(step),
                                float(dist_threshold), int(min_votes), _ptr(votes), _ptr(keep), _ptr(count), _ptr(ws), _stream()),
          "nm_surface_filter")
    return dict(votes=votes, keep=keep.view(torch.bool), count=count, workspace=ws, origins=origins, per_ray_o=per_ray_o,
                dirs=dirs, depth=depth, opacity=opacity, min_opacity=mo, height=height, width=width)


def surface_gather(flt, rgb, count=None):
    """The pixels `surface_filter` kept, in row-major pixel order (nm_surface_gather) -> (points (N,3), normals (N,3) = -dirs,
    colours (N,3) fp32 as rendered, colours (N,3) uint8 = trunc(clamp(rgb * 255, 0, 255)) with NaN -> 0 -- numpy's `u1` cast
    truncates the same way inside [0, 256) and WRAPS outside it, which nobody wants in a colour: the clamp is deliberate).
    `count` = N when the caller already read it; otherwise flt["count"] is read here (one D2H copy)."""
    lib = _lib.load()
    dev = flt["dirs"].device
    n = int(flt["count"].item()) if count is None else int(count)
    rgb = _dev32(rgb, dev, "rgb").reshape(-1, 3)
    if rgb.shape[0] != flt["height"] * flt["width"]:
        raise ValueError("surface_gather: rgb does not match the filtered image")
    points, normals, colors = (torch.empty(n, 3, dtype=torch.float32, device=dev) for _ in range(3))
    colors_u8 = torch.empty(n, 3, dtype=torch.uint8, device=dev)
    if n:
        check(lib.nm_surface_gather(_ptr(flt["workspace"]), _ptr(flt["origins"]), flt["per_ray_o"], _ptr(flt["dirs"]),
                                    _ptr(flt["depth"]), _ptr(flt["opacity"]), flt["min_opacity"], _ptr(rgb), flt["height"],
                                    flt["width"], 0, n, _ptr(points), _ptr(normals), _ptr(colors), _ptr(colors_u8), _stream()),
              "nm_surface_gather")
    return points, normals, colors, colors_u8


def export_ply(points, normals, colors_u8, filename, binary=False):
    """Point cloud -> PLY (nm_export_ply): x y z nx ny nz as float, red green blue as uchar; ascii (default, the reference's
    `text = True`) or binary_little_endian.  Host or device arrays; colours must already be uint8."""
    import os

    def host(x, dtype):
        if isinstance(x, torch.Tensor):
            x = x.detach().cpu().numpy()
        x = np.asarray(x)
        if dtype is np.uint8 and x.dtype != np.uint8:
            raise ValueError("export_ply: colours must be uint8 (see surface_gather for the conversion rule)")
        return np.ascontiguousarray(x, dtype=dtype).reshape(-1, 3)

    p, nrm, c = host(points, np.float32), host(normals, np.float32), host(colors_u8, np.uint8)
    if not len(p) == len(nrm) == len(c):
        raise ValueError("export_ply: points, normals and colours disagree on the vertex count")
    ptr = lambda a: C.c_void_p(a.ctypes.data) if len(a) else C.c_void_p(None)  # noqa: E731
    check(_lib.load().nm_export_ply(ptr(p), ptr(nrm), ptr(c), len(p), int(bool(binary)), os.fsencode(filename)), "nm_export_ply")
