"""The image SSIM kernel (nm_image_ssim) at 800 x 800 x 3 and 1792 x 1792 x 3 under HIP events: after a warm-up, windows of
back-to-back launches through the C ABI (no host read in between), per-call time = window / launches, median and spread over the
windows; with and without the map.  Beside it the same formula written with torch device ops on the same box (fp64, the taps
applied as 11 shifted slices along each axis, the fixed-point sum as rint + sum), timed the same way, and checked to give the
kernel's sums.  The kernel's time is also given as a share of one mesh_render view's rasterisation (0.73 ms at 800 x 800:
README.md), and the bytes it must move once (two fp32 images in, the fp64 map out) are held against the time.

    python tests/tools/time_image_ssim.py [--sizes 800 1792] [--launches 1000] [--windows 7] [--out profiles/r16_image_ssim.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nerfmeshes_amd import _lib, hip_ops  # noqa: E402

HALF = [float.fromhex(t) for t in ("0x1.0d956b52a1d6cp-10", "0x1.f1fe01ae5a5b8p-8", "0x1.26eb175d83f67p-5", "0x1.bff0fe8e98418p-4",
                                   "0x1.b43c3f52b19f2p-3", "0x1.106560aa892c0p-2")]
TAPS = HALF + HALF[-2::-1]
RASTER_MS_800 = 0.73                      # nm_mesh_rasterize per 800 x 800 view of the full-resolution mesh (README.md)


def stats(times):
    times = sorted(times)
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1]}


def windows(fn, launches, count, warmup=10):
    """per-call milliseconds of `count` windows of `launches` back-to-back calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(count):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / launches)
    return out


def torch_ssim(a, b):
    """the rule of include/nerfmeshes_hip.h ("Image SSIM") with torch ops -> (map, (C,2) int64 sums)"""
    x, y = a.double(), b.double()
    f = torch.stack((x, y, x * x, y * y, x * y))
    height, width = f.shape[1], f.shape[2]
    h = TAPS[0] * f[:, :, 0:width - 10]
    for k in range(1, 11):
        h = h + TAPS[k] * f[:, :, k:k + width - 10]
    v = TAPS[0] * h[:, 0:height - 10]
    for k in range(1, 11):
        v = v + TAPS[k] * h[:, k:k + height - 10]
    ux, uy, uxx, uyy, uxy = v
    c1, c2 = 0.01 * 0.01, 0.03 * 0.03
    ux2, uy2, uxuy = ux * ux, uy * uy, ux * uy
    s = (((2.0 * ux) * uy + c1) * (2.0 * (uxy - uxuy) + c2)) / (((ux2 + uy2) + c1) * (((uxx - ux2) + (uyy - uy2)) + c2))
    finite = torch.isfinite(s)
    fixed = torch.round(torch.where(finite, s, torch.zeros_like(s)) * 4294967296.0).to(torch.int64)
    return s, torch.stack((fixed.sum(dim=(0, 1)), (~finite).sum(dim=(0, 1))), dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[800, 1792])
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_image_ssim needs a MI355X: nothing is timed without one")
    lib = _lib.load()
    out = {"device": torch.cuda.get_device_name(0), "channels": 3, "launches_per_window": opt.launches, "windows": opt.windows,
           "tile": [24, 32], "rasterize_ms_per_800_view": RASTER_MS_800, "sizes": {}}
    for size in opt.sizes:
        gen = torch.Generator(device="cuda").manual_seed(size)
        a = torch.rand(size, size, 3, device="cuda", generator=gen)
        b = (a + 0.05 * torch.randn(size, size, 3, device="cuda", generator=gen)).contiguous()
        ssim_map = torch.empty(size - 10, size - 10, 3, dtype=torch.float64, device="cuda")
        sums = torch.empty(3, 2, dtype=torch.int64, device="cuda")
        stream = hip_ops._stream()

        def kernel(with_map):
            rc = lib.nm_image_ssim(hip_ops._ptr(a), hip_ops._ptr(b), size, size, 3, hip_ops._ptr(ssim_map if with_map else None),
                                   hip_ops._ptr(sums), stream)
            _lib.check(rc, "nm_image_ssim")

        row = {"kernel_with_map": stats(windows(lambda: kernel(True), opt.launches, opt.windows)),
               "kernel_sums_only": stats(windows(lambda: kernel(False), opt.launches, opt.windows))}
        kernel(True)
        want = sums.cpu()
        got_map, got = torch_ssim(a, b)
        row["torch_ops_give_the_kernels_sums"] = bool(torch.equal(got.cpu(), want))
        row["torch_ops_give_the_kernels_map"] = bool(torch.equal(got_map, ssim_map))
        row["torch_ops"] = stats(windows(lambda: torch_ssim(a, b), max(opt.launches // 20, 5), opt.windows, warmup=3))
        row["ssim"] = hip_ops.image_ssim(a, b)["ssim"]
        in_bytes, map_bytes = 2 * 4 * size * size * 3, 8 * (size - 10) * (size - 10) * 3
        row["bytes_that_must_move"] = {"sums_only": in_bytes, "with_map": in_bytes + map_bytes}
        row["gb_per_s_with_map"] = (in_bytes + map_bytes) / (row["kernel_with_map"]["median_ms"] * 1e-3) / 1e9
        row["gb_per_s_sums_only"] = in_bytes / (row["kernel_sums_only"]["median_ms"] * 1e-3) / 1e9
        # 5 fields x (11 products + 10 sums) in each pass, the horizontal pass over (24 + 10) / 24 of the rows, + 3 products per tap
        row["fp64_operations"] = int((size - 10) * (size - 10) * 3 * (105 * (1 + 34 / 24) + 33 * 34 / 24 + 20))
        row["fp64_gflops_sums_only"] = row["fp64_operations"] / (row["kernel_sums_only"]["median_ms"] * 1e-3) / 1e9
        row["torch_over_kernel"] = row["torch_ops"]["median_ms"] / row["kernel_sums_only"]["median_ms"]
        if size == 800:
            row["share_of_one_view_rasterisation"] = row["kernel_sums_only"]["median_ms"] / RASTER_MS_800
        out["sizes"][str(size)] = row
        print(json.dumps({str(size): row}), flush=True)
        del got_map, got
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
