// Structural similarity of two images (eval_nerf --ssim, mesh_render --ssim, mesh_nerf --render-ssim; DESIGN.md, "Image SSIM"):
// Wang et al. 2004 with the 11-tap Gaussian window, over the valid windows only, in fp64 with every operation rounded on its own
// (-ffp-contract=off, IEEE division), the mean as an int64 sum of llrint(S 2^32).  Integer addition is associative, so the sums do
// not depend on the order the workgroups ran in, and a numpy restatement (tests/image_ssim.py) reproduces the map, the sums and
// the mean bit for bit.  THE RULE is written out in include/nerfmeshes_hip.h ("Image SSIM"); the comments below name its
// paragraphs.
// One kernel, one launch per image pair.  A workgroup of 256 threads takes IS_TH x IS_TW = 24 x 32 outputs of one channel:
//   stage    the (24 + 10) x (32 + 10) pixels of that channel of both images into LDS as fp32 (zeros beyond the image: they
//            only reach outputs that are not stored);
//   "filter" horizontal: one thread per (row, column) of 34 x 32 forms the five fields from the 11 staged pixels to its right
//            and writes five fp64 values into LDS; vertical: a thread owns 3 consecutive rows of one column, reads the 13
//            values of a field once and keeps the 3 sums in registers;
//   "pixel", "mean": S per output, the optional store, then the fixed-point values and the non-finite count summed over the
//            wave (shuffles), over the 4 waves (LDS), and ONE integer atomicAdd per workgroup into the channel's sum (a second
//            one into its count only when the workgroup counted something).
// LDS: 2 x 34 x 42 x 4 + 5 x 34 x 32 x 8 + 64 = 55 008 bytes, static: two workgroups fit a CU's 160 KiB with room to spare.
// Nothing allocates and nothing synchronises with the host: the entry can be captured into a graph.
#include "nm_internal.h"

namespace nm {

constexpr int IS_R = NM_IMAGE_SSIM_WINDOW - 1;      // 10: rows and columns a window reaches beyond its first pixel
constexpr int IS_TH = 24, IS_TW = 32;               // outputs of a workgroup
constexpr int IS_IH = IS_TH + IS_R, IS_IW = IS_TW + IS_R;
constexpr int IS_ROWS = 3;                          // rows per thread of the vertical pass: 256 threads = 32 columns x 8 groups of 3
static_assert(IS_TW * (IS_TH / IS_ROWS) == 256, "one thread per column and group of rows");

// "window": the 11 taps, as constants
#define IS_TAPS                                                                                                                 \
    { 0x1.0d956b52a1d6cp-10, 0x1.f1fe01ae5a5b8p-8, 0x1.26eb175d83f67p-5, 0x1.bff0fe8e98418p-4, 0x1.b43c3f52b19f2p-3,            \
      0x1.106560aa892c0p-2, 0x1.b43c3f52b19f2p-3, 0x1.bff0fe8e98418p-4, 0x1.26eb175d83f67p-5, 0x1.f1fe01ae5a5b8p-8,             \
      0x1.0d956b52a1d6cp-10 }

__device__ __forceinline__ bool is_finite64(double v) {
    return (__double_as_longlong(v) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll;
}

__global__ __launch_bounds__(256) void image_ssim_kernel(const float* __restrict__ a, const float* __restrict__ b, int height, int width,
                                                         int channels, double* __restrict__ map, unsigned long long* sums) {
    constexpr double w[NM_IMAGE_SSIM_WINDOW] = IS_TAPS;
    __shared__ float sa[IS_IH][IS_IW], sb[IS_IH][IS_IW];
    __shared__ double sh[5][IS_IH][IS_TW];
    __shared__ long long wave_sum[4];
    __shared__ long long wave_bad[4];
    const int tid = threadIdx.x, ch = blockIdx.z;
    const int row0 = blockIdx.y * IS_TH, col0 = blockIdx.x * IS_TW;          // first output = first input of the tile
    const int out_h = height - IS_R, out_w = width - IS_R;

    for (int i = tid; i < IS_IH * IS_IW; i += 256) {
        const int r = i / IS_IW, c = i - r * IS_IW;
        const int gr = row0 + r, gc = col0 + c;
        float va = 0.0f, vb = 0.0f;
        if (gr < height && gc < width) {
            const int64_t at = ((int64_t)gr * width + gc) * channels + ch;
            va = a[at];
            vb = b[at];
        }
        sa[r][c] = va;
        sb[r][c] = vb;
    }
    __syncthreads();

    // "fields", "filter": horizontal
    for (int i = tid; i < IS_IH * IS_TW; i += 256) {
        const int r = i / IS_TW, c = i - r * IS_TW;
        double x = (double)sa[r][c], y = (double)sb[r][c];
        double xx = x * x, yy = y * y, xy = x * y;
        double hx = w[0] * x, hy = w[0] * y, hxx = w[0] * xx, hyy = w[0] * yy, hxy = w[0] * xy;
#pragma unroll
        for (int k = 1; k < NM_IMAGE_SSIM_WINDOW; ++k) {
            x = (double)sa[r][c + k];
            y = (double)sb[r][c + k];
            xx = x * x; yy = y * y; xy = x * y;
            const double px = w[k] * x, py = w[k] * y, pxx = w[k] * xx, pyy = w[k] * yy, pxy = w[k] * xy;
            hx = hx + px; hy = hy + py; hxx = hxx + pxx; hyy = hyy + pyy; hxy = hxy + pxy;
        }
        sh[0][r][c] = hx; sh[1][r][c] = hy; sh[2][r][c] = hxx; sh[3][r][c] = hyy; sh[4][r][c] = hxy;
    }
    __syncthreads();

    // "filter": vertical, 3 rows of one column per thread
    const int c = tid & (IS_TW - 1), r0 = (tid / IS_TW) * IS_ROWS;
    double u[5][IS_ROWS];
#pragma unroll
    for (int f = 0; f < 5; ++f) {
        double h[IS_ROWS + IS_R];
#pragma unroll
        for (int k = 0; k < IS_ROWS + IS_R; ++k) h[k] = sh[f][r0 + k][c];
#pragma unroll
        for (int i = 0; i < IS_ROWS; ++i) {
            double v = w[0] * h[i];
#pragma unroll
            for (int k = 1; k < NM_IMAGE_SSIM_WINDOW; ++k) { const double p = w[k] * h[i + k]; v = v + p; }
            u[f][i] = v;
        }
    }

    // "pixel", "mean"
    constexpr double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    long long sum = 0, bad = 0;
#pragma unroll
    for (int i = 0; i < IS_ROWS; ++i) {
        const int gr = row0 + r0 + i, gc = col0 + c;
        if (gr < out_h && gc < out_w) {
            const double ux = u[0][i], uy = u[1][i], uxx = u[2][i], uyy = u[3][i], uxy = u[4][i];
            const double ux2 = ux * ux, uy2 = uy * uy, uxuy = ux * uy;
            const double vx = uxx - ux2, vy = uyy - uy2, vxy = uxy - uxuy;
            const double n1 = (2.0 * ux) * uy + C1, n2 = 2.0 * vxy + C2;
            const double d1 = (ux2 + uy2) + C1, d2 = (vx + vy) + C2;
            const double num = n1 * n2, den = d1 * d2;
            const double s = num / den;
            if (map) map[((int64_t)gr * out_w + gc) * channels + ch] = s;
            if (is_finite64(s)) sum += llrint(s * 4294967296.0);
            else ++bad;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off);
        bad += __shfl_xor(bad, off);
    }
    if ((tid & 63) == 0) { wave_sum[tid >> 6] = sum; wave_bad[tid >> 6] = bad; }
    __syncthreads();
    if (tid == 0) {
        const long long total = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
        const long long total_bad = (wave_bad[0] + wave_bad[1]) + (wave_bad[2] + wave_bad[3]);
        atomicAdd(sums + 2 * ch + NM_IMAGE_SSIM_SUM, (unsigned long long)total);      // two's complement: a negative sum wraps back
        if (total_bad) atomicAdd(sums + 2 * ch + NM_IMAGE_SSIM_NONFINITE, (unsigned long long)total_bad);
    }
}

}  // namespace nm

using namespace nm;

extern "C" {

int nm_image_ssim(const float* d_a, const float* d_b, int32_t height, int32_t width, int32_t channels, double* d_map, int64_t* d_sums,
                  void* stream) {
    NM_REQUIRE(d_a != nullptr && d_b != nullptr && d_sums != nullptr, "bad argument");
    NM_REQUIRE(height >= NM_IMAGE_SSIM_WINDOW && width >= NM_IMAGE_SSIM_WINDOW, "image ssim: image must be at least 11x11");
    NM_REQUIRE(height <= NM_IMAGE_SSIM_MAX_SIDE && width <= NM_IMAGE_SSIM_MAX_SIDE, "image ssim: the sides must be at most 16384");
    NM_REQUIRE(channels >= 1 && channels <= NM_IMAGE_SSIM_MAX_CHANNELS, "image ssim: channels must be in [1, 4]");
    hipStream_t s = static_cast<hipStream_t>(stream);
    NM_HIP_CHECK(hipMemsetAsync(d_sums, 0, sizeof(int64_t) * 2 * channels, s));
    const dim3 grid((width - IS_R + IS_TW - 1) / IS_TW, (height - IS_R + IS_TH - 1) / IS_TH, channels);
    hipLaunchKernelGGL(image_ssim_kernel, grid, dim3(256), 0, s, d_a, d_b, (int)height, (int)width, (int)channels, d_map,
                       reinterpret_cast<unsigned long long*>(d_sums));
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
