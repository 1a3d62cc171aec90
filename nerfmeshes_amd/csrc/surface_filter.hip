// Surface point cloud (mesh_surface_ray): the post-processing of one rendered view on the device.  The reference
// (src/mesh_surface_ray.py:115-141) takes the surface point p = o + d * depth of every ray, counts for every pixel how many
// pixels of its (2 step + 1)^2 window (clamped at the image border, centre and clamped duplicates included) have a surface
// point closer than sqrt(dist_threshold), keeps the pixel when enough do and its depth is positive, and compacts points,
// -d and the colours with boolean-mask indexing.  Here:
//   1. surface_filter   a workgroup (64 x 4 threads) owns a 64-column x 16-row image tile; the surface points of the tile plus a
//                       step-wide halo are computed ONCE into LDS (three fp32 planes: consecutive lanes read consecutive
//                       words of a plane, so no padding is needed), every thread then votes over its window from LDS for its
//                       4 rows.  The keep bits leave each wave as one __ballot word per (row, 64-column segment): the words in
//                       memory order are the pixels in row-major order.
//   2. surface_scan     the ordered compaction of compact.h over those words: one workgroup takes the prefix sums of their
//                       popcounts and the total, so the output order is the pixel order whatever order the tiles ran in.
//   3. surface_gather   one thread per pixel: a kept pixel's row is its rank among the set bits.
// All arithmetic is fp32 with two roundings per multiply-add (-ffp-contract=off) in torch's order of operations, so votes,
// mask and gathered rows equal the restated reference (tests/surface_filter.py) bit for bit.
// Memory-bound and small: 28 -- 44 B read and at most 41 B written per pixel, 640 000 pixels per view.
#include <math.h>

#include "compact.h"
#include "nm_internal.h"

namespace nm {

constexpr int SF_TW = 64;          // tile columns = one wave = one ballot word
constexpr int SF_TH = 16;          // tile rows: 4 waves x 4 rows
constexpr int SF_ROWS_PER_WAVE = 4;
constexpr int SF_MAX_STEP = 8;

struct SfIn {
    const float* origins;    // (1,3) shared or (H*W,3)
    const float* dirs;       // (H*W,3)
    const float* depth;      // (H*W)
    const float* opacity;    // (H*W) or null
    float min_opacity;
    int per_ray_o;
    int height, width;
};

__device__ __forceinline__ float sf_depth(const SfIn& in, int64_t pix) {
    const float z = in.depth[pix];
    if (in.opacity == nullptr) return z;
    return in.opacity[pix] >= in.min_opacity ? z : 0.0f;
}

__device__ __forceinline__ void sf_point(const SfIn& in, int64_t pix, float z, float (&p)[3]) {
    const float* o = in.origins + (in.per_ray_o ? 3 * pix : 0);
    const float* d = in.dirs + 3 * pix;
#pragma unroll
    for (int k = 0; k < 3; ++k) { const float t = d[k] * z; p[k] = o[k] + t; }
}

__global__ __launch_bounds__(256) void surface_filter(SfIn in, int step, float thr, int min_votes, int words_per_row,
                                                      int32_t* __restrict__ votes_out, uint8_t* __restrict__ keep_out,
                                                      unsigned long long* __restrict__ words) {
    extern __shared__ float sf_lds[];
    const int pw = SF_TW + 2 * step, ph = SF_TH + 2 * step, plane = pw * ph;
    float* sx = sf_lds;
    float* sy = sf_lds + plane;
    float* sz = sf_lds + 2 * plane;
    const int c0 = blockIdx.x * SF_TW, r0 = blockIdx.y * SF_TH;
    const int tid = threadIdx.y * SF_TW + threadIdx.x;
    for (int i = tid; i < plane; i += 256) {
        const int tr = i / pw, tc = i - tr * pw;
        const int r = min(max(r0 - step + tr, 0), in.height - 1), c = min(max(c0 - step + tc, 0), in.width - 1);
        const int64_t pix = (int64_t)r * in.width + c;
        float p[3];
        sf_point(in, pix, sf_depth(in, pix), p);
        sx[i] = p[0]; sy[i] = p[1]; sz[i] = p[2];
    }
    __syncthreads();
    const int col = c0 + threadIdx.x;
    for (int k = 0; k < SF_ROWS_PER_WAVE; ++k) {
        const int lr = threadIdx.y * SF_ROWS_PER_WAVE + k, row = r0 + lr;
        if (row >= in.height) break;                                  // uniform over the wave
        const bool inside = col < in.width;
        int votes = 0;
        bool keep = false;
        if (inside) {
            const int ci = (lr + step) * pw + threadIdx.x + step;
            const float px = sx[ci], py = sy[ci], pz = sz[ci];
            for (int a = -step; a <= step; ++a) {
                const int base = ci + a * pw;
                for (int b = -step; b <= step; ++b) {
                    const float dx = sx[base + b] - px, dy = sy[base + b] - py, dz = sz[base + b] - pz;
                    const float d2 = (dx * dx + dy * dy) + dz * dz;   // torch's sum over a last dimension of 3
                    votes += d2 < thr ? 1 : 0;
                }
            }
            const int64_t pix = (int64_t)row * in.width + col;
            keep = votes >= min_votes && sf_depth(in, pix) > 0.0f;
            if (votes_out) votes_out[pix] = votes;
            if (keep_out) keep_out[pix] = keep ? 1 : 0;
        }
        const unsigned long long word = __ballot(keep);
        if (threadIdx.x == 0) words[(int64_t)row * words_per_row + blockIdx.x] = word;
    }
}

// one workgroup: the prefix sums of the image's words (compact.h) and the number of kept pixels
__global__ __launch_bounds__(SCAN_THREADS) void surface_scan(const unsigned long long* __restrict__ words, int64_t nwords,
                                                             uint32_t* __restrict__ prefix, int64_t* __restrict__ total,
                                                             int64_t* __restrict__ count_out) {
    const uint32_t kept = popcount_prefix_sums(words, nwords, prefix);
    if (threadIdx.x == 0) {
        *total = (int64_t)kept;
        if (count_out) *count_out = (int64_t)kept;
    }
}

struct SfOut {
    float* points;
    float* normals;
    float* colors;
    uint8_t* colors_u8;
};

__device__ __forceinline__ uint8_t sf_u8(float c) {
    const float v = fminf(fmaxf(c * 255.0f, 0.0f), 255.0f);        // fmaxf(NaN, 0) = 0
    return (uint8_t)(int)v;                                          // truncation, as numpy's cast to u1
}

__global__ __launch_bounds__(256) void surface_gather(SfIn in, const float* __restrict__ rgb, int words_per_row,
                                                      const unsigned long long* __restrict__ words,
                                                      const uint32_t* __restrict__ prefix, int64_t row_offset,
                                                      int64_t capacity, SfOut out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t w = t >> 6;
    const int lane = (int)(t & 63);
    if (w >= (int64_t)in.height * words_per_row) return;
    const int row = (int)(w / words_per_row), col = (int)(w - (int64_t)row * words_per_row) * SF_TW + lane;
    if (col >= in.width) return;
    if (!bit_test(words + w, lane)) return;
    const int64_t dst = row_offset + bit_rank(words + w, prefix + w, lane);
    if (dst < 0 || dst >= capacity) return;                          // never past the caller's arrays
    const int64_t pix = (int64_t)row * in.width + col;
    float p[3];
    sf_point(in, pix, sf_depth(in, pix), p);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (out.points) out.points[3 * dst + k] = p[k];
        if (out.normals) out.normals[3 * dst + k] = -in.dirs[3 * pix + k];
        if (rgb) {
            const float c = rgb[3 * pix + k];
            if (out.colors) out.colors[3 * dst + k] = c;
            if (out.colors_u8) out.colors_u8[3 * dst + k] = sf_u8(c);
        }
    }
}

static int64_t sf_words(int64_t h, int64_t w) { return h * ((w + SF_TW - 1) / SF_TW); }

struct SfWorkspace { unsigned long long* words; uint32_t* prefix; int64_t* total; int64_t bytes; };

static SfWorkspace sf_carve(const void* ws, int64_t nwords) {
    Carver c(ws, 16);
    SfWorkspace s;
    s.words = c.take<unsigned long long>(nwords);
    s.prefix = c.take<uint32_t>(nwords);
    s.total = c.take<int64_t>(2);                                    // the count and 8 spare bytes
    s.bytes = c.offset;
    return s;
}

static bool sf_sizes_ok(int32_t h, int32_t w) { return h > 0 && w > 0 && (int64_t)h * w <= (int64_t(1) << 30); }

}  // namespace nm

using namespace nm;

extern "C" {

int64_t nm_surface_filter_workspace_bytes(int32_t height, int32_t width) {
    if (!sf_sizes_ok(height, width)) return 0;
    return sf_carve(nullptr, sf_words(height, width)).bytes;
}

int nm_surface_filter(const float* d_origins, int per_ray_o, const float* d_dirs, const float* d_depth,
                      const float* d_opacity, double min_opacity, int32_t height, int32_t width, int32_t step,
                      double dist_threshold, int32_t min_votes, int32_t* d_votes, uint8_t* d_keep, int64_t* d_count,
                      void* d_workspace, void* stream) {
    NM_REQUIRE(sf_sizes_ok(height, width), "surface filter: height and width must be positive, height * width <= 2^30");
    NM_REQUIRE(step >= 0 && step <= SF_MAX_STEP, "surface filter: step must be in [0, 8]");
    NM_REQUIRE(d_origins && d_dirs && d_depth && d_workspace, "bad argument");
    const SfIn in{d_origins, d_dirs, d_depth, d_opacity, (float)min_opacity, per_ray_o ? 1 : 0, (int)height, (int)width};
    const int wpr = (width + SF_TW - 1) / SF_TW;
    const int64_t nwords = sf_words(height, width);
    const SfWorkspace ws = sf_carve(d_workspace, nwords);
    const size_t lds = sizeof(float) * 3 * (SF_TW + 2 * step) * (SF_TH + 2 * step);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // `fp32 tensor < Python float` compares in fp32: the threshold is rounded once, here
    hipLaunchKernelGGL(surface_filter, dim3((unsigned)wpr, (unsigned)((height + SF_TH - 1) / SF_TH)), dim3(SF_TW, 4), lds, s, in,
                       (int)step, (float)dist_threshold, (int)min_votes, wpr, d_votes, d_keep, ws.words);
    NM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(surface_scan, dim3(1), dim3(SCAN_THREADS), 0, s, ws.words, nwords, ws.prefix, ws.total, d_count);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

int nm_surface_gather(const void* d_workspace, const float* d_origins, int per_ray_o, const float* d_dirs,
                      const float* d_depth, const float* d_opacity, double min_opacity, const float* d_rgb, int32_t height,
                      int32_t width, int64_t row_offset, int64_t capacity, float* d_points, float* d_normals,
                      float* d_colors, uint8_t* d_colors_u8, void* stream) {
    NM_REQUIRE(sf_sizes_ok(height, width), "surface gather: height and width must be positive, height * width <= 2^30");
    NM_REQUIRE(row_offset >= 0 && capacity >= row_offset, "surface gather: bad row offset / capacity");
    NM_REQUIRE(d_workspace && d_origins && d_dirs && d_depth, "bad argument");
    NM_REQUIRE(d_rgb || (!d_colors && !d_colors_u8), "surface gather: colour outputs need the rendered colours");
    if (capacity == row_offset) return 0;
    const SfIn in{d_origins, d_dirs, d_depth, d_opacity, (float)min_opacity, per_ray_o ? 1 : 0, (int)height, (int)width};
    const int wpr = (width + SF_TW - 1) / SF_TW;
    const int64_t nwords = sf_words(height, width);
    const SfWorkspace ws = sf_carve(d_workspace, nwords);
    const SfOut out{d_points, d_normals, d_colors, d_colors_u8};
    hipLaunchKernelGGL(surface_gather, dim3(launch_grid(nwords * 64)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       in, d_rgb, wpr, ws.words, ws.prefix, row_offset, capacity, out);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
