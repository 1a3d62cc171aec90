// Fusion of rendered depth maps into a truncated signed distance field (mesh_nerf --geometry tsdf; DESIGN.md, "TSDF geometry"):
// every voxel of a range of the grid is projected into every view, the depth the view saw along that pixel is compared with the
// voxel's own camera depth, and the truncated differences are averaged.  fp64 with every operation rounded on its own
// (-ffp-contract=off, IEEE division), the views in index order, so that a numpy restatement (tests/tsdf_fuse.py) reproduces the
// field, the observation counts and the three voxel counters bit for bit.  THE RULE is written out in include/nerfmeshes_hip.h
// ("TSDF fusion"); the comments below name its paragraphs.  The order of the operations, for voxel p and view v:
//   dx = px - tx, dy = py - ty, dz = pz - tz
//   cx = (r00 dx + r10 dy) + r20 dz      cy = (r01 dx + r11 dy) + r21 dz      cz = (r02 dx + r12 dy) + r22 dz      z = -cz
//   col = rint((cx / z) focal + 0.5 W)   row = rint(0.5 H - (cy / z) focal)
//   s = z - D                            t = max(-1, s / trunc)               sum = sum + t
//   phi = (float)(sum / (double) n)
// Three kernels, all on the caller's stream, in the caller's workspace:
//   views    the host's nm_view array -> 16 doubles per view in the workspace (rotation by columns, position, focal), batches of
//            16 views passed by value: no host memory is read after the call returns;
//   hit      "hit": depth and the opacity test merged into one fp32 map -- the depth of a hit, 0 for a miss --, so that the
//            loop over the views has ONE gather per voxel and view;
//   fuse     one lane per voxel along the fastest axis, the loop over the views INSIDE: sum, n and the occluded flag live in
//            registers and every voxel is written once.  The view's 13 constants are read through a wave-uniform pointer (scalar
//            loads); a view in front of which no lane of the wave lies is skipped before its two divisions.  "counters": the
//            three classes are counted per wave (ballot + popcount), added over the 4 waves in LDS, and one integer atomicAdd
//            per workgroup and non-zero class reaches the device counters: integer addition does not depend on the order the
//            workgroups ran in.
// Nothing allocates and nothing synchronises with the host: the entry can be captured into a graph.
#include "nm_internal.h"

namespace nm {

constexpr int TF_ROW = 16;                  // doubles per view of the table: r00 r10 r20 | r01 r11 r21 | r02 r12 r22 | tx ty tz | focal | 3 unused
constexpr int TF_BATCH = 16;                // views per launch of the table kernel: 2 KiB of kernel arguments
constexpr int TF_MAX_SIDE = 16384;

struct TsdfViewBatch { double row[TF_BATCH][TF_ROW]; };

inline int64_t tsdf_table_bytes(int64_t num_views) { return (num_views * TF_ROW * (int64_t)sizeof(double) + 255) & ~(int64_t)255; }

__global__ __launch_bounds__(TF_BATCH * TF_ROW) void tsdf_views_kernel(const TsdfViewBatch batch, int views, double* __restrict__ table) {
    const int i = threadIdx.x;
    if (i < views * TF_ROW) table[i] = batch.row[i / TF_ROW][i % TF_ROW];
}

__device__ __forceinline__ bool tf_finite32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// "hit": D is finite and > 0, and the opacity -- where there is one -- is >= min_opacity (a NaN opacity is not)
__global__ __launch_bounds__(256) void tsdf_hit_kernel(const float* __restrict__ depth, const float* __restrict__ opacity, int64_t pixels,
                                                       double min_opacity, float* __restrict__ hit) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * 256) {
        const float d = depth[i];
        bool ok = tf_finite32(d) && d > 0.0f;
        if (opacity != nullptr) ok = ok && ((double)opacity[i] >= min_opacity);
        hit[i] = ok ? d : 0.0f;
    }
}

__global__ __launch_bounds__(256) void tsdf_fuse_kernel(const double* __restrict__ table, int num_views, const float* __restrict__ hit,
                                                        int height, int width, const float* __restrict__ ax0,
                                                        const float* __restrict__ ax1, const float* __restrict__ ax2, int n1, int n2,
                                                        int64_t first, int64_t count, double trunc, double near,
                                                        float* __restrict__ field, int32_t* __restrict__ observations,
                                                        unsigned long long* counts) {
    __shared__ int wave_counts[4][3];
    const int tid = threadIdx.x;
    const int64_t gid = (int64_t)blockIdx.x * 256 + tid;
    const bool live = gid < count;                      // no lane leaves early: the wave votes below need all of them
    double px = 0.0, py = 0.0, pz = 0.0;
    if (live) {
        const int64_t idx = first + gid;
        const int64_t rest = idx / n2;
        const int i2 = (int)(idx - rest * n2);
        const int64_t i0 = rest / n1;
        const int i1 = (int)(rest - i0 * n1);
        px = (double)ax0[i0];
        py = (double)ax1[i1];
        pz = (double)ax2[i2];
    }
    const double half_w = 0.5 * (double)width, half_h = 0.5 * (double)height;
    const double last_col = (double)(width - 1), last_row = (double)(height - 1);
    const int64_t image = (int64_t)height * width;
    double sum = 0.0;
    int n = 0;
    bool occluded = false;
    for (int v = 0; v < num_views; ++v) {
        const double* __restrict__ c = table + (int64_t)v * TF_ROW;              // the same in every lane
        const double dx = px - c[9], dy = py - c[10], dz = pz - c[11];
        const double z0 = c[6] * dx, z1 = c[7] * dy, z2 = c[8] * dz;
        const double cz = (z0 + z1) + z2;
        const double z = -cz;
        bool in = live && (z >= near);
        if (!__any(in)) continue;
        const double x0 = c[0] * dx, x1 = c[1] * dy, x2 = c[2] * dz;
        const double y0 = c[3] * dx, y1 = c[4] * dy, y2 = c[5] * dz;
        const double cx = (x0 + x1) + x2, cy = (y0 + y1) + y2;
        const double focal = c[12];
        const double qx = cx / z, qy = cy / z;
        const double fx = qx * focal, fy = qy * focal;
        const double col = rint(fx + half_w), row = rint(half_h - fy);           // round half to even
        in = in && col >= 0.0 && col <= last_col && row >= 0.0 && row <= last_row;
        if (in) {
            const float d = hit[(int64_t)v * image + (int64_t)(int)row * width + (int)col];
            if (d > 0.0f) {
                const double s = z - (double)d;
                if (s > trunc) {
                    occluded = true;
                } else {
                    const double q = s / trunc;
                    const double t = q < -1.0 ? -1.0 : q;
                    sum = sum + t;
                    ++n;
                }
            } else {                                                             // the ray saw free space all the way
                sum = sum + -1.0;
                ++n;
            }
        }
    }
    if (live) {
        field[gid] = n > 0 ? (float)(sum / (double)n) : (occluded ? 1.0f : -1.0f);
        if (observations != nullptr) observations[gid] = n;
    }
    // "counters"
    const int seen = __popcll(__ballot(live && n > 0));
    const int inside = __popcll(__ballot(live && n == 0 && occluded));
    const int outside = __popcll(__ballot(live && n == 0 && !occluded));
    if ((tid & 63) == 0) {
        wave_counts[tid >> 6][NM_TSDF_OBSERVED] = seen;
        wave_counts[tid >> 6][NM_TSDF_INTERIOR] = inside;
        wave_counts[tid >> 6][NM_TSDF_OUTSIDE] = outside;
    }
    __syncthreads();
    if (tid < 3) {
        const int total = (wave_counts[0][tid] + wave_counts[1][tid]) + (wave_counts[2][tid] + wave_counts[3][tid]);
        if (total) atomicAdd(counts + tid, (unsigned long long)total);
    }
}

}  // namespace nm

using namespace nm;

extern "C" {

int64_t nm_tsdf_workspace_bytes(int64_t num_views, int32_t height, int32_t width) {
    if (num_views < 1 || num_views > NM_TSDF_MAX_VIEWS || height < 1 || width < 1 || height > TF_MAX_SIDE || width > TF_MAX_SIDE) return 0;
    return tsdf_table_bytes(num_views) + num_views * (int64_t)height * width * (int64_t)sizeof(float);
}

int nm_tsdf_integrate(const nm_view* views, int64_t num_views, const float* d_depth, const float* d_opacity, const float* d_ax0,
                      const float* d_ax1, const float* d_ax2, int32_t n0, int32_t n1, int32_t n2, int64_t first, int64_t count,
                      double trunc, double near, double min_opacity, void* d_workspace, float* d_field, int32_t* d_observations,
                      int64_t* d_counts, void* stream) {
    NM_REQUIRE(views != nullptr && d_depth != nullptr && d_ax0 != nullptr && d_ax1 != nullptr && d_ax2 != nullptr
                   && d_workspace != nullptr && d_counts != nullptr,
               "bad argument");
    NM_REQUIRE(num_views >= 1 && num_views <= NM_TSDF_MAX_VIEWS, "tsdf: the number of views must be in [1, 1024]");
    const int32_t height = views[0].height, width = views[0].width;
    NM_REQUIRE(height >= 1 && width >= 1 && height <= TF_MAX_SIDE && width <= TF_MAX_SIDE, "tsdf: the image sides must be in [1, 16384]");
    for (int64_t v = 0; v < num_views; ++v) {
        NM_REQUIRE(views[v].height == height && views[v].width == width, "tsdf: every view must have the same height and width");
        NM_REQUIRE(views[v].use_ndc == 0, "tsdf: NDC views are not supported");
        NM_REQUIRE(views[v].focal > 0.0 && views[v].focal < HUGE_VAL, "tsdf: focal must be finite and > 0");
    }
    NM_REQUIRE(trunc > 0.0 && trunc < HUGE_VAL, "tsdf: trunc must be finite and > 0");
    NM_REQUIRE(near > 0.0 && near < HUGE_VAL, "tsdf: near must be finite and > 0");
    NM_REQUIRE(min_opacity == min_opacity, "tsdf: min_opacity must not be NaN");
    NM_REQUIRE(n0 >= 1 && n1 >= 1 && n2 >= 1, "tsdf: the grid must have at least one voxel per axis");
    NM_REQUIRE((int64_t)n0 * n1 <= INT64_MAX / n2, "tsdf: the grid is beyond the supported sizes");
    const int64_t total = (int64_t)n0 * n1 * n2;
    NM_REQUIRE(first >= 0 && count >= 0 && first <= total && count <= total - first, "tsdf: the voxel range lies outside the grid");
    NM_REQUIRE(d_field != nullptr || count == 0, "bad argument");
    const int64_t blocks = (count + 255) / 256;
    NM_REQUIRE(blocks <= 0x7fffffffll, "tsdf: the voxel range is too long for one call");
    hipStream_t s = static_cast<hipStream_t>(stream);
    NM_HIP_CHECK(hipMemsetAsync(d_counts, 0, sizeof(int64_t) * 3, s));
    if (count == 0) return 0;

    double* table = static_cast<double*>(d_workspace);
    float* hit = reinterpret_cast<float*>(static_cast<char*>(d_workspace) + tsdf_table_bytes(num_views));
    for (int64_t v0 = 0; v0 < num_views; v0 += TF_BATCH) {
        TsdfViewBatch batch;
        memset(&batch, 0, sizeof(batch));
        const int n = (int)(num_views - v0 < TF_BATCH ? num_views - v0 : TF_BATCH);
        for (int k = 0; k < n; ++k) {
            const nm_view& w = views[v0 + k];
            double* r = batch.row[k];
            for (int col = 0; col < 3; ++col)
                for (int a = 0; a < 3; ++a) r[3 * col + a] = (double)w.c2w[4 * a + col];     // column `col` of the rotation
            for (int a = 0; a < 3; ++a) r[9 + a] = (double)w.c2w[4 * a + 3];
            r[12] = w.focal;
        }
        hipLaunchKernelGGL(tsdf_views_kernel, dim3(1), dim3(TF_BATCH * TF_ROW), 0, s, batch, n, table + v0 * TF_ROW);
        NM_HIP_CHECK(hipGetLastError());
    }
    const int64_t pixels = num_views * (int64_t)height * width;
    const int64_t hit_blocks = (pixels + 255) / 256;
    hipLaunchKernelGGL(tsdf_hit_kernel, dim3((unsigned)(hit_blocks < 4096 ? hit_blocks : 4096)), dim3(256), 0, s, d_depth, d_opacity, pixels,
                       min_opacity, hit);
    NM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(tsdf_fuse_kernel, dim3((unsigned)blocks), dim3(256), 0, s, table, (int)num_views, hit, (int)height, (int)width, d_ax0,
                       d_ax1, d_ax2, (int)n1, (int)n2, first, count, trunc, near, d_field, d_observations,
                       reinterpret_cast<unsigned long long*>(d_counts));
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
