// Super-sampled marching cubes (mesh_nerf --super-sampling ss): the plain res^3 mesh, then every EDGE vertex moved along
// its own edge to the first sign change among the ss samples strictly inside that edge.  The reference's sketch
// (src/mesh_nerf.py:95-128) builds three grids that are (ss+1)-times denser along one axis each -- ~1 G points at 480^3,
// ss = 2 -- although only the ss samples inside the ~1 % of edges the surface cuts can change the result; here only
// those are generated (nm_mc_edge_points), evaluated (nm_mlp_sample_density) and used (nm_mc_refine_vertices).
// The edge of a vertex comes from the emit pass's vertex scratch (nm_mc_vertex_edges, marching_cubes.hip).
// Both kernels are one thread per vertex and move ~12 (ss+1) + 16 bytes per vertex: no workspace, no atomics.
#include <math.h>

#include "nm_internal.h"

namespace nm {

constexpr double MC_SK_EPS = 2.220446049250313e-16;   // skimage's "FLT_EPSILON" (marching_cubes.hip: SK_EPS)
constexpr int MC_SS_MAX = 64;

struct AxisPtrs { const float* p[3]; };

__device__ __forceinline__ const float* axis_sel(const AxisPtrs& a, int k) { return k == 0 ? a.p[0] : (k == 1 ? a.p[1] : a.p[2]); }

// key -> (i0, i1, i2, axis), the edge's lower voxel clamped into the grid (keys come from nm_mc_vertex_edges; a stray key
// must not turn into a stray address)
__device__ __forceinline__ void decode_key(int64_t key, int n0, int n1, int n2, int (&i)[3], int& axis) {
    axis = (int)(key & 3);
    const int64_t vox = key >> 2, plane = (int64_t)n1 * n2;
    int64_t z = vox / plane;
    const int64_t rem = vox - z * plane;
    const int64_t y = rem / n2, x = rem - y * n2;
    i[0] = (int)min(max(z, (int64_t)0), (int64_t)n0 - 1);
    i[1] = (int)min(max(y, (int64_t)0), (int64_t)n1 - 1);
    i[2] = (int)min(max(x, (int64_t)0), (int64_t)n2 - 1);
}

__global__ __launch_bounds__(256) void mc_edge_points(const int64_t* __restrict__ keys, int64_t nverts, int n0, int n1, int n2,
                                                      int ss, AxisPtrs base, AxisPtrs fine, float* __restrict__ points) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nverts) return;
    int i[3], axis;
    decode_key(keys[r], n0, n1, n2, i, axis);
    const int n[3] = {n0, n1, n2};
    float p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = axis_sel(base, k)[i[k]];
    float* out = points + r * 3 * ss;
    if (axis == 3) {                   // centre vertex: any in-range point, never looked at
        for (int s = 0; s < ss; ++s) { out[3 * s] = p[0]; out[3 * s + 1] = p[1]; out[3 * s + 2] = p[2]; }
        return;
    }
    const int n_a = axis == 0 ? n[0] : (axis == 1 ? n[1] : n[2]);
    const int ia = min(axis == 0 ? i[0] : (axis == 1 ? i[1] : i[2]), n_a - 2);
    const float* f = axis_sel(fine, axis) + (int64_t)ia * (ss + 1);
    for (int s = 1; s <= ss; ++s) {
        const float c = f[s];
        float* q = out + 3 * (s - 1);
        q[0] = axis == 0 ? c : p[0];
        q[1] = axis == 1 ? c : p[1];
        q[2] = axis == 2 ? c : p[2];
    }
}

__global__ __launch_bounds__(256) void mc_refine(const float* __restrict__ vol, int n0, int n1, int n2, int zg0, double iso,
                                                 const int64_t* __restrict__ keys, int64_t nverts, int ss,
                                                 const float* __restrict__ fine_sigma, float* __restrict__ verts) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nverts) return;
    const int64_t key = keys[r];
    const int axis = (int)(key & 3);
    if (axis == 3) return;                                   // centre vertices keep their position
    const int64_t vox = (key >> 2) - (int64_t)zg0 * n1 * n2;  // the slab's local voxel
    const int64_t plane = (int64_t)n1 * n2;
    if (vox < 0 || vox >= (int64_t)n0 * plane) return;
    const int64_t z = vox / plane, rem = vox - z * plane, y = rem / n2, x = rem - y * n2;
    const int64_t ia = axis == 0 ? z : (axis == 1 ? y : x);
    const int n_a = axis == 0 ? n0 : (axis == 1 ? n1 : n2);
    if (ia + 1 >= n_a) return;                               // not an edge of this volume
    const int64_t step = axis == 0 ? plane : (axis == 1 ? (int64_t)n2 : 1);
    double prev = (double)vol[vox] - iso;
    const double hi = (double)vol[vox + step] - iso;
    const float* f = fine_sigma + r * ss;
    int m = -1;
    double dm = 0.0, dn = 0.0;
    for (int s = 0; s <= ss; ++s) {                          // the first sign change, counted from the lower end
        const double next = s < ss ? (double)f[s] - iso : hi;
        if ((prev > 0) != (next > 0)) { m = s; dm = prev; dn = next; break; }
        prev = next;
    }
    if (m < 0) return;                                       // not a cut edge: nothing to move
    const double w1 = 1.0 / (MC_SK_EPS + fabs(dm)), w2 = 1.0 / (MC_SK_EPS + fabs(dn));
    const double t = ((double)m + w2 / (w1 + w2)) / (double)(ss + 1);
    const int64_t ig = axis == 0 ? ia + zg0 : ia;            // vertices carry global plane indices
    verts[3 * r + axis] = (float)((double)ig + t);
}

static bool fine_fits(int n, int ss) { return (int64_t)(n - 1) * (ss + 1) + 1 <= INT32_MAX; }

}  // namespace nm

using namespace nm;

extern "C" {

int nm_mc_edge_points(const int64_t* d_keys, int64_t V, int32_t n0, int32_t n1, int32_t n2, int32_t ss,
                      const float* d_base0, const float* d_base1, const float* d_base2, const float* d_fine0,
                      const float* d_fine1, const float* d_fine2, float* d_points, void* stream) {
    NM_REQUIRE(ss >= 0 && ss <= MC_SS_MAX, "super sampling must be in [0, 64]");
    NM_REQUIRE(n0 >= 2 && n1 >= 2 && n2 >= 2, "Input array must be at least 2x2x2.");
    NM_REQUIRE(fine_fits(n0, ss) && fine_fits(n1, ss) && fine_fits(n2, ss), "super sampling: a fine axis does not fit int32");
    NM_REQUIRE(V >= 0 && V < (int64_t(1) << 40), "bad vertex count");
    if (V == 0) return 0;
    NM_REQUIRE(d_keys && d_base0 && d_base1 && d_base2, "bad argument");
    if (ss == 0) return 0;
    NM_REQUIRE(d_fine0 && d_fine1 && d_fine2 && d_points, "bad argument");
    const AxisPtrs base{{d_base0, d_base1, d_base2}}, fine{{d_fine0, d_fine1, d_fine2}};
    hipLaunchKernelGGL(mc_edge_points, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), d_keys, V,
                       (int)n0, (int)n1, (int)n2, (int)ss, base, fine, d_points);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

int nm_mc_refine_vertices(const float* d_volume, int32_t n0, int32_t n1, int32_t n2, int32_t z_global, double iso,
                          const int64_t* d_keys, int64_t V, int32_t ss, const float* d_fine_sigma, float* d_verts,
                          void* stream) {
    NM_REQUIRE(ss >= 0 && ss <= MC_SS_MAX, "super sampling must be in [0, 64]");
    NM_REQUIRE(n0 >= 2 && n1 >= 2 && n2 >= 2, "Input array must be at least 2x2x2.");
    NM_REQUIRE(z_global >= 0 && (int64_t)z_global + n0 <= INT32_MAX, "bad global plane index");
    NM_REQUIRE(fine_fits(n0 + z_global, ss) && fine_fits(n1, ss) && fine_fits(n2, ss), "super sampling: a fine axis does not fit int32");
    NM_REQUIRE(V >= 0 && V < (int64_t(1) << 40), "bad vertex count");
    if (V == 0) return 0;
    NM_REQUIRE(d_volume && d_keys && d_verts && (ss == 0 || d_fine_sigma), "bad argument");
    hipLaunchKernelGGL(mc_refine, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), d_volume,
                       (int)n0, (int)n1, (int)n2, (int)z_global, iso, d_keys, V, (int)ss, d_fine_sigma, d_verts);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
