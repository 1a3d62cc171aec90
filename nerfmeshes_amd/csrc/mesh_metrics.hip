// Mesh quality (mesh_chamfer, mesh_nerf --target-mesh, the validation chamfer branch; DESIGN.md, "Mesh quality: chamfer
// distance").  Three pieces, every fp32 operation individually rounded (-ffp-contract=off, sqrtf / division correctly
// rounded), so that tests/mesh_metrics.py restates them in numpy bit for bit:
//   1. mm_face_areas / mm_face_weights / mm_scan   area-proportional sampling weights of a triangle mesh as INTEGERS: the area
//                       of a face is 0.5 * |e1 x e2|; the largest area m = f * 2^e (f in [0.5, 1)) is an exact reduction
//                       (non-negative float bits compare as unsigned integers: one atomicMax); the weight of face i is
//                       trunc(area_i * 2^(32-e)), a power-of-two scaling, exact in fp64.  Their inclusive prefix sums (uint64,
//                       the one-workgroup scan of compact.h) are exact and independent of the order anything ran in.
//   2. mm_sample        one thread per draw (u0, u1, u2): t = trunc(u0 * total), face = first i with cdf[i] > t by binary
//                       search (a zero-weight face can never be chosen), pytorch3d's barycentric weights from (u1, u2).
//   3. mm_nearest       the hot kernel: for every query row of x the smallest squared distance to a row of y and the smallest
//                       j that attains it.  A lane keeps 8 queries in registers (four float2 pairs: the three subtractions,
//                       three products and two additions are written on 2-vectors and lower to v_pk_add_f32 /
//                       v_pk_mul_f32); the y rows are read through a wave-uniform address, i.e. by scalar loads into SGPRs
//                       that all 64 lanes share; the only per-pair work besides the 8 flops is one v_min_f32.  The index is
//                       kept off the inner loop: y is walked in tiles of 64 rows, the lane remembers the first tile whose
//                       minimum lowered its running minimum, and rescans that one tile at the end for the first j whose d2
//                       equals the minimum (the same instructions give the same bits).  When the queries alone cannot fill
//                       the device the y rows are split over blockIdx.y and the partial results merge with a 64-bit atomicMin
//                       on (float bits of d2) << 32 | j: non-negative floats order as integers and ties go to the smaller j,
//                       whatever order the workgroups ran in.
//                       NaN: the tile minimum starts as NaN and v_min_f32 returns its non-NaN operand, so a NaN pair never
//                       lowers anything and a tile without a valid pair stays NaN; a row that no pair wins gets (+inf, -1).
// Nothing here allocates or synchronises; the wrappers read the 32-byte header of nm_mesh_face_weights once.
#include <math.h>

#include "compact.h"
#include "nm_internal.h"

namespace nm {

struct MmHeader {                      // the first 32 bytes of nm_mesh_face_weights' workspace
    unsigned long long bad_faces;      // faces with a vertex index outside [0, nv): area 0, weight 0
    unsigned long long total;          // cdf[F-1]
    unsigned int max_bits;             // float bits of the largest area
    unsigned int pad[3];
};

// c = e1 x e2 with e1 = v1 - v0, e2 = v2 - v0; returns |c| = sqrt((cx cx + cy cy) + cz cz)
__device__ __forceinline__ float mm_cross(const float* __restrict__ verts, const int (&v)[3], float (&p)[3][3], float (&c)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) p[a][k] = verts[3 * (int64_t)v[a] + k];
    float e1[3], e2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { e1[k] = p[1][k] - p[0][k]; e2[k] = p[2][k] - p[0][k]; }
    c[0] = e1[1] * e2[2] - e1[2] * e2[1];
    c[1] = e1[2] * e2[0] - e1[0] * e2[2];
    c[2] = e1[0] * e2[1] - e1[1] * e2[0];
    return sqrtf((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
}

__device__ __forceinline__ float mm_area(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t f, int nv,
                                         bool& bad) {
    int v[3];
    bad = !load_face(faces, f, nv, v);
    if (bad) return 0.0f;
    float p[3][3], c[3];
    const float area = 0.5f * mm_cross(verts, v, p, c);
    return area < INFINITY ? area : 0.0f;                            // NaN and +inf count as 0
}

__global__ __launch_bounds__(64) void mm_header_init(MmHeader* hdr) {
    if (threadIdx.x == 0) { hdr->bad_faces = 0ull; hdr->total = 0ull; hdr->max_bits = 0u; }
}

__global__ __launch_bounds__(256) void mm_face_areas(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                     int64_t nf, int nv, float* __restrict__ areas, MmHeader* hdr) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    unsigned int best = 0u;
    unsigned long long nbad = 0ull;
    for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < nf; f += stride) {
        bool bad;
        const float area = mm_area(verts, faces, f, nv, bad);
        if (areas) areas[f] = area;
        nbad += bad;
        best = max(best, __float_as_uint(area));                     // area >= +0: the bits order as the values
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        best = max(best, (unsigned int)__shfl_xor((int)best, off, 64));
        nbad += __shfl_xor(nbad, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (best) atomicMax(&hdr->max_bits, best);
        if (nbad) atomicAdd(&hdr->bad_faces, nbad);
    }
}

// weight = trunc((double) area * 2^(32-e)), m = f * 2^e: written where the prefix sums will stand
__global__ __launch_bounds__(256) void mm_face_weights(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                       int64_t nf, int nv, const MmHeader* __restrict__ hdr,
                                                       unsigned long long* __restrict__ cdf) {
    const double m = (double)__uint_as_float(hdr->max_bits);         // written by the previous launch
    const double scale = m > 0.0 ? ldexp(1.0, 32 - (ilogb(m) + 1)) : 0.0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < nf; f += stride) {
        bool bad;
        const float area = mm_area(verts, faces, f, nv, bad);
        cdf[f] = (unsigned long long)((double)area * scale);         // < 2^32; the product is exact
    }
}

// in-place inclusive prefix sums: compact.h's scan on the 64-bit weights themselves, one workgroup
__global__ __launch_bounds__(SCAN_THREADS) void mm_scan(unsigned long long* __restrict__ cdf, int64_t n, MmHeader* hdr) {
    __shared__ alignas(16) ScanLds<unsigned long long> lds;
    scan_reset(lds);
    for (int64_t start = 0; start < n; start += SCAN_THREADS) {
        const int64_t i = start + threadIdx.x;
        const unsigned long long inclusive = scan_step(i < n ? cdf[i] : 0ull, lds);
        if (i < n) cdf[i] = inclusive;
    }
    if (threadIdx.x == 0) hdr->total = lds.carry;
}

__global__ __launch_bounds__(256) void mm_sample(const float* __restrict__ u, int64_t n, const float* __restrict__ verts, int nv,
                                                 const int32_t* __restrict__ faces, int64_t nf,
                                                 const unsigned long long* __restrict__ cdf, float* __restrict__ points,
                                                 int32_t* __restrict__ face_ids, float* __restrict__ normals) {
    const unsigned long long total = cdf[nf - 1];
    if (total == 0ull) return;                                       // nothing can be sampled: the wrapper reports it
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float u0 = u[3 * i], u1 = u[3 * i + 1], u2 = u[3 * i + 2];
        unsigned long long t = u0 > 0.0f ? (unsigned long long)((double)u0 * (double)total) : 0ull;
        if (t >= total) t = total - 1;                               // only for a draw outside [0, 1)
        int64_t lo = 0, hi = nf - 1;                                 // cdf[nf-1] = total > t: the answer is in [lo, hi]
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (cdf[mid] > t) hi = mid; else lo = mid + 1;
        }
        if (face_ids) face_ids[i] = (int32_t)lo;
        if (!points && !normals) continue;
        int v[3];
        float p[3][3], c[3];
        const bool ok = load_face(faces, lo, nv, v);                   // false only for a cdf that is not this mesh's
        const float len = ok ? mm_cross(verts, v, p, c) : 0.0f;
        const float s = sqrtf(u1);
        const float w0 = 1.0f - s, w1 = s * (1.0f - u2), w2 = s * u2;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (points) points[3 * i + k] = ok ? (w0 * p[0][k] + w1 * p[1][k]) + w2 * p[2][k] : NAN;
            if (normals) normals[3 * i + k] = ok ? c[k] / len : NAN;
        }
    }
}

// ---- nearest neighbour -----------------------------------------------------------------------
typedef float mm_f2 __attribute__((ext_vector_type(2)));

constexpr int NN_THREADS = 256;
constexpr int NN_PAIRS = 4;                          // float2 pairs of queries per lane
constexpr int NN_Q = 2 * NN_PAIRS;                   // queries per lane
constexpr int NN_BLOCK_Q = NN_THREADS * NN_Q;        // queries per workgroup
constexpr int NN_TILE = 64;                          // y rows per tile (the granularity of the index rescan)
constexpr int64_t NN_TARGET_BLOCKS = 2048;           // the y rows are split until the launch has about this many workgroups
constexpr int64_t NN_MIN_CHUNK = 2048;               // ... but never into pieces shorter than this
constexpr unsigned long long NN_EMPTY = (0x7F800000ull << 32) | 0xFFFFFFFFull;   // (+inf, -1)

__device__ __forceinline__ float nn_d2(float qx, float qy, float qz, float yx, float yy, float yz) {
    const float dx = qx - yx, dy = qy - yy, dz = qz - yz;
    return (dx * dx + dy * dy) + dz * dz;
}

__global__ __launch_bounds__(256) void mm_nearest_init(unsigned long long* __restrict__ keys, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) keys[i] = NN_EMPTY;
}

__global__ __launch_bounds__(256) void mm_nearest_finish(const unsigned long long* __restrict__ keys, int64_t n,
                                                         float* __restrict__ dist2, int32_t* __restrict__ index) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    dist2[i] = __uint_as_float((unsigned int)(k >> 32));
    index[i] = (int32_t)(unsigned int)k;                             // 0xFFFFFFFF -> -1
}

// blockIdx.x: NN_BLOCK_Q queries; blockIdx.y: rows [chunk * y, min(m, chunk * (y + 1))) of y, chunk a multiple of NN_TILE
__global__ __launch_bounds__(NN_THREADS) void mm_nearest(const float* __restrict__ x, int64_t n, const float* __restrict__ y,
                                                         int64_t m, int64_t chunk, float* __restrict__ dist2,
                                                         int32_t* __restrict__ index, unsigned long long* __restrict__ keys) {
    const int64_t q0 = (int64_t)blockIdx.x * NN_BLOCK_Q + threadIdx.x;
    mm_f2 qx[NN_PAIRS], qy[NN_PAIRS], qz[NN_PAIRS], best[NN_PAIRS];
    int tile_of[NN_Q];
#pragma unroll
    for (int p = 0; p < NN_PAIRS; ++p) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int64_t q = q0 + (int64_t)(2 * p + h) * NN_THREADS;
            q = q < n ? q : n - 1;                                   // n >= 1 here; the surplus lanes repeat the last query
            qx[p][h] = x[3 * q]; qy[p][h] = x[3 * q + 1]; qz[p][h] = x[3 * q + 2];
            best[p][h] = INFINITY;
            tile_of[2 * p + h] = -1;
        }
    }
    const int64_t j0 = (int64_t)blockIdx.y * chunk;
    const int64_t j1 = j0 + chunk < m ? j0 + chunk : m;
    const int tiles = (int)((j1 - j0 + NN_TILE - 1) / NN_TILE);
    for (int t = 0; t < tiles; ++t) {
        const int64_t ts = j0 + (int64_t)t * NN_TILE;
        const int cnt = (int)(j1 - ts < NN_TILE ? j1 - ts : NN_TILE);
        const float* __restrict__ yt = y + 3 * ts;                   // wave-uniform: scalar loads
        mm_f2 tmin[NN_PAIRS];
#pragma unroll
        for (int p = 0; p < NN_PAIRS; ++p) tmin[p] = mm_f2{NAN, NAN};
        if (cnt == NN_TILE) {
#pragma unroll 8
            for (int j = 0; j < NN_TILE; ++j) {
                const float yx = yt[3 * j], yy = yt[3 * j + 1], yz = yt[3 * j + 2];
#pragma unroll
                for (int p = 0; p < NN_PAIRS; ++p) {
                    const mm_f2 dx = qx[p] - yx, dy = qy[p] - yy, dz = qz[p] - yz;
                    const mm_f2 d2 = (dx * dx + dy * dy) + dz * dz;
                    tmin[p][0] = __builtin_fminf(tmin[p][0], d2[0]);
                    tmin[p][1] = __builtin_fminf(tmin[p][1], d2[1]);
                }
            }
        } else {
            for (int j = 0; j < cnt; ++j) {
                const float yx = yt[3 * j], yy = yt[3 * j + 1], yz = yt[3 * j + 2];
#pragma unroll
                for (int p = 0; p < NN_PAIRS; ++p) {
                    const mm_f2 dx = qx[p] - yx, dy = qy[p] - yy, dz = qz[p] - yz;
                    const mm_f2 d2 = (dx * dx + dy * dy) + dz * dz;
                    tmin[p][0] = __builtin_fminf(tmin[p][0], d2[0]);
                    tmin[p][1] = __builtin_fminf(tmin[p][1], d2[1]);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < NN_PAIRS; ++p) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float tm = tmin[p][h];
                // a lower minimum, or the first tile with a valid pair at all (its minimum may be +inf)
                if (tm < best[p][h] || (tile_of[2 * p + h] < 0 && tm == tm)) {
                    best[p][h] = tm;
                    tile_of[2 * p + h] = t;
                }
            }
        }
    }
#pragma unroll
    for (int p = 0; p < NN_PAIRS; ++p) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t q = q0 + (int64_t)(2 * p + h) * NN_THREADS;
            const int t = tile_of[2 * p + h];
            if (q >= n) continue;
            const float b = best[p][h];
            int found = -1;
            if (t >= 0) {
                const int64_t ts = j0 + (int64_t)t * NN_TILE;
                const int cnt = (int)(j1 - ts < NN_TILE ? j1 - ts : NN_TILE);
                for (int j = cnt - 1; j >= 0; --j) {                 // backwards: the first match is what remains
                    const float* yr = y + 3 * (ts + j);
                    if (nn_d2(qx[p][h], qy[p][h], qz[p][h], yr[0], yr[1], yr[2]) == b) found = (int)(ts + j);
                }
            }
            if (keys) {
                if (found >= 0)
                    atomicMin(keys + q, ((unsigned long long)__float_as_uint(b) << 32) | (unsigned long long)(unsigned)found);
            } else {
                dist2[q] = found >= 0 ? b : INFINITY;
                index[q] = found;
            }
        }
    }
}

// rows of y per blockIdx.y: all of them unless the queries alone leave the device idle
static int64_t nn_chunk(int64_t n, int64_t m) {
    const int64_t bx = (n + NN_BLOCK_Q - 1) / NN_BLOCK_Q;
    int64_t splits = bx ? (NN_TARGET_BLOCKS + bx - 1) / bx : 1;
    const int64_t most = m / NN_MIN_CHUNK;
    if (splits > most) splits = most;
    if (splits > 65535) splits = 65535;
    if (splits <= 1) return m;
    const int64_t chunk = (m + splits - 1) / splits;
    return (chunk + NN_TILE - 1) / NN_TILE * NN_TILE;
}

}  // namespace nm

using namespace nm;

extern "C" {

int64_t nm_mesh_face_weights_workspace_bytes(void) { return 256; }

int nm_mesh_face_weights(const float* d_verts, int64_t num_vertices, const int32_t* d_faces, int64_t num_faces, float* d_areas,
                         uint64_t* d_cdf, void* d_workspace, void* stream) {
    if (require_mesh("mesh face weights", num_vertices, num_faces)) return 2;
    NM_REQUIRE(d_workspace && (num_faces == 0 || (d_faces && d_verts && d_cdf)), "bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    MmHeader* hdr = static_cast<MmHeader*>(d_workspace);
    const int nv = (int)num_vertices;
    hipLaunchKernelGGL(mm_header_init, dim3(1), dim3(64), 0, s, hdr);
    NM_HIP_CHECK(hipGetLastError());
    if (num_faces == 0) return 0;
    const unsigned grid = launch_grid(num_faces, GRID_CAP);
    hipLaunchKernelGGL(mm_face_areas, dim3(grid), dim3(256), 0, s, d_verts, d_faces, num_faces, nv, d_areas, hdr);
    NM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(mm_face_weights, dim3(grid), dim3(256), 0, s, d_verts, d_faces, num_faces, nv, hdr,
                       reinterpret_cast<unsigned long long*>(d_cdf));
    NM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(mm_scan, dim3(1), dim3(SCAN_THREADS), 0, s, reinterpret_cast<unsigned long long*>(d_cdf), num_faces, hdr);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

int nm_mesh_sample_points(const float* d_u, int64_t num_points, const float* d_verts, int64_t num_vertices, const int32_t* d_faces,
                          int64_t num_faces, const uint64_t* d_cdf, float* d_points, int32_t* d_face_ids, float* d_normals,
                          void* stream) {
    NM_REQUIRE(mesh_size_ok(num_vertices) && mesh_size_ok(num_faces) && mesh_size_ok(num_points),
               "mesh sample points: point, vertex and face counts must be in [0, 2^31 - 64)");
    NM_REQUIRE(num_points == 0 || (num_faces > 0 && num_vertices > 0), "mesh sample points: a mesh without faces cannot be sampled");
    NM_REQUIRE(num_points == 0 || (d_u && d_verts && d_faces && d_cdf), "bad argument");
    if (num_points == 0 || (!d_points && !d_face_ids && !d_normals)) return 0;
    hipLaunchKernelGGL(mm_sample, dim3(launch_grid(num_points, GRID_CAP)), dim3(256), 0, static_cast<hipStream_t>(stream), d_u,
                       num_points, d_verts, (int)num_vertices, d_faces, num_faces, reinterpret_cast<const unsigned long long*>(d_cdf),
                       d_points, d_face_ids, d_normals);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

int64_t nm_points_nearest_workspace_bytes(int64_t num_x, int64_t num_y) {
    if (!mesh_size_ok(num_x) || !mesh_size_ok(num_y)) return 0;
    return align_up(num_x * 8, 256) + 256;
}

int nm_points_nearest(const float* d_x, int64_t num_x, const float* d_y, int64_t num_y, float* d_dist2, int32_t* d_index,
                      void* d_workspace, void* stream) {
    NM_REQUIRE(mesh_size_ok(num_x) && mesh_size_ok(num_y), "points nearest: both point counts must be in [0, 2^31 - 64)");
    NM_REQUIRE(num_x == 0 || (d_x && d_dist2 && d_index && d_workspace), "bad argument");
    NM_REQUIRE(num_y == 0 || d_y, "bad argument");
    if (num_x == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned long long* keys = static_cast<unsigned long long*>(d_workspace);
    const unsigned flat = launch_grid(num_x);
    const int64_t chunk = nn_chunk(num_x, num_y);
    const bool split = num_y == 0 || chunk < num_y;                  // no rows of y: the empty keys are the answer
    if (split) {
        hipLaunchKernelGGL(mm_nearest_init, dim3(flat), dim3(256), 0, s, keys, num_x);
        NM_HIP_CHECK(hipGetLastError());
    }
    if (num_y) {
        const dim3 grid((unsigned)((num_x + NN_BLOCK_Q - 1) / NN_BLOCK_Q), (unsigned)((num_y + chunk - 1) / chunk));
        hipLaunchKernelGGL(mm_nearest, grid, dim3(NN_THREADS), 0, s, d_x, num_x, d_y, num_y, chunk, d_dist2, d_index,
                           split ? keys : nullptr);
        NM_HIP_CHECK(hipGetLastError());
    }
    if (split) {
        hipLaunchKernelGGL(mm_nearest_finish, dim3(flat), dim3(256), 0, s, keys, num_x, d_dist2, d_index);
        NM_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
