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
//   4. pm_records / pm_nearest / pm_finish   the exact distance of every query to the TRIANGLES of a mesh (mesh_chamfer --surface
//                       exact; the arithmetic contract is in include/nerfmeshes_hip.h, "Point to mesh").  A prepass writes one
//                       record of PM_REC floats per face (corners, edge vectors, n = ab x ac, the three 1/|e|^2 and 1/|n|^2; all
//                       NaN for a face with an index out of range, so that none of its pairs can win).  The hot kernel is
//                       mm_nearest with the point replaced by the record: 4 queries per lane in two float2 pairs, the record
//                       read through a wave-uniform address (scalar loads), the per-pair value written once as a template
//                       (pm_pair<mm_f2> in the inner loop, pm_pair<float> in the index rescan: the same operations, hence the
//                       same bits), the tile minimum / first-lowering-tile / rescan rule and the 64-bit atomicMin merge over
//                       blockIdx.y unchanged.  pm_finish decodes the keys and writes the winning face's normal.
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
static int64_t nn_chunk(int64_t n, int64_t m, int64_t block_q) {
    const int64_t bx = (n + block_q - 1) / block_q;
    int64_t splits = bx ? (NN_TARGET_BLOCKS + bx - 1) / bx : 1;
    const int64_t most = m / NN_MIN_CHUNK;
    if (splits > most) splits = most;
    if (splits > 65535) splits = 65535;
    if (splits <= 1) return m;
    const int64_t chunk = (m + splits - 1) / splits;
    return (chunk + NN_TILE - 1) / NN_TILE * NN_TILE;
}

// ---- point to mesh ---------------------------------------------------------------------------
constexpr int PM_REC = 28;                           // floats per face record (16-byte multiple)
constexpr int PM_A = 0, PM_B = 3, PM_C = 6, PM_AB = 9, PM_BC = 12, PM_CA = 15, PM_N = 18, PM_RAB = 21, PM_RBC = 22, PM_RCA = 23,
              PM_RNN = 24;
constexpr int PM_PAIRS = 2;                          // float2 pairs of queries per lane
constexpr int PM_Q = 2 * PM_PAIRS;
constexpr int PM_BLOCK_Q = NN_THREADS * PM_Q;

__device__ __forceinline__ float pm_dot3(const float (&u)[3], const float (&v)[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

__global__ __launch_bounds__(256) void pm_records(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t nf,
                                                  int nv, float* __restrict__ rec) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < nf; f += stride) {
        float* __restrict__ r = rec + PM_REC * f;
        int v[3];
        if (!load_face(faces, f, nv, v)) {
#pragma unroll
            for (int k = 0; k < PM_REC; ++k) r[k] = NAN;
            continue;
        }
        float p[3][3], n[3], ab[3], bc[3], ca[3];
        mm_cross(verts, v, p, n);
#pragma unroll
        for (int k = 0; k < 3; ++k) { ab[k] = p[1][k] - p[0][k]; bc[k] = p[2][k] - p[1][k]; ca[k] = p[0][k] - p[2][k]; }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            r[PM_A + k] = p[0][k]; r[PM_B + k] = p[1][k]; r[PM_C + k] = p[2][k];
            r[PM_AB + k] = ab[k]; r[PM_BC + k] = bc[k]; r[PM_CA + k] = ca[k]; r[PM_N + k] = n[k];
        }
        r[PM_RAB] = 1.0f / pm_dot3(ab, ab);
        r[PM_RBC] = 1.0f / pm_dot3(bc, bc);
        r[PM_RCA] = 1.0f / pm_dot3(ca, ca);
        r[PM_RNN] = 1.0f / pm_dot3(n, n);            // nn = 0 gives +inf: the plane term is then inf or NaN, i.e. unused
        r[25] = r[26] = r[27] = 0.0f;
    }
}

// the per-element pieces of the contract, for one query (float) and for two (mm_f2)
__device__ __forceinline__ float pm_clamp01(float t) { return __builtin_fminf(__builtin_fmaxf(t, 0.0f), 1.0f); }
__device__ __forceinline__ mm_f2 pm_clamp01(mm_f2 t) { return mm_f2{pm_clamp01(t[0]), pm_clamp01(t[1])}; }
__device__ __forceinline__ float pm_min(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ mm_f2 pm_min(mm_f2 a, mm_f2 b) { return mm_f2{pm_min(a[0], b[0]), pm_min(a[1], b[1])}; }
// the plane term where the projection falls inside the face and the term is finite, else +inf
__device__ __forceinline__ float pm_plane(float i1, float i2, float i3, float pl) {
    return (i1 >= 0.0f && i2 >= 0.0f && i3 >= 0.0f && pl < INFINITY) ? pl : INFINITY;
}
__device__ __forceinline__ mm_f2 pm_plane(mm_f2 i1, mm_f2 i2, mm_f2 i3, mm_f2 pl) {
    return mm_f2{pm_plane(i1[0], i2[0], i3[0], pl[0]), pm_plane(i1[1], i2[1], i3[1], pl[1])};
}
// m where `sum` is a number, else NaN
__device__ __forceinline__ float pm_unless_nan(float sum, float m) { return sum == sum ? m : NAN; }
__device__ __forceinline__ mm_f2 pm_unless_nan(mm_f2 sum, mm_f2 m) {
    return mm_f2{pm_unless_nan(sum[0], m[0]), pm_unless_nan(sum[1], m[1])};
}

template <class T>
__device__ __forceinline__ T pm_seg(T qx, T qy, T qz, float ex, float ey, float ez, float r) {
    const T t = pm_clamp01(((qx * ex + qy * ey) + qz * ez) * r);
    const T dx = qx - t * ex, dy = qy - t * ey, dz = qz - t * ez;
    return (dx * dx + dy * dy) + dz * dz;
}

// dot(n, e x q)
template <class T>
__device__ __forceinline__ T pm_side(float nx, float ny, float nz, float ex, float ey, float ez, T qx, T qy, T qz) {
    const T cx = ey * qz - ez * qy, cy = ez * qx - ex * qz, cz = ex * qy - ey * qx;
    return (nx * cx + ny * cy) + nz * cz;
}

// the squared distance of query (px, py, pz) to the face of record r; NaN when a segment term is
template <class T>
__device__ __forceinline__ T pm_pair(T px, T py, T pz, const float* __restrict__ r) {
    const T apx = px - r[PM_A], apy = py - r[PM_A + 1], apz = pz - r[PM_A + 2];
    const T bpx = px - r[PM_B], bpy = py - r[PM_B + 1], bpz = pz - r[PM_B + 2];
    const T cpx = px - r[PM_C], cpy = py - r[PM_C + 1], cpz = pz - r[PM_C + 2];
    const T s1 = pm_seg(apx, apy, apz, r[PM_AB], r[PM_AB + 1], r[PM_AB + 2], r[PM_RAB]);
    const T s2 = pm_seg(bpx, bpy, bpz, r[PM_BC], r[PM_BC + 1], r[PM_BC + 2], r[PM_RBC]);
    const T s3 = pm_seg(cpx, cpy, cpz, r[PM_CA], r[PM_CA + 1], r[PM_CA + 2], r[PM_RCA]);
    const float nx = r[PM_N], ny = r[PM_N + 1], nz = r[PM_N + 2];
    const T i1 = pm_side(nx, ny, nz, r[PM_AB], r[PM_AB + 1], r[PM_AB + 2], apx, apy, apz);
    const T i2 = pm_side(nx, ny, nz, r[PM_BC], r[PM_BC + 1], r[PM_BC + 2], bpx, bpy, bpz);
    const T i3 = pm_side(nx, ny, nz, r[PM_CA], r[PM_CA + 1], r[PM_CA + 2], cpx, cpy, cpz);
    const T h = (nx * apx + ny * apy) + nz * apz;
    const T pl = pm_plane(i1, i2, i3, (h * h) * r[PM_RNN]);
    // every term is >= +0 or NaN: the sum is NaN exactly when one of the three segment terms is
    return pm_unless_nan((s1 + s2) + s3, pm_min(pm_min(s1, s2), pm_min(s3, pl)));
}

// blockIdx.x: PM_BLOCK_Q queries; blockIdx.y: faces [chunk * y, min(nf, chunk * (y + 1))), chunk a multiple of NN_TILE
__global__ __launch_bounds__(NN_THREADS) void pm_nearest(const float* __restrict__ x, int64_t n, const float* __restrict__ rec,
                                                         int64_t nf, int64_t chunk, float* __restrict__ dist2,
                                                         int32_t* __restrict__ face, unsigned long long* __restrict__ keys) {
    const int64_t q0 = (int64_t)blockIdx.x * PM_BLOCK_Q + threadIdx.x;
    mm_f2 qx[PM_PAIRS], qy[PM_PAIRS], qz[PM_PAIRS], best[PM_PAIRS];
    int tile_of[PM_Q];
#pragma unroll
    for (int p = 0; p < PM_PAIRS; ++p) {
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
    const int64_t j1 = j0 + chunk < nf ? j0 + chunk : nf;
    const int tiles = (int)((j1 - j0 + NN_TILE - 1) / NN_TILE);
    for (int t = 0; t < tiles; ++t) {
        const int64_t ts = j0 + (int64_t)t * NN_TILE;
        const int cnt = (int)(j1 - ts < NN_TILE ? j1 - ts : NN_TILE);
        const float* __restrict__ rt = rec + PM_REC * ts;            // wave-uniform: scalar loads
        mm_f2 tmin[PM_PAIRS];
#pragma unroll
        for (int p = 0; p < PM_PAIRS; ++p) tmin[p] = mm_f2{NAN, NAN};
#pragma unroll 2
        for (int j = 0; j < cnt; ++j) {
#pragma unroll
            for (int p = 0; p < PM_PAIRS; ++p) tmin[p] = pm_min(tmin[p], pm_pair<mm_f2>(qx[p], qy[p], qz[p], rt + PM_REC * j));
        }
#pragma unroll
        for (int p = 0; p < PM_PAIRS; ++p) {
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
    for (int p = 0; p < PM_PAIRS; ++p) {
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
                for (int j = cnt - 1; j >= 0; --j)                   // backwards: the first match is what remains
                    if (pm_pair<float>(qx[p][h], qy[p][h], qz[p][h], rec + PM_REC * (ts + j)) == b) found = (int)(ts + j);
            }
            if (keys) {
                if (found >= 0)
                    atomicMin(keys + q, ((unsigned long long)__float_as_uint(b) << 32) | (unsigned long long)(unsigned)found);
            } else {
                dist2[q] = found >= 0 ? b : INFINITY;
                face[q] = found;
            }
        }
    }
}

// keys (when the faces were split) -> dist2 / face; the winning face's normal c / |c| as mm_sample writes it
__global__ __launch_bounds__(256) void pm_finish(const unsigned long long* __restrict__ keys, int64_t n, float* __restrict__ dist2,
                                                 int32_t* __restrict__ face, const float* __restrict__ verts, int nv,
                                                 const int32_t* __restrict__ faces, float* __restrict__ normals) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int f;
    if (keys) {
        const unsigned long long k = keys[i];
        dist2[i] = __uint_as_float((unsigned int)(k >> 32));
        face[i] = f = (int32_t)(unsigned int)k;                      // 0xFFFFFFFF -> -1
    } else {
        f = face[i];
    }
    if (!normals) return;
    int v[3];
    float p[3][3], c[3] = {0.0f, 0.0f, 0.0f};
    const float len = f >= 0 && load_face(faces, f, nv, v) ? mm_cross(verts, v, p, c) : 0.0f;   // a winner's indices are in range
#pragma unroll
    for (int k = 0; k < 3; ++k) normals[3 * i + k] = c[k] / len;     // no winner: 0 / 0
}

struct PmWorkspace {
    float* rec;
    unsigned long long* keys;
};

static int64_t pm_carve(void* base, int64_t num_x, int64_t num_faces, PmWorkspace* w) {
    Carver carve{static_cast<char*>(base), 256};
    float* rec = carve.take<float>(num_faces * PM_REC);
    unsigned long long* keys = carve.take<unsigned long long>(num_x);
    if (w) { w->rec = rec; w->keys = keys; }
    return carve.offset + 256;
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
    const int64_t chunk = nn_chunk(num_x, num_y, NN_BLOCK_Q);
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

int64_t nm_points_to_mesh_workspace_bytes(int64_t num_x, int64_t num_faces) {
    if (!mesh_size_ok(num_x) || !mesh_size_ok(num_faces)) return 0;
    return pm_carve(nullptr, num_x, num_faces, nullptr);
}

int nm_points_to_mesh(const float* d_x, int64_t num_x, const float* d_verts, int64_t num_vertices, const int32_t* d_faces,
                      int64_t num_faces, float* d_dist2, int32_t* d_face, float* d_face_normals, void* d_workspace, void* stream) {
    if (require_mesh("points to mesh", num_vertices, num_faces)) return 2;
    NM_REQUIRE(mesh_size_ok(num_x), "points to mesh: the point count must be in [0, 2^31 - 64)");
    NM_REQUIRE(num_x == 0 || (d_x && d_dist2 && d_face && d_workspace), "bad argument");
    NM_REQUIRE(num_faces == 0 || (d_verts && d_faces), "bad argument");
    if (num_x == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    PmWorkspace w;
    pm_carve(d_workspace, num_x, num_faces, &w);
    const int nv = (int)num_vertices;
    const unsigned flat = launch_grid(num_x);
    const int64_t chunk = nn_chunk(num_x, num_faces, PM_BLOCK_Q);
    const bool split = num_faces == 0 || chunk < num_faces;          // no face: the empty keys are the answer
    if (split) {
        hipLaunchKernelGGL(mm_nearest_init, dim3(flat), dim3(256), 0, s, w.keys, num_x);
        NM_HIP_CHECK(hipGetLastError());
    }
    if (num_faces) {
        hipLaunchKernelGGL(pm_records, dim3(launch_grid(num_faces, GRID_CAP)), dim3(256), 0, s, d_verts, d_faces, num_faces, nv, w.rec);
        NM_HIP_CHECK(hipGetLastError());
        const dim3 grid((unsigned)((num_x + PM_BLOCK_Q - 1) / PM_BLOCK_Q), (unsigned)((num_faces + chunk - 1) / chunk));
        hipLaunchKernelGGL(pm_nearest, grid, dim3(NN_THREADS), 0, s, d_x, num_x, w.rec, num_faces, chunk, d_dist2, d_face,
                           split ? w.keys : nullptr);
        NM_HIP_CHECK(hipGetLastError());
    }
    if (split || d_face_normals) {
        hipLaunchKernelGGL(pm_finish, dim3(flat), dim3(256), 0, s, split ? w.keys : nullptr, num_x, d_dist2, d_face, d_verts, nv,
                           d_faces, d_face_normals);
        NM_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
