// Taubin smoothing of an indexed triangle mesh (mesh_nerf --smooth-iters; DESIGN.md, "Mesh smoothing"): the sibling of
// mesh_simplify.hip.  A uniform umbrella Laplacian applied with a positive factor (lambda), then a negative one (mu): the
// voxel staircase and the density noise go, the volume stays.  Every decision is integer work and every per-vertex sum is an
// exact integer sum, so the output bytes do not depend on the order the workgroups ran in, on the order inside a neighbour
// list or on the numbering, and a numpy restatement (tests/mesh_smooth.py) reproduces them bit for bit.  Every fp32 / fp64
// operation below is rounded on its own (-ffp-contract=off), division and sqrt correctly rounded.
//   build (nm_mesh_smooth_build)
//   1. sm_vertices      a vertex with a non-finite coordinate is BAD (counted); the largest |coordinate| of the others is
//                       taken as an integer max over the float bits (a wave's max first, one atomicMax per wave).
//   2. sm_insert_edges  a face with an index outside [0, V) is BAD (counted, nothing of it is dereferenced), one with two
//                       equal corners DEGENERATE (counted, no edge).  Every other face brings its three undirected edges
//                       min << 32 | max to an open-addressing table (capacity: a power of two >= 6 F, linear probing), claimed
//                       by a 64-bit compare-and-swap on an empty key (all ones: no index has bit 31).  Each slot carries a
//                       face count.  The thread whose compare-and-swap claims a slot -- and only that one -- increments
//                       degree[] of both ends: a neighbour counts once however many faces share the edge.  The table is
//                       shared by workgroups on all XCDs, whose L2s are not coherent: inside this launch EVERY access to it,
//                       to the counts and to degree[] is an agent-scope atomic.  A probe walk is bounded by the capacity and
//                       waits for nobody (mesh_simplify.hip's rules).
//   3. sm_boundary      one thread per slot: an edge with face count 1 is a BOUNDARY edge and its two ends are boundary
//                       vertices (atomicOr into one bit per vertex); one with count > 2 is NON-MANIFOLD, and not boundary.
//   4. sm_scan          the exclusive prefix sums of degree[] (compact.h's scan_step, 64-bit: up to 6 F entries) are the
//                       offsets of the neighbour lists; boundary and isolated (degree 0) vertices are counted.
//   5. sm_fill          one thread per slot writes each end into the other's list at an atomic cursor.  The order inside a
//                       list is arbitrary; nothing below depends on it.
//   run (nm_mesh_smooth_run): one launch per half-step, one thread per vertex, sums in registers: no atomics, no LDS.  Reads
//   come from the previous half-step's positions, writes go to the other buffer.  With e = the binary exponent of the largest
//   |coordinate| of the INPUT mesh (every |x| < 2^e) and shift = 40 - e:
//                       q  = (int64) rint(ldexp((double) x, shift)), clamped to [-2^43, 2^43] (a NaN to the lower bound; the
//                            clamp never acts on a sane mesh, it makes the bound hold for EVERY input)
//                       hi = sum (q >> 20), lo = sum (q & 0xFFFFF) over the neighbours, per component: |hi| < 2^23 * 2^31 and
//                            lo < 2^20 * 2^31, so both int64 sums are exact in any order
//                       m  = ldexp(((double) hi * 2^20 + (double) lo) / (double) degree, -shift)
//                       x' = (float)((double) x + (double) f * (m - (double) x))           f = lambda or mu
//                       A boundary vertex (unless NM_MESH_SMOOTH_FREE_BOUNDARY) and a vertex of degree 0 are copied bit for bit.
//   normals (nm_mesh_vertex_normals): per non-degenerate face the fp32 unit normal of cross(b - a, c - a) times flip,
//   quantised as mesh_simplify.hip quantises normals and added to the three corners with int64 atomics; a vertex's normal is
//   the normalised float sum (ms_emit_vertices' rounding sequence), its input normal (or zero) when the sum is the zero vector.
// The only host round trip is the one that returns the counts (nm_mesh_smooth_build).
#include "compact.h"
#include "nm_internal.h"

namespace nm {

constexpr int SM_BITS = 40;                      // |q| <= 2^40 for every coordinate of the input mesh
constexpr double SM_QMAX = 8796093022208.0;      // 2^43: the largest |q| of any later position
constexpr double SM_SPLIT = 1048576.0;           // 2^20: q = (q >> 20) * 2^20 + (q & 0xFFFFF)
constexpr double SM_QUANTUM = 1073741824.0;      // 2^30 quanta per unit of a normal component
constexpr int SM_MAX_ITERATIONS = 1000;

struct SmHeader {
    unsigned long long edges, boundary_edges, nonmanifold_edges, boundary_vertices, isolated_vertices, degenerate;
    unsigned long long bad_vertices, bad_faces;
    unsigned long long entries;                  // the neighbour lists' total length: 2 * edges
    unsigned maxbits, pad0;                      // float bits of the largest finite |coordinate|
    unsigned long long pad[6];
};
static_assert(sizeof(SmHeader) == 128, "the header is two lines");

// frexp's exponent of the positive float with these bits: the e with 2^(e-1) <= x < 2^e (0 for x = 0)
__host__ __device__ inline int sm_exponent(unsigned bits) {
    const int field = (int)(bits >> 23) & 0xff;
    const unsigned mantissa = bits & 0x7fffffu;
    if (field) return field - 126;
    return mantissa ? (31 - __builtin_clz(mantissa)) - 148 : 0;                 // a subnormal is mantissa * 2^-149
}

__global__ __launch_bounds__(256) void sm_init(unsigned long long* __restrict__ keys, unsigned* __restrict__ counts, uint64_t cap,
                                               unsigned* __restrict__ degree, unsigned* __restrict__ cursor, int64_t nv,
                                               unsigned long long* __restrict__ bwords, int64_t nvw, SmHeader* hdr) {
    const uint64_t stride = (uint64_t)gridDim.x * 256, first = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    for (uint64_t i = first; i < cap; i += stride) {
        keys[i] = EMPTY_KEY;
        counts[i] = 0u;
    }
    for (uint64_t i = first; i < (uint64_t)nv; i += stride) degree[i] = cursor[i] = 0u;
    for (uint64_t i = first; i < (uint64_t)nvw; i += stride) bwords[i] = 0ull;
    if (first < sizeof(SmHeader) / 8) reinterpret_cast<unsigned long long*>(hdr)[first] = 0ull;
}

// one thread per vertex, whole waves (the votes)
__global__ __launch_bounds__(256) void sm_vertices(const float* __restrict__ verts, int nv, SmHeader* hdr) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    unsigned most = 0u;
    if (v < nv) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned bits = __float_as_uint(verts[3 * v + k]) & 0x7fffffffu;
            bad = bad || bits >= 0x7f800000u;                                   // infinite or a NaN
            most = bits > most ? bits : most;
        }
        if (bad) most = 0u;
    }
    const unsigned long long bads = __ballot(bad);
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const unsigned other = __shfl_xor(most, off, 64);
        most = other > most ? other : most;
    }
    if ((threadIdx.x & 63) == 0) {
        if (bads) atomicAdd(&hdr->bad_vertices, (unsigned long long)__popcll(bads));
        if (most) atomicMax(&hdr->maxbits, most);
    }
}

__global__ __launch_bounds__(256) void sm_insert_edges(const int32_t* __restrict__ faces, int64_t nf, int nv, unsigned long long* keys,
                                                       unsigned* counts, uint64_t cap, unsigned* degree, SmHeader* hdr) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int c[3] = {0, 0, 0};
    const bool in = f < nf;
    const bool ok = in && load_face(faces, f, nv, c);
    const bool flat = ok && (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]);
    if (ok && !flat) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int a = c[k], b = c[(k + 1) % 3];
            const unsigned lo = (unsigned)(a < b ? a : b), hi = (unsigned)(a < b ? b : a);
            bool claimed;                        // at most 3 F edges live in >= 6 F slots
            const uint64_t s = find_or_insert(keys, cap, ((unsigned long long)lo << 32) | hi, claimed);
            if (s >= cap) continue;
            __hip_atomic_fetch_add(counts + s, 1u, NM_RELAXED_AGENT);
            if (claimed) {
                __hip_atomic_fetch_add(degree + lo, 1u, NM_RELAXED_AGENT);
                __hip_atomic_fetch_add(degree + hi, 1u, NM_RELAXED_AGENT);
            }
        }
    }
    const unsigned long long bad = __ballot(in && !ok), deg = __ballot(flat);
    if ((threadIdx.x & 63) == 0) {
        if (bad) atomicAdd(&hdr->bad_faces, (unsigned long long)__popcll(bad));
        if (deg) atomicAdd(&hdr->degenerate, (unsigned long long)__popcll(deg));
    }
}

// one thread per slot (grid-stride in whole waves): the edge counts and the boundary bits
__global__ __launch_bounds__(256) void sm_boundary(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ counts,
                                                   uint64_t cap, unsigned long long* bwords, SmHeader* hdr) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    unsigned long long edges = 0, open = 0, fans = 0;
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < cap; s += stride) {   // cap is a multiple of 64
        const unsigned long long key = keys[s];
        const bool edge = key != EMPTY_KEY;
        const unsigned n = edge ? counts[s] : 0u;
        if (n == 1u) {
            const unsigned a = (unsigned)(key >> 32), b = (unsigned)key;
            atomicOr(bwords + (a >> 6), 1ull << (a & 63));
            atomicOr(bwords + (b >> 6), 1ull << (b & 63));
        }
        edges += (unsigned long long)__popcll(__ballot(edge));
        open += (unsigned long long)__popcll(__ballot(n == 1u));
        fans += (unsigned long long)__popcll(__ballot(n > 2u));
    }
    if ((threadIdx.x & 63) == 0) {
        if (edges) atomicAdd(&hdr->edges, edges);
        if (open) atomicAdd(&hdr->boundary_edges, open);
        if (fans) atomicAdd(&hdr->nonmanifold_edges, fans);
    }
}

// one workgroup: offsets[v] = degree[0] + ... + degree[v - 1], the boundary and the isolated vertices counted on the way
__global__ __launch_bounds__(SCAN_THREADS) void sm_scan(const unsigned* __restrict__ degree, int64_t nv,
                                                        const unsigned long long* __restrict__ bwords,
                                                        unsigned long long* __restrict__ offsets, SmHeader* hdr) {
    __shared__ alignas(16) ScanLds<unsigned long long> lds;
    __shared__ unsigned long long tallies[2];
    if (threadIdx.x < 2) tallies[threadIdx.x] = 0ull;
    scan_reset(lds);
    unsigned long long pinned = 0, alone = 0;
    for (int64_t start = 0; start < nv; start += SCAN_THREADS) {
        const int64_t v = start + threadIdx.x;
        const unsigned long long own = v < nv ? degree[v] : 0ull;
        const unsigned long long inclusive = scan_step(own, lds);
        if (v < nv) {
            offsets[v] = inclusive - own;
            pinned += bit_test(bwords, v) ? 1ull : 0ull;
            alone += own == 0ull ? 1ull : 0ull;
        }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        pinned += __shfl_xor(pinned, off, 64);
        alone += __shfl_xor(alone, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&tallies[0], pinned);
        atomicAdd(&tallies[1], alone);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        hdr->entries = lds.carry;
        hdr->boundary_vertices = tallies[0];
        hdr->isolated_vertices = tallies[1];
    }
}

__global__ __launch_bounds__(256) void sm_fill(const unsigned long long* __restrict__ keys, uint64_t cap,
                                               const unsigned* __restrict__ degree, const unsigned long long* __restrict__ offsets,
                                               unsigned* cursor, int32_t* __restrict__ neighbours) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < cap; s += stride) {
        const unsigned long long key = keys[s];
        if (key == EMPTY_KEY) continue;
        const unsigned a = (unsigned)(key >> 32), b = (unsigned)key;
        const unsigned at_a = atomicAdd(cursor + a, 1u), at_b = atomicAdd(cursor + b, 1u);
        if (at_a < degree[a]) neighbours[offsets[a] + at_a] = (int32_t)b;       // never past a list's end
        if (at_b < degree[b]) neighbours[offsets[b] + at_b] = (int32_t)a;
    }
}

__device__ __forceinline__ long long sm_quantise(float x, int shift) {
    double s = ldexp((double)x, shift);
    s = !(s >= -SM_QMAX) ? -SM_QMAX : (s > SM_QMAX ? SM_QMAX : s);
    return (long long)rint(s);
}

// one half-step with factor f: src -> dst, one thread per vertex
__global__ __launch_bounds__(256) void sm_half_step(const float* __restrict__ src, float* __restrict__ dst, int nv,
                                                    const unsigned* __restrict__ degree,
                                                    const unsigned long long* __restrict__ offsets,
                                                    const int32_t* __restrict__ neighbours,
                                                    const unsigned long long* __restrict__ bwords, int free_boundary, float f,
                                                    const SmHeader* __restrict__ hdr) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    float x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = src[3 * v + k];
    const unsigned n = degree[v], maxbits = hdr->maxbits;
    if (n == 0u || maxbits == 0u || (!free_boundary && bit_test(bwords, v))) {
#pragma unroll
        for (int k = 0; k < 3; ++k) dst[3 * v + k] = x[k];
        return;
    }
    const int shift = SM_BITS - sm_exponent(maxbits);
    const int32_t* list = neighbours + offsets[v];
    long long hi[3] = {0, 0, 0}, lo[3] = {0, 0, 0};
    for (unsigned i = 0; i < n; ++i) {
        const int64_t u = list[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const long long q = sm_quantise(src[3 * u + k], shift);
            hi[k] += q >> 20;
            lo[k] += q & 0xFFFFF;
        }
    }
    const double members = (double)n, factor = (double)f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double high = (double)hi[k] * SM_SPLIT;
        const double total = high + (double)lo[k];
        const double mean = ldexp(total / members, -shift);
        const double own = (double)x[k];
        const double step = factor * (mean - own);
        dst[3 * v + k] = (float)(own + step);
    }
}

__global__ __launch_bounds__(256) void sn_clear(long long* __restrict__ nsum, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) nsum[i] = 0ll;
}

__global__ __launch_bounds__(256) void sn_faces(const float* __restrict__ verts, int nv, const int32_t* __restrict__ faces,
                                                int64_t nf, float flip, long long* nsum) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int c[3];
    if (f >= nf || !load_face(faces, f, nv, c) || c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) return;
    float p[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) p[j][k] = verts[3 * (int64_t)c[j] + k];
    float u[3], w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        u[k] = p[1][k] - p[0][k];
        w[k] = p[2][k] - p[0][k];
    }
    float n[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float left = u[(k + 1) % 3] * w[(k + 2) % 3], right = u[(k + 2) % 3] * w[(k + 1) % 3];
        n[k] = left - right;
    }
    const float xx = n[0] * n[0], yy = n[1] * n[1], zz = n[2] * n[2];
    const float xy = xx + yy;
    const float len = sqrtf(xy + zz);
    if (!(len > 0.0f) || !is_finite(len)) return;                          // zero, infinite or a NaN
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float unit = n[k] / len;
        const long long q = (long long)rint((double)(unit * flip) * SM_QUANTUM);
        if (q) {
            __hip_atomic_fetch_add(nsum + 3 * (int64_t)c[0] + k, q, NM_RELAXED_AGENT);
            __hip_atomic_fetch_add(nsum + 3 * (int64_t)c[1] + k, q, NM_RELAXED_AGENT);
            __hip_atomic_fetch_add(nsum + 3 * (int64_t)c[2] + k, q, NM_RELAXED_AGENT);
        }
    }
}

__global__ __launch_bounds__(256) void sn_emit(const long long* __restrict__ nsum, const float* __restrict__ in_normals, int nv,
                                               float* __restrict__ out_normals) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const long long s0 = nsum[3 * v], s1 = nsum[3 * v + 1], s2 = nsum[3 * v + 2];
    if (s0 == 0 && s1 == 0 && s2 == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out_normals[3 * v + k] = in_normals ? in_normals[3 * v + k] : 0.0f;
        return;
    }
    const float sx = (float)s0, sy = (float)s1, sz = (float)s2;
    const float xx = sx * sx, yy = sy * sy, zz = sz * sz;
    const float xy = xx + yy;
    const float len = sqrtf(xy + zz);
    out_normals[3 * v + 0] = sx / len;
    out_normals[3 * v + 1] = sy / len;
    out_normals[3 * v + 2] = sz / len;
}

// the smallest power of two >= 6 n: twice the most edges n faces bring (at least 64)
static uint64_t sm_capacity(int64_t nf) {
    uint64_t cap = 64;
    while (cap < 6 * (uint64_t)nf) cap <<= 1;
    return cap;
}

struct SmWorkspace {
    SmHeader* hdr;
    unsigned* degree;
    unsigned long long* offsets;
    unsigned* cursor;
    unsigned long long* bwords;
    float* other;                                // the second position buffer of the half-steps
    long long* nsum;                             // nm_mesh_vertex_normals' sums
    int32_t* neighbours;                         // everything up to here does not depend on the face count
    unsigned long long* keys;
    unsigned* counts;
    uint64_t cap;
    int64_t nvw, bytes;
};

static SmWorkspace sm_carve(const void* ws, int64_t nv, int64_t nf) {
    Carver c(ws, 256);
    SmWorkspace w;
    w.cap = sm_capacity(nf);
    w.nvw = (nv + 63) / 64;
    w.hdr = c.take<SmHeader>(1);
    w.degree = c.take<unsigned>(nv);
    w.offsets = c.take<unsigned long long>(nv);
    w.cursor = c.take<unsigned>(nv);
    w.bwords = c.take<unsigned long long>(w.nvw);
    w.other = c.take<float>(3 * nv);
    w.nsum = c.take<long long>(3 * nv);
    w.neighbours = c.take<int32_t>(6 * nf);      // int64 arithmetic: 6 F never wraps
    w.keys = c.take<unsigned long long>((int64_t)w.cap);
    w.counts = c.take<unsigned>((int64_t)w.cap);
    w.bytes = c.offset;
    return w;
}

static unsigned sm_slot_grid(uint64_t cap) { return launch_grid((int64_t)cap, GRID_CAP); }

}  // namespace nm

using namespace nm;

extern "C" {

int64_t nm_mesh_smooth_workspace_bytes(int64_t num_vertices, int64_t num_faces) {
    if (!mesh_size_ok(num_vertices) || !mesh_size_ok(num_faces)) return 0;
    return sm_carve(nullptr, num_vertices, num_faces).bytes;
}

int nm_mesh_smooth_build(const float* d_verts, int64_t num_vertices, const int32_t* d_faces, int64_t num_faces, void* d_workspace,
                         int64_t* h_counts, void* stream) {
    if (require_mesh("mesh smooth", num_vertices, num_faces)) return 2;
    NM_REQUIRE(d_workspace && h_counts && (num_vertices == 0 || d_verts) && (num_faces == 0 || d_faces), "bad argument");
    const SmWorkspace w = sm_carve(d_workspace, num_vertices, num_faces);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nv = (int)num_vertices;
    hipLaunchKernelGGL(sm_init, dim3(sm_slot_grid(w.cap)), dim3(256), 0, s, w.keys, w.counts, w.cap, w.degree, w.cursor,
                       num_vertices, w.bwords, w.nvw, w.hdr);
    NM_HIP_CHECK(hipGetLastError());
    if (nv) {
        hipLaunchKernelGGL(sm_vertices, dim3(launch_grid(num_vertices)), dim3(256), 0, s, d_verts, nv, w.hdr);
        NM_HIP_CHECK(hipGetLastError());
    }
    if (num_faces) {
        hipLaunchKernelGGL(sm_insert_edges, dim3(launch_grid(num_faces)), dim3(256), 0, s, d_faces, num_faces, nv, w.keys, w.counts,
                           w.cap, w.degree, w.hdr);
        NM_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(sm_boundary, dim3(sm_slot_grid(w.cap)), dim3(256), 0, s, w.keys, w.counts, w.cap, w.bwords, w.hdr);
        NM_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(sm_scan, dim3(1), dim3(SCAN_THREADS), 0, s, w.degree, num_vertices, w.bwords, w.offsets, w.hdr);
    NM_HIP_CHECK(hipGetLastError());
    if (num_faces) {
        hipLaunchKernelGGL(sm_fill, dim3(sm_slot_grid(w.cap)), dim3(256), 0, s, w.keys, w.cap, w.degree, w.offsets, w.cursor,
                           w.neighbours);
        NM_HIP_CHECK(hipGetLastError());
    }
    SmHeader h;
    NM_HIP_CHECK(hipMemcpyAsync(&h, w.hdr, sizeof(SmHeader), hipMemcpyDeviceToHost, s));
    NM_HIP_CHECK(hipStreamSynchronize(s));
    h_counts[NM_MESH_SMOOTH_EDGES] = (int64_t)h.edges;
    h_counts[NM_MESH_SMOOTH_BOUNDARY_EDGES] = (int64_t)h.boundary_edges;
    h_counts[NM_MESH_SMOOTH_NONMANIFOLD_EDGES] = (int64_t)h.nonmanifold_edges;
    h_counts[NM_MESH_SMOOTH_BOUNDARY_VERTICES] = (int64_t)h.boundary_vertices;
    h_counts[NM_MESH_SMOOTH_ISOLATED_VERTICES] = (int64_t)h.isolated_vertices;
    h_counts[NM_MESH_SMOOTH_DEGENERATE] = (int64_t)h.degenerate;
    h_counts[NM_MESH_SMOOTH_BAD_VERTICES] = (int64_t)h.bad_vertices;
    h_counts[NM_MESH_SMOOTH_BAD_FACES] = (int64_t)h.bad_faces;
    h_counts[NM_MESH_SMOOTH_EXPONENT] = (int64_t)sm_exponent(h.maxbits);
    return 0;
}

int nm_mesh_smooth_run(const void* d_workspace, const float* d_verts, int64_t num_vertices, int32_t iterations, float lambda,
                       float mu, int32_t flags, float* d_out_verts, void* stream) {
    NM_REQUIRE(mesh_size_ok(num_vertices), "mesh smooth: vertex and face counts must be in [0, 2^31 - 64)");
    NM_REQUIRE(iterations >= 0 && iterations <= SM_MAX_ITERATIONS, "mesh smooth: iterations must be in [0, 1000]");
    NM_REQUIRE(lambda > 0.0f && lambda <= 1.0f, "mesh smooth: lambda must be in (0, 1]");     // a NaN fails the comparisons
    NM_REQUIRE(mu >= -1.0f && mu <= 0.0f, "mesh smooth: mu must be in [-1, 0]");
    NM_REQUIRE((flags & ~NM_MESH_SMOOTH_FREE_BOUNDARY) == 0, "mesh smooth: unknown flags");
    NM_REQUIRE(d_workspace && (num_vertices == 0 || (d_verts && d_out_verts)), "bad argument");
    NM_REQUIRE(num_vertices == 0 || d_verts != d_out_verts, "mesh smooth: the output must not be the input");
    if (num_vertices == 0) return 0;
    const SmWorkspace w = sm_carve(d_workspace, num_vertices, 0);                // what a half-step reads lies in front of the face part
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nv = (int)num_vertices;
    const int steps = iterations * (mu == 0.0f ? 1 : 2);
    if (steps == 0) {
        NM_HIP_CHECK(hipMemcpyAsync(d_out_verts, d_verts, sizeof(float) * 3 * (size_t)nv, hipMemcpyDeviceToDevice, s));
        return 0;
    }
    const unsigned grid = launch_grid(num_vertices);
    const float* src = d_verts;
    for (int i = 0; i < steps; ++i) {                                            // the last one writes the caller's array
        float* dst = (steps - 1 - i) % 2 == 0 ? d_out_verts : w.other;
        const float f = (mu == 0.0f || i % 2 == 0) ? lambda : mu;
        hipLaunchKernelGGL(sm_half_step, dim3(grid), dim3(256), 0, s, src, dst, nv, w.degree, w.offsets, w.neighbours, w.bwords,
                           flags & NM_MESH_SMOOTH_FREE_BOUNDARY, f, w.hdr);
        NM_HIP_CHECK(hipGetLastError());
        src = dst;
    }
    return 0;
}

int nm_mesh_vertex_normals(const float* d_verts, int64_t num_vertices, const int32_t* d_faces, int64_t num_faces,
                           const float* d_in_normals, int32_t flip, void* d_workspace, float* d_out_normals, void* stream) {
    if (require_mesh("mesh smooth", num_vertices, num_faces)) return 2;
    NM_REQUIRE(flip == 1 || flip == -1, "mesh vertex normals: flip must be +1 or -1");
    NM_REQUIRE(d_workspace && (num_vertices == 0 || (d_verts && d_out_normals)) && (num_faces == 0 || d_faces), "bad argument");
    if (num_vertices == 0) return 0;
    const SmWorkspace w = sm_carve(d_workspace, num_vertices, num_faces);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nv = (int)num_vertices;
    hipLaunchKernelGGL(sn_clear, dim3(launch_grid(3 * num_vertices, GRID_CAP)), dim3(256), 0, s, w.nsum, 3 * num_vertices);
    NM_HIP_CHECK(hipGetLastError());
    if (num_faces) {
        hipLaunchKernelGGL(sn_faces, dim3(launch_grid(num_faces)), dim3(256), 0, s, d_verts, nv, d_faces, num_faces, (float)flip,
                           w.nsum);
        NM_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(sn_emit, dim3(launch_grid(num_vertices)), dim3(256), 0, s, w.nsum, d_in_normals, nv, d_out_normals);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
