// Connected components of an indexed triangle mesh and the filter built on them (mesh_nerf --min-component-faces /
// --keep-largest; DESIGN.md, "Mesh components").  Two vertices are connected when a triangle holds both; a component's LABEL is
// its smallest vertex index, its SIZE its number of triangles; a vertex in no triangle is a component of size 0.  Everything
// is integer work on the arrays marching cubes left on the device:
//   1. cc_init / cc_union_faces / cc_flatten   lock-free union-find over the triangles, two unions per face.  A root is always
//                       hooked under a SMALLER index, so parent[v] <= v holds at every moment, every walk moves to strictly
//                       smaller indices (no loop can spin, whatever the other workgroups do meanwhile) and the root a tree ends
//                       with is its smallest member: the canonical label, independent of face order, launch geometry and of
//                       which thread won a race.  parent[] is shared by workgroups on all XCDs, whose L2s are not coherent and
//                       whose L1s are never refreshed: inside the union and the flatten launch EVERY access to it is an
//                       agent-scope atomic (relaxed load, compare-and-swap, min) -- they are served by the memory side, never
//                       by a CU's L1 or a stale line -- and never a plain load.  Everything else relies on kernel boundaries.
//   2. cc_count         triangles per label with integer atomics (exact, order-independent); equal labels are first
//                       aggregated within a wave, so a mesh that is one big component does one add per wave, not per triangle.
//   3. cc_round / cc_mask   selection on the device: the min_faces threshold, then for keep_largest = K the K best roots by
//                       (count descending, label ascending) as K rounds of a 64-bit max-reduction over the key
//                       count << 32 | (2^32 - 1 - label): round r takes the largest key below round r-1's.  The keep bits of
//                       vertices and faces leave each wave as one ballot word.
//   4. subset_scan / subset_compact_*   the ordered compaction of compact.h over both sets of words (mesh_subset.hip): the
//                       output order is the input order, whatever order the workgroups ran in, and a kept vertex's new index
//                       is its rank among the set bits, which is numpy's cumsum(keep) - 1.
// The only host round trip is the one that returns the output sizes (nm_mesh_components_select).
#include "compact.h"
#include "nm_internal.h"

namespace nm {

constexpr int CC_KMAX = NM_MESH_KEEP_LARGEST_MAX;

struct CcHeader {
    unsigned long long bad_faces;      // faces with a vertex index outside [0, nv): left out of everything
    unsigned long long pad[7];
    unsigned long long totals[4];      // vertices kept, faces kept, components seen, components kept
    unsigned long long pad2[4];
};

__device__ __forceinline__ int cc_load(int* p) { return __hip_atomic_load(p, NM_RELAXED_AGENT); }

// Root of v, halving the path on the way.  parent[x] <= x always and values only decrease, so v strictly decreases in every
// iteration: at most v of them, and the two `>=` exits end the walk even on memory that is not a forest.
__device__ __forceinline__ int cc_find(int* parent, int v) {
    for (;;) {
        const int p = cc_load(parent + v);
        if (p >= v) return v;
        const int g = cc_load(parent + p);
        if (g >= p) return p;
        __hip_atomic_fetch_min(parent + v, g, NM_RELAXED_AGENT);   // g is an ancestor of v and smaller
        v = g;
    }
}

// Hooks the larger of the two roots under the smaller.  A failed compare-and-swap means another thread hooked that root
// meanwhile, under something smaller: the pair (a, b) decreases with every retry, so the loop ends.
__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        int expected = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, NM_RELAXED_AGENT)) return;
        if (expected >= hi) return;                                  // cannot happen on a forest; never spin
        a = expected;
        b = lo;
    }
}

__global__ __launch_bounds__(256) void cc_init(int* __restrict__ parent, int* __restrict__ counts, int nv, CcHeader* hdr) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nv; v += stride) {
        parent[v] = (int)v;
        counts[v] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) hdr->bad_faces = 0;
}

__global__ __launch_bounds__(256) void cc_union_faces(const int32_t* __restrict__ faces, int64_t nf, int nv, int* parent,
                                                      CcHeader* hdr) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < nf; f += stride) {
        int v[3];
        if (!load_face(faces, f, nv, v)) {
            atomicAdd(&hdr->bad_faces, 1ull);
            continue;
        }
        cc_union(parent, v[0], v[1]);
        cc_union(parent, v[1], v[2]);
    }
}

// label[v] = the root of v.  The halving writes of other threads go on during this launch: parent[] is still read and written
// with agent-scope atomics only.
__global__ __launch_bounds__(256) void cc_flatten(int* parent, int* __restrict__ labels, int nv) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nv; v += stride) labels[v] = cc_find(parent, (int)v);
}

// counts[label] += 1 per triangle; lanes of a wave that hold the same label add once, their number
__global__ __launch_bounds__(256) void cc_count(const int32_t* __restrict__ faces, int64_t nf, int nv,
                                                const int* __restrict__ labels, int* counts) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t rounds = (nf + stride - 1) / stride;               // uniform trip count: the ballots below need whole waves
    for (int64_t it = 0; it < rounds; ++it) {
        const int64_t f = it * stride + (int64_t)blockIdx.x * 256 + threadIdx.x;
        int v[3];
        bool todo = f < nf && load_face(faces, f, nv, v);
        const int label = todo ? labels[v[0]] : -1;
        unsigned long long left = __ballot(todo);
        while (left) {                                               // uniform over the wave
            const int leader = __ffsll((long long)left) - 1;
            const int want = __shfl(label, leader, 64);
            const unsigned long long same = __ballot(todo && label == want);
            if (lane == leader) atomicAdd(counts + want, (int)__popcll(same));
            if (label == want) todo = false;
            left &= ~same;
        }
    }
}

__device__ __forceinline__ unsigned long long cc_key(int count, int label) {
    return ((unsigned long long)(unsigned)count << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)label);   // never 0
}

__global__ __launch_bounds__(256) void cc_select_init(unsigned long long* best, CcHeader* hdr) {
    for (int i = threadIdx.x; i <= CC_KMAX; i += 256) best[i] = 0ull;
    if (threadIdx.x < 4) hdr->totals[threadIdx.x] = 0ull;
}

// round r of the selection: best[r] = the largest key of a surviving root below best[r-1] (0: none is left)
__global__ __launch_bounds__(256) void cc_round(const int* __restrict__ labels, const int* __restrict__ counts, int nv,
                                                long long min_faces, int r, unsigned long long* best) {
    const unsigned long long below = r ? best[r - 1] : ~0ull;        // written by the previous launch
    if (below == 0ull) return;
    const int64_t stride = (int64_t)gridDim.x * 256;
    unsigned long long m = 0ull;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nv; v += stride) {
        if (labels[v] != (int)v) continue;
        const int c = counts[v];
        const unsigned long long key = cc_key(c, (int)v);
        if ((long long)c >= min_faces && key < below && key > m) m = key;
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const unsigned long long o = __shfl_xor(m, off, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(best + r, m);
}

__device__ __forceinline__ bool cc_keeps(const int* __restrict__ counts, int nv, int root, long long min_faces,
                                         unsigned long long threshold) {
    if ((unsigned)root >= (unsigned)nv) return false;                // labels that are not nm_mesh_components' own: no access
    const int c = counts[root];
    return (long long)c >= min_faces && cc_key(c, root) >= threshold;
}

// keep bits of the vertices (one ballot word per 64) + the numbers of components seen and kept
__global__ __launch_bounds__(256) void cc_mask_vertices(const int* __restrict__ labels, const int* __restrict__ counts, int nv,
                                                        long long min_faces, int keep_largest,
                                                        const unsigned long long* __restrict__ best,
                                                        unsigned long long* __restrict__ words, CcHeader* hdr) {
    const unsigned long long threshold = keep_largest ? best[keep_largest - 1] : 0ull;   // 0: fewer than K survive, keep them all
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = v < nv;
    const int root = valid ? labels[v] : 0;
    const bool keep = valid && cc_keeps(counts, nv, root, min_faces, threshold);
    const bool is_root = valid && root == (int)v;
    store_keep_word(words, v, nv, keep);
    const unsigned long long seen = __ballot(is_root), kept = __ballot(is_root && keep);
    if ((threadIdx.x & 63) == 0) {                                   // a wave beyond the last word has no root to count
        if (seen) atomicAdd(&hdr->totals[2], (unsigned long long)__popcll(seen));
        if (kept) atomicAdd(&hdr->totals[3], (unsigned long long)__popcll(kept));
    }
}

__global__ __launch_bounds__(256) void cc_mask_faces(const int32_t* __restrict__ faces, int64_t nf, int nv,
                                                     const int* __restrict__ labels, const int* __restrict__ counts,
                                                     long long min_faces, int keep_largest,
                                                     const unsigned long long* __restrict__ best,
                                                     unsigned long long* __restrict__ words) {
    const unsigned long long threshold = keep_largest ? best[keep_largest - 1] : 0ull;
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int v[3];
    store_keep_word(words, f, nf, f < nf && load_face(faces, f, nv, v) && cc_keeps(counts, nv, labels[v[0]], min_faces, threshold));
}

struct CcWorkspace {
    CcHeader* hdr;
    int* parent;
    unsigned long long* best;
    SubsetBits bits;
    int64_t bytes;
};

static CcWorkspace cc_carve(const void* ws, int64_t nv, int64_t nf) {
    Carver c(ws, 256);
    CcWorkspace w;
    w.hdr = c.take<CcHeader>(1);
    w.parent = c.take<int>(nv);
    w.best = c.take<unsigned long long>(CC_KMAX + 1);
    w.bits = take_subset_bits(c, nv, nf);
    w.bytes = c.offset;
    return w;
}

}  // namespace nm

using namespace nm;

extern "C" {

int64_t nm_mesh_components_workspace_bytes(int64_t num_vertices, int64_t num_faces) {
    if (!mesh_size_ok(num_vertices) || !mesh_size_ok(num_faces)) return 0;
    return cc_carve(nullptr, num_vertices, num_faces).bytes;
}

int nm_mesh_components(const int32_t* d_faces, int64_t num_faces, int64_t num_vertices, int32_t* d_labels,
                       int32_t* d_face_counts, void* d_workspace, void* stream) {
    if (require_mesh("mesh components", num_vertices, num_faces)) return 2;
    NM_REQUIRE(d_workspace && (num_faces == 0 || d_faces) && (num_vertices == 0 || (d_labels && d_face_counts)), "bad argument");
    const CcWorkspace w = cc_carve(d_workspace, num_vertices, num_faces);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nv = (int)num_vertices;
    const unsigned vgrid = launch_grid(num_vertices, GRID_CAP), fgrid = launch_grid(num_faces, GRID_CAP);
    hipLaunchKernelGGL(cc_init, dim3(vgrid), dim3(256), 0, s, w.parent, d_face_counts, nv, w.hdr);
    NM_HIP_CHECK(hipGetLastError());
    if (num_faces) {
        hipLaunchKernelGGL(cc_union_faces, dim3(fgrid), dim3(256), 0, s, d_faces, num_faces, nv, w.parent, w.hdr);
        NM_HIP_CHECK(hipGetLastError());
    }
    if (num_vertices) {
        hipLaunchKernelGGL(cc_flatten, dim3(vgrid), dim3(256), 0, s, w.parent, d_labels, nv);
        NM_HIP_CHECK(hipGetLastError());
    }
    if (num_faces) {
        hipLaunchKernelGGL(cc_count, dim3(fgrid), dim3(256), 0, s, d_faces, num_faces, nv, d_labels, d_face_counts);
        NM_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

int nm_mesh_components_select(const int32_t* d_faces, int64_t num_faces, int64_t num_vertices, const int32_t* d_labels,
                              const int32_t* d_face_counts, int64_t min_faces, int32_t keep_largest, void* d_workspace,
                              int64_t* h_vertices_kept, int64_t* h_faces_kept, int64_t* h_components,
                              int64_t* h_components_kept, void* stream) {
    if (require_mesh("mesh components", num_vertices, num_faces)) return 2;
    NM_REQUIRE(min_faces >= 0, "mesh components: min_faces must be >= 0");
    NM_REQUIRE(keep_largest >= 0 && keep_largest <= CC_KMAX, "mesh components: keep_largest must be in [0, 1024]");
    NM_REQUIRE(d_workspace && (num_faces == 0 || d_faces) && (num_vertices == 0 || (d_labels && d_face_counts)) &&
               h_vertices_kept && h_faces_kept && h_components && h_components_kept, "bad argument");
    const CcWorkspace w = cc_carve(d_workspace, num_vertices, num_faces);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nv = (int)num_vertices;
    hipLaunchKernelGGL(cc_select_init, dim3(1), dim3(256), 0, s, w.best, w.hdr);
    for (int r = 0; r < keep_largest && nv; ++r)
        hipLaunchKernelGGL(cc_round, dim3(launch_grid(num_vertices, GRID_CAP)), dim3(256), 0, s, d_labels, d_face_counts, nv,
                           (long long)min_faces, r, w.best);
    NM_HIP_CHECK(hipGetLastError());
    if (nv)
        hipLaunchKernelGGL(cc_mask_vertices, dim3(launch_grid(num_vertices)), dim3(256), 0, s, d_labels, d_face_counts, nv,
                           (long long)min_faces, (int)keep_largest, w.best, w.bits.vwords, w.hdr);
    if (num_faces)
        hipLaunchKernelGGL(cc_mask_faces, dim3(launch_grid(num_faces)), dim3(256), 0, s, d_faces, num_faces, nv, d_labels,
                           d_face_counts, (long long)min_faces, (int)keep_largest, w.best, w.bits.fwords);
    NM_HIP_CHECK(hipGetLastError());
    if (const int rc = subset_scan(w.bits, w.hdr->totals, s)) return rc;
    CcHeader h;
    NM_HIP_CHECK(hipMemcpyAsync(&h, w.hdr, sizeof(CcHeader), hipMemcpyDeviceToHost, s));
    NM_HIP_CHECK(hipStreamSynchronize(s));
    if (h.bad_faces) {
        set_error("mesh components: " + std::to_string(h.bad_faces) + " faces have a vertex index outside [0, num_vertices)");
        return 2;
    }
    *h_vertices_kept = (int64_t)h.totals[0];
    *h_faces_kept = (int64_t)h.totals[1];
    *h_components = (int64_t)h.totals[2];
    *h_components_kept = (int64_t)h.totals[3];
    return 0;
}

int nm_mesh_components_compact(const void* d_workspace, const int32_t* d_faces, int64_t num_faces, int64_t num_vertices,
                               const float* d_verts, const float* d_normals, const float* d_values, const int64_t* d_keys,
                               int64_t vertices_kept, int64_t faces_kept, float* d_out_verts, int32_t* d_out_faces,
                               float* d_out_normals, float* d_out_values, int64_t* d_out_keys, void* stream) {
    if (require_mesh("mesh components", num_vertices, num_faces)) return 2;
    NM_REQUIRE_COMPACT_OUTPUTS("mesh components", d_workspace && (num_faces == 0 || d_faces),
                               (!d_verts || d_out_verts) && (!d_normals || d_out_normals) && (!d_values || d_out_values) &&
                                   (!d_keys || d_out_keys));
    const CcWorkspace w = cc_carve(d_workspace, num_vertices, num_faces);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nv = (int)num_vertices;
    const SubsetRows rows{d_verts, d_normals, d_values, reinterpret_cast<const long long*>(d_keys),
                          d_out_verts, d_out_normals, d_out_values, reinterpret_cast<long long*>(d_out_keys)};
    if (const int rc = subset_compact_vertices(rows, nv, vertices_kept, w.bits, s)) return rc;
    return subset_compact_faces(d_faces, num_faces, nv, faces_kept, w.bits, nullptr, d_out_faces, nullptr, s);
}

}  // extern "C"
