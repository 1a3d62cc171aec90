// The subset of a mesh that mesh_components.hip, mesh_simplify.hip and mesh_raster.hip's hidden-face filter leave: the one
// copy of the kernels behind compact.h's subset_scan / subset_compact_vertices / subset_compact_faces.  The units write the
// keep words; from there on the compaction is the same for all three -- the prefix sums of both sets of words in one launch,
// then one thread per vertex / per face that places its row by bit_rank.  The options are null pointers, tested once per
// thread and the same for every thread of the launch: a row the caller does not have, the representatives' map, the face
// indices.
#include "compact.h"

namespace nm {

// workgroup 0 the vertex words, workgroup 1 the face words
__global__ __launch_bounds__(SCAN_THREADS) void subset_scan_kernel(const unsigned long long* __restrict__ vwords, int64_t nvw,
                                                                   uint32_t* __restrict__ vprefix,
                                                                   const unsigned long long* __restrict__ fwords, int64_t nfw,
                                                                   uint32_t* __restrict__ fprefix,
                                                                   unsigned long long* __restrict__ totals) {
    const bool f = blockIdx.x != 0;
    const uint32_t kept = popcount_prefix_sums(f ? fwords : vwords, f ? nfw : nvw, f ? fprefix : vprefix);
    if (threadIdx.x == 0) totals[blockIdx.x] = kept;
}

__global__ __launch_bounds__(256) void subset_compact_vertices_kernel(SubsetRows a, int nv, int64_t capacity,
                                                                      const unsigned long long* __restrict__ words,
                                                                      const uint32_t* __restrict__ prefix) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv || !bit_test(words, v)) return;
    const int64_t dst = bit_rank(words, prefix, v);
    if (dst >= capacity) return;                                     // never past the caller's arrays
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (a.verts) a.out_verts[3 * dst + k] = a.verts[3 * v + k];
        if (a.normals) a.out_normals[3 * dst + k] = a.normals[3 * v + k];
    }
    if (a.values) a.out_values[dst] = a.values[v];
    if (a.keys) a.out_keys[dst] = a.keys[v];
}

__global__ __launch_bounds__(256) void subset_compact_faces_kernel(const int32_t* __restrict__ faces, int64_t nf, int nv,
                                                                   int64_t capacity, const unsigned long long* __restrict__ fwords,
                                                                   const uint32_t* __restrict__ fprefix,
                                                                   const unsigned long long* __restrict__ vwords,
                                                                   const uint32_t* __restrict__ vprefix, const int* __restrict__ rep,
                                                                   int32_t* __restrict__ out_faces,
                                                                   int32_t* __restrict__ out_face_index) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf || !bit_test(fwords, f)) return;
    int v[3];
    if (!load_face(faces, f, nv, v)) return;                         // such a face never has its bit set
    if (rep) {                                                       // nothing out of range is read: rep[] only at a valid corner
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = rep[v[k]];
        if ((unsigned)v[0] >= (unsigned)nv || (unsigned)v[1] >= (unsigned)nv || (unsigned)v[2] >= (unsigned)nv) return;
    }
    const int64_t dst = bit_rank(fwords, fprefix, f);
    if (dst >= capacity) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) out_faces[3 * dst + k] = (int32_t)bit_rank(vwords, vprefix, v[k]);
    if (out_face_index) out_face_index[dst] = (int32_t)f;
}

int subset_scan(const SubsetBits& b, unsigned long long* totals, hipStream_t stream) {
    hipLaunchKernelGGL(subset_scan_kernel, dim3(2), dim3(SCAN_THREADS), 0, stream, b.vwords, b.nvw, b.vprefix, b.fwords, b.nfw,
                       b.fprefix, totals);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

int subset_compact_vertices(const SubsetRows& rows, int nv, int64_t capacity, const SubsetBits& b, hipStream_t stream) {
    if (!capacity || !(rows.verts || rows.normals || rows.values || rows.keys)) return 0;
    hipLaunchKernelGGL(subset_compact_vertices_kernel, dim3(launch_grid(nv)), dim3(256), 0, stream, rows, nv, capacity, b.vwords,
                       b.vprefix);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

int subset_compact_faces(const int32_t* faces, int64_t nf, int nv, int64_t capacity, const SubsetBits& b, const int* rep,
                         int32_t* out_faces, int32_t* out_face_index, hipStream_t stream) {
    if (!capacity) return 0;
    hipLaunchKernelGGL(subset_compact_faces_kernel, dim3(launch_grid(nf)), dim3(256), 0, stream, faces, nf, nv, capacity, b.fwords,
                       b.fprefix, b.vwords, b.vprefix, rep, out_faces, out_face_index);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace nm
