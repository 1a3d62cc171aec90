// Ordered compaction on the device, shared by surface_filter.hip, mesh_components.hip, mesh_simplify.hip, mesh_smooth.hip and mesh_metrics.hip:
// keep bits (one __ballot word per 64 elements, the words in element order) -> prefix sums of the words' popcounts -> every kept
// element's output row is the prefix of its word + the popcount of the lower bits, which is numpy's cumsum(keep) - 1.  The output
// order is the input order by construction, whatever order the workgroups ran in: there is no atomic queue.
// The prefix sums are taken by ONE workgroup of SCAN_THREADS threads that walks the values SCAN_THREADS at a time: a __shfl_up
// ladder within each wave, the waves' sums in LDS, a serial sum over the waves in front and a carry that runs from chunk to
// chunk.  10 400 words (an 800 x 800 view) or 15 700 (a million vertices) are a few microseconds of one CU.
// The host half is what every unit around such a scan needs: the size guard, the launch grid and the workspace carver.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nm {

// ---- device ---------------------------------------------------------------------------------
constexpr int SCAN_THREADS = 1024;               // the workgroup of every kernel that calls scan_step: 16 waves

template <typename T>
struct ScanLds {                                 // declare it __shared__ alignas(16): the waves' sums are then read four at a time
    T wave[SCAN_THREADS / 64];                   // inclusive sum of every wave of the current chunk
    T carry;                                     // sum of all chunks so far
};

template <typename T>
__device__ __forceinline__ void scan_reset(ScanLds<T>& lds) {
    if (threadIdx.x == 0) lds.carry = 0;
    __syncthreads();
}

// One chunk: thread t brings `own` (0 beyond the end) and gets the inclusive prefix over everything the workgroup has seen so
// far, `own` included; lds.carry advances by the chunk's sum.  Every thread of the workgroup must call it, the same number of
// times: there are three barriers inside.  After the last call lds.carry is the total, readable by every thread.
template <typename T>
__device__ __forceinline__ T scan_step(T own, ScanLds<T>& lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = own;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T up = __shfl_up(inc, off, 64);
        if (lane >= off) inc += up;
    }
    if (lane == 63) lds.wave[wave] = inc;
    __syncthreads();
    T before = lds.carry;
    for (int w = 0; w < wave; ++w) before += lds.wave[w];
    __syncthreads();                             // every thread has read the carry ...
    if (threadIdx.x == SCAN_THREADS - 1) lds.carry = before + inc;
    __syncthreads();                             // ... before the last one moves it on; the next chunk sees the new one
    return before + inc;
}

// prefix[i] = the number of set bits in words[0 .. i) (uint32: fewer than 2^31 elements); returns their total
__device__ __forceinline__ uint32_t popcount_prefix_sums(const unsigned long long* __restrict__ words, int64_t nwords,
                                                         uint32_t* __restrict__ prefix) {
    __shared__ alignas(16) ScanLds<uint32_t> lds;
    scan_reset(lds);
    for (int64_t start = 0; start < nwords; start += SCAN_THREADS) {
        const int64_t i = start + threadIdx.x;
        const uint32_t own = i < nwords ? (uint32_t)__popcll(words[i]) : 0u;
        const uint32_t inclusive = scan_step(own, lds);
        if (i < nwords) prefix[i] = inclusive - own;
    }
    return lds.carry;
}

__device__ __forceinline__ bool bit_test(const unsigned long long* __restrict__ words, int64_t i) {
    return (words[i >> 6] >> (i & 63)) & 1ull;
}

// rank of a set bit among the set: numpy's cumsum(keep) - 1
__device__ __forceinline__ int64_t bit_rank(const unsigned long long* __restrict__ words, const uint32_t* __restrict__ prefix,
                                            int64_t i) {
    return (int64_t)prefix[i >> 6] + __popcll(words[i >> 6] & ((1ull << (i & 63)) - 1ull));
}

// splitmix64's finaliser: the hash of the open-addressing tables (mesh_simplify.hip, mesh_smooth.hip)
__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// the three vertex indices of face f -> false: one lies outside [0, nv) (a negative index fails the unsigned comparison)
__device__ __forceinline__ bool load_face(const int32_t* __restrict__ faces, int64_t f, int nv, int (&v)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = faces[3 * f + k];
    return (unsigned)v[0] < (unsigned)nv && (unsigned)v[1] < (unsigned)nv && (unsigned)v[2] < (unsigned)nv;
}

// ---- host -----------------------------------------------------------------------------------
// element counts the mesh / point-cloud entries take: 32-bit indices with room for a last partial word of 64
inline bool mesh_size_ok(int64_t n) { return n >= 0 && n < (int64_t(1) << 31) - 64; }

// workgroups of 256 threads for n elements, at least one; cap > 0: at most that many (GRID_CAP for the kernels that walk their
// elements in a grid-stride loop)
constexpr int64_t GRID_CAP = 2048;
inline unsigned launch_grid(int64_t n, int64_t cap = 0) {
    const int64_t g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : cap > 0 && g > cap ? cap : g);
}

inline int64_t align_up(int64_t bytes, int64_t alignment) { return (bytes + alignment - 1) / alignment * alignment; }

// Hands out the members of a workspace in order, each padded to `alignment`.  A unit has ONE function that carves its
// workspace; its *_workspace_bytes entry is that function run on a null base (`offset` at the end), so the size and the
// layout cannot disagree.
struct Carver {
    char* base;
    int64_t alignment;
    int64_t offset = 0;
    Carver(const void* workspace, int64_t alignment_)
        : base(static_cast<char*>(const_cast<void*>(workspace))), alignment(alignment_) {}
    template <typename T>
    T* take(int64_t count) {
        T* p = base ? reinterpret_cast<T*>(base + offset) : nullptr;
        offset += align_up(count * (int64_t)sizeof(T), alignment);
        return p;
    }
};

}  // namespace nm
