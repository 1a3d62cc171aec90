// Ordered compaction on the device, shared by surface_filter.hip, mesh_components.hip, mesh_simplify.hip, mesh_smooth.hip,
// mesh_raster.hip and mesh_metrics.hip:
// keep bits (one __ballot word per 64 elements, the words in element order) -> prefix sums of the words' popcounts -> every kept
// element's output row is the prefix of its word + the popcount of the lower bits, which is numpy's cumsum(keep) - 1.  The output
// order is the input order by construction, whatever order the workgroups ran in: there is no atomic queue.
// The prefix sums are taken by ONE workgroup of SCAN_THREADS threads that walks the values SCAN_THREADS at a time: a __shfl_up
// ladder within each wave, the waves' sums in LDS, a serial sum over the waves in front and a carry that runs from chunk to
// chunk.  10 400 words (an 800 x 800 view) or 15 700 (a million vertices) are a few microseconds of one CU.
// The host half is what every unit around such a scan needs: the size guard, the launch grid and the workspace carver.
// A SUBSET OF A MESH -- keep bits of the vertices and of the faces -- is compacted the same way by the three units that drop
// parts of one (components, simplify, hidden faces): SubsetBits names the four arrays in a unit's workspace, and the kernels
// behind subset_scan / subset_compact_vertices / subset_compact_faces live once, in mesh_subset.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nm_internal.h"

// every access to memory that workgroups on several XCDs share within one launch: relaxed, agent scope (served by the memory side)
#define NM_RELAXED_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

namespace nm {

// ---- device ---------------------------------------------------------------------------------
__host__ __device__ __forceinline__ bool is_finite(float x) { return x - x == 0.0f; }   // false for an infinity and a NaN

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

// The keep bits of one wave's 64 elements: element i of n brings `keep`, lane 0 stores the ballot as words[i >> 6] where that
// word exists.  Whole waves must call it.  -> the word, for the callers that count its bits.
__device__ __forceinline__ unsigned long long store_keep_word(unsigned long long* __restrict__ words, int64_t i, int64_t n,
                                                              bool keep) {
    const unsigned long long word = __ballot(keep);
    if ((threadIdx.x & 63) == 0 && (i >> 6) < (n + 63) / 64) words[i >> 6] = word;
    return word;
}

// splitmix64's finaliser: the hash of the open-addressing tables (mesh_simplify.hip, mesh_smooth.hip)
__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

constexpr unsigned long long EMPTY_KEY = ~0ull;  // a slot of those tables that nobody has claimed: no key has bit 63

__device__ __forceinline__ unsigned long long* key_of(unsigned long long* slot) { return slot; }
template <typename Slot>
__device__ __forceinline__ unsigned long long* key_of(Slot* slot) { return &slot->key; }

// The slot of `key` in a table of `cap` slots (a power of two; linear probing): bare keys, or a struct with a `key` member.
// claimed = this thread's compare-and-swap put the key there.  The table is shared by workgroups on all XCDs: every access is
// an agent-scope atomic.  The walk waits for nobody -- a failed compare-and-swap returns the occupant, which either is the key
// or sends the walk on -- and the callers size the table so that an empty slot always ends it; `cap` iterations bound it all
// the same (-> cap: not placed).
template <typename Slot>
__device__ __forceinline__ uint64_t find_or_insert(Slot* table, uint64_t cap, unsigned long long key, bool& claimed) {
    uint64_t s = mix64(key) & (cap - 1);
    claimed = false;
    for (uint64_t i = 0; i < cap; ++i, s = (s + 1) & (cap - 1)) {
        unsigned long long k = __hip_atomic_load(key_of(table + s), NM_RELAXED_AGENT);
        if (k == EMPTY_KEY && __hip_atomic_compare_exchange_strong(key_of(table + s), &k, key, __ATOMIC_RELAXED, NM_RELAXED_AGENT)) {
            claimed = true;
            return s;
        }
        if (k == key) return s;                  // found, or the thread that beat us to the slot brought the same key
    }
    return cap;
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

// what every mesh entry asks of the two counts, in the words of the unit `what`: 0 or 2
inline int require_mesh(const char* what, int64_t num_vertices, int64_t num_faces) {
    NM_REQUIRE(mesh_size_ok(num_vertices) && mesh_size_ok(num_faces),
               std::string(what) + ": vertex and face counts must be in [0, 2^31 - 64)");
    NM_REQUIRE(num_faces == 0 || num_vertices > 0, std::string(what) + ": faces without vertices");
    return 0;
}

// What the _compact / _emit entry of a subset asks of its counts and outputs, written where the entry's own parameters
// vertices_kept, faces_kept, num_vertices, num_faces and d_out_faces are in scope.  args_ok: the entry's pointer check,
// rows_ok: every per-vertex input has its output.
#define NM_REQUIRE_COMPACT_OUTPUTS(what, args_ok, rows_ok)                                                              \
    NM_REQUIRE(vertices_kept >= 0 && vertices_kept <= num_vertices && faces_kept >= 0 && faces_kept <= num_faces,       \
               what ": the kept counts must lie within the mesh's");                                                   \
    NM_REQUIRE(args_ok, "bad argument");                                                                                \
    NM_REQUIRE(vertices_kept == 0 || (rows_ok), what ": an input array without its output");                            \
    NM_REQUIRE(faces_kept == 0 || d_out_faces, what ": null face output")

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

// ---- a subset of a mesh -----------------------------------------------------------------------
// keep bits and their prefix sums for the vertices and for the faces: four members of a unit's workspace
struct SubsetBits {
    unsigned long long* vwords;
    uint32_t* vprefix;
    unsigned long long* fwords;
    uint32_t* fprefix;
    int64_t nvw, nfw;
};

// the four arrays from a unit's carver, at the point in its order where they stand; faces_first: the face pair in front
inline SubsetBits take_subset_bits(Carver& c, int64_t nv, int64_t nf, bool faces_first = false) {
    SubsetBits b;
    b.nvw = (nv + 63) / 64;
    b.nfw = (nf + 63) / 64;
    if (faces_first) {
        b.fwords = c.take<unsigned long long>(b.nfw);
        b.fprefix = c.take<uint32_t>(b.nfw);
    }
    b.vwords = c.take<unsigned long long>(b.nvw);
    b.vprefix = c.take<uint32_t>(b.nvw);
    if (!faces_first) {
        b.fwords = c.take<unsigned long long>(b.nfw);
        b.fprefix = c.take<uint32_t>(b.nfw);
    }
    return b;
}

// per-vertex rows in, kept rows out; a null input is a row the caller does not have
struct SubsetRows {
    const float* verts;  const float* normals;  const float* values;  const long long* keys;
    float* out_verts;    float* out_normals;    float* out_values;    long long* out_keys;
};

// The launchers of mesh_subset.hip: 0, or 1 with nm_last_error set.
// Both prefix arrays from both word arrays in one launch; totals[0] = vertices kept, totals[1] = faces kept (device memory).
int subset_scan(const SubsetBits& bits, unsigned long long* totals, hipStream_t stream);
// The kept vertices' rows in their order, at most `capacity` of them; nothing to do without a row or with capacity 0.
int subset_compact_vertices(const SubsetRows& rows, int nv, int64_t capacity, const SubsetBits& bits, hipStream_t stream);
// The kept faces in their order, at most `capacity`, their corners renumbered to the kept vertices.  rep (nullable): every
// corner goes through rep[] first, and a face with a corner or a representative outside [0, nv) is skipped.  out_face_index
// (nullable): the kept faces' own indices.
int subset_compact_faces(const int32_t* faces, int64_t nf, int nv, int64_t capacity, const SubsetBits& bits, const int* rep,
                         int32_t* out_faces, int32_t* out_face_index, hipStream_t stream);

}  // namespace nm
