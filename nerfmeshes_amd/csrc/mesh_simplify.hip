// Mesh simplification by vertex clustering (Rossignac--Borrel; mesh_nerf --simplify-cell; DESIGN.md, "Mesh simplification"):
// the sibling of mesh_components.hip.  Vertices that fall into one cell of a uniform grid become one vertex, faces are
// re-pointed, the degenerate and the duplicate ones go, and so do the clusters no face is left on.  Every decision is integer
// work and every sum is an exact integer sum, so the output bytes do not depend on the order the workgroups ran in, and a
// numpy restatement (tests/mesh_simplify.py) reproduces them bit for bit.  Every fp32 / fp64 operation below is rounded on
// its own (-ffp-contract=off), division and sqrt correctly rounded.
//   1. ms_insert        cell of a vertex: c = floorf((x - origin) / cell) per axis; a vertex with a non-finite coordinate or
//                       a c outside [0, 2^21) is BAD: counted, inserted nowhere.  The packed 63-bit cell cx | cy << 21 | cz << 42
//                       is the key of an open-addressing table of 64-byte slots (capacity: a power of two >= 2 V, linear
//                       probing), claimed by a 64-bit compare-and-swap on an empty key (all ones: no cell has bit 63).  The
//                       table is shared by workgroups on all XCDs, whose L2s are not coherent: inside this launch EVERY access
//                       to it is an agent-scope atomic (relaxed load, compare-and-swap, min, add), never a plain load
//                       (mesh_components.hip's rule for parent[]).  A probe walk is bounded by the capacity and waits for
//                       nobody: a failed compare-and-swap returns the occupant, which either is the key or sends the walk on.
//                       Per slot: the REPRESENTATIVE = the smallest member index (atomicMin: canonical, whoever won the
//                       claim), the member count, and three + three int64 sums:
//                         position  lo = origin + c * cell; t = (x - lo) / cell; q = (int64) rint((double) t * 2^30), clamped
//                                   to [-2^31, 2^31] (t lies in [0, 1] up to rounding: the clamp never acts on a sane mesh; it
//                                   makes the bound below hold for EVERY input)
//                         normal    q = (int64) rint((double) n * 2^30) per component, of the members whose three components
//                                   are finite and at most 2 in magnitude (a unit normal's are at most 1); another member
//                                   contributes nothing
//                       Overflow: |q| <= 2^31 and a cluster has fewer than 2^31 members (V < 2^31 - 64), so every |sum| is
//                       below 2^31 * 2^31 = 2^62 < 2^63: the int64 sums are exact, whatever order the adds arrived in.
//                       Optionally (NM_MESH_SIMPLIFY_AGGREGATE) the lanes of a wave that hold the same slot are summed in
//                       registers first and their leader adds once (cc_count's ballots): the same integers either way.
//   2. ms_representatives   rep[v] = the representative of v's cluster (-1 for a bad vertex); the clusters are counted.
//   3. ms_insert_faces  every corner becomes its representative.  A face with an index outside [0, V) or a bad vertex is BAD
//                       (counted, left out); one with two equal corners is DEGENERATE.  The others enter a second table
//                       (power of two >= 2 F) that holds one FACE INDEX per slot: claimed by compare-and-swap, lowered by
//                       atomicMin.  A candidate compares its canonical triple (smallest corner rotated to the front: the cyclic
//                       order, hence the winding, is kept -- opposite windings are different faces) with the occupant's,
//                       computed from the occupant's own row: all occupants a slot ever has carry the same triple, so there is
//                       no key to store and no bound on V.  Same rules: agent-scope atomics only, bounded walks, no waiting.
//   4. ms_mark          a face stays when it is the index its slot ended with: of duplicates the smallest.  Keep bits leave
//                       each wave as one ballot word; the representatives of kept faces' corners get their bit by atomicOr.
//   5. subset_scan / ms_emit_vertices / subset_compact_faces   the ordered compaction of compact.h over both sets of words
//                       (the faces through rep[]: mesh_subset.hip): kept faces in input order with their corners in their own
//                       order; kept clusters by ascending representative (numpy: new = cumsum(used) - 1), which is marching
//                       cubes' scan order.  A cluster of ONE member emits that member's
//                       rows bit for bit; a larger one
//                         p = (float)((double) lo + (double) cell * ((double) S / ((double) n * 2^30)))
//                         normal = s / sqrt((sx sx + sy sy) + sz sz) with s = (float) S per component, or the representative's
//                                  own normal when S is the zero vector
// The only host round trip is the one that returns the counts (nm_mesh_simplify_cluster).
#include "compact.h"
#include "nm_internal.h"

namespace nm {

constexpr float MS_CELLS = 2097152.0f;           // 2^21 cells per axis
constexpr double MS_QUANTUM = 1073741824.0;      // 2^30 quanta per cell edge / per unit of a normal component
constexpr double MS_QMAX = 2147483648.0;         // 2^31: the largest |q|
constexpr float MS_NORMAL_MAX = 2.0f;            // the largest normal component that is summed

struct MsSlot {                                  // 64 bytes: one vertex's atomics land in one line
    unsigned long long key;
    long long psum[3];
    long long nsum[3];
    int rep;
    unsigned count;
};
static_assert(sizeof(MsSlot) == 64, "one slot per 64 bytes");

struct MsHeader {
    unsigned long long clusters, degenerate, duplicate, bad_vertices, bad_faces;
    unsigned long long pad[3];
    unsigned long long totals[2];                // vertices kept, faces kept
    unsigned long long pad2[6];
};

struct MsGrid { float o[3]; float cell; };

// cell of a vertex -> false: bad
__device__ __forceinline__ bool ms_cell(const MsGrid& g, const float (&x)[3], float (&c)[3], unsigned long long& key) {
    bool ok = true;
    key = 0ull;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c[k] = floorf((x[k] - g.o[k]) / g.cell);
        ok = ok && isfinite(x[k]) && c[k] >= 0.0f && c[k] < MS_CELLS;            // a NaN fails both comparisons
        key |= (unsigned long long)(ok ? (unsigned)c[k] : 0u) << (21 * k);
    }
    return ok;
}

__device__ __forceinline__ long long ms_quantise(float t) {
    double s = (double)t * MS_QUANTUM;
    s = !(s >= -MS_QMAX) ? -MS_QMAX : (s > MS_QMAX ? MS_QMAX : s);
    return (long long)rint(s);
}

__global__ __launch_bounds__(256) void ms_init(MsSlot* __restrict__ table, uint64_t cap, int* __restrict__ ftab, uint64_t fcap,
                                               unsigned long long* __restrict__ vwords, int64_t nvw, MsHeader* hdr) {
    const uint64_t stride = (uint64_t)gridDim.x * 256, first = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    MsSlot empty;
    empty.key = EMPTY_KEY;
#pragma unroll
    for (int k = 0; k < 3; ++k) empty.psum[k] = empty.nsum[k] = 0;
    empty.rep = 0x7fffffff;
    empty.count = 0u;
    for (uint64_t i = first; i < cap; i += stride) table[i] = empty;
    for (uint64_t i = first; i < fcap; i += stride) ftab[i] = -1;
    for (uint64_t i = first; i < (uint64_t)nvw; i += stride) vwords[i] = 0ull;
    if (first < sizeof(MsHeader) / 8) reinterpret_cast<unsigned long long*>(hdr)[first] = 0ull;
}

__device__ __forceinline__ void ms_add(long long* p, long long q) {
    if (q) __hip_atomic_fetch_add(p, q, NM_RELAXED_AGENT);
}

// One thread per vertex, whole waves (the aggregation votes).  slot_of[v] = v's slot; rep[v] = -1 marks a bad vertex.
template <bool AGGREGATE>
__global__ __launch_bounds__(256) void ms_insert(const float* __restrict__ verts, const float* __restrict__ normals, int nv,
                                                 MsGrid g, MsSlot* table, uint64_t cap, uint32_t* __restrict__ slot_of,
                                                 int* __restrict__ rep, MsHeader* hdr) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = v < nv;
    bool todo = valid;
    unsigned long long s = cap;
    long long q[6] = {0, 0, 0, 0, 0, 0};
    if (valid) {
        float x[3], c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = verts[3 * v + k];
        unsigned long long key;
        todo = ms_cell(g, x, c, key);
        if (todo) {
            bool claimed;                        // whoever claims the slot: at most V cells live in >= 2 V slots
            s = find_or_insert(table, cap, key, claimed);
            todo = s < cap;
        }
        slot_of[v] = todo ? (uint32_t)s : 0u;
        rep[v] = todo ? 0 : -1;
        if (todo) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float step = c[k] * g.cell;
                const float lo = g.o[k] + step;
                q[k] = ms_quantise((x[k] - lo) / g.cell);
            }
            if (normals) {
                float n[3];
                bool ok = true;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    n[k] = normals[3 * v + k];
                    ok = ok && isfinite(n[k]) && fabsf(n[k]) <= MS_NORMAL_MAX;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) q[3 + k] = ok ? (long long)rint((double)n[k] * MS_QUANTUM) : 0ll;
            }
        }
    }
    const unsigned long long bad = __ballot(valid && !todo);
    if (lane == 0 && bad) atomicAdd(&hdr->bad_vertices, (unsigned long long)__popcll(bad));
    if (!AGGREGATE) {
        if (todo) {
            MsSlot* slot = table + s;
            __hip_atomic_fetch_min(&slot->rep, (int)v, NM_RELAXED_AGENT);
            __hip_atomic_fetch_add(&slot->count, 1u, NM_RELAXED_AGENT);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                ms_add(slot->psum + k, q[k]);
                ms_add(slot->nsum + k, q[3 + k]);
            }
        }
        return;
    }
    unsigned long long left = __ballot(todo);
    while (left) {                                                   // uniform over the wave
        const int leader = __ffsll((long long)left) - 1;
        const unsigned long long want = __shfl(s, leader, 64);
        const bool mine = todo && s == want;
        const unsigned long long same = __ballot(mine);
        const unsigned members = (unsigned)__popcll(same);
        long long r[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) r[k] = mine ? q[k] : 0ll;
        if (members > 1) {
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                if (k >= 3 && !normals) break;
#pragma unroll
                for (int off = 32; off; off >>= 1) r[k] += __shfl_xor(r[k], off, 64);
            }
        }
        if (lane == leader) {                                        // the group's lowest lane: its smallest vertex index
            MsSlot* slot = table + want;
            __hip_atomic_fetch_min(&slot->rep, (int)v, NM_RELAXED_AGENT);
            __hip_atomic_fetch_add(&slot->count, members, NM_RELAXED_AGENT);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                ms_add(slot->psum + k, r[k]);
                ms_add(slot->nsum + k, r[3 + k]);
            }
        }
        if (mine) todo = false;
        left &= ~same;
    }
}

__global__ __launch_bounds__(256) void ms_representatives(const MsSlot* __restrict__ table, const uint32_t* __restrict__ slot_of,
                                                          int* __restrict__ rep, int nv, MsHeader* hdr) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int r = -1;
    if (v < nv && rep[v] != -1) rep[v] = r = table[slot_of[v]].rep;
    const unsigned long long heads = __ballot(v < nv && r == (int)v);
    if ((threadIdx.x & 63) == 0 && heads) atomicAdd(&hdr->clusters, (unsigned long long)__popcll(heads));
}

// the representatives of face f's corners -> false: an index outside [0, nv) or a bad vertex (nothing out of range is read)
__device__ __forceinline__ bool ms_corners(const int32_t* __restrict__ faces, int64_t f, int nv, const int* __restrict__ rep,
                                           int (&r)[3]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int v = faces[3 * f + k];
        const bool in = (unsigned)v < (unsigned)nv;
        r[k] = in ? rep[v] : -1;
        ok = ok && in && (unsigned)r[k] < (unsigned)nv;
    }
    return ok;
}

__device__ __forceinline__ bool ms_degenerate(const int (&r)[3]) { return r[0] == r[1] || r[1] == r[2] || r[0] == r[2]; }

// the smallest corner to the front, the cyclic order kept
__device__ __forceinline__ void ms_canonical(const int (&r)[3], int (&t)[3]) {
    const int k = (r[0] <= r[1] && r[0] <= r[2]) ? 0 : (r[1] <= r[2] ? 1 : 2);
    t[0] = r[k];
    t[1] = r[(k + 1) % 3];
    t[2] = r[(k + 2) % 3];
}

__global__ __launch_bounds__(256) void ms_insert_faces(const int32_t* __restrict__ faces, int64_t nf, int nv,
                                                       const int* __restrict__ rep, int* ftab, uint64_t fcap,
                                                       uint32_t* __restrict__ fslot) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int r[3], t[3];
    if (f >= nf || !ms_corners(faces, f, nv, rep, r) || ms_degenerate(r)) return;
    ms_canonical(r, t);
    uint64_t s = mix64(mix64(((unsigned long long)(unsigned)t[0] << 32) | (unsigned)t[1]) ^ (unsigned long long)(unsigned)t[2]) & (fcap - 1);
    uint32_t placed = 0u;                                            // a walk that ran out (it cannot: <= F triples in >= 2 F slots)
    for (uint64_t i = 0; i < fcap; ++i, s = (s + 1) & (fcap - 1)) {  // leaves slot 0 unowned by f: the face counts as a duplicate
        int o = __hip_atomic_load(ftab + s, NM_RELAXED_AGENT);
        if (o == -1 && __hip_atomic_compare_exchange_strong(ftab + s, &o, (int)f, __ATOMIC_RELAXED, NM_RELAXED_AGENT)) {
            placed = (uint32_t)s;
            break;
        }
        int ro[3], to[3];                                            // o: a face that entered the table, so a valid one
        if ((int64_t)o < 0 || (int64_t)o >= nf || !ms_corners(faces, o, nv, rep, ro)) continue;
        ms_canonical(ro, to);
        if (to[0] == t[0] && to[1] == t[1] && to[2] == t[2]) {
            __hip_atomic_fetch_min(ftab + s, (int)f, NM_RELAXED_AGENT);
            placed = (uint32_t)s;
            break;
        }
    }
    fslot[f] = placed;
}

// keep bits of the faces (one ballot word per 64), the counts, and the used bits of the representatives
__global__ __launch_bounds__(256) void ms_mark(const int32_t* __restrict__ faces, int64_t nf, int nv, const int* __restrict__ rep,
                                               const int* __restrict__ ftab, const uint32_t* __restrict__ fslot,
                                               unsigned long long* __restrict__ fwords, unsigned long long* vwords, MsHeader* hdr) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int r[3] = {0, 0, 0};
    const bool in = f < nf;
    const bool ok = in && ms_corners(faces, f, nv, rep, r);
    const bool flat = ok && ms_degenerate(r);
    const bool live = ok && !flat;
    const bool keep = live && ftab[fslot[f]] == (int)f;
    store_keep_word(fwords, f, nf, keep);
    const unsigned long long bad = __ballot(in && !ok), deg = __ballot(flat), dup = __ballot(live && !keep);
    if (keep) {
#pragma unroll
        for (int k = 0; k < 3; ++k) atomicOr(vwords + (r[k] >> 6), 1ull << (r[k] & 63));
    }
    if ((threadIdx.x & 63) == 0) {                                   // a wave beyond the last word has no face to count
        if (bad) atomicAdd(&hdr->bad_faces, (unsigned long long)__popcll(bad));
        if (deg) atomicAdd(&hdr->degenerate, (unsigned long long)__popcll(deg));
        if (dup) atomicAdd(&hdr->duplicate, (unsigned long long)__popcll(dup));
    }
}

__global__ __launch_bounds__(256) void ms_emit_vertices(const float* __restrict__ verts, const float* __restrict__ normals, int nv,
                                                        MsGrid g, const MsSlot* __restrict__ table,
                                                        const uint32_t* __restrict__ slot_of,
                                                        const unsigned long long* __restrict__ vwords,
                                                        const uint32_t* __restrict__ vprefix, int64_t capacity,
                                                        float* __restrict__ out_verts, float* __restrict__ out_normals) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv || !bit_test(vwords, v)) return;                       // set bits are representatives: good vertices
    const int64_t dst = bit_rank(vwords, vprefix, v);
    if (dst >= capacity) return;                                     // never past the caller's arrays
    const MsSlot slot = table[slot_of[v]];
    float x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = verts[3 * v + k];
    if (slot.count <= 1u) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            out_verts[3 * dst + k] = x[k];
            if (normals) out_normals[3 * dst + k] = normals[3 * v + k];
        }
        return;
    }
    float c[3];
    unsigned long long key;
    ms_cell(g, x, c, key);
    const double members = (double)slot.count * MS_QUANTUM;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float step = c[k] * g.cell;
        const float lo = g.o[k] + step;
        const double mean = (double)slot.psum[k] / members;
        const double offset = (double)g.cell * mean;
        out_verts[3 * dst + k] = (float)((double)lo + offset);
    }
    if (!normals) return;
    if (slot.nsum[0] == 0 && slot.nsum[1] == 0 && slot.nsum[2] == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out_normals[3 * dst + k] = normals[3 * v + k];
        return;
    }
    const float sx = (float)slot.nsum[0], sy = (float)slot.nsum[1], sz = (float)slot.nsum[2];
    const float xx = sx * sx, yy = sy * sy, zz = sz * sz;
    const float xy = xx + yy;
    const float len = sqrtf(xy + zz);
    out_normals[3 * dst + 0] = sx / len;
    out_normals[3 * dst + 1] = sy / len;
    out_normals[3 * dst + 2] = sz / len;
}

// the smallest power of two >= 2 n (at least 64)
static uint64_t ms_capacity(int64_t n) {
    uint64_t cap = 64;
    while (cap < 2 * (uint64_t)n) cap <<= 1;
    return cap;
}

struct MsWorkspace {
    MsHeader* hdr;
    MsSlot* table;
    uint32_t* slot_of;
    int* rep;
    int* ftab;
    uint32_t* fslot;
    SubsetBits bits;
    uint64_t cap, fcap;
    int64_t bytes;
};

static MsWorkspace ms_carve(const void* ws, int64_t nv, int64_t nf) {
    Carver c(ws, 256);
    MsWorkspace w;
    w.cap = ms_capacity(nv);
    w.fcap = ms_capacity(nf);
    w.hdr = c.take<MsHeader>(1);
    w.table = c.take<MsSlot>((int64_t)w.cap);
    w.slot_of = c.take<uint32_t>(nv);
    w.rep = c.take<int>(nv);
    w.ftab = c.take<int>((int64_t)w.fcap);
    w.fslot = c.take<uint32_t>(nf);
    w.bits = take_subset_bits(c, nv, nf);
    w.bytes = c.offset;
    return w;
}

// compact.h's is_finite under the name that the grid requirements' texts carry (NM_REQUIRE quotes its condition)
static bool ms_finite(float x) { return is_finite(x); }

}  // namespace nm

using namespace nm;

#define MS_REQUIRE_GRID(ox, oy, oz, cell)                                                                                \
    NM_REQUIRE(ms_finite(cell) && cell > 0.0f, "mesh simplify: the cell size must be finite and > 0");                   \
    NM_REQUIRE(ms_finite(ox) && ms_finite(oy) && ms_finite(oz), "mesh simplify: the origin must be finite")

extern "C" {

int64_t nm_mesh_simplify_workspace_bytes(int64_t num_vertices, int64_t num_faces) {
    if (!mesh_size_ok(num_vertices) || !mesh_size_ok(num_faces)) return 0;
    return ms_carve(nullptr, num_vertices, num_faces).bytes;
}

int nm_mesh_simplify_cluster(const float* d_verts, int64_t num_vertices, const int32_t* d_faces, int64_t num_faces,
                             const float* d_normals, float origin_x, float origin_y, float origin_z, float cell, int32_t flags,
                             void* d_workspace, int64_t* h_counts, void* stream) {
    if (require_mesh("mesh simplify", num_vertices, num_faces)) return 2;
    MS_REQUIRE_GRID(origin_x, origin_y, origin_z, cell);
    NM_REQUIRE((flags & ~NM_MESH_SIMPLIFY_AGGREGATE) == 0, "mesh simplify: unknown flags");
    NM_REQUIRE(d_workspace && h_counts && (num_vertices == 0 || d_verts) && (num_faces == 0 || d_faces), "bad argument");
    const MsWorkspace w = ms_carve(d_workspace, num_vertices, num_faces);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nv = (int)num_vertices;
    const MsGrid g{{origin_x, origin_y, origin_z}, cell};
    const unsigned vgrid = launch_grid(num_vertices), fgrid = launch_grid(num_faces);
    const uint64_t most = w.cap > w.fcap ? w.cap : w.fcap;
    hipLaunchKernelGGL(ms_init, dim3((unsigned)(most / 256 > 4096 ? 4096 : most / 256 ? most / 256 : 1)), dim3(256), 0, s, w.table,
                       w.cap, w.ftab, w.fcap, w.bits.vwords, w.bits.nvw, w.hdr);
    NM_HIP_CHECK(hipGetLastError());
    if (nv) {
        if (flags & NM_MESH_SIMPLIFY_AGGREGATE)
            hipLaunchKernelGGL(ms_insert<true>, dim3(vgrid), dim3(256), 0, s, d_verts, d_normals, nv, g, w.table, w.cap,
                               w.slot_of, w.rep, w.hdr);
        else
            hipLaunchKernelGGL(ms_insert<false>, dim3(vgrid), dim3(256), 0, s, d_verts, d_normals, nv, g, w.table, w.cap,
                               w.slot_of, w.rep, w.hdr);
        NM_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(ms_representatives, dim3(vgrid), dim3(256), 0, s, w.table, w.slot_of, w.rep, nv, w.hdr);
        NM_HIP_CHECK(hipGetLastError());
    }
    if (num_faces) {
        hipLaunchKernelGGL(ms_insert_faces, dim3(fgrid), dim3(256), 0, s, d_faces, num_faces, nv, w.rep, w.ftab, w.fcap,
                           w.fslot);
        NM_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(ms_mark, dim3(fgrid), dim3(256), 0, s, d_faces, num_faces, nv, w.rep, w.ftab, w.fslot, w.bits.fwords,
                           w.bits.vwords, w.hdr);
        NM_HIP_CHECK(hipGetLastError());
    }
    if (const int rc = subset_scan(w.bits, w.hdr->totals, s)) return rc;
    MsHeader h;
    NM_HIP_CHECK(hipMemcpyAsync(&h, w.hdr, sizeof(MsHeader), hipMemcpyDeviceToHost, s));
    NM_HIP_CHECK(hipStreamSynchronize(s));
    h_counts[NM_MESH_SIMPLIFY_CLUSTERS] = (int64_t)h.clusters;
    h_counts[NM_MESH_SIMPLIFY_VERTICES_KEPT] = (int64_t)h.totals[0];
    h_counts[NM_MESH_SIMPLIFY_FACES_KEPT] = (int64_t)h.totals[1];
    h_counts[NM_MESH_SIMPLIFY_DEGENERATE] = (int64_t)h.degenerate;
    h_counts[NM_MESH_SIMPLIFY_DUPLICATE] = (int64_t)h.duplicate;
    h_counts[NM_MESH_SIMPLIFY_BAD_VERTICES] = (int64_t)h.bad_vertices;
    h_counts[NM_MESH_SIMPLIFY_BAD_FACES] = (int64_t)h.bad_faces;
    return 0;
}

int nm_mesh_simplify_emit(const void* d_workspace, const float* d_verts, int64_t num_vertices, const int32_t* d_faces,
                          int64_t num_faces, const float* d_normals, float origin_x, float origin_y, float origin_z, float cell,
                          int64_t vertices_kept, int64_t faces_kept, float* d_out_verts, int32_t* d_out_faces,
                          float* d_out_normals, void* stream) {
    if (require_mesh("mesh simplify", num_vertices, num_faces)) return 2;
    MS_REQUIRE_GRID(origin_x, origin_y, origin_z, cell);
    NM_REQUIRE_COMPACT_OUTPUTS("mesh simplify", d_workspace && (num_vertices == 0 || d_verts) && (num_faces == 0 || d_faces),
                               d_out_verts && (!d_normals || d_out_normals));
    const MsWorkspace w = ms_carve(d_workspace, num_vertices, num_faces);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nv = (int)num_vertices;
    const MsGrid g{{origin_x, origin_y, origin_z}, cell};
    if (vertices_kept) {
        hipLaunchKernelGGL(ms_emit_vertices, dim3(launch_grid(num_vertices)), dim3(256), 0, s, d_verts, d_normals, nv, g, w.table,
                           w.slot_of, w.bits.vwords, w.bits.vprefix, vertices_kept, d_out_verts, d_out_normals);
        NM_HIP_CHECK(hipGetLastError());
    }
    return subset_compact_faces(d_faces, num_faces, nv, faces_kept, w.bits, w.rep, d_out_faces, nullptr, s);
}

}  // extern "C"
