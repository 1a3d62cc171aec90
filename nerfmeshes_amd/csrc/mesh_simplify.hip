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
// QUADRIC PLACEMENT (mesh_nerf --simplify-placement quadric; nm_mesh_simplify_quadric_faces + nm_mesh_simplify_emit_quadric)
// changes one thing: the position of a cluster of two or more members is the point of its cell that is closest, in the least
// squares sense, to the planes of the faces around it (Lindstrom's quadric-optimal representative), not the members' mean.
//   3b. ms_quadric_faces   one thread per face, whole waves, after steps 1-4.  A face that is not BAD contributes once per
//                       corner k to the cluster of that corner, in integers, on a lattice of 2^8 points per cell edge that is
//                       local to the corner's cell: u = (int64) rint((double) t * 2^8) per axis, clamped to [-2^9, 2^9]; with
//                       C = (int64) c, e1 = (C1 - C0) * 2^8 + (u1 - u0) and e2 likewise for the third corner (cyclic order from
//                       k).  An edge component beyond 2^9 (two cells) makes the corner FAR: counted, no contribution.
//                       Else nrm = e1 x e2 (area^2 weighting), d = -(nrm . u0), and the corner adds the six nrm_i nrm_j, the
//                       three nrm_i d and 1 to its cluster's row of a SECOND per-slot array (MsQuadric, 128 bytes; MsSlot stays
//                       as it is) by agent-scope relaxed 64-bit adds -- the rule of ms_insert: every access to the shared array
//                       inside the launch is such an atomic; zero addends are skipped.
//                       Overflow: |e| <= 2^9 gives |nrm_i| <= 2 * 2^9 * 2^9 = 2^19, so |nrm_i nrm_j| <= 2^38; |u0| <= 2^9 gives
//                       |d| <= 3 * 2^19 * 2^9 = 3 * 2^28 and |nrm_i d| <= 3 * 2^47 < 2^49.  The row counts its contributions
//                       (64 bits: fewer than 3 * 2^31 corners exist).  A cluster that ends with more than 2^13 is CROWDED: its
//                       sums are never read, it gets the mean, and whatever the adds wrapped to is irrelevant.  One that ends
//                       with at most 2^13 saw exactly that many adds, so every partial |sum of A| <= 2^13 * 2^38 = 2^51 and
//                       every partial |sum of B| < 2^13 * 2^49 = 2^62 < 2^63: exact, whatever order the adds arrived in.
//                       NM_MESH_SIMPLIFY_AGGREGATE: ms_insert's ballot loop once per corner -- the lanes of a wave whose
//                       corner k shares a slot are summed in registers, their leader adds once: the same integers.
//   5b. ms_emit_vertices<true>   a kept cluster of n >= 2 members with 1 <= contributions <= 2^13 and a positive trace solves
//                       (A + tr * 2^-6 I) delta = -(A m + b) around the mean m (lattice units) by the adjugate, a fixed sequence
//                       of individually rounded fp64 operations on the exact sums (msq_place); the regulariser bounds the
//                       condition number by about 200 and leaves the vertex at the mean along directions no plane constrains.
//                       det <= 0 or a non-finite delta: SINGULAR, the mean.  x = m + delta is clamped to the cell [0, 2^8]
//                       (CLAMPED) and p = (float)((double) lo + (double) cell * (x / 2^8)).  The kept clusters' SOLVED /
//                       CROWDED / SINGULAR / CLAMPED counts leave each wave as one atomic each.
// The only host round trips are the ones that return counts (nm_mesh_simplify_cluster, nm_mesh_simplify_emit_quadric).
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

constexpr double MSQ_LATTICE = 256.0;            // 2^8 lattice points per cell edge
constexpr long long MSQ_REACH = 512;             // 2^9: the largest |u| and the largest edge component (two cells)
constexpr unsigned long long MSQ_MAX_CONTRIBUTIONS = 8192ull;   // 2^13: a cluster with more is CROWDED
constexpr double MSQ_LAMBDA = 0.015625;          // 2^-6 of the trace on the diagonal

struct MsQuadric {                               // 128 bytes: one corner's atomics land in one line
    long long a[6];                              // sum of nrm nrm^T: 00 01 02 11 12 22
    long long b[3];                              // sum of nrm d
    unsigned long long contributions;
    double frac[3];                              // the adaptive levels' (msa_place): the placed point in units of the cell,
    unsigned long long err;                      //   the largest d2 of a corner as the bits of a non-negative double (msa_error),
    unsigned status, far;                        //   msq_place's status, and whether a corner of the row was FAR
    unsigned long long pad;
};
static_assert(sizeof(MsQuadric) == 128 && offsetof(MsQuadric, frac) == 80, "one quadric per 128 bytes");

struct MsQuadricHeader {                         // NM_MESH_SIMPLIFY_QUADRIC_* order
    unsigned long long solved, crowded, singular, clamped, far;
    unsigned long long pad[3];
};

enum : unsigned { MSQ_SOLVED = 1u, MSQ_CROWDED = 2u, MSQ_SINGULAR = 4u, MSQ_CLAMPED = 8u };

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

__device__ __forceinline__ long long msq_lattice(float t) {
    double s = (double)t * MSQ_LATTICE;
    s = !(s >= -(double)MSQ_REACH) ? -(double)MSQ_REACH : (s > (double)MSQ_REACH ? (double)MSQ_REACH : s);
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

// lattice coordinates and integer cell of the good vertex v
__device__ __forceinline__ void msq_vertex(const float* __restrict__ verts, int v, const MsGrid& g, long long (&cell)[3],
                                           long long (&u)[3]) {
    float x[3], c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = verts[3 * (int64_t)v + k];
    unsigned long long key;
    ms_cell(g, x, c, key);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float step = c[k] * g.cell;
        const float lo = g.o[k] + step;
        cell[k] = (long long)c[k];
        u[k] = msq_lattice((x[k] - lo) / g.cell);
    }
}

// One thread per face, whole waves (the votes), after ms_representatives: rep[] tells the bad vertices, slot_of[] the rows.
template <bool AGGREGATE>
__global__ __launch_bounds__(256) void ms_quadric_faces(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                        int64_t nf, int nv, MsGrid g, const uint32_t* __restrict__ slot_of,
                                                        const int* __restrict__ rep, uint64_t cap, MsQuadric* quad,
                                                        MsQuadricHeader* qh) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int r[3];
    const bool live = f < nf && ms_corners(faces, f, nv, rep, r);
    long long cell[3][3], u[3][3];
    uint32_t slot[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int j = 0; j < 3; ++j) cell[k][j] = u[k][j] = 0;
        if (live) {
            const int v = faces[3 * f + k];
            msq_vertex(verts, v, g, cell[k], u[k]);
            slot[k] = slot_of[v];
        }
    }
    unsigned far = 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
        long long e1[3], e2[3];
        bool todo = live && slot[k] < cap;                             // a slot of this table: nothing else is ever addressed
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            e1[j] = (cell[k1][j] - cell[k][j]) * (long long)MSQ_LATTICE + (u[k1][j] - u[k][j]);
            e2[j] = (cell[k2][j] - cell[k][j]) * (long long)MSQ_LATTICE + (u[k2][j] - u[k][j]);
            todo = todo && e1[j] >= -MSQ_REACH && e1[j] <= MSQ_REACH && e2[j] >= -MSQ_REACH && e2[j] <= MSQ_REACH;
        }
        far += (unsigned)__popcll(__ballot(live && !todo));
        long long q[9];
        {
#pragma unroll
            for (int j = 0; j < 3; ++j) {                              // the bounds above hold for what is multiplied
                e1[j] = todo ? e1[j] : 0ll;
                e2[j] = todo ? e2[j] : 0ll;
            }
            const long long n0 = e1[1] * e2[2] - e1[2] * e2[1];
            const long long n1 = e1[2] * e2[0] - e1[0] * e2[2];
            const long long n2 = e1[0] * e2[1] - e1[1] * e2[0];
            const long long d = -(n0 * u[k][0] + n1 * u[k][1] + n2 * u[k][2]);
            q[0] = n0 * n0; q[1] = n0 * n1; q[2] = n0 * n2; q[3] = n1 * n1; q[4] = n1 * n2; q[5] = n2 * n2;
            q[6] = n0 * d;  q[7] = n1 * d;  q[8] = n2 * d;
        }
        if (!AGGREGATE) {
            if (todo) {
                MsQuadric* row = quad + slot[k];
#pragma unroll
                for (int i = 0; i < 6; ++i) ms_add(row->a + i, q[i]);
#pragma unroll
                for (int i = 0; i < 3; ++i) ms_add(row->b + i, q[6 + i]);
                __hip_atomic_fetch_add(&row->contributions, 1ull, NM_RELAXED_AGENT);
            }
            continue;
        }
        unsigned long long left = __ballot(todo);
        while (left) {                                                   // uniform over the wave
            const int leader = __ffsll((long long)left) - 1;
            const uint32_t want = __shfl(slot[k], leader, 64);
            const bool mine = todo && slot[k] == want;
            const unsigned long long same = __ballot(mine);
            long long s[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) s[i] = mine ? q[i] : 0ll;
            if (__popcll(same) > 1) {
#pragma unroll
                for (int i = 0; i < 9; ++i) {
#pragma unroll
                    for (int off = 32; off; off >>= 1) s[i] += __shfl_xor(s[i], off, 64);
                }
            }
            if (lane == leader) {
                MsQuadric* row = quad + want;
#pragma unroll
                for (int i = 0; i < 6; ++i) ms_add(row->a + i, s[i]);
#pragma unroll
                for (int i = 0; i < 3; ++i) ms_add(row->b + i, s[6 + i]);
                __hip_atomic_fetch_add(&row->contributions, (unsigned long long)__popcll(same), NM_RELAXED_AGENT);
            }
            if (mine) todo = false;
            left &= ~same;
        }
    }
    if (lane == 0 && far) atomicAdd(&qh->far, (unsigned long long)far);
}

// The quadric-optimal place of a cluster: frac[] comes in as the members' mean in units of the cell and leaves as x / 2^8 when
// the cluster is SOLVED; every other status leaves the mean.  Every operation is an fp64 operation rounded on its own.
__device__ __forceinline__ unsigned msq_place(const MsQuadric& q, double (&frac)[3]) {
    if (q.contributions > MSQ_MAX_CONTRIBUTIONS) return MSQ_CROWDED;
    if (q.contributions == 0ull) return 0u;
    const double a00 = (double)q.a[0], a01 = (double)q.a[1], a02 = (double)q.a[2];
    const double a11 = (double)q.a[3], a12 = (double)q.a[4], a22 = (double)q.a[5];
    const double b0 = (double)q.b[0], b1 = (double)q.b[1], b2 = (double)q.b[2];
    const double tr = (a00 + a11) + a22;
    if (!(tr > 0.0)) return 0u;
    const double m0 = frac[0] * MSQ_LATTICE, m1 = frac[1] * MSQ_LATTICE, m2 = frac[2] * MSQ_LATTICE;
    const double ridge = tr * MSQ_LAMBDA;
    const double M00 = a00 + ridge, M11 = a11 + ridge, M22 = a22 + ridge, M01 = a01, M02 = a02, M12 = a12;
    const double r0 = -(((a00 * m0 + a01 * m1) + a02 * m2) + b0);
    const double r1 = -(((a01 * m0 + a11 * m1) + a12 * m2) + b1);
    const double r2 = -(((a02 * m0 + a12 * m1) + a22 * m2) + b2);
    const double c00 = M11 * M22 - M12 * M12;
    const double c01 = M02 * M12 - M01 * M22;
    const double c02 = M01 * M12 - M02 * M11;
    const double c11 = M00 * M22 - M02 * M02;
    const double c12 = M01 * M02 - M00 * M12;
    const double c22 = M00 * M11 - M01 * M01;
    const double det = (M00 * c00 + M01 * c01) + M02 * c02;
    const double d0 = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
    const double d1 = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
    const double d2 = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
    if (!(det > 0.0) || !(d0 - d0 == 0.0) || !(d1 - d1 == 0.0) || !(d2 - d2 == 0.0)) return MSQ_SINGULAR;
    double x[3] = {m0 + d0, m1 + d1, m2 + d2};
    unsigned status = MSQ_SOLVED;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (x[k] < 0.0) { x[k] = 0.0; status |= MSQ_CLAMPED; }
        if (x[k] > MSQ_LATTICE) { x[k] = MSQ_LATTICE; status |= MSQ_CLAMPED; }
        frac[k] = x[k] / MSQ_LATTICE;
    }
    return status;
}

// the normal row of a cluster of two or more members whose representative is v
__device__ __forceinline__ void ms_cluster_normal(const MsSlot& slot, const float* __restrict__ normals, int64_t v,
                                                  float* __restrict__ out) {
    if (slot.nsum[0] == 0 && slot.nsum[1] == 0 && slot.nsum[2] == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = normals[3 * v + k];
        return;
    }
    const float sx = (float)slot.nsum[0], sy = (float)slot.nsum[1], sz = (float)slot.nsum[2];
    const float xx = sx * sx, yy = sy * sy, zz = sz * sz;
    const float xy = xx + yy;
    const float len = sqrtf(xy + zz);
    out[0] = sx / len;
    out[1] = sy / len;
    out[2] = sz / len;
}

// the rows of the kept cluster whose representative is v -> its MSQ_* status (0 under mean placement)
template <bool QUADRIC>
__device__ __forceinline__ unsigned ms_emit_cluster(int64_t v, const float* __restrict__ verts, const float* __restrict__ normals,
                                                    const MsGrid& g, const MsSlot* __restrict__ table,
                                                    const MsQuadric* __restrict__ quad, const uint32_t* __restrict__ slot_of,
                                                    const unsigned long long* __restrict__ vwords,
                                                    const uint32_t* __restrict__ vprefix, int64_t capacity,
                                                    float* __restrict__ out_verts, float* __restrict__ out_normals) {
    const int64_t dst = bit_rank(vwords, vprefix, v);
    if (dst >= capacity) return 0u;                                  // never past the caller's arrays
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
        return 0u;
    }
    float c[3];
    unsigned long long key;
    ms_cell(g, x, c, key);
    const double members = (double)slot.count * MS_QUANTUM;
    double frac[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) frac[k] = (double)slot.psum[k] / members;
    const unsigned status = QUADRIC ? msq_place(quad[slot_of[v]], frac) : 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float step = c[k] * g.cell;
        const float lo = g.o[k] + step;
        const double offset = (double)g.cell * frac[k];
        out_verts[3 * dst + k] = (float)((double)lo + offset);
    }
    if (normals) ms_cluster_normal(slot, normals, v, out_normals + 3 * dst);
    return status;
}

// QUADRIC: quad and qh are the second workspace's; the launch is in whole waves and the statuses are counted per wave
template <bool QUADRIC>
__global__ __launch_bounds__(256) void ms_emit_vertices(const float* __restrict__ verts, const float* __restrict__ normals, int nv,
                                                        MsGrid g, const MsSlot* __restrict__ table,
                                                        const MsQuadric* __restrict__ quad,
                                                        const uint32_t* __restrict__ slot_of,
                                                        const unsigned long long* __restrict__ vwords,
                                                        const uint32_t* __restrict__ vprefix, int64_t capacity,
                                                        float* __restrict__ out_verts, float* __restrict__ out_normals,
                                                        MsQuadricHeader* qh) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned status = 0u;
    if (v < nv && bit_test(vwords, v))                                 // set bits are representatives: good vertices
        status = ms_emit_cluster<QUADRIC>(v, verts, normals, g, table, quad, slot_of, vwords, vprefix, capacity, out_verts,
                                          out_normals);
    if (!QUADRIC) return;
    const unsigned long long solved = __ballot(status & MSQ_SOLVED), crowded = __ballot(status & MSQ_CROWDED);
    const unsigned long long singular = __ballot(status & MSQ_SINGULAR), clamped = __ballot(status & MSQ_CLAMPED);
    if ((threadIdx.x & 63) == 0) {
        if (solved) atomicAdd(&qh->solved, (unsigned long long)__popcll(solved));
        if (crowded) atomicAdd(&qh->crowded, (unsigned long long)__popcll(crowded));
        if (singular) atomicAdd(&qh->singular, (unsigned long long)__popcll(singular));
        if (clamped) atomicAdd(&qh->clamped, (unsigned long long)__popcll(clamped));
    }
}

// ADAPTIVE LEVELS (mesh_nerf --simplify-levels L; nm_mesh_simplify_adaptive_level / _faces / _emit; DESIGN.md, "Adaptive
// clustering"): steps 1, 2 and 3b run once per level l = L .. 0 on the grid (origin, cell * 2^l) -- the multiplication is exact
// in fp32, so c_l = c_0 >> l per axis and the grids nest --, each level from the faces directly, in the same two workspaces;
// the overflow bounds above hold per level as they stand.  Then, per level:
//   msa_place    one lane per slot of the vertex table: an occupied slot of two or more members runs msq_place on its row and
//                parks frac[] (x / 2^8 when SOLVED, the mean else) and the status in the row's spare bytes.
//   msa_error    (l >= 1) one thread per face, whole waves: every corner that contributed to a SOLVED row -- the same u, e1, e2,
//                nrm and FAR rule as ms_quadric_faces -- with nrm != 0 gives, with x = frac * 2^8 (exact),
//                  d2 = ((n0 (x0 - u0) + n1 (x1 - u1)) + n2 (x2 - u2))^2 / ((n0 n0 + n1 n1) + n2 n2)
//                in fp64, every operation rounded on its own; the row keeps the largest by an agent-scope atomicMax on the
//                bits (d2 >= 0: the order of the bits is the order of the values, and a maximum does not depend on the order
//                it was taken in).  A FAR corner marks its row (atomicOr).  NM_MESH_SIMPLIFY_AGGREGATE_FACES: the lanes of a
//                wave whose corner k shares a row take their maximum in registers, their leader issues one atomic.
//   msa_assign   one lane per vertex that no coarser level took: its cell is ACCEPTED when it has one member, or when its row is
//                SOLVED (so neither CROWDED nor SINGULAR, and with a contribution), has no FAR corner and d2 <= tol^2 (level
//                0: always).  The vertex then takes the cell's representative and the level; the representative stages the
//                cluster's position, normal and status rows at its own index, by step 5 / 5b's rules with this level's grid.
//                Acceptance is a property of the cell and the members of a cell share every coarser cell, so they were all
//                still free and all decide alike: the chosen cells partition the vertices.  Refusals are counted once per
//                cluster, by the first reason of: crowded, no contribution (or zero trace), singular, far, error.
//   msa_emit     the staged rows of the kept clusters through the ordered compaction; statuses and levels are counted per wave.
// The faces go through the final rep[] by steps 3 -- 5 unchanged.  Host round trips: the two that return counts.
constexpr int MSA_MAX_LEVELS = 8;
constexpr int MSA_LEVEL_FIELDS = 8;              // NM_MESH_SIMPLIFY_LEVEL_* order

struct MsaHeader {
    unsigned long long level[MSA_MAX_LEVELS + 1][MSA_LEVEL_FIELDS];
    unsigned long long kept[MSA_MAX_LEVELS + 1];
    unsigned long long status[4];                // kept clusters: solved, crowded, singular, clamped
    unsigned long long far;                      // level 0's FAR corners
    unsigned long long pad[2];
};
enum : int { MSA_VERTICES = 0, MSA_CLUSTERS, MSA_REFUSED_ERROR, MSA_REFUSED_CROWDED, MSA_REFUSED_SINGULAR, MSA_REFUSED_FAR,
             MSA_REFUSED_EMPTY, MSA_MAX_D2 };

__global__ __launch_bounds__(256) void msa_place(const MsSlot* __restrict__ table, uint64_t cap, MsQuadric* __restrict__ quad) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= cap) return;
    const MsSlot slot = table[s];
    if (slot.key == EMPTY_KEY || slot.count <= 1u) return;
    const double members = (double)slot.count * MS_QUANTUM;
    double frac[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) frac[k] = (double)slot.psum[k] / members;
    const MsQuadric q = quad[s];
    const unsigned status = msq_place(q, frac);
#pragma unroll
    for (int k = 0; k < 3; ++k) quad[s].frac[k] = frac[k];
    quad[s].status = status;
}

// One thread per face, whole waves (the votes), after msa_place.  frac and status of a row are the previous launch's: plain
// loads; err and far are this launch's: agent-scope atomics only.
template <bool AGGREGATE>
__global__ __launch_bounds__(256) void msa_error(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t nf,
                                                 int nv, MsGrid g, const uint32_t* __restrict__ slot_of,
                                                 const int* __restrict__ rep, uint64_t cap, MsQuadric* quad) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int r[3];
    const bool live = f < nf && ms_corners(faces, f, nv, rep, r);
    long long cell[3][3], u[3][3];
    uint32_t slot[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int j = 0; j < 3; ++j) cell[k][j] = u[k][j] = 0;
        if (live) {
            const int v = faces[3 * f + k];
            msq_vertex(verts, v, g, cell[k], u[k]);
            slot[k] = slot_of[v];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
        long long e1[3], e2[3];
        const bool mine_row = live && slot[k] < cap;                   // a slot of this table: nothing else is ever addressed
        bool todo = mine_row;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            e1[j] = (cell[k1][j] - cell[k][j]) * (long long)MSQ_LATTICE + (u[k1][j] - u[k][j]);
            e2[j] = (cell[k2][j] - cell[k][j]) * (long long)MSQ_LATTICE + (u[k2][j] - u[k][j]);
            todo = todo && e1[j] >= -MSQ_REACH && e1[j] <= MSQ_REACH && e2[j] >= -MSQ_REACH && e2[j] <= MSQ_REACH;
        }
        if (mine_row && !todo) __hip_atomic_fetch_or(&quad[slot[k]].far, 1u, NM_RELAXED_AGENT);
        unsigned long long bits = 0ull;
        if (todo && (quad[slot[k]].status & MSQ_SOLVED)) {
            const long long n0 = e1[1] * e2[2] - e1[2] * e2[1];
            const long long n1 = e1[2] * e2[0] - e1[0] * e2[2];
            const long long n2 = e1[0] * e2[1] - e1[1] * e2[0];
            if (n0 | n1 | n2) {
                const MsQuadric* row = quad + slot[k];
                const double x0 = row->frac[0] * MSQ_LATTICE, x1 = row->frac[1] * MSQ_LATTICE, x2 = row->frac[2] * MSQ_LATTICE;
                const double d0 = (double)n0, d1 = (double)n1, d2 = (double)n2;
                const double p0 = d0 * (x0 - (double)u[k][0]), p1 = d1 * (x1 - (double)u[k][1]), p2 = d2 * (x2 - (double)u[k][2]);
                const double s = (p0 + p1) + p2;
                const double q0 = d0 * d0, q1 = d1 * d1, q2 = d2 * d2;
                const double den = (q0 + q1) + q2;
                const double ss = s * s;
                bits = (unsigned long long)__double_as_longlong(ss / den);
            }
        }
        if (!AGGREGATE) {
            if (bits) __hip_atomic_fetch_max(&quad[slot[k]].err, bits, NM_RELAXED_AGENT);
            continue;
        }
        bool open = bits != 0ull;
        unsigned long long left = __ballot(open);
        while (left) {                                                   // uniform over the wave
            const int leader = __ffsll((long long)left) - 1;
            const uint32_t want = __shfl(slot[k], leader, 64);
            const bool mine = open && slot[k] == want;
            const unsigned long long same = __ballot(mine);
            unsigned long long m = mine ? bits : 0ull;
            if (__popcll(same) > 1) {
#pragma unroll
                for (int off = 32; off; off >>= 1) {
                    const unsigned long long other = __shfl_xor(m, off, 64);
                    m = other > m ? other : m;
                }
            }
            if (lane == leader) __hip_atomic_fetch_max(&quad[want].err, m, NM_RELAXED_AGENT);
            if (mine) open = false;
            left &= ~same;
        }
    }
}

struct MsaStage {                                // per vertex; rows are written at representatives only
    int* rep;                                    // the final representative (-1: a bad vertex)
    signed char* level;                          // the level that took the vertex (-1: none yet)
    unsigned char* status;                       // the staged cluster's MSQ_* status
    float* pos;
    float* nrm;
};

// One thread per vertex, whole waves (the counts).  table, slot_of, rep and quad are this level's, all of earlier launches.
__global__ __launch_bounds__(256) void msa_assign(const float* __restrict__ verts, const float* __restrict__ normals, int nv,
                                                  MsGrid g, int level, double tol2, const MsSlot* __restrict__ table,
                                                  const MsQuadric* __restrict__ quad, const uint32_t* __restrict__ slot_of,
                                                  const int* __restrict__ rep, MsaStage st, MsaHeader* hdr) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool accepted = false, head = false, refused = false;
    unsigned status = 0u, far = 0u;
    unsigned long long err = 0ull;
    unsigned count = 0u;
    if (v < nv) {
        const int r = rep[v];
        if (r < 0) {
            if (level == 0) st.rep[v] = -1;                          // a bad vertex of the finest grid is in no cluster
        } else if (st.level[v] < 0) {
            const uint32_t s = slot_of[v];
            const MsSlot slot = table[s];
            count = slot.count;
            if (count >= 2u) {
                status = quad[s].status;
                far = quad[s].far;
                err = quad[s].err;
            }
            accepted = level == 0 || count <= 1u ||
                       ((status & MSQ_SOLVED) && !far && __longlong_as_double((long long)err) <= tol2);
            head = r == (int)v;
            refused = head && !accepted;
            if (accepted) {
                st.rep[v] = r;
                st.level[v] = (signed char)level;
            }
            if (head && accepted) {
                float x[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) x[k] = verts[3 * v + k];
                st.status[v] = (unsigned char)(count >= 2u ? status : 0u);
                if (count <= 1u) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        st.pos[3 * v + k] = x[k];
                        if (normals) st.nrm[3 * v + k] = normals[3 * v + k];
                    }
                } else {
                    float c[3];
                    unsigned long long key;
                    ms_cell(g, x, c, key);
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const float step = c[k] * g.cell;
                        const float lo = g.o[k] + step;
                        const double offset = (double)g.cell * quad[s].frac[k];
                        st.pos[3 * v + k] = (float)((double)lo + offset);
                    }
                    if (normals) ms_cluster_normal(slot, normals, v, st.nrm + 3 * v);
                    if (level > 0 && err) atomicMax(&hdr->level[level][MSA_MAX_D2], err);
                }
            }
        }
    }
    const bool crowded = refused && (status & MSQ_CROWDED), empty = refused && status == 0u;
    const bool singular = refused && (status & MSQ_SINGULAR);
    const bool solved = refused && (status & MSQ_SOLVED);
    const unsigned long long took = __ballot(accepted), heads = __ballot(head && accepted);
    const unsigned long long b_crowded = __ballot(crowded), b_empty = __ballot(empty), b_singular = __ballot(singular);
    const unsigned long long b_far = __ballot(solved && far), b_error = __ballot(solved && !far);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* row = hdr->level[level];
        if (took) atomicAdd(row + MSA_VERTICES, (unsigned long long)__popcll(took));
        if (heads) atomicAdd(row + MSA_CLUSTERS, (unsigned long long)__popcll(heads));
        if (b_error) atomicAdd(row + MSA_REFUSED_ERROR, (unsigned long long)__popcll(b_error));
        if (b_crowded) atomicAdd(row + MSA_REFUSED_CROWDED, (unsigned long long)__popcll(b_crowded));
        if (b_singular) atomicAdd(row + MSA_REFUSED_SINGULAR, (unsigned long long)__popcll(b_singular));
        if (b_far) atomicAdd(row + MSA_REFUSED_FAR, (unsigned long long)__popcll(b_far));
        if (b_empty) atomicAdd(row + MSA_REFUSED_EMPTY, (unsigned long long)__popcll(b_empty));
    }
}

// One thread per vertex, whole waves: the staged rows of the kept clusters, in the order of their representatives.
__global__ __launch_bounds__(256) void msa_emit(int nv, int levels, MsaStage st, bool normals,
                                                const unsigned long long* __restrict__ vwords,
                                                const uint32_t* __restrict__ vprefix, int64_t capacity,
                                                float* __restrict__ out_verts, float* __restrict__ out_normals, MsaHeader* hdr) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned status = 0u;
    int level = -1;
    if (v < nv && bit_test(vwords, v)) {                               // set bits are representatives: good vertices
        const int64_t dst = bit_rank(vwords, vprefix, v);
        if (dst < capacity) {                                          // never past the caller's arrays
            status = st.status[v];
            level = st.level[v];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                out_verts[3 * dst + k] = st.pos[3 * v + k];
                if (normals) out_normals[3 * dst + k] = st.nrm[3 * v + k];
            }
        }
    }
    const unsigned long long solved = __ballot(status & MSQ_SOLVED), crowded = __ballot(status & MSQ_CROWDED);
    const unsigned long long singular = __ballot(status & MSQ_SINGULAR), clamped = __ballot(status & MSQ_CLAMPED);
    const bool first = (threadIdx.x & 63) == 0;
    if (first) {
        if (solved) atomicAdd(&hdr->status[0], (unsigned long long)__popcll(solved));
        if (crowded) atomicAdd(&hdr->status[1], (unsigned long long)__popcll(crowded));
        if (singular) atomicAdd(&hdr->status[2], (unsigned long long)__popcll(singular));
        if (clamped) atomicAdd(&hdr->status[3], (unsigned long long)__popcll(clamped));
    }
    for (int l = 0; l <= levels; ++l) {                                // uniform over the wave
        const unsigned long long at = __ballot(level == l);
        if (first && at) atomicAdd(&hdr->kept[l], (unsigned long long)__popcll(at));
    }
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

struct MsQuadricWorkspace {
    MsQuadricHeader* hdr;
    MsQuadric* quad;                             // row s belongs to slot s of the vertex table
    uint64_t cap;
    int64_t bytes;
};

static MsQuadricWorkspace msq_carve(const void* ws, int64_t nv) {
    Carver c(ws, 256);
    MsQuadricWorkspace w;
    w.cap = ms_capacity(nv);
    w.hdr = c.take<MsQuadricHeader>(1);
    w.quad = c.take<MsQuadric>((int64_t)w.cap);
    w.bytes = c.offset;
    return w;
}

struct MsaWorkspace {
    MsaHeader* hdr;
    MsaStage stage;
    int64_t bytes;
};

static MsaWorkspace msa_carve(const void* ws, int64_t nv) {
    Carver c(ws, 256);
    MsaWorkspace w;
    w.hdr = c.take<MsaHeader>(1);
    w.stage.rep = c.take<int>(nv);
    w.stage.level = c.take<signed char>(nv);
    w.stage.status = c.take<unsigned char>(nv);
    w.stage.pos = c.take<float>(3 * nv);
    w.stage.nrm = c.take<float>(3 * nv);
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
        hipLaunchKernelGGL(ms_emit_vertices<false>, dim3(launch_grid(num_vertices)), dim3(256), 0, s, d_verts, d_normals, nv, g,
                           w.table, (const MsQuadric*)nullptr, w.slot_of, w.bits.vwords, w.bits.vprefix, vertices_kept, d_out_verts,
                           d_out_normals, (MsQuadricHeader*)nullptr);
        NM_HIP_CHECK(hipGetLastError());
    }
    return subset_compact_faces(d_faces, num_faces, nv, faces_kept, w.bits, w.rep, d_out_faces, nullptr, s);
}

int64_t nm_mesh_simplify_quadric_workspace_bytes(int64_t num_vertices, int64_t num_faces) {
    if (!mesh_size_ok(num_vertices) || !mesh_size_ok(num_faces)) return 0;
    return msq_carve(nullptr, num_vertices).bytes;
}

int nm_mesh_simplify_quadric_faces(const void* d_workspace, const float* d_verts, int64_t num_vertices, const int32_t* d_faces,
                                   int64_t num_faces, float origin_x, float origin_y, float origin_z, float cell, int32_t flags,
                                   void* d_quadric_workspace, void* stream) {
    if (require_mesh("mesh simplify", num_vertices, num_faces)) return 2;
    MS_REQUIRE_GRID(origin_x, origin_y, origin_z, cell);
    NM_REQUIRE((flags & ~NM_MESH_SIMPLIFY_AGGREGATE) == 0, "mesh simplify: unknown flags");
    NM_REQUIRE(d_workspace && d_quadric_workspace && (num_vertices == 0 || d_verts) && (num_faces == 0 || d_faces), "bad argument");
    const MsWorkspace w = ms_carve(d_workspace, num_vertices, num_faces);
    const MsQuadricWorkspace q = msq_carve(d_quadric_workspace, num_vertices);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const MsGrid g{{origin_x, origin_y, origin_z}, cell};
    NM_HIP_CHECK(hipMemsetAsync(d_quadric_workspace, 0, (size_t)q.bytes, s));
    if (num_faces) {
        if (flags & NM_MESH_SIMPLIFY_AGGREGATE)
            hipLaunchKernelGGL(ms_quadric_faces<true>, dim3(launch_grid(num_faces)), dim3(256), 0, s, d_verts, d_faces, num_faces,
                               (int)num_vertices, g, w.slot_of, w.rep, q.cap, q.quad, q.hdr);
        else
            hipLaunchKernelGGL(ms_quadric_faces<false>, dim3(launch_grid(num_faces)), dim3(256), 0, s, d_verts, d_faces, num_faces,
                               (int)num_vertices, g, w.slot_of, w.rep, q.cap, q.quad, q.hdr);
        NM_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

int nm_mesh_simplify_emit_quadric(const void* d_workspace, void* d_quadric_workspace, const float* d_verts, int64_t num_vertices,
                                  const int32_t* d_faces, int64_t num_faces, const float* d_normals, float origin_x,
                                  float origin_y, float origin_z, float cell, int64_t vertices_kept, int64_t faces_kept,
                                  float* d_out_verts, int32_t* d_out_faces, float* d_out_normals, int64_t* h_counts,
                                  void* stream) {
    if (require_mesh("mesh simplify", num_vertices, num_faces)) return 2;
    MS_REQUIRE_GRID(origin_x, origin_y, origin_z, cell);
    NM_REQUIRE_COMPACT_OUTPUTS("mesh simplify",
                               d_workspace && d_quadric_workspace && h_counts && (num_vertices == 0 || d_verts) &&
                                   (num_faces == 0 || d_faces),
                               d_out_verts && (!d_normals || d_out_normals));
    const MsWorkspace w = ms_carve(d_workspace, num_vertices, num_faces);
    const MsQuadricWorkspace q = msq_carve(d_quadric_workspace, num_vertices);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nv = (int)num_vertices;
    const MsGrid g{{origin_x, origin_y, origin_z}, cell};
    NM_HIP_CHECK(hipMemsetAsync(q.hdr, 0, offsetof(MsQuadricHeader, far), s));   // the four counts of this call; far is the face pass's
    if (vertices_kept) {
        hipLaunchKernelGGL(ms_emit_vertices<true>, dim3(launch_grid(num_vertices)), dim3(256), 0, s, d_verts, d_normals, nv, g,
                           w.table, (const MsQuadric*)q.quad, w.slot_of, w.bits.vwords, w.bits.vprefix, vertices_kept, d_out_verts,
                           d_out_normals, q.hdr);
        NM_HIP_CHECK(hipGetLastError());
    }
    if (const int rc = subset_compact_faces(d_faces, num_faces, nv, faces_kept, w.bits, w.rep, d_out_faces, nullptr, s)) return rc;
    MsQuadricHeader h;
    NM_HIP_CHECK(hipMemcpyAsync(&h, q.hdr, sizeof(MsQuadricHeader), hipMemcpyDeviceToHost, s));
    NM_HIP_CHECK(hipStreamSynchronize(s));
    h_counts[NM_MESH_SIMPLIFY_QUADRIC_SOLVED] = (int64_t)h.solved;
    h_counts[NM_MESH_SIMPLIFY_QUADRIC_CROWDED] = (int64_t)h.crowded;
    h_counts[NM_MESH_SIMPLIFY_QUADRIC_SINGULAR] = (int64_t)h.singular;
    h_counts[NM_MESH_SIMPLIFY_QUADRIC_CLAMPED] = (int64_t)h.clamped;
    h_counts[NM_MESH_SIMPLIFY_QUADRIC_FAR] = (int64_t)h.far;
    return 0;
}

int64_t nm_mesh_simplify_adaptive_workspace_bytes(int64_t num_vertices, int64_t num_faces) {
    if (!mesh_size_ok(num_vertices) || !mesh_size_ok(num_faces)) return 0;
    return msa_carve(nullptr, num_vertices).bytes;
}

#define MSA_REQUIRE_LEVELS(levels)                                                                                        \
    NM_REQUIRE(levels >= 1 && levels <= NM_MESH_SIMPLIFY_MAX_LEVELS, "mesh simplify: levels must be in [1, 8]")

int nm_mesh_simplify_adaptive_level(const float* d_verts, int64_t num_vertices, const int32_t* d_faces, int64_t num_faces,
                                    const float* d_normals, float origin_x, float origin_y, float origin_z, float cell,
                                    int32_t level, int32_t levels, double max_error, int32_t flags, void* d_workspace,
                                    void* d_quadric_workspace, void* d_adaptive_workspace, void* stream) {
    if (require_mesh("mesh simplify", num_vertices, num_faces)) return 2;
    MS_REQUIRE_GRID(origin_x, origin_y, origin_z, cell);
    MSA_REQUIRE_LEVELS(levels);
    NM_REQUIRE(level >= 0 && level <= levels, "mesh simplify: the level must be in [0, levels]");
    const float cell_l = ldexpf(cell, level);                        // exact: a power of two
    NM_REQUIRE(ms_finite(cell_l), "mesh simplify: the coarsest cell size must be finite");
    NM_REQUIRE(max_error >= 0.0, "mesh simplify: the error bound must be >= 0");                  // a NaN fails
    NM_REQUIRE((flags & ~(NM_MESH_SIMPLIFY_AGGREGATE | NM_MESH_SIMPLIFY_AGGREGATE_FACES)) == 0, "mesh simplify: unknown flags");
    NM_REQUIRE(d_workspace && d_quadric_workspace && d_adaptive_workspace && (num_vertices == 0 || d_verts) &&
                   (num_faces == 0 || d_faces), "bad argument");
    const MsWorkspace w = ms_carve(d_workspace, num_vertices, num_faces);
    const MsQuadricWorkspace q = msq_carve(d_quadric_workspace, num_vertices);
    const MsaWorkspace a = msa_carve(d_adaptive_workspace, num_vertices);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nv = (int)num_vertices;
    const MsGrid g{{origin_x, origin_y, origin_z}, cell_l};
    const unsigned vgrid = launch_grid(num_vertices), fgrid = launch_grid(num_faces);
    // tol_l in lattice units of this level's cell, squared: four fp64 operations in this order
    const double cell64 = (double)cell_l;
    const double in_cells = max_error / cell64;
    const double tol = in_cells * MSQ_LATTICE;
    const double tol2 = tol * tol;
    if (level == levels) {                                           // the first level of a run: nothing is assigned yet
        NM_HIP_CHECK(hipMemsetAsync(a.hdr, 0, sizeof(MsaHeader), s));
        if (nv) NM_HIP_CHECK(hipMemsetAsync(a.stage.level, 0xff, (size_t)nv, s));
    }
    // the face table and the keep words are the final faces' (nm_mesh_simplify_adaptive_faces): only level 0 clears them
    const uint64_t fcap = level == 0 ? w.fcap : 0;
    const int64_t nvw = level == 0 ? w.bits.nvw : 0;
    const uint64_t most = w.cap > fcap ? w.cap : fcap;
    hipLaunchKernelGGL(ms_init, dim3((unsigned)(most / 256 > 4096 ? 4096 : most / 256 ? most / 256 : 1)), dim3(256), 0, s, w.table,
                       w.cap, w.ftab, fcap, w.bits.vwords, nvw, w.hdr);
    NM_HIP_CHECK(hipGetLastError());
    NM_HIP_CHECK(hipMemsetAsync(d_quadric_workspace, 0, (size_t)q.bytes, s));
    if (!nv) return 0;
    if (flags & NM_MESH_SIMPLIFY_AGGREGATE)
        hipLaunchKernelGGL(ms_insert<true>, dim3(vgrid), dim3(256), 0, s, d_verts, d_normals, nv, g, w.table, w.cap, w.slot_of,
                           w.rep, w.hdr);
    else
        hipLaunchKernelGGL(ms_insert<false>, dim3(vgrid), dim3(256), 0, s, d_verts, d_normals, nv, g, w.table, w.cap, w.slot_of,
                           w.rep, w.hdr);
    NM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ms_representatives, dim3(vgrid), dim3(256), 0, s, w.table, w.slot_of, w.rep, nv, w.hdr);
    NM_HIP_CHECK(hipGetLastError());
    const bool aggregate = flags & NM_MESH_SIMPLIFY_AGGREGATE_FACES;
    if (num_faces) {
        if (aggregate)
            hipLaunchKernelGGL(ms_quadric_faces<true>, dim3(fgrid), dim3(256), 0, s, d_verts, d_faces, num_faces, nv, g, w.slot_of,
                               w.rep, q.cap, q.quad, q.hdr);
        else
            hipLaunchKernelGGL(ms_quadric_faces<false>, dim3(fgrid), dim3(256), 0, s, d_verts, d_faces, num_faces, nv, g, w.slot_of,
                               w.rep, q.cap, q.quad, q.hdr);
        NM_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(msa_place, dim3((unsigned)(w.cap / 256 ? w.cap / 256 : 1)), dim3(256), 0, s, (const MsSlot*)w.table, w.cap,
                       q.quad);
    NM_HIP_CHECK(hipGetLastError());
    if (num_faces && level > 0) {
        if (aggregate)
            hipLaunchKernelGGL(msa_error<true>, dim3(fgrid), dim3(256), 0, s, d_verts, d_faces, num_faces, nv, g, w.slot_of, w.rep,
                               q.cap, q.quad);
        else
            hipLaunchKernelGGL(msa_error<false>, dim3(fgrid), dim3(256), 0, s, d_verts, d_faces, num_faces, nv, g, w.slot_of, w.rep,
                               q.cap, q.quad);
        NM_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(msa_assign, dim3(vgrid), dim3(256), 0, s, d_verts, d_normals, nv, g, (int)level, tol2,
                       (const MsSlot*)w.table, (const MsQuadric*)q.quad, w.slot_of, (const int*)w.rep, a.stage, a.hdr);
    NM_HIP_CHECK(hipGetLastError());
    if (level == 0)
        NM_HIP_CHECK(hipMemcpyAsync(&a.hdr->far, &q.hdr->far, sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
    return 0;
}

int nm_mesh_simplify_adaptive_faces(const int32_t* d_faces, int64_t num_faces, int64_t num_vertices, int32_t levels,
                                    void* d_workspace, void* d_adaptive_workspace, int64_t* h_counts, void* stream) {
    if (require_mesh("mesh simplify", num_vertices, num_faces)) return 2;
    MSA_REQUIRE_LEVELS(levels);
    NM_REQUIRE(d_workspace && d_adaptive_workspace && h_counts && (num_faces == 0 || d_faces), "bad argument");
    const MsWorkspace w = ms_carve(d_workspace, num_vertices, num_faces);
    const MsaWorkspace a = msa_carve(d_adaptive_workspace, num_vertices);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nv = (int)num_vertices;
    const unsigned fgrid = launch_grid(num_faces);
    if (num_faces) {
        hipLaunchKernelGGL(ms_insert_faces, dim3(fgrid), dim3(256), 0, s, d_faces, num_faces, nv, (const int*)a.stage.rep, w.ftab,
                           w.fcap, w.fslot);
        NM_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(ms_mark, dim3(fgrid), dim3(256), 0, s, d_faces, num_faces, nv, (const int*)a.stage.rep,
                           (const int*)w.ftab, (const uint32_t*)w.fslot, w.bits.fwords, w.bits.vwords, w.hdr);
        NM_HIP_CHECK(hipGetLastError());
    }
    if (const int rc = subset_scan(w.bits, w.hdr->totals, s)) return rc;
    MsHeader h;
    MsaHeader ah;
    NM_HIP_CHECK(hipMemcpyAsync(&h, w.hdr, sizeof(MsHeader), hipMemcpyDeviceToHost, s));
    NM_HIP_CHECK(hipMemcpyAsync(&ah, a.hdr, sizeof(MsaHeader), hipMemcpyDeviceToHost, s));
    NM_HIP_CHECK(hipStreamSynchronize(s));
    unsigned long long clusters = 0;
    for (int l = 0; l <= levels; ++l) {
        clusters += ah.level[l][MSA_CLUSTERS];
        for (int k = 0; k < MSA_LEVEL_FIELDS; ++k)
            h_counts[NM_MESH_SIMPLIFY_COUNTS + l * NM_MESH_SIMPLIFY_LEVEL_FIELDS + k] = (int64_t)ah.level[l][k];
    }
    h_counts[NM_MESH_SIMPLIFY_CLUSTERS] = (int64_t)clusters;
    h_counts[NM_MESH_SIMPLIFY_VERTICES_KEPT] = (int64_t)h.totals[0];
    h_counts[NM_MESH_SIMPLIFY_FACES_KEPT] = (int64_t)h.totals[1];
    h_counts[NM_MESH_SIMPLIFY_DEGENERATE] = (int64_t)h.degenerate;
    h_counts[NM_MESH_SIMPLIFY_DUPLICATE] = (int64_t)h.duplicate;
    h_counts[NM_MESH_SIMPLIFY_BAD_VERTICES] = (int64_t)h.bad_vertices;
    h_counts[NM_MESH_SIMPLIFY_BAD_FACES] = (int64_t)h.bad_faces;
    return 0;
}

int nm_mesh_simplify_adaptive_emit(const void* d_workspace, void* d_adaptive_workspace, const int32_t* d_faces, int64_t num_faces,
                                   int64_t num_vertices, int32_t levels, int32_t with_normals, int64_t vertices_kept,
                                   int64_t faces_kept, float* d_out_verts, int32_t* d_out_faces, float* d_out_normals,
                                   int64_t* h_counts, void* stream) {
    if (require_mesh("mesh simplify", num_vertices, num_faces)) return 2;
    MSA_REQUIRE_LEVELS(levels);
    NM_REQUIRE_COMPACT_OUTPUTS("mesh simplify", d_workspace && d_adaptive_workspace && h_counts && (num_faces == 0 || d_faces),
                               d_out_verts && (!with_normals || d_out_normals));
    const MsWorkspace w = ms_carve(d_workspace, num_vertices, num_faces);
    const MsaWorkspace a = msa_carve(d_adaptive_workspace, num_vertices);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nv = (int)num_vertices;
    NM_HIP_CHECK(hipMemsetAsync(a.hdr->kept, 0, sizeof(a.hdr->kept) + sizeof(a.hdr->status), s));   // the counts of this call
    if (vertices_kept) {
        hipLaunchKernelGGL(msa_emit, dim3(launch_grid(num_vertices)), dim3(256), 0, s, nv, (int)levels, a.stage, with_normals != 0,
                           (const unsigned long long*)w.bits.vwords, (const uint32_t*)w.bits.vprefix, vertices_kept, d_out_verts,
                           d_out_normals, a.hdr);
        NM_HIP_CHECK(hipGetLastError());
    }
    if (const int rc = subset_compact_faces(d_faces, num_faces, nv, faces_kept, w.bits, a.stage.rep, d_out_faces, nullptr, s))
        return rc;
    MsaHeader ah;
    NM_HIP_CHECK(hipMemcpyAsync(&ah, a.hdr, sizeof(MsaHeader), hipMemcpyDeviceToHost, s));
    NM_HIP_CHECK(hipStreamSynchronize(s));
    for (int k = 0; k < 4; ++k) h_counts[k] = (int64_t)ah.status[k];
    h_counts[NM_MESH_SIMPLIFY_QUADRIC_FAR] = (int64_t)ah.far;
    for (int l = 0; l <= levels; ++l) h_counts[NM_MESH_SIMPLIFY_QUADRIC_COUNTS + l] = (int64_t)ah.kept[l];
    return 0;
}

}  // extern "C"
