// Software rasteriser of an indexed triangle mesh (mesh_render, mesh_nerf --render-views; DESIGN.md, "Mesh render"): which face
// a pinhole camera sees at every pixel, at what depth, with which barycentrics.  Coverage is exact integer work and visibility
// is a 64-bit minimum, so the output bytes do not depend on the order the workgroups ran in or on which path drew a face, and
// a numpy restatement (tests/mesh_raster.py) reproduces them bit for bit.  Every fp32 / fp64 operation below is rounded on its
// own (-ffp-contract=off), division correctly rounded.  THE RULE (also in include/nerfmeshes_hip.h and tests/mesh_raster.py):
//   vertex    in fp64, with R = c2w[:3,:3], t = c2w[:3,3]:  d = (double) p - (double) t;  xc = (R00 dx + R10 dy) + R20 dz, yc and
//             zc with columns 1 and 2;  w = (float)(-zc);  u = (xc / (double) w) focal + width 0.5;  v = -(yc / (double) w) focal
//             + height 0.5;  X = rint(u 256), Y = rint(v 256): 8 sub-pixel bits.  Pixel (row j, column i) is sampled at
//             (X, Y) = (256 i, 256 j): get_ray_bundle's convention, no half-pixel offset; w is the distance along the camera's
//             axis (the NeRF's depth_map, measured along the unit ray, is w times the pixel's |(x, y, -1)|).
//             A vertex is NOT FINITE when a coordinate or w is not finite, OUT OF RANGE when not |u 256| <= 2^24 or not
//             |v 256| <= 2^24 (every edge function then stays below 2^51).
//   face      rejected, and counted under the FIRST reason that holds: an index outside [0, V) (never dereferenced); a corner
//             not finite; a corner with w < near (there is no near-plane clipping); a corner out of range; back-facing
//             (A > 0: clockwise on the screen, whose Y points down) under NM_MESH_RASTER_CULL_BACK; no pixel centre inside the
//             bounding box clipped to the screen; A == 0.  A = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0), int64.
//   coverage  e0 = (X2 - X1)(Py - Y1) - (Y2 - Y1)(Px - X1), e1 and e2 with the corners rotated, int64; for A < 0 every e, every
//             edge vector and A change sign, which is the face with two corners swapped and the barycentrics kept in the
//             face's own corner order.  A pixel is inside when every e > 0, or e == 0 on a top or left edge (edge vector
//             (dx, dy): dy < 0, or dy == 0 and dx > 0): a sheet of triangles covers every pixel exactly once.
//   depth     lk = (double) ek / (double) A;  ik = 1.0 / (double) wk;  q = (l0 i0 + l1 i1) + l2 i2;  depth = (float)(1.0 / q);
//             bk = (float)((lk ik) / q).  A pixel whose depth is not finite or not > 0 is not covered.
//   winner    the minimum over the covering faces of (bits of depth) << 32 | face index: the nearest, an exact tie to the
//             smallest index.
// Kernels: mr_vertices (one thread per vertex -> X, Y, w in the workspace), mr_faces (one lane per face: rejects, counts and the
// walk over a small bounding box; a face whose clipped box holds more than large_threshold pixel centres goes to a queue by a
// wave-aggregated append), mr_large (a fixed grid whose waves claim queue entries from a device counter, 64 lanes striding
// over the box), mr_resolve (one thread per pixel: the winner's barycentrics recomputed, the three outputs, the covered count
// by ballot).  A pixel's word is read before it is written and the atomicMin issued only where the word read is above the
// lane's own: the words only ever fall, so a stale read costs an atomic and never changes the result.  Nothing allocates and
// nothing synchronises with the host: both entries can be captured into a graph.
//
// Hidden faces (mesh_nerf --cull-hidden-views; DESIGN.md, "Hidden faces"; the rule in include/nerfmeshes_hip.h, restated in
// tests/mesh_visibility.py): nm_mesh_visibility_views runs the three passes above per view, without mr_resolve, and
// mv_mark_pixels (one thread per pixel) raises the seen bit of every pixel's winner; _select grows the seen set `rings` times
// over shared vertices (mv_mark_corners: the corners of the kept faces; mv_grow: the faces with a marked corner, one ballot word
// per wave) and takes the prefix sums of compact.h (subset_scan); _compact writes the kept rows in their order (subset_compact_*).  The bits only rise, as the
// pixels' words only fall: a bit read as set costs no atomic, exactly one atomic per bit finds it clear, and that one is
// counted -- new_faces[k] does not depend on the order of the workgroups because the views run in stream order.
#include "compact.h"
#include "nm_internal.h"

namespace nm {

constexpr int MR_MAX_SIDE = 16384;               // image sides in [1, 2^14]: 256 * side stays below 2^23
constexpr double MR_RANGE = 16777216.0;          // 2^24
constexpr int MR_OUT_OF_RANGE = INT32_MIN;       // MrVertex::x of a vertex that is out of range
constexpr unsigned long long MR_EMPTY = ~0ull;
constexpr unsigned MR_LARGE_GRID = 1024;         // workgroups of mr_large: 4 per CU, 4 waves each

struct MrVertex { int32_t x, y; float w; };      // w is a NaN: not finite
struct MrHeader { unsigned queued, claimed; unsigned pad[62]; };
static_assert(sizeof(MrVertex) == 12 && sizeof(MrHeader) == 256, "workspace layout");

struct MrCamera {
    double rot[9], origin[3];                    // (double) of the fp32 pose
    double focal, half_w, half_h;
    int32_t height, width;
};

__global__ __launch_bounds__(256) void mr_vertices(const float* __restrict__ verts, int nv, const MrCamera cam,
                                                   MrVertex* __restrict__ out) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const float px = verts[3 * v], py = verts[3 * v + 1], pz = verts[3 * v + 2];
    const double dx = (double)px - cam.origin[0], dy = (double)py - cam.origin[1], dz = (double)pz - cam.origin[2];
    const double xa = cam.rot[0] * dx, xb = cam.rot[3] * dy, xd = cam.rot[6] * dz;
    const double ya = cam.rot[1] * dx, yb = cam.rot[4] * dy, yd = cam.rot[7] * dz;
    const double za = cam.rot[2] * dx, zb = cam.rot[5] * dy, zd = cam.rot[8] * dz;
    const double xc = (xa + xb) + xd, yc = (ya + yb) + yd, zc = (za + zb) + zd;
    const float w = (float)(-zc);
    MrVertex r;
    const bool finite = is_finite(px) && is_finite(py) && is_finite(pz) && is_finite(w);
    r.w = finite ? w : __uint_as_float(0x7fc00000u);
    const double wd = (double)w;
    const double ux = (xc / wd) * cam.focal, uy = -(yc / wd) * cam.focal;
    const double sx = (ux + cam.half_w) * 256.0, sy = (uy + cam.half_h) * 256.0;
    const bool in_range = fabs(sx) <= MR_RANGE && fabs(sy) <= MR_RANGE;          // a NaN fails both
    r.x = in_range ? (int32_t)rint(sx) : MR_OUT_OF_RANGE;
    r.y = in_range ? (int32_t)rint(sy) : 0;
    out[v] = r;
}

// A face that passed every reject: the edge vectors and the edge functions' values at pixel (0, 0), signs normalised to A > 0
struct MrSetup {
    long long a;                                 // the doubled area, > 0
    long long ex[3], ey[3], e0[3];               // ek(i, j) = e0[k] + 256 (ex[k] j - ey[k] i);  (ex, ey) is edge k's vector
    int bias[3];                                 // 0 on a top or left edge, else 1: inside is ek >= bias
    double iw[3];                                // 1 / w of the three corners
    int imin, imax, jmin, jmax;                  // the pixel centres in the bounding box, clipped to the screen
};

enum { MR_DRAW = 0, MR_BAD_INDEX, MR_NOT_FINITE, MR_NEAR, MR_RANGE_REJECT, MR_CULLED, MR_OFF_SCREEN, MR_DEGENERATE };

// the reason face f is rejected under, or MR_DRAW with `s` filled in
__device__ __forceinline__ int mr_setup(const int32_t* __restrict__ faces, int64_t f, int nv, const MrVertex* __restrict__ vtx,
                                        float near, int cull_back, int height, int width, MrSetup& s) {
    int c[3];
    if (!load_face(faces, f, nv, c)) return MR_BAD_INDEX;
    MrVertex p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = vtx[c[k]];
    if (!is_finite(p[0].w) || !is_finite(p[1].w) || !is_finite(p[2].w)) return MR_NOT_FINITE;
    if (p[0].w < near || p[1].w < near || p[2].w < near) return MR_NEAR;
    if (p[0].x == MR_OUT_OF_RANGE || p[1].x == MR_OUT_OF_RANGE || p[2].x == MR_OUT_OF_RANGE) return MR_RANGE_REJECT;
    const long long x0 = p[0].x, y0 = p[0].y, x1 = p[1].x, y1 = p[1].y, x2 = p[2].x, y2 = p[2].y;
    const long long area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0);
    if (cull_back && area > 0) return MR_CULLED;
    const long long xlo = min(x0, min(x1, x2)), xhi = max(x0, max(x1, x2));
    const long long ylo = min(y0, min(y1, y2)), yhi = max(y0, max(y1, y2));
    const long long ilo = max((xlo + 255) >> 8, 0ll), ihi = min(xhi >> 8, (long long)width - 1);
    const long long jlo = max((ylo + 255) >> 8, 0ll), jhi = min(yhi >> 8, (long long)height - 1);
    if (ilo > ihi || jlo > jhi) return MR_OFF_SCREEN;
    if (area == 0) return MR_DEGENERATE;
    const long long sign = area < 0 ? -1 : 1;
    s.a = sign * area;
    const long long vx[3] = {x1, x2, x0}, vy[3] = {y1, y2, y0}, nx[3] = {x2, x0, x1}, ny[3] = {y2, y0, y1};
#pragma unroll
    for (int k = 0; k < 3; ++k) {                // edge k runs from corner k + 1 to corner k + 2: the one opposite corner k
        s.ex[k] = sign * (nx[k] - vx[k]);
        s.ey[k] = sign * (ny[k] - vy[k]);
        s.e0[k] = s.ey[k] * vx[k] - s.ex[k] * vy[k];
        s.bias[k] = (s.ey[k] < 0 || (s.ey[k] == 0 && s.ex[k] > 0)) ? 0 : 1;
        s.iw[k] = 1.0 / (double)p[k].w;
    }
    s.imin = (int)ilo; s.imax = (int)ihi; s.jmin = (int)jlo; s.jmax = (int)jhi;
    return MR_DRAW;
}

// pixel (row j, column i) against a face: covered -> its depth and barycentrics
__device__ __forceinline__ bool mr_pixel(const MrSetup& s, int i, int j, float& depth, float (&bary)[3]) {
    long long e[3];
    bool inside = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e[k] = s.e0[k] + 256 * (s.ex[k] * j - s.ey[k] * i);
        inside = inside && e[k] >= s.bias[k];
    }
    if (!inside) return false;
    const double area = (double)s.a;
    double t[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double l = (double)e[k] / area;
        t[k] = l * s.iw[k];
    }
    const double q = (t[0] + t[1]) + t[2];
    depth = (float)(1.0 / q);
#pragma unroll
    for (int k = 0; k < 3; ++k) bary[k] = (float)(t[k] / q);
    return is_finite(depth) && depth > 0.0f;
}

__device__ __forceinline__ void mr_write(unsigned long long* zbuf, int64_t pixel, float depth, int64_t f) {
    const unsigned long long word = ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned long long)f;
    if (__hip_atomic_load(zbuf + pixel, NM_RELAXED_AGENT) > word) __hip_atomic_fetch_min(zbuf + pixel, word, NM_RELAXED_AGENT);
}

// a whole wave's covered (face, pixel) pairs in one integer atomic
__device__ __forceinline__ void mr_count_fragments(unsigned long long fragments, int lane, unsigned long long* counts) {
#pragma unroll
    for (int off = 32; off; off >>= 1) fragments += __shfl_xor(fragments, off, 64);
    if (lane == 0 && fragments) atomicAdd(counts + NM_MESH_RASTER_FRAGMENTS, fragments);
}

// one lane per face, whole waves (the votes)
__global__ __launch_bounds__(256) void mr_faces(const int32_t* __restrict__ faces, int64_t nf, int nv,
                                                const MrVertex* __restrict__ vtx, float near, int cull_back, int height, int width,
                                                long long large_threshold, unsigned long long* zbuf, int32_t* __restrict__ queue,
                                                MrHeader* hdr, unsigned long long* counts) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    MrSetup s;
    int reason = -1;
    if (f < nf) reason = mr_setup(faces, f, nv, vtx, near, cull_back, height, width, s);
    bool large = false;
    if (reason == MR_DRAW)
        large = (long long)(s.imax - s.imin + 1) * (long long)(s.jmax - s.jmin + 1) > large_threshold;
    const unsigned long long larges = __ballot(large);
    if (larges) {                                // one atomic per wave; the order inside the queue does not matter
        unsigned base = 0;
        const int leader = __ffsll((long long)larges) - 1;
        if (lane == leader) base = __hip_atomic_fetch_add(&hdr->queued, (unsigned)__popcll(larges), NM_RELAXED_AGENT);
        base = __shfl(base, leader, 64);
        if (large) queue[base + __popcll(larges & ((1ull << lane) - 1ull))] = (int32_t)f;     // at most nf entries: one per face
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const unsigned long long votes = __ballot(reason == r);
        if (lane == 0 && votes) atomicAdd(counts + r, (unsigned long long)__popcll(votes));
    }
    if (lane == 0 && larges) atomicAdd(counts + NM_MESH_RASTER_LARGE, (unsigned long long)__popcll(larges));
    unsigned long long fragments = 0;
    if (reason == MR_DRAW && !large)
        for (int j = s.jmin; j <= s.jmax; ++j)
            for (int i = s.imin; i <= s.imax; ++i) {
                float depth, bary[3];
                if (mr_pixel(s, i, j, depth, bary)) {
                    mr_write(zbuf, (int64_t)j * width + i, depth, f);
                    ++fragments;
                }
            }
    mr_count_fragments(fragments, lane, counts);
}

// one wave per queued face; the waves claim entries from hdr->claimed until the queue is empty
__global__ __launch_bounds__(256) void mr_large(const int32_t* __restrict__ faces, int nv, const MrVertex* __restrict__ vtx,
                                                float near, int cull_back, int height, int width, unsigned long long* zbuf,
                                                const int32_t* __restrict__ queue, MrHeader* hdr, unsigned long long* counts) {
    const int lane = threadIdx.x & 63;
    unsigned long long fragments = 0;
    const unsigned queued = hdr->queued;         // written by the launch in front
    // a wave beyond the queue's length has nothing to wait for: an empty queue costs the launch and not one atomic
    if (((unsigned)blockIdx.x * 256u + threadIdx.x) / 64u >= queued) return;
    for (;;) {
        unsigned at = 0;
        if (lane == 0) at = __hip_atomic_fetch_add(&hdr->claimed, 1u, NM_RELAXED_AGENT);
        at = __shfl(at, 0, 64);
        if (at >= queued) break;
        const int64_t f = queue[at];
        MrSetup s;
        if (mr_setup(faces, f, nv, vtx, near, cull_back, height, width, s) != MR_DRAW) continue;   // never: it was drawn when queued
        const int64_t bw = s.imax - s.imin + 1, pixels = bw * (int64_t)(s.jmax - s.jmin + 1);
        for (int64_t p = lane; p < pixels; p += 64) {
            const int j = s.jmin + (int)(p / bw), i = s.imin + (int)(p % bw);
            float depth, bary[3];
            if (mr_pixel(s, i, j, depth, bary)) {
                mr_write(zbuf, (int64_t)j * width + i, depth, f);
                ++fragments;
            }
        }
    }
    mr_count_fragments(fragments, lane, counts);                                 // the whole wave left the loop together
}

// one thread per pixel, whole waves (the vote)
__global__ __launch_bounds__(256) void mr_resolve(const int32_t* __restrict__ faces, int64_t nf, int nv,
                                                  const MrVertex* __restrict__ vtx, float near, int cull_back, int height, int width,
                                                  const unsigned long long* __restrict__ zbuf, int32_t* __restrict__ face_id,
                                                  float* __restrict__ depth_out, float* __restrict__ bary_out,
                                                  unsigned long long* counts) {
    const int64_t pixel = (int64_t)blockIdx.x * 256 + threadIdx.x, pixels = (int64_t)height * width;
    bool covered = false;
    if (pixel < pixels) {
        const unsigned long long word = zbuf[pixel];
        int32_t id = -1;
        float depth = 0.0f, bary[3] = {0.0f, 0.0f, 0.0f};
        const int64_t f = (int64_t)(word & 0xffffffffull);
        MrSetup s;
        if (word != MR_EMPTY && f < nf && mr_setup(faces, f, nv, vtx, near, cull_back, height, width, s) == MR_DRAW &&
            mr_pixel(s, (int)(pixel % width), (int)(pixel / width), depth, bary)) {
            id = (int32_t)f;
            covered = true;
        } else {
            depth = bary[0] = bary[1] = bary[2] = 0.0f;
        }
        face_id[pixel] = id;
        depth_out[pixel] = depth;
#pragma unroll
        for (int k = 0; k < 3; ++k) bary_out[3 * pixel + k] = bary[k];
    }
    const unsigned long long votes = __ballot(covered);
    if ((threadIdx.x & 63) == 0 && votes) atomicAdd(counts + NM_MESH_RASTER_COVERED, (unsigned long long)__popcll(votes));
}

// out = (b0 a0 + b1 a1) + b2 a2 per channel; the background row where nothing was drawn (or the face is not one of the mesh)
__global__ __launch_bounds__(256) void mr_interpolate(const int32_t* __restrict__ face_id, const float* __restrict__ bary,
                                                      int64_t pixels, const int32_t* __restrict__ faces, int64_t nf,
                                                      const float* __restrict__ attr, int nv, int channels,
                                                      const float* __restrict__ background, float* __restrict__ out) {
    const int64_t pixel = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pixel >= pixels) return;
    const int64_t f = face_id[pixel];
    int c[3];
    if (f < 0 || f >= nf || !load_face(faces, f, nv, c)) {
        for (int k = 0; k < channels; ++k) out[pixel * channels + k] = background[k];
        return;
    }
    const float b0 = bary[3 * pixel], b1 = bary[3 * pixel + 1], b2 = bary[3 * pixel + 2];
    for (int k = 0; k < channels; ++k) {
        const float t0 = b0 * attr[(int64_t)c[0] * channels + k], t1 = b1 * attr[(int64_t)c[1] * channels + k];
        const float t2 = b2 * attr[(int64_t)c[2] * channels + k];
        out[pixel * channels + k] = (t0 + t1) + t2;
    }
}

// ---- hidden faces (nm_mesh_visibility_*) ------------------------------------------------------
struct MvHeader {
    unsigned long long bad_faces;      // faces with a vertex index outside [0, nv): never dereferenced, never kept
    unsigned long long faces_seen;     // set bits of the seen words
    unsigned long long totals[2];      // vertices kept, faces kept
    unsigned long long pad[4];
    unsigned long long counts[24];     // where a view's raster counts go when the caller does not want them
};
static_assert(sizeof(MvHeader) == 256 && NM_MESH_RASTER_COUNTS <= 24, "workspace layout");

__device__ __forceinline__ bool mv_raise(unsigned long long* words, int64_t i) {
    // sets bit i -> true when THIS call found it clear.  Bits only rise: a bit read as set stays set and costs no atomic; a stale
    // read of a clear bit costs the atomic, whose answer is the truth -- exactly one caller per bit gets `true`.
    const unsigned long long bit = 1ull << (i & 63);
    if (__hip_atomic_load(words + (i >> 6), NM_RELAXED_AGENT) & bit) return false;
    return !(__hip_atomic_fetch_or(words + (i >> 6), bit, NM_RELAXED_AGENT) & bit);
}

// one thread per pixel, whole waves (the votes): the winner's seen bit, the faces this view saw first, the covered pixels
__global__ __launch_bounds__(256) void mv_mark_pixels(const unsigned long long* __restrict__ zbuf, int64_t pixels, int64_t nf,
                                                      unsigned long long* seen, unsigned long long* new_faces,
                                                      unsigned long long* counts) {
    const int64_t pixel = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const unsigned long long word = pixel < pixels ? zbuf[pixel] : MR_EMPTY;
    const bool covered = word != MR_EMPTY && (int64_t)(word & 0xffffffffull) < nf;
    const int f = covered ? (int)(word & 0xffffffffull) : -1;
    const int left = __shfl_up(f, 1, 64);                            // a run of pixels on one face: its first lane speaks for it
    const bool first = covered && !(lane > 0 && left == f) && mv_raise(seen, f);
    const unsigned long long firsts = __ballot(first), votes = __ballot(covered);
    if (lane == 0 && firsts) atomicAdd(new_faces, (unsigned long long)__popcll(firsts));
    if (lane == 0 && votes) atomicAdd(counts + NM_MESH_RASTER_COVERED, (unsigned long long)__popcll(votes));
}

// kept = seen (a face with a bad index is never drawn, so never seen); the header's two counts
__global__ __launch_bounds__(256) void mv_begin(const int32_t* __restrict__ faces, int64_t nf, int nv,
                                                const unsigned long long* __restrict__ seen, unsigned long long* __restrict__ fwords,
                                                MvHeader* hdr) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int v[3];
    const bool valid = f < nf && load_face(faces, f, nv, v);
    const bool keep = valid && bit_test(seen, f);
    const unsigned long long word = store_keep_word(fwords, f, nf, keep), bad = __ballot(f < nf && !valid);
    if ((threadIdx.x & 63) == 0) {                                   // a wave beyond the last word has no face to count
        if (word) atomicAdd(&hdr->faces_seen, (unsigned long long)__popcll(word));
        if (bad) atomicAdd(&hdr->bad_faces, (unsigned long long)__popcll(bad));
    }
}

// the vertex bit of every corner of every kept face
__global__ __launch_bounds__(256) void mv_mark_corners(const int32_t* __restrict__ faces, int64_t nf, int nv,
                                                       const unsigned long long* __restrict__ fwords, unsigned long long* vwords) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int v[3];
    if (f >= nf || !bit_test(fwords, f) || !load_face(faces, f, nv, v)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) mv_raise(vwords, v[k]);
}

// a face with valid indices and a marked corner becomes kept; the vertex bits are the launch in front's, complete
__global__ __launch_bounds__(256) void mv_grow(const int32_t* __restrict__ faces, int64_t nf, int nv,
                                               const unsigned long long* __restrict__ vwords, unsigned long long* __restrict__ fwords) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int v[3];
    store_keep_word(fwords, f, nf,
                    f < nf && load_face(faces, f, nv, v) && (bit_test(vwords, v[0]) || bit_test(vwords, v[1]) || bit_test(vwords, v[2])));
}

struct MrWorkspace {
    unsigned long long* zbuf;
    MrHeader* hdr;
    MrVertex* vtx;
    int32_t* queue;
    int64_t bytes;
};

static MrWorkspace mr_carve(const void* ws, int64_t nv, int64_t nf, int64_t height, int64_t width) {
    Carver c(ws, 256);
    MrWorkspace w;
    w.zbuf = c.take<unsigned long long>(height * width);
    w.hdr = c.take<MrHeader>(1);
    w.vtx = c.take<MrVertex>(nv);
    w.queue = c.take<int32_t>(nf);
    w.bytes = c.offset;
    return w;
}

// Everything whose size V and F decide comes first and the visibility words last: nm_mesh_visibility_select and _compact find
// their members without knowing the image sizes the workspace was made for.
struct MvWorkspace {
    MvHeader* hdr;
    unsigned long long* seen;
    SubsetBits bits;                             // the face pair in front
    MrWorkspace raster;
    int64_t bytes;
};

static MvWorkspace mv_carve(const void* ws, int64_t nv, int64_t nf, int64_t pixels) {
    Carver c(ws, 256);
    MvWorkspace w;
    w.hdr = c.take<MvHeader>(1);
    w.seen = c.take<unsigned long long>((nf + 63) / 64);
    w.bits = take_subset_bits(c, nv, nf, true);
    w.raster.hdr = c.take<MrHeader>(1);
    w.raster.vtx = c.take<MrVertex>(nv);
    w.raster.queue = c.take<int32_t>(nf);
    w.raster.zbuf = c.take<unsigned long long>(pixels);
    w.bytes = w.raster.bytes = c.offset;
    return w;
}

static bool mr_side_ok(int64_t n) { return n >= 1 && n <= MR_MAX_SIDE; }

// What nm_mesh_rasterize and the nm_mesh_visibility_* entries ask of a view, in one place: 0 or 2
static int mr_check_view(const nm_view* view) {
    NM_REQUIRE(view->use_ndc == 0, "mesh raster: an NDC view has no pinhole projection to rasterise with");
    NM_REQUIRE(mr_side_ok(view->height) && mr_side_ok(view->width), "mesh raster: height and width must be in [1, 16384]");
    NM_REQUIRE(view->focal > 0.0 && view->focal - view->focal == 0.0, "mesh raster: focal must be finite and > 0");
    return 0;
}

static int mr_check_limits(float near, int32_t large_threshold) {
    NM_REQUIRE(near > 0.0f && near - near == 0.0f, "mesh raster: near must be finite and > 0");        // a NaN fails the comparison
    NM_REQUIRE(large_threshold >= 0, "mesh raster: large_threshold must be >= 0");
    return 0;
}

// The passes both entries share: the words, the queue and the counts cleared, the vertex stage and the two face paths.  After
// it w.zbuf holds every pixel's winner and counts[] everything but NM_MESH_RASTER_COVERED.
static int mr_draw(const nm_view* view, const float* d_verts, int64_t num_vertices, const int32_t* d_faces, int64_t num_faces,
                   float near, int cull, int32_t large_threshold, const MrWorkspace& w, unsigned long long* counts, hipStream_t s) {
    const int height = view->height, width = view->width, nv = (int)num_vertices;
    MrCamera cam;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) cam.rot[3 * r + c] = (double)view->c2w[4 * r + c];
        cam.origin[r] = (double)view->c2w[4 * r + 3];
    }
    cam.focal = view->focal;
    cam.half_w = (double)width * 0.5;
    cam.half_h = (double)height * 0.5;
    cam.height = height;
    cam.width = width;
    NM_HIP_CHECK(hipMemsetAsync(w.zbuf, 0xff, sizeof(unsigned long long) * (size_t)height * (size_t)width, s));
    NM_HIP_CHECK(hipMemsetAsync(w.hdr, 0, sizeof(MrHeader), s));
    NM_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(int64_t) * NM_MESH_RASTER_COUNTS, s));
    if (num_faces) {
        hipLaunchKernelGGL(mr_vertices, dim3(launch_grid(num_vertices)), dim3(256), 0, s, d_verts, nv, cam, w.vtx);
        NM_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(mr_faces, dim3(launch_grid(num_faces)), dim3(256), 0, s, d_faces, num_faces, nv, w.vtx, near, cull, height,
                           width, (long long)large_threshold, w.zbuf, w.queue, w.hdr, counts);
        NM_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(mr_large, dim3(MR_LARGE_GRID), dim3(256), 0, s, d_faces, nv, w.vtx, near, cull, height, width, w.zbuf,
                           w.queue, w.hdr, counts);
        NM_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

}  // namespace nm

using namespace nm;

extern "C" {

int64_t nm_mesh_raster_workspace_bytes(int64_t num_vertices, int64_t num_faces, int32_t height, int32_t width) {
    if (!mesh_size_ok(num_vertices) || !mesh_size_ok(num_faces) || !mr_side_ok(height) || !mr_side_ok(width)) return 0;
    return mr_carve(nullptr, num_vertices, num_faces, height, width).bytes;
}

int nm_mesh_rasterize(const nm_view* view, const float* d_verts, int64_t num_vertices, const int32_t* d_faces, int64_t num_faces,
                      float near, int32_t flags, int32_t large_threshold, void* d_workspace, int32_t* d_face_id, float* d_depth,
                      float* d_bary, int64_t* d_counts, void* stream) {
    NM_REQUIRE(view != nullptr, "bad argument");
    if (mr_check_view(view) || require_mesh("mesh raster", num_vertices, num_faces) || mr_check_limits(near, large_threshold)) return 2;
    NM_REQUIRE((flags & ~NM_MESH_RASTER_CULL_BACK) == 0, "mesh raster: unknown flags");
    NM_REQUIRE(d_workspace && d_face_id && d_depth && d_bary && d_counts && (num_vertices == 0 || d_verts) &&
               (num_faces == 0 || d_faces), "bad argument");
    const int height = view->height, width = view->width;
    const int64_t pixels = (int64_t)height * width;
    const MrWorkspace w = mr_carve(d_workspace, num_vertices, num_faces, height, width);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int cull = flags & NM_MESH_RASTER_CULL_BACK;
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(d_counts);
    if (const int rc = mr_draw(view, d_verts, num_vertices, d_faces, num_faces, near, cull, large_threshold, w, counts, s)) return rc;
    hipLaunchKernelGGL(mr_resolve, dim3(launch_grid(pixels)), dim3(256), 0, s, d_faces, num_faces, (int)num_vertices, w.vtx, near, cull,
                       height, width, w.zbuf, d_face_id, d_depth, d_bary, counts);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

int64_t nm_mesh_visibility_workspace_bytes(int64_t num_vertices, int64_t num_faces, int32_t max_height, int32_t max_width) {
    if (!mesh_size_ok(num_vertices) || !mesh_size_ok(num_faces) || !mr_side_ok(max_height) || !mr_side_ok(max_width)) return 0;
    return mv_carve(nullptr, num_vertices, num_faces, (int64_t)max_height * max_width).bytes;
}

int nm_mesh_visibility_views(const nm_view* views, int64_t num_views, const float* d_verts, int64_t num_vertices,
                             const int32_t* d_faces, int64_t num_faces, float near, int32_t large_threshold, int32_t clear,
                             void* d_workspace, int64_t* d_new_faces, int64_t* d_reject_counts, void* stream) {
    NM_REQUIRE(num_views >= 0, "mesh visibility: num_views must be >= 0");
    NM_REQUIRE(num_views == 0 || (views && d_new_faces), "bad argument");
    for (int64_t k = 0; k < num_views; ++k)
        if (mr_check_view(views + k)) return 2;
    if (require_mesh("mesh raster", num_vertices, num_faces) || mr_check_limits(near, large_threshold)) return 2;
    NM_REQUIRE(d_workspace && (num_vertices == 0 || d_verts) && (num_faces == 0 || d_faces), "bad argument");
    const MvWorkspace w = mv_carve(d_workspace, num_vertices, num_faces, 0);      // the visibility words come last
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (clear && w.bits.nfw) NM_HIP_CHECK(hipMemsetAsync(w.seen, 0, sizeof(unsigned long long) * (size_t)w.bits.nfw, s));
    if (num_views) NM_HIP_CHECK(hipMemsetAsync(d_new_faces, 0, sizeof(int64_t) * (size_t)num_views, s));
    for (int64_t k = 0; k < num_views; ++k) {
        unsigned long long* counts = d_reject_counts ? reinterpret_cast<unsigned long long*>(d_reject_counts) + k * NM_MESH_RASTER_COUNTS
                                                     : w.hdr->counts;
        if (const int rc = mr_draw(views + k, d_verts, num_vertices, d_faces, num_faces, near, 0, large_threshold, w.raster, counts, s))
            return rc;
        if (!num_faces) continue;
        const int64_t pixels = (int64_t)views[k].height * views[k].width;
        hipLaunchKernelGGL(mv_mark_pixels, dim3(launch_grid(pixels)), dim3(256), 0, s, w.raster.zbuf, pixels, num_faces, w.seen,
                           reinterpret_cast<unsigned long long*>(d_new_faces) + k, counts);
        NM_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

int nm_mesh_visibility_select(const int32_t* d_faces, int64_t num_faces, int64_t num_vertices, int32_t rings, void* d_workspace,
                              int64_t* h_vertices_kept, int64_t* h_faces_kept, int64_t* h_faces_seen, int64_t* h_bad_faces,
                              void* stream) {
    if (require_mesh("mesh raster", num_vertices, num_faces)) return 2;
    NM_REQUIRE(rings >= 0 && rings <= NM_MESH_VISIBILITY_MAX_RINGS, "mesh visibility: rings must be in [0, 1024]");
    NM_REQUIRE(d_workspace && (num_faces == 0 || d_faces) && h_vertices_kept && h_faces_kept && h_faces_seen && h_bad_faces,
               "bad argument");
    const MvWorkspace w = mv_carve(d_workspace, num_vertices, num_faces, 0);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nv = (int)num_vertices;
    const unsigned fgrid = launch_grid(num_faces);
    const SubsetBits& b = w.bits;
    NM_HIP_CHECK(hipMemsetAsync(w.hdr, 0, sizeof(MvHeader), s));
    if (num_faces) {
        hipLaunchKernelGGL(mv_begin, dim3(fgrid), dim3(256), 0, s, d_faces, num_faces, nv, w.seen, b.fwords, w.hdr);
        NM_HIP_CHECK(hipGetLastError());
    }
    for (int r = 0; r <= rings && num_faces; ++r) {                  // the last round only leaves the final vertex bits
        NM_HIP_CHECK(hipMemsetAsync(b.vwords, 0, sizeof(unsigned long long) * (size_t)b.nvw, s));
        hipLaunchKernelGGL(mv_mark_corners, dim3(fgrid), dim3(256), 0, s, d_faces, num_faces, nv, b.fwords, b.vwords);
        NM_HIP_CHECK(hipGetLastError());
        if (r == rings) break;
        hipLaunchKernelGGL(mv_grow, dim3(fgrid), dim3(256), 0, s, d_faces, num_faces, nv, b.vwords, b.fwords);
        NM_HIP_CHECK(hipGetLastError());
    }
    if (!num_faces && b.nvw) NM_HIP_CHECK(hipMemsetAsync(b.vwords, 0, sizeof(unsigned long long) * (size_t)b.nvw, s));
    if (const int rc = subset_scan(b, w.hdr->totals, s)) return rc;
    MvHeader h;
    NM_HIP_CHECK(hipMemcpyAsync(&h, w.hdr, sizeof(MvHeader), hipMemcpyDeviceToHost, s));
    NM_HIP_CHECK(hipStreamSynchronize(s));
    *h_vertices_kept = (int64_t)h.totals[0];
    *h_faces_kept = (int64_t)h.totals[1];
    *h_faces_seen = (int64_t)h.faces_seen;
    *h_bad_faces = (int64_t)h.bad_faces;
    return 0;
}

int nm_mesh_visibility_compact(const void* d_workspace, const int32_t* d_faces, int64_t num_faces, int64_t num_vertices,
                               const float* d_verts, const float* d_normals, int64_t vertices_kept, int64_t faces_kept,
                               float* d_out_verts, int32_t* d_out_faces, float* d_out_normals, int32_t* d_out_face_index,
                               void* stream) {
    if (require_mesh("mesh raster", num_vertices, num_faces)) return 2;
    NM_REQUIRE_COMPACT_OUTPUTS("mesh visibility", d_workspace && (num_faces == 0 || d_faces),
                               (!d_verts || d_out_verts) && (!d_normals || d_out_normals));
    const MvWorkspace w = mv_carve(d_workspace, num_vertices, num_faces, 0);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nv = (int)num_vertices;
    const SubsetRows rows{d_verts, d_normals, nullptr, nullptr, d_out_verts, d_out_normals, nullptr, nullptr};
    if (const int rc = subset_compact_vertices(rows, nv, vertices_kept, w.bits, s)) return rc;
    return subset_compact_faces(d_faces, num_faces, nv, faces_kept, w.bits, nullptr, d_out_faces, d_out_face_index, s);
}

int nm_mesh_interpolate(const int32_t* d_face_id, const float* d_bary, int64_t num_pixels, const int32_t* d_faces, int64_t num_faces,
                        const float* d_attributes, int64_t num_vertices, int32_t channels, const float* d_background, float* d_out,
                        void* stream) {
    NM_REQUIRE(channels >= 1 && channels <= NM_MESH_INTERPOLATE_MAX_CHANNELS, "mesh interpolate: channels must be in [1, 16]");
    NM_REQUIRE(num_pixels >= 0 && num_pixels <= (int64_t)MR_MAX_SIDE * MR_MAX_SIDE, "mesh interpolate: pixels must be in [0, 2^28]");
    if (require_mesh("mesh raster", num_vertices, num_faces)) return 2;
    NM_REQUIRE(d_background && (num_pixels == 0 || (d_face_id && d_bary && d_out)) && (num_faces == 0 || d_faces) &&
               (num_vertices == 0 || d_attributes), "bad argument");
    if (num_pixels == 0) return 0;
    hipLaunchKernelGGL(mr_interpolate, dim3(launch_grid(num_pixels)), dim3(256), 0, static_cast<hipStream_t>(stream), d_face_id,
                       d_bary, num_pixels, d_faces, num_faces, d_attributes, (int)num_vertices, channels, d_background, d_out);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
