// Texture atlas of a mesh (mesh_nerf --texture-res, mesh_render --appearance; DESIGN.md, "Texture atlas"): every face gets the
// same right-triangle chart on a barycentric lattice of n intervals per side, two charts tile one cell of (n + 3) x (n + 2)
// texels, the cells tile the image in closed form.  Every index is a formula, so nothing is compacted and the bytes do not
// depend on the order the workgroups ran in; every fp32 operation is rounded on its own (-ffp-contract=off), division and
// square root correctly rounded, and a numpy restatement (tests/mesh_texture.py) reproduces every array bit for bit.  THE RULE
// is written out in include/nerfmeshes_hip.h ("Texture atlas of a mesh"); the comments below name its paragraphs.
// Kernels, all gather-only with one thread per output element: mt_samples (one thread per sample: position and direction; the
// two counts by ballot, one integer atomic per wave), mt_fill (one thread per texel: cell -> face -> lattice point, then copy,
// extrapolate or zero, and quantise), mt_uv (one thread per face corner), mt_lookup (one thread per pixel: the bilinear fetch).
// Nothing allocates and nothing synchronises with the host: every entry can be captured into a graph.
#include "compact.h"
#include "nm_internal.h"

namespace nm {

struct MtLayout { int n, cw, ch, cols, rows, width, height, samples; int64_t faces, cells; };   // samples: T

// "atlas": false when n or F is out of range or the image would be wider than NM_MESH_TEXTURE_MAX_SIDE
static bool mt_layout(int64_t faces, int n, MtLayout& l) {
    if (n < 1 || n > NM_MESH_TEXTURE_MAX_RES || !mesh_size_ok(faces)) return false;
    l.n = n;
    l.cw = n + 3;
    l.ch = n + 2;
    l.samples = (n + 1) * (n + 2) / 2;
    l.faces = faces;
    l.cells = (faces + 1) / 2;
    for (int64_t cols = 1; cols * l.cw <= NM_MESH_TEXTURE_MAX_SIDE; ++cols) {
        const int64_t rows = (l.cells + cols - 1) / cols;
        if (cols * l.cw >= rows * l.ch) {
            l.cols = (int)cols;
            l.rows = (int)rows;
            l.width = (int)(cols * l.cw);
            l.height = (int)(rows * l.ch);
            return true;
        }
    }
    return false;
}


// "lattice": index within the face of the point (i, j)
__device__ __forceinline__ int mt_index(int n, int i, int j) { return j * (n + 1) - j * (j - 1) / 2 + i; }

// ... and its inverse: the row from a square root, corrected by whole rows (the estimate is within one of the answer)
__device__ __forceinline__ void mt_point(int n, int index, int& i, int& j) {
    const int s = 2 * n + 3;
    int row = (int)(((float)s - sqrtf((float)(s * s - 8 * index))) * 0.5f);
    row = min(max(row, 0), n);
    while (row > 0 && mt_index(n, 0, row) > index) --row;
    while (row < n && mt_index(n, 0, row + 1) <= index) ++row;
    j = row;
    i = index - mt_index(n, 0, row);
}

__device__ __forceinline__ float mt_length(const float (&v)[3]) {
    const float xx = v[0] * v[0], yy = v[1] * v[1], zz = v[2] * v[2];
    return sqrtf((xx + yy) + zz);
}

// "sample"; whole waves (the votes)
__global__ __launch_bounds__(256) void mt_samples(const float* __restrict__ verts, int nv, const int32_t* __restrict__ faces,
                                                  const float* __restrict__ normals, int n, int per_face, float minus_flip,
                                                  int64_t first, int64_t samples, float* __restrict__ positions,
                                                  float* __restrict__ directions, unsigned long long* counts) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool fallback = false, bad = false;
    if (s < samples) {
        const int64_t f = first + s / per_face;
        int i, j, c[3];
        mt_point(n, (int)(s % per_face), i, j);
        float p[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f};
        if (!load_face(faces, f, nv, c)) {
            bad = true;
        } else {
            const float fn = (float)n;
            const float b0 = (float)(n - i - j) / fn, b1 = (float)i / fn, b2 = (float)j / fn;
            float q[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int a = 0; a < 3; ++a) q[k][a] = verts[3 * (int64_t)c[k] + a];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float t0 = b0 * q[0][a], t1 = b1 * q[1][a], t2 = b2 * q[2][a];
                const float v = (t0 + t1) + t2;
                p[a] = v != v ? __uint_as_float(0x7fc00000u) : v;
            }
            bool have = false;
            if (normals) {
                float m[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float t0 = b0 * normals[3 * (int64_t)c[0] + a], t1 = b1 * normals[3 * (int64_t)c[1] + a];
                    const float t2 = b2 * normals[3 * (int64_t)c[2] + a];
                    m[a] = (t0 + t1) + t2;
                }
                const float len = mt_length(m);
                if (len > 0.0f && is_finite(len)) {
                    have = true;
#pragma unroll
                    for (int a = 0; a < 3; ++a) d[a] = -(m[a] / len);
                }
            }
            if (!have) {
                fallback = true;
                float e1[3], e2[3], g[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) { e1[a] = q[1][a] - q[0][a]; e2[a] = q[2][a] - q[0][a]; }
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const int b = (a + 1) % 3, e = (a + 2) % 3;
                    const float l = e1[b] * e2[e], r = e1[e] * e2[b];
                    g[a] = l - r;
                }
                const float len = mt_length(g);
                if (len > 0.0f && is_finite(len)) {
#pragma unroll
                    for (int a = 0; a < 3; ++a) d[a] = (g[a] / len) * minus_flip;
                } else {
                    d[0] = 0.0f; d[1] = 0.0f; d[2] = -1.0f;
                }
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) { positions[3 * s + a] = p[a]; directions[3 * s + a] = d[a]; }
    }
    const unsigned long long fallbacks = __ballot(fallback), bads = __ballot(bad);
    if ((threadIdx.x & 63) == 0) {
        if (fallbacks) atomicAdd(counts + NM_MESH_TEXTURE_FALLBACK, (unsigned long long)__popcll(fallbacks));
        if (bads) atomicAdd(counts + NM_MESH_TEXTURE_BAD_INDEX, (unsigned long long)__popcll(bads));
    }
}

// "quantise"
__device__ __forceinline__ uint8_t mt_u8(float c) {
    if (c != c) return 0;
    const float t = fminf(fmaxf(c, 0.0f), 1.0f) * 255.0f;
    return (uint8_t)(t + 0.5f);
}

// "cell", "atlas", "gutter", "empty": one thread per texel
__global__ __launch_bounds__(256) void mt_fill(const float* __restrict__ colors, const MtLayout l, uint8_t* __restrict__ atlas) {
    const int64_t texel = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (texel >= (int64_t)l.height * l.width) return;
    const int x = (int)(texel % l.width), y = (int)(texel / l.width);
    const int a = x % l.cw, b = y % l.ch, n = l.n;
    const int64_t cell = (int64_t)(y / l.ch) * l.cols + x / l.cw;
    const bool lower = a + b <= n + 1;
    const int64_t f = 2 * cell + (lower ? 0 : 1);
    const int i = lower ? a : n + 2 - a, j = lower ? b : n + 1 - b;
    float c[3] = {0.0f, 0.0f, 0.0f};
    if (cell < l.cells && f < l.faces) {
        const float* rows = colors + 3 * f * (int64_t)l.samples;
        if (i + j <= n) {
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = rows[3 * mt_index(n, i, j) + k];
        } else if (i == 0 || j == 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = rows[3 * (i == 0 ? mt_index(n, 0, n) : mt_index(n, n, 0)) + k];
        } else {
            const int left = mt_index(n, i - 1, j), below = mt_index(n, i, j - 1), corner = mt_index(n, i - 1, j - 1);
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = (rows[3 * left + k] + rows[3 * below + k]) - rows[3 * corner + k];
        }
    }
    const bool used = cell < l.cells && f < l.faces;
#pragma unroll
    for (int k = 0; k < 3; ++k) atlas[3 * texel + k] = used ? mt_u8(c[k]) : (uint8_t)0;
}

// "uv": one thread per face corner
__global__ __launch_bounds__(256) void mt_uv(const MtLayout l, float* __restrict__ uv) {
    const int64_t corner = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (corner >= 3 * l.faces) return;
    const int64_t f = corner / 3, cell = f / 2;
    const int k = (int)(corner % 3), n = l.n;
    const int i = k == 1 ? n : 0, j = k == 2 ? n : 0;
    const bool lower = (f & 1) == 0;
    const int x = (int)(cell % l.cols) * l.cw + (lower ? i : n + 2 - i), y = (int)(cell / l.cols) * l.ch + (lower ? j : n + 1 - j);
    uv[2 * corner] = (float)(2 * x + 1) / (float)(2 * l.width);
    uv[2 * corner + 1] = (float)(2 * (l.height - y) - 1) / (float)(2 * l.height);
}

// "lookup": one thread per pixel
__global__ __launch_bounds__(256) void mt_lookup(const int32_t* __restrict__ face_id, const float* __restrict__ bary, int64_t pixels,
                                                 const float* __restrict__ face_uv, int64_t nf, const uint8_t* __restrict__ texture,
                                                 int th, int tw, const float* __restrict__ background, float* __restrict__ out) {
    const int64_t pixel = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pixel >= pixels) return;
    const int64_t f = face_id[pixel];
    float uv[2] = {0.0f, 0.0f};
    bool ok = f >= 0 && f < nf;
    if (ok) {
        const float b0 = bary[3 * pixel], b1 = bary[3 * pixel + 1], b2 = bary[3 * pixel + 2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const float t0 = b0 * face_uv[6 * f + a], t1 = b1 * face_uv[6 * f + 2 + a], t2 = b2 * face_uv[6 * f + 4 + a];
            uv[a] = (t0 + t1) + t2;
        }
        ok = is_finite(uv[0]) && is_finite(uv[1]);
    }
    if (!ok) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out[3 * pixel + k] = background[k];
        return;
    }
    const float sx = uv[0] * (float)tw, sy = (1.0f - uv[1]) * (float)th;
    const float tx = fminf(fmaxf(sx - 0.5f, 0.0f), (float)(tw - 1)), ty = fminf(fmaxf(sy - 0.5f, 0.0f), (float)(th - 1));
    const float flx = floorf(tx), fly = floorf(ty);
    const int ix0 = (int)flx, iy0 = (int)fly, ix1 = min(ix0 + 1, tw - 1), iy1 = min(iy0 + 1, th - 1);
    const float fx = tx - flx, fy = ty - fly;
    const uint8_t* r0 = texture + 3 * (int64_t)iy0 * tw;
    const uint8_t* r1 = texture + 3 * (int64_t)iy1 * tw;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float c00 = (float)r0[3 * ix0 + k] / 255.0f, c10 = (float)r0[3 * ix1 + k] / 255.0f;
        const float c01 = (float)r1[3 * ix0 + k] / 255.0f, c11 = (float)r1[3 * ix1 + k] / 255.0f;
        const float dt = c10 - c00, db = c11 - c01;
        const float pt = fx * dt, pb = fx * db;
        const float top = c00 + pt, bottom = c01 + pb;
        const float dv = bottom - top;
        const float pv = fy * dv;
        out[3 * pixel + k] = top + pv;
    }
}

static bool mt_side_ok(int64_t n) { return n >= 1 && n <= NM_MESH_TEXTURE_MAX_SIDE; }

}  // namespace nm

using namespace nm;

#define MT_LAYOUT(l, faces, n)                                                                                                  \
    MtLayout l;                                                                                                                  \
    NM_REQUIRE(n >= 1 && n <= NM_MESH_TEXTURE_MAX_RES, "mesh texture: the resolution n must be in [1, 255]");                    \
    NM_REQUIRE(mesh_size_ok(faces), "mesh texture: the face count must be in [0, 2^31 - 64)");                                   \
    NM_REQUIRE(mt_layout(faces, n, l), "mesh texture: the atlas would be wider than 16384 texels")

extern "C" {

int nm_mesh_texture_layout(int64_t num_faces, int32_t n, int64_t* h_layout) {
    NM_REQUIRE(h_layout != nullptr, "bad argument");
    MT_LAYOUT(l, num_faces, n);
    h_layout[NM_MESH_TEXTURE_W] = l.width;
    h_layout[NM_MESH_TEXTURE_H] = l.height;
    h_layout[NM_MESH_TEXTURE_COLS] = l.cols;
    h_layout[NM_MESH_TEXTURE_ROWS] = l.rows;
    h_layout[NM_MESH_TEXTURE_T] = l.samples;
    return 0;
}

int nm_mesh_texture_samples(const float* d_verts, int64_t num_vertices, const int32_t* d_faces, int64_t num_faces,
                            const float* d_normals, int32_t n, int32_t flip, int64_t first, int64_t count, float* d_positions,
                            float* d_directions, int64_t* d_counts, void* stream) {
    NM_REQUIRE(n >= 1 && n <= NM_MESH_TEXTURE_MAX_RES, "mesh texture: the resolution n must be in [1, 255]");
    if (require_mesh("mesh texture", num_vertices, num_faces)) return 2;
    NM_REQUIRE(flip == 1 || flip == -1, "mesh texture: flip must be +1 or -1");
    NM_REQUIRE(first >= 0 && count >= 0 && first <= num_faces && count <= num_faces - first,
               "mesh texture: the window must lie inside [0, F]");
    const int per_face = (n + 1) * (n + 2) / 2;
    const int64_t samples = count * per_face;
    NM_REQUIRE(mesh_size_ok(samples), "mesh texture: the samples of one window must be fewer than 2^31 - 64");
    NM_REQUIRE(d_counts && (samples == 0 || (d_positions && d_directions)) && (num_faces == 0 || d_faces) &&
               (num_vertices == 0 || d_verts), "bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    NM_HIP_CHECK(hipMemsetAsync(d_counts, 0, sizeof(int64_t) * NM_MESH_TEXTURE_COUNTS, s));
    if (samples == 0) return 0;
    hipLaunchKernelGGL(mt_samples, dim3(launch_grid(samples)), dim3(256), 0, s, d_verts, (int)num_vertices, d_faces, d_normals, (int)n,
                       per_face, (float)(-flip), first, samples, d_positions, d_directions,
                       reinterpret_cast<unsigned long long*>(d_counts));
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

int nm_mesh_texture_fill(const float* d_colors, int64_t num_faces, int32_t n, uint8_t* d_atlas, void* stream) {
    MT_LAYOUT(l, num_faces, n);
    const int64_t texels = (int64_t)l.height * l.width;
    NM_REQUIRE((texels == 0 || d_atlas) && (num_faces == 0 || d_colors), "bad argument");
    if (texels == 0) return 0;
    hipLaunchKernelGGL(mt_fill, dim3(launch_grid(texels)), dim3(256), 0, static_cast<hipStream_t>(stream), d_colors, l, d_atlas);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

int nm_mesh_texture_uv(int64_t num_faces, int32_t n, float* d_face_uv, void* stream) {
    MT_LAYOUT(l, num_faces, n);
    NM_REQUIRE(num_faces == 0 || d_face_uv, "bad argument");
    if (num_faces == 0) return 0;
    hipLaunchKernelGGL(mt_uv, dim3(launch_grid(3 * num_faces)), dim3(256), 0, static_cast<hipStream_t>(stream), l, d_face_uv);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

int nm_mesh_texture_lookup(const int32_t* d_face_id, const float* d_bary, int64_t num_pixels, const float* d_face_uv,
                           int64_t num_faces, const uint8_t* d_texture, int32_t tex_height, int32_t tex_width,
                           const float* d_background, float* d_out, void* stream) {
    NM_REQUIRE(num_pixels >= 0 && num_pixels <= (int64_t)NM_MESH_TEXTURE_MAX_SIDE * NM_MESH_TEXTURE_MAX_SIDE,
               "mesh texture: pixels must be in [0, 2^28]");
    NM_REQUIRE(mesh_size_ok(num_faces), "mesh texture: the face count must be in [0, 2^31 - 64)");
    NM_REQUIRE(mt_side_ok(tex_height) && mt_side_ok(tex_width), "mesh texture: the texture's sides must be in [1, 16384]");
    NM_REQUIRE(d_background && d_texture && (num_pixels == 0 || (d_face_id && d_bary && d_out)) && (num_faces == 0 || d_face_uv),
               "bad argument");
    if (num_pixels == 0) return 0;
    hipLaunchKernelGGL(mt_lookup, dim3(launch_grid(num_pixels)), dim3(256), 0, static_cast<hipStream_t>(stream), d_face_id, d_bary,
                       num_pixels, d_face_uv, num_faces, d_texture, (int)tex_height, (int)tex_width, d_background, d_out);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
