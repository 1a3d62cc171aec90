// d sigma / d x at arbitrary points (nm_mlp_density_grad): the gradient of the raw density FlexibleNeRFModel.forward returns
// (src/nerf/models.py:60-80) with respect to the input point -- what mesh_nerf --normals network turns into vertex normals.
//
// The matrix work reuses the training kernels.  Per chunk of points: the taping forward (nm_mlp_forward_train; every point a
// one-sample ray, p = o + d * 0 == o), the delta chain (nm_mlp_backward_ex) seeded with d radiance = (0, 0, 0, 1), and then
// the one kernel of this file.  It contracts the deltas that reach the encoding,
//     g_enc = delta_1 . (W0 W1)   [or delta_0 . W1 when the chain runs down to layer1's output]
//           + sum over the skip layers s of  delta_s . W_s[:, H : H + dx],
// with the Jacobian of the positional encoding [x | sin(b_k x_c) | cos(b_k x_c)] (src/nerf/modules.py:26-34, c-major):
//     d x_c = g[c] (include_input) + sum_k b_k (cos(b_k x_c) g_sin[c F + k] - sin(b_k x_c) g_cos[c F + k]).
// layer1 has no activation (models.py:62), so W1^T W0^T delta_1 = (W0 W1)^T delta_1: the product M = W0 W1 (H x dx) is formed once
// per call, as are the skip layers' encoding columns; all of them come out of the handle's PACKED image (the values the forward /
// delta kernels of the same call use), never out of the live tensors.
//
// The contraction runs on fp32 MFMA (v_mfma_f32_16x16x4_f32), the weights as the A operand, so that a tile's result has the
// encoding column in the rows and the point in the columns: D[e][p], lane = point, its 4 registers = 4 columns.  The weights are
// packed once per call into the A-operand order [block][j][r][column tile][lane]; the deltas are the B operand, read straight from
// the delta rows (k-step (j, r) of lane group g takes k = 16 j + 4 g + r: any order of k is a valid contraction, this one lets a
// lane read 4 consecutive floats of its row).  The epilogue maps each of its columns to (coordinate, band, sin | cos | identity),
// weights it and sums the 4 lane groups with two butterflies: every point's arithmetic is the same sequence whatever its place in
// the batch.
#include <algorithm>

#include "nm_internal.h"

namespace nm {

constexpr int IG_MAX_CT = 13;     // encoding columns in tiles of 16: 6 * 32 + 3 = 195 (the layer-wise path's limit) -> 13
constexpr int IG_WAVES = 4;       // waves per workgroup
constexpr int IG_PT = 2;          // 16-point tiles per wave (the A operand is loaded once for both)
constexpr int64_t IG_LW_CHUNK = 32768;          // layer-wise handles: every launch is this many rows (see ig_plan)
constexpr int64_t IG_MAX_CHUNK = 65536;
constexpr int64_t IG_CHUNK_BYTES = 2ll << 30;   // fused handles: the largest power-of-two chunk whose workspace stays below this

typedef float ig_f32x4 __attribute__((ext_vector_type(4)));

// the encoding Jacobian's weight of one column: b cos(b x) (sin column) or -b sin(b x) (cos column).  Out of line: the epilogue
// calls it for every column of every tile, and an inlined sincosf (with its large-argument reduction) in each would keep the
// epilogue from being unrolled -- the accumulators must stay in registers.
__device__ __attribute__((noinline)) float ig_jacobian(float band, float x, int is_cos) {
    float sn, cs;
    sincosf(band * x, &sn, &cs);
    return is_cos ? -(band * sn) : band * cs;
}

// the skip layer of contraction block b >= 1: the b-th set bit of the skip mask (blocks follow the layers' order)
__device__ __forceinline__ int ig_skip_layer(uint32_t mask, int b) {
    int seen = 0;
    for (int i = 0; i < 32; ++i)
        if ((mask >> i) & 1u)
            if (++seen == b) return i;
    return 0;
}

// every (tensor, element) of the packed image the contraction needs, out of the image itself: layer1.weight (H, dx) and
// layers_xyz[i].weight at wall + i * H * (H + dx), each in its own nn.Linear layout (an element may sit in the image more than
// once, always with the same value)
__global__ __launch_bounds__(256) void ig_scatter_kernel(const int32_t* __restrict__ index, const float* __restrict__ blob, int64_t count,
                                                         int num_layers, int64_t layer_floats, float* __restrict__ w1,
                                                         float* __restrict__ wall) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= count) return;
    const int32_t s = index[p];
    if (s < 0) return;
    const int t = s >> 24, e = s & 0xffffff;
    if (t == T_L1W) w1[e] = blob[p];
    else if (t >= T_XYZ0 && t < T_XYZ0 + 2 * (num_layers - 1) && ((t - T_XYZ0) & 1) == 0) wall[(int64_t)((t - T_XYZ0) >> 1) * layer_floats + e] = blob[p];
}

struct IgPackArgs {
    const float* w1;        // (H, dx)
    const float* wall;      // layers_xyz[i].weight at i * H * (H + dx)
    float* gp;              // [nb][hj][4][ct][64]
    float2* cols;           // [16 ct]: (band, code) per encoding column; code -1 none | c identity | 4 + c sin | 8 + c cos
    float bands[MAX_FREQ_XYZ];
    uint32_t skip_mask;
    int32_t nb, H, hj, dx, ct, stop, fx, inc;
};

// The A-operand image of all contraction blocks, and the per-column table of the epilogue.  Block 0 is M = W0 W1 (stop: the delta
// chain ended at layers_xyz[0]'s pre-activation) or W1; block b >= 1 is the encoding columns of the b-th skip layer.  M is summed
// over i in order with fmaf: one fixed result per call.
__global__ __launch_bounds__(256) void ig_pack_kernel(const IgPackArgs a, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < 16 * a.ct) {
        const int e = (int)idx, base = a.inc ? 3 : 0;
        float band = 0.0f;
        int code = -1;
        if (e < a.dx) {
            if (a.inc && e < 3) code = e;
            else {
                const int q = e - base, is_cos = q >= 3 * a.fx ? 1 : 0, arg = q - (is_cos ? 3 * a.fx : 0);
                const int c = arg / a.fx, k = arg - c * a.fx;
                band = a.bands[k];
                code = (is_cos ? 8 : 4) + c;
            }
        }
        a.cols[e] = make_float2(band, __int_as_float(code));
    }
    if (idx >= total) return;
    const int lane = (int)(idx & 63);
    int64_t rest = idx >> 6;
    const int ct = (int)(rest % a.ct);
    rest /= a.ct;
    const int r = (int)(rest & 3);
    rest >>= 2;
    const int j = (int)(rest % a.hj), b = (int)(rest / a.hj);
    const int k = 16 * j + 4 * (lane >> 4) + r, col = 16 * ct + (lane & 15);
    float v = 0.0f;
    if (k < a.H && col < a.dx) {
        if (b > 0) {
            const int s = ig_skip_layer(a.skip_mask, b);
            v = a.wall[(int64_t)s * a.H * (a.H + a.dx) + (int64_t)k * (a.H + a.dx) + a.H + col];
        } else if (a.stop) {
            const float* w0 = a.wall + (int64_t)k * a.H;     // layers_xyz[0] is never a skip layer: (H, H)
            for (int i = 0; i < a.H; ++i) v = fmaf(w0[i], a.w1[(int64_t)i * a.dx + col], v);
        } else {
            v = a.w1[(int64_t)k * a.dx + col];
        }
    }
    a.gp[idx] = v;
}

// (0, 0, 0, 1) per row (d sigma / d radiance) and t = 0
__global__ __launch_bounds__(256) void ig_seed_kernel(float4* __restrict__ grad_out, float* __restrict__ t, int64_t rows) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    grad_out[r] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    t[r] = 0.0f;
}

struct IgArgs {
    const float* gp;
    const float2* cols;
    const float* d_h;         // delta planes (L, rows, H) of this chunk
    int64_t plane_stride;     // rows * H
    const float* points;      // (n, 3)
    float* out;               // (n, 3)
    int64_t n;
    uint32_t skip_mask;
    int32_t nb, H, hj, plane0;
};

template <int CT>
__global__ __launch_bounds__(IG_WAVES * 64) void input_grad_kernel(const IgArgs a) {
    const int lane = threadIdx.x & 63, g = lane >> 4, col = lane & 15;
    const int wave = threadIdx.x >> 6;
    const int64_t p0 = ((int64_t)blockIdx.x * IG_WAVES + wave) * (16 * IG_PT);
    if (p0 >= a.n) return;                                   // uniform per wave
    int64_t row[IG_PT];
    bool ok[IG_PT];
#pragma unroll
    for (int pt = 0; pt < IG_PT; ++pt) {
        row[pt] = p0 + 16 * pt + col;
        ok[pt] = row[pt] < a.n;
    }
    ig_f32x4 acc[IG_PT][CT];
#pragma unroll
    for (int pt = 0; pt < IG_PT; ++pt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[pt][ct] = ig_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int H = a.H;
    for (int b = 0; b < a.nb; ++b) {
        const int plane = b == 0 ? a.plane0 : 1 + ig_skip_layer(a.skip_mask, b);
        const float* dp = a.d_h + (int64_t)plane * a.plane_stride;
        const float* gb = a.gp + (int64_t)b * a.hj * 4 * CT * 64 + lane;
        for (int j = 0; j < a.hj; ++j) {
            const int k0 = 16 * j + 4 * g;
            float dv[IG_PT][4];
#pragma unroll
            for (int pt = 0; pt < IG_PT; ++pt)
#pragma unroll
                for (int r = 0; r < 4; ++r) dv[pt][r] = (ok[pt] && k0 + r < H) ? dp[row[pt] * H + k0 + r] : 0.0f;
            const float* gj = gb + (int64_t)j * 4 * CT * 64;
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    const float w = gj[(r * CT + ct) * 64];
#pragma unroll
                    for (int pt = 0; pt < IG_PT; ++pt)
                        acc[pt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, dv[pt][r], acc[pt][ct], 0, 0, 0);
                }
        }
    }
    // epilogue: register r of tile ct holds g_enc[point = col][column 16 ct + 4 g + r]
#pragma unroll
    for (int pt = 0; pt < IG_PT; ++pt) {
        float x[3] = {0.0f, 0.0f, 0.0f};
        if (ok[pt])
            for (int c = 0; c < 3; ++c) x[c] = a.points[row[pt] * 3 + c];
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float2 info = a.cols[16 * ct + 4 * g + r];
                const int code = __float_as_int(info.y);
                if (code < 0) continue;
                const int c = code & 3;
                const float v = acc[pt][ct][r];
                const float xc = c == 0 ? x[0] : (c == 1 ? x[1] : x[2]);
                const float d = code < 4 ? v : ig_jacobian(info.x, xc, code >= 8) * v;
                if (c == 0) s0 += d;
                else if (c == 1) s1 += d;
                else s2 += d;
            }
        s0 += __shfl_xor(s0, 16); s1 += __shfl_xor(s1, 16); s2 += __shfl_xor(s2, 16);
        s0 += __shfl_xor(s0, 32); s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
        if (ok[pt] && g == 0) {
            float* o = a.out + row[pt] * 3;
            o[0] = s0; o[1] = s1; o[2] = s2;
        }
    }
}

using IgKernel = void (*)(const IgArgs);
static IgKernel ig_kernel(int ct) {
    switch (ct) {
        case 1: return input_grad_kernel<1>;   case 2: return input_grad_kernel<2>;   case 3: return input_grad_kernel<3>;
        case 4: return input_grad_kernel<4>;   case 5: return input_grad_kernel<5>;   case 6: return input_grad_kernel<6>;
        case 7: return input_grad_kernel<7>;   case 8: return input_grad_kernel<8>;   case 9: return input_grad_kernel<9>;
        case 10: return input_grad_kernel<10>; case 11: return input_grad_kernel<11>; case 12: return input_grad_kernel<12>;
        case 13: return input_grad_kernel<13>;
        default: return nullptr;
    }
}

// The shape of one call's work.  Fused families evaluate every row independently of the others and of the launch's size, so a
// chunk is min(chunk, rows left).  The layer-wise path sizes its GEMM tiling by the batch, so it always runs IG_LW_CHUNK rows
// (the tail zero-padded): a point's result never depends on n, its offset or the chunking.
struct IgPlan {
    bool lw, tuned, flat, stop;
    int L, H, dx, hj, ct, nb;
    int64_t chunk;
};

struct IgLayout {
    size_t gp, cols, w1, wall, gout, t, pts, rad, th, tfeat, tv, mh, mv, dh, dfeat, dv, dlast, total;
};

static IgLayout ig_layout(const IgPlan& p, int64_t rows) {
    IgLayout l{};
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; };
    const int64_t H = p.H, L = p.L, tiles = (rows + 15) / 16;
    const bool view = !p.flat;
    l.gp = take((size_t)p.nb * p.hj * 4 * p.ct * 64 * 4);
    l.cols = take((size_t)16 * p.ct * 8);
    l.w1 = take((size_t)H * p.dx * 4);
    l.wall = take((size_t)(L - 1) * H * (H + p.dx) * 4);
    l.gout = take((size_t)rows * 16);
    l.t = take((size_t)rows * 4);
    l.pts = p.lw ? take((size_t)rows * 12) : 0;
    l.rad = take((size_t)rows * 16);
    l.th = take((size_t)L * rows * H * 4);
    l.tfeat = view ? take((size_t)rows * H * 4) : 0;
    l.tv = view ? take((size_t)rows * (H / 2) * 4) : 0;
    l.mh = p.tuned ? take((size_t)L * tiles * 64 * 8) : 0;
    l.mv = p.tuned && view ? take((size_t)tiles * 64 * 8) : 0;
    l.dh = take((size_t)L * rows * H * 4);
    l.dfeat = view ? take((size_t)rows * H * 4) : 0;
    l.dv = view ? take((size_t)rows * (H / 2) * 4) : 0;
    l.dlast = take((size_t)rows * 16);
    l.total = off;
    return l;
}

static IgPlan ig_plan(const nm_mlp* m) {
    const nm_mlp_desc& d = m->desc;
    IgPlan p{};
    p.lw = m->lw != nullptr;
    p.tuned = !p.lw && m->plan->generic_nt == 0;
    p.flat = d.use_viewdirs == 0;
    p.stop = nm_mlp_backward_stops_at_xyz0(m) != 0;
    p.L = d.num_layers; p.H = d.hidden_size;
    p.dx = 6 * d.num_encoding_fn_xyz + (d.include_input_xyz ? 3 : 0);
    p.hj = (p.H + 15) / 16;
    p.ct = (p.dx + 15) / 16;
    p.nb = 1;
    for (int i = 0; i < d.num_layers - 1; ++i)
        if (i % d.skip_step == 0 && i > 0 && i != d.num_layers - 1) ++p.nb;     // models.py:63-65
    if (p.lw) p.chunk = IG_LW_CHUNK;
    else {
        p.chunk = IG_MAX_CHUNK;
        while (p.chunk > 1024 && ig_layout(p, p.chunk).total > (size_t)IG_CHUNK_BYTES) p.chunk /= 2;
    }
    return p;
}

static int64_t ig_rows(const IgPlan& p, int64_t n) { return p.lw ? p.chunk : std::min(p.chunk, n); }

}  // namespace nm

using namespace nm;

extern "C" {

int64_t nm_mlp_density_grad_workspace_bytes(const nm_mlp* m, int64_t n) {
    if (!m || n < 0) return -1;
    if (n == 0 || m->precision != NM_PREC_F32) return 0;
    const IgPlan p = ig_plan(m);
    return (int64_t)ig_layout(p, ig_rows(p, n)).total;
}

int nm_mlp_density_grad(nm_mlp* m, const float* d_points, int64_t n, void* d_workspace, int64_t workspace_bytes, float* d_grad,
                        void* stream_) {
    NM_REQUIRE(m && n >= 0 && (n == 0 || (d_points && d_grad && d_workspace)), "bad argument");
    NM_REQUIRE(m->precision == NM_PREC_F32, "density_grad: geometry is fp32 by contract (bf16x3 handle)");
    if (n == 0) return 0;
    const IgPlan p = ig_plan(m);
    NM_REQUIRE(p.ct >= 1 && p.ct <= IG_MAX_CT, "density_grad: encoding wider than 208 columns");
    const int64_t rows_max = ig_rows(p, n);
    const IgLayout l = ig_layout(p, rows_max);
    NM_REQUIRE(workspace_bytes >= (int64_t)l.total, "density_grad: workspace too small (nm_mlp_density_grad_workspace_bytes)");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    char* ws = static_cast<char*>(d_workspace);
    auto F = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };

    // once per call: the weights out of the packed image, the A-operand image, the seeds
    const int64_t blob = (int64_t)m->blob_floats;
    hipLaunchKernelGGL(ig_scatter_kernel, dim3((unsigned)((blob + 255) / 256)), dim3(256), 0, stream, m->d_index,
                       static_cast<const float*>(m->d_blob), blob, p.L, (int64_t)p.H * (p.H + p.dx), F(l.w1), F(l.wall));
    IgPackArgs pk{};
    pk.w1 = F(l.w1); pk.wall = F(l.wall); pk.gp = F(l.gp); pk.cols = reinterpret_cast<float2*>(ws + l.cols);
    for (int f = 0; f < MAX_FREQ_XYZ; ++f) pk.bands[f] = m->base.bands_xyz[f];
    pk.skip_mask = 0;
    for (int i = 0; i < p.L - 1; ++i)
        if (i % m->desc.skip_step == 0 && i > 0 && i != p.L - 1) pk.skip_mask |= 1u << i;
    pk.nb = p.nb; pk.H = p.H; pk.hj = p.hj; pk.dx = p.dx; pk.ct = p.ct; pk.stop = p.stop ? 1 : 0;
    pk.fx = m->desc.num_encoding_fn_xyz; pk.inc = m->desc.include_input_xyz ? 1 : 0;
    const int64_t gp_total = (int64_t)p.nb * p.hj * 4 * p.ct * 64;
    hipLaunchKernelGGL(ig_pack_kernel, dim3((unsigned)((gp_total + 255) / 256)), dim3(256), 0, stream, pk, gp_total);
    hipLaunchKernelGGL(ig_seed_kernel, dim3((unsigned)((rows_max + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<float4*>(ws + l.gout), F(l.t), rows_max);
    NM_HIP_CHECK(hipGetLastError());

    IgArgs ga{};
    ga.gp = F(l.gp); ga.cols = reinterpret_cast<const float2*>(ws + l.cols);
    ga.skip_mask = pk.skip_mask; ga.nb = p.nb; ga.H = p.H; ga.hj = p.hj; ga.plane0 = p.stop ? 1 : 0;
    const IgKernel kernel = ig_kernel(p.ct);
    for (int64_t first = 0; first < n; first += p.chunk) {
        const int64_t cnt = std::min(p.chunk, n - first), rows = p.lw ? p.chunk : cnt;
        const float* pts = d_points + first * 3;
        if (p.lw) {          // a fixed-size batch: this chunk's points, zeros behind them
            NM_HIP_CHECK(hipMemcpyAsync(F(l.pts), pts, (size_t)cnt * 12, hipMemcpyDeviceToDevice, stream));
            if (rows > cnt) NM_HIP_CHECK(hipMemsetAsync(F(l.pts) + cnt * 3, 0, (size_t)(rows - cnt) * 12, stream));
            pts = F(l.pts);
        }
        nm_mlp_tape tape{};
        tape.d_h = F(l.th);
        tape.d_feat = p.flat ? nullptr : F(l.tfeat);
        tape.d_v = p.flat ? nullptr : F(l.tv);
        tape.d_mask_h = p.tuned ? reinterpret_cast<uint64_t*>(ws + l.mh) : nullptr;
        tape.d_mask_v = p.tuned && !p.flat ? reinterpret_cast<uint64_t*>(ws + l.mv) : nullptr;
        tape.skip_h0 = p.stop ? 1 : 0;
        // every point a one-sample ray: origin = the point, direction = the point (the view branch's input; sigma does not read
        // it), t = 0
        if (int rc = nm_mlp_forward_train(m, pts, 1, pts, F(l.t), rows, 1, &tape, F(l.rad), stream_)) return rc;
        nm_mlp_deltas dl{};
        dl.d_h = F(l.dh);
        dl.d_feat = p.flat ? nullptr : F(l.dfeat);
        dl.d_v = p.flat ? nullptr : F(l.dv);
        dl.d_last = F(l.dlast);
        if (int rc = nm_mlp_backward_ex(m, rows, &tape, F(l.rad), F(l.gout), &dl, p.stop ? NM_BACKWARD_STOP_AT_XYZ0 : 0, stream_))
            return rc;
        ga.d_h = F(l.dh);
        ga.plane_stride = rows * p.H;
        ga.points = d_points + first * 3;
        ga.out = d_grad + first * 3;
        ga.n = cnt;
        const int64_t per_block = 16 * IG_PT * IG_WAVES;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((cnt + per_block - 1) / per_block)), dim3(IG_WAVES * 64), 0, stream, ga);
        NM_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
