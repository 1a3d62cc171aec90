// Internal declarations shared by the HIP translation units of libnerfmeshes_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>

#include "../../include/nerfmeshes_hip.h"
#include "mlp_pack.h"

namespace nm {

void set_error(const std::string& msg);

#define NM_HIP_CHECK(expr)                                                                   \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            ::nm::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));              \
            return 1;                                                                        \
        }                                                                                    \
    } while (0)

#define NM_REQUIRE(cond, msg)                                                                \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            ::nm::set_error(std::string(msg) + " [" #cond "]");                              \
            return 2;                                                                        \
        }                                                                                    \
    } while (0)

// ---- fused MLP ------------------------------------------------------------------------------
constexpr int KC = 8;          // k-steps (of 4 input features) per LDS weight chunk
constexpr int MAX_FREQ_XYZ = 32;   // frequency bands a handle keeps per encoding (the fused kernels take up to 15 / 16 functions,
constexpr int MAX_FREQ_DIR = 32;   // the layer-wise path up to 32: nerf_layerwise.h)

enum MlpMode : int { MODE_POINTS = 0, MODE_RAYS = 1, MODE_GRID = 2, MODE_VIEW = 3 };

// Pinhole rays generated inside the consuming kernel from the camera pose (get_ray_bundle,
// /root/reference/src/nerf/nerf_helpers.py:226-277, optionally followed by ndc_rays, :280-307): ray r of a launch
// is pixel `first + r` (row-major).  nm_ray_bundle and nm_view_rays materialise rays through nm_gen_ray and ndc_rays_kernel
// calls nm_ndc_ray, so a render from the pose is bit-identical to a render from a materialised ray buffer.
struct RayGen {
    float rot[9];            // c2w[:3,:3], row-major
    float origin[3];         // c2w[:3,3]
    int32_t height, width;
    float focal;
    int32_t enabled;
    int32_t ndc;             // apply ndc_rays(H, W, focal, near, o, d) to every generated ray
    float ndc_near, c_w, c_h, two_near, m_two_near;   // fp64 host constants of ndc_rays rounded to fp32, as torch does
    int64_t first;
};

__device__ __forceinline__ float nm_norm3(float x, float y, float z) {
    return sqrtf(fmaf(z, z, fmaf(y, y, x * x)));  // matches at::norm(p=2) on CPU bit for bit
}

// ndc_rays (nerf_helpers.py:280-307), op for op: python-float scalars enter every tensor op rounded to fp32
__device__ __forceinline__ void nm_ndc_ray(float near32, float c_w, float c_h, float two_near, float m_two_near,
                                           float (&o)[3], float (&d)[3]) {
    const float t = -(near32 + o[2]) / d[2];
    float q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { const float td = t * d[a]; q[a] = o[a] + td; }
    const float o0 = (c_w * q[0]) / q[2];
    const float o1 = (c_h * q[1]) / q[2];
    const float rq = 1.0f / q[2];            // python-float / tensor is Tensor.__rtruediv__ = reciprocal() * scalar
    const float o2 = 1.0f + rq * two_near;
    const float d0 = c_w * (d[0] / d[2] - q[0] / q[2]);
    const float d1 = c_h * (d[1] / d[2] - q[1] / q[2]);
    const float d2 = rq * m_two_near;
    o[0] = o0; o[1] = o1; o[2] = o2;
    d[0] = d0; d[1] = d1; d[2] = d2;
}

__device__ __forceinline__ void nm_gen_ray(const RayGen& g, int64_t ray, float (&o)[3], float (&d)[3]) {
    const int64_t pix = g.first + ray;
    const int row = (int)(pix / g.width), colx = (int)(pix - (int64_t)row * g.width);
    const float x = ((float)colx - (float)(g.width * 0.5)) / g.focal;
    const float y = -((float)row - (float)(g.height * 0.5)) / g.focal;
    const float z = -1.0f;
    const float n = nm_norm3(x, y, z);
    const float dx = x / n, dy = y / n, dz = z / n;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        d[a] = (dx * g.rot[3 * a] + dy * g.rot[3 * a + 1]) + dz * g.rot[3 * a + 2];
        o[a] = g.origin[a];
    }
    if (g.ndc) nm_ndc_ray(g.ndc_near, g.c_w, g.c_h, g.two_near, g.m_two_near, o, d);
}

// Kernel arguments (passed by value).
struct MlpArgs {
    const char* wstream;     // packed MFMA A-operand stream, stage after stage
    const float* bias;       // layer1 | layers_xyz.* | fc_feat | layers_dir.0 | fc_alpha.b | fc_rgb.b[3]  (concatenated)
    const float* walpha;     // [4 lane groups][H/4 k-steps]
    const float* wrgb;       // [3][4][H/8]
    float bands_xyz[MAX_FREQ_XYZ];
    float bands_dir[MAX_FREQ_DIR];
    uint32_t skip_mask;      // bit i set: layers_xyz[i] consumes cat(hidden, xyz_enc)
    int32_t mode;
    // inputs: POINTS: a=points b=dirs | RAYS: a=origins b=dirs c=t | GRID: a,b,c = axis values
    const float* a;
    const float* b;
    const float* c;
    int64_t n;               // samples to evaluate
    int64_t first;           // GRID: flat index of the first point
    int32_t samples;         // RAYS: samples per ray
    int32_t origins_per_ray; // RAYS
    int32_t n1, n2;          // GRID: sizes of axis 1 and 2
    float* out;              // (n,4) or (n,) when density only
    // training tape (nm_mlp_forward_train only; see nm_mlp_tape in the public header)
    float* tape_h;           // (L, n, H): layer1 output, then the post-ReLU output of every layers_xyz[i]
    float* tape_feat;        // (n, H)  relu(fc_feat(x))
    float* tape_v;           // (n, H/2), rows tape_v_ld floats apart
    uint64_t* mask_h;        // (L, tiles, 64): layers_xyz[0..L-2] then fc_feat; per lane, bit 4*tile+reg = activation > 0
    uint64_t* mask_v;        // (tiles, 64)
    int64_t tiles;           // ceil(n / 16)
    float* tape_encx;        // (n, 64) or null: the positional-encoding row of every sample point, reference column order
    float* tape_encd;        // (n, 64) or null: likewise for the view direction (tuned family only: nm_mlp_tape.d_enc_*)
    int32_t tape_v_ld;       // floats per row of tape_v (nm_mlp_tape.v_stride; H/2 when the caller left it 0)
    int32_t tape_skip_h0;    // tuned taping kernels: do not write tape_h[0] (nm_mlp_tape.skip_h0: layer1's output, which a backward that
                             // takes layer1's and layers_xyz[0]'s gradients by linearity never reads)
    RayGen gen;              // VIEW: rays generated from the pose (c = t as in RAYS; a, b unused)
    // generic-shape kernels only (mlp_device_g.h): the encodings' run-time description
    const void* g_tab;       // device: GEncArg[2][96] (xyz, dir; two parts of 48): coordinate and frequency band of every encoding argument
    int32_t g_nsx, g_idx, g_chx;   // xyz: k-steps that carry arguments, 1 = an identity step follows, whole chunks in the stream
    int32_t g_nsd, g_idd, g_chd;   // direction encoding likewise (g_chd = 0: no encoded direction columns at all)
    int32_t g_h, g_hd;             // the REAL widths hidden_size and hidden_size // 2: row strides of the generic training tape
    // render-internal evaluation (render_impl in ray_ops.hip only; launch_mlp clears all four where the plan has no kernel_skip)
    int32_t skip_empty;      // a workgroup tile on which no sample has raw sigma > 0 gets {0, 0, 0, sigma} and skips the colour branch
    int32_t ray_tiles;       // RAYS / VIEW with samples % 16 == 0: a tile is wg_samples / 16 adjacent rays x 16 consecutive samples
    uint32_t* skip_count;    // null, or the launch's counter of skipped tiles (profiling: mlp_api.hip)
    uint32_t* tile_queue;    // skip_empty launches: the device word their workgroups claim tiles from (mlp_device_r3.h), zero when the
                             // launch starts; launch_mlp sets it from the handle
    // Ray termination (mlp_device_r3.h): att[depth slot][ray, padded to whole ray blocks] = an upper bound of log2 of the product of
    // the ray's transmittance factors over the slots up to this one (0: nothing known), zero when the launch starts.  Set by
    // render_impl together with att_floats, the floats there are; launch_mlp clears it unless the launch takes part and sets att_blocks.
    float* att;
    int64_t att_floats;
    uint32_t att_blocks;     // ray blocks of the launch: tile it = depth slot it / att_blocks of ray block it % att_blocks
    uint32_t* dead_count;    // null, or the launch's counter of terminated tiles (profiling: mlp_api.hip)
};

// Workgroup iterations of a tuned forward launch: THE expression, shared by launch_mlp (grid size) and the kernels (loop bound).
// Linear order: wg_samples consecutive samples per tile.  ray_tiles: ceil(rays / (wg_samples / 16)) ray blocks x samples / 16 depth slots.
__host__ __device__ inline int64_t mlp_wg_iters(const MlpArgs& a, int wg_samples) {
    if (a.ray_tiles) {
        const int rays_per_tile = wg_samples / 16;
        return (a.n / a.samples + rays_per_tile - 1) / rays_per_tile * (a.samples / 16);
    }
    return (a.n + wg_samples - 1) / wg_samples;
}

// Kernel arguments of the backward (delta propagation) kernel.
struct MlpBwdArgs {
    const char* wstream;     // transposed A-operand stream: layers_dir.0^T | fc_feat^T | layers_xyz[L-2..0]^T
    const float* walpha;
    const float* wrgb;
    const float* radiance;   // (n,4) forward output (sigmoid(rgb), sigma)
    const float* grad_out;   // (n,4) dL/d(radiance)
    const uint64_t* mask_h;
    const uint64_t* mask_v;
    int64_t n, tiles;
    float* d_h;              // (L, n, H) gradient at layer1's output, then at every layers_xyz[i] pre-activation
    float* d_feat;           // (n, H)
    float* d_v;              // (n, H/2)
    float* d_last;           // (n, 4): pre-sigmoid rgb gradient, sigma gradient
    // generic-shape backward (mlp_device_g.h): ReLU' comes from the taped activations instead of masks
    const float* tape_h;     // (L, n, H)
    const float* tape_feat;  // (n, H)
    const float* tape_v;     // (n, H / 2)
    int32_t g_h, g_hd;       // real widths (row strides)
    int32_t stop_at_xyz0;    // tuned delta kernel: do not apply layers_xyz[0]^T (d_h[0] is not produced; NM_BACKWARD_STOP_AT_XYZ0)
};

// Flat addressing of the trainable tensors (index maps of the packed blob: TensorId << 24 | element, mlp_pack.h)
struct WeightPtrs { const float* p[T_COUNT]; };

// host-side description of one template instantiation of the fused forward kernel
struct MlpPlan {
    int H, FX, FD, NW, KCH, variant;
    int ring_bytes;
    void (*kernel)(const MlpArgs, const int, const int);
    int wg_samples;      // samples one workgroup evaluates per iteration
    int wg_per_cu;       // workgroups co-resident on a CU
    void (*kernel_flat)(const MlpArgs, const int, const int);   // the FLAT instantiation (use_viewdirs = 0 networks), or null
    int generic_nt;      // 0: a tuned plan for exactly (H, FX, FD) | NT: the generic family's width class (mlp_device_g.h), H = 16 NT
    void (*kernel_tape)(const MlpArgs, const int, const int);        // generic family: the taping forward ...
    void (*kernel_bwd)(const MlpBwdArgs, const int, const int);      // ... and the delta kernel (null for tuned plans: nerf_train.hip)
    void (*kernel_skip)(const MlpArgs, const int, const int);        // the instantiation that implements MlpArgs::skip_empty / ray_tiles
                                                                     // (mlp_kernel3<..., SKIP>), or null
};

// hipFuncAttributeMaxDynamicSharedMemorySize of a kernel, raised once per (device, kernel) and whenever a launch needs more --
// not on every launch --, under a lock (the attribute is per device; two host threads would otherwise race on it).
int ensure_dynamic_lds(const void* kernel, int bytes);

// ---- launch helpers shared by nerf_mlp.hip, nerf_train.hip and mlp_api.hip ---------------------------------------------
// The handle's device must be current for the launch (the stream belongs to it): a model on cuda:1 used from a process
// whose current device is cuda:0 is switched to for the call and switched back.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int want) {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != want && hipSetDevice(want) == hipSuccess) prev = cur;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

constexpr int TILE_QUEUE_SLOTS = 16, TILE_QUEUE_STRIDE = 32;    // words of nm_mlp::d_tile_queue; uint32_t between two of them

// Persistent-style grid for wg_iters workgroup iterations with `resident` workgroups co-resident on the chip: a few workgroups
// per CU queue so the tail is balanced, and the per-workgroup iteration count is even across the grid where possible.
inline unsigned persistent_grid(int64_t wg_iters, int64_t resident) {
    int64_t grid = wg_iters < resident * 4 ? wg_iters : resident * 4;
    if (wg_iters > grid) {
        const int64_t rounds = (wg_iters + grid - 1) / grid;
        grid = (wg_iters + rounds - 1) / rounds;
    }
    return (unsigned)grid;
}

// What a tuned kernel keeps in LDS behind its weight ring: every bias, fc_alpha and `head_floats` of colour-head rows (3 H / 2:
// fc_rgb; 3 H: the fc_out rows of a use_viewdirs = 0 network)
inline int tuned_cache_bytes(int H, int L, int head_floats) { return ((H * (1 + L) + H / 2 + 4 + H + head_floats) * 4 + 255) & ~255; }

// Dynamic LDS of a plan's forward kernels for an L-layer network: the generic family's own layout (g_lds_bytes, mlp_device_g.h),
// else the plan's ring + the tuned cache (nerf_mlp.hip)
int forward_lds_bytes(const MlpPlan& p, int H, int L, int head_floats);

// the handle's MlpArgs for MODE_RAYS (mlp_api.hip)
MlpArgs ray_mode_args(const nm_mlp* m, const float* d_origins, int origins_per_ray, const float* d_dirs, const float* d_t, int64_t rays,
                      int32_t samples, float* d_radiance);

// The general weight-gradient kernel (nerf_dw_g.hip) as a plain GEMM C = A^T B with a short contraction and a wide output:
// the engine of the layer-wise network path (nerf_layerwise.hip).  `partial` receives the (out_pad x in_pad) result.
struct DwgGemmGeometry { int wa, wb, ta, tb, nba, nbb, out_pad; int64_t in_pad; };
DwgGemmGeometry dwg_gemm_geometry(int out, int64_t in);
struct DwgEpilogue { float* out; const float* bias; const float* mask; int64_t ld; int act; };   // act: 0 none, 1 ReLU, 2 sigmoid
int dwg_gemm(const float* A, int out, int lda, const float* B, int64_t in, int64_t ldb, int rows, float* partial, hipStream_t stream,
             const DwgEpilogue* epilogue = nullptr);

// ---- what the two weight-gradient units share (nerf_dw.hip: the kernels tuned for the shipped shapes; nerf_dw_g.hip: any shape)
constexpr int DW_MAX_JOBS = 16;          // products of one shape in one launch (nm_weight_grad_batch)
constexpr int HEAD_MAX_PARTS = 512;      // sample slices of a head-gradient launch (sizes nm_head_grad_workspace_bytes_ex)
// One job of the order-fixed second pass over the per-workgroup partials (dw_reduce_batch_kernel / dw_reduce_g_kernel): out[o][out_col0 + c]
struct DwReduceJob { const float* partial; const float* partial_bias; float* out; float* out_bias; int32_t out_ld, out_col0; };
struct DwReduceBatch { DwReduceJob job[DW_MAX_JOBS]; };
// the heads' second pass (head_reduce_kernel, nerf_dw_g.hip): out[e] = sum_p partial[p][e], e < elems, and (out_bias non-null) the 4 bias sums
void launch_head_reduce(const float* partial, const float* partial_bias, int parts, int elems, float* out, float* out_bias,
                        hipStream_t stream);

// The render path's two network calls (ray_ops.hip: render_impl): rays from buffers (`gen` null) or from the pose, into WORKSPACE
// radiance that only the compositor reads, with MlpArgs::skip_empty set -- a sample with raw sigma <= 0 has alpha == weight == 0
// exactly (no noise is added on this path), so the rgb of a tile without density is written as zeros instead of being computed.
// `d_att` (att_floats floats of workspace): the ray-termination table of MlpArgs::att; the launch zeroes what it uses of it.
int nm_mlp_eval_render_internal(nm_mlp* m, const RayGen* gen, const float* d_origins, int origins_per_ray, const float* d_dirs,
                                const float* d_t, int64_t rays, int32_t samples, float* d_radiance, float* d_att, int64_t att_floats,
                                hipStream_t stream);

}  // namespace nm

// The opaque handle of the C ABI.
struct nm_mlp {
    nm_mlp_desc desc;
    int device;
    const nm::MlpPlan* plan;
    void* d_blob;            // one device allocation holding stream + bias + walpha + wrgb
    size_t blob_bytes;
    nm::MlpArgs base;        // weight-related fields filled in
    nm::MlpBwdArgs bwd;      // likewise for the backward kernel
    int32_t* d_index;        // source of every float of the blob (tensor id << 24 | element, -1 = 0.0f)
    size_t blob_floats;
    int64_t flops_full, flops_density;
    int num_cus;
    // opt-in "bf16x3" precision (mlp_device_b3.h): the same parameters as three bf16 planes per (k-block, tile) unit
    int precision;           // NM_PREC_F32 | NM_PREC_BF16X3
    void* d_stream_b3;       // units x 3 KiB
    float* d_tmp_b3;         // gathered fp32 image [unit][lane][8] the planes are split from
    int32_t* d_index_b3;
    size_t b3_units;
    void* d_enc_tab;         // generic plans: GEncArg[2][48]
    void* lw;                // layer-wise path (nerf_layerwise.h: LwNet*): networks beyond the fused families' limits, else null
    // stale-parameter guard (nm_mlp_weights_current): [0] = checksum of the packed image the LAST gather wrote, [1] = scratch
    // of a verification pass over the caller's live tensors (device, 2 x 8 bytes); how many gathers ran since create
    unsigned long long* d_check;
    int64_t refresh_count;
    // float offset, in the packed image, of the plain copies nm_mlp_linear_layer1_finish reads: layers_xyz[0].weight (H, H),
    // layer1.weight^T (dx, H), layer1.bias (H); 0: none (layer-wise path, one-layer networks)
    size_t plain_off;
    // Tile queues of the skipping render kernel (MlpArgs::tile_queue): TILE_QUEUE_SLOTS counter words, one cache line apart, allocated
    // with the handle.  Every such launch takes the next word in turn and zeroes it in stream order in front of the kernel, so launches
    // queued behind each other on one stream never share a live word, and launches on different streams do only when more than
    // TILE_QUEUE_SLOTS of them are in flight at once.
    uint32_t* d_tile_queue;
    mutable uint32_t tile_queue_turn;
};
