// Fused FlexibleNeRFModel forward for gfx950 (MI355X): positional encoding -> trunk -> sigma /
// feature -> view branch -> rgb in ONE kernel, fp32 MFMA (v_mfma_f32_16x16x4_f32), activations
// never leave registers, weights streamed L2 -> LDS with global_load_lds (direct-to-LDS DMA).
//
// The kernel template itself lives in mlp_device.h (shared with the training kernels of nerf_train.hip);
// this file holds the plan table and the launcher.
// Replaces (reference file:line under /root/reference/src):
//   nerf/modules.py:26-34      PositionalEncoding.forward      (expand, mul, view, sin, cos, cat)
//   nerf/models.py:60-80       FlexibleNeRFModel.forward       (12x addmm, 9x relu, 3x cat, sigmoid)
//   models/model_helpers.py:32-35 intervals_to_ray_points      (RAYS mode prologue)
//   mesh_nerf.py:37-40         grid point generation           (GRID mode prologue)
//
// Dataflow.  The network is evaluated transposed: out^T[feature][sample] = W[feature][k] * act^T[k][sample].
// One wave owns 16 samples (the 16 MFMA columns).  For v_mfma_f32_16x16x4_f32
//   A (weights): lane l holds W[row = l&15][k = l>>4]           (one VGPR)
//   B (activ.) : lane l holds act[k = l>>4][sample = l&15]      (one VGPR)
//   D          : lane l, reg r holds out[row = 4*(l>>4)+r][sample = l&15]
// so D of tile nt, register r is exactly the B operand of the NEXT layer's k-step s = 4*nt + r, in
// which lane group g = l>>4 supplies input feature k = 16*nt + 4*g + r.  The packer (mlp_pack.h: an
// index map built once on the host; mlp_api.hip: one gather kernel) permutes the weight columns accordingly, which
// is why bias+ReLU'd accumulators feed the next layer's MFMAs directly: no LDS round trip, no transposes, no HBM traffic for
// activations.  Weights (2.4 MB / model, L2-resident) are the only streamed operand:
// every workgroup pulls the same linear "A-operand stream" through a 2-deep LDS ring in 8-k-step
// chunks; each lane reads its operands for 4 consecutive output tiles with one conflict-free
// ds_read_b128.
//
// Roofline: MFMA (fp32 matrix peak 157.3 TFLOP/s).  593 408 MAC per sample for the 8x256 net; the
// kernel issues 9 280 MFMAs (1 024 MAC each) per 16-sample tile = 99.9 % useful work.
#include <cstdlib>
#include <iterator>
#include <vector>

#include "nm_internal.h"
#include "mlp_device.h"
#include "mlp_device_r3.h"
#include "mlp_device_b3.h"
#include "mlp_device_g.h"

namespace nm {

// ---- host side: plan table + launcher ------------------------------------------------------
template <int H, int FX, int FD, int NW, int KCH>
static MlpPlan make_plan() {
    return MlpPlan{H, FX, FD, NW, KCH, 0, 2 * Net<H, FX, FD, KCH>::LDSBUF, &mlp_kernel<H, FX, FD, NW, KCH, false>,
                   NW * 16, 8 / NW, &mlp_kernel<H, FX, FD, NW, KCH, false, true>, 0, nullptr, nullptr};
}

// SKIP: install the render path's instantiation (mlp_device_r3.h) -- where it stays within its sibling's register budget
template <int H, int FX, int FD, int NW, int KCH, bool SKIP = true>
static MlpPlan make_plan3() {
    return MlpPlan{H, FX, FD, NW, KCH, 0, 3 * Net<H, FX, FD, KCH>::LDSBUF, &mlp_kernel3<H, FX, FD, NW, KCH>,
                   NW * 16, 8 / NW, &mlp_kernel3<H, FX, FD, NW, KCH, true>, 0, nullptr, nullptr,
                   SKIP ? &mlp_kernel3<H, FX, FD, NW, KCH, false, SKIP> : nullptr};
}

// One plan per tuned shape.  The A/B variants of rounds 1 -- 5 that used to sit next to them (profiles/r0*_mlp_variants.json,
// DESIGN.md 3.1) were measured and retired: source last present in 94bb324.
static const MlpPlan g_tuned_plans[] = {
    // production: the round-2 kernel (3-slot ring, operand stream across boundaries, staggered scalar-addressed DMA)
    // for the 256- and 128-wide networks; 64-wide networks (2-tile view layer) keep the round-1 dataflow
    make_plan3<256, 10, 4, 8, 8>(),
    make_plan3<128, 10, 4, 8, 8>(),
    make_plan<64, 10, 4, 8, 8>(),
    make_plan3<256, 6, 4, 8, 8>(),
    // no SKIP instance for 128 / 6: it spills 12 VGPRs where this kernel spills 9, so that shape's render keeps this kernel
    make_plan3<128, 6, 4, 8, 8, false>(),
    make_plan<64, 6, 4, 8, 8>(),
};

// the generic-shape family (mlp_device_g.h), instantiated in nerf_mlp_generic_{a..d,s}.hip, in ascending width
void generic_plans_a(std::vector<MlpPlan>&);
void generic_plans_b(std::vector<MlpPlan>&);
void generic_plans_c(std::vector<MlpPlan>&);
void generic_plans_d(std::vector<MlpPlan>&);
void generic_plans_s(std::vector<MlpPlan>&);
void generic_plans_a_long(std::vector<MlpPlan>&);      // the same classes with two-part encoding stages (variant G_LONG_VARIANT)
void generic_plans_b_long(std::vector<MlpPlan>&);
void generic_plans_c_long(std::vector<MlpPlan>&);
void generic_plans_d_long(std::vector<MlpPlan>&);
void generic_plans_s_long(std::vector<MlpPlan>&);
void generic_plans_s_long_upper(std::vector<MlpPlan>&);

static const std::vector<MlpPlan>& all_plans() {
    static const std::vector<MlpPlan> plans = [] {
        std::vector<MlpPlan> v(std::begin(g_tuned_plans), std::end(g_tuned_plans));
        generic_plans_a(v); generic_plans_b(v); generic_plans_c(v); generic_plans_d(v); generic_plans_s(v);
        generic_plans_a_long(v); generic_plans_b_long(v); generic_plans_c_long(v); generic_plans_d_long(v); generic_plans_s_long(v); generic_plans_s_long_upper(v);
        return v;
    }();
    return plans;
}

// opt-in bf16x3 precision (mlp_device_b3.h)
struct B3Plan {
    int H, FX, FD;
    void (*kernel)(const MlpArgs, const int, const int);
    int chunk_units;                                            // units per ring slot (a stage must span two chunks)
};
static const B3Plan g_b3_plans[] = {
    {256, 10, 4, &mlp_kernel_b3<256, 10, 4, 8>, B3_CHUNK_UNITS},
    {256, 6, 4, &mlp_kernel_b3<256, 6, 4, 8>, B3_CHUNK_UNITS},
    // round 5: the narrower shipped shapes (the fern configs' 8x128, config 1's 4x64): smaller chunks so that every stage still
    // spans two of them; the same kernel otherwise
    {128, 10, 4, &mlp_kernel_b3<128, 10, 4, 8, 8>, 8},
    {128, 6, 4, &mlp_kernel_b3<128, 6, 4, 8, 8>, 8},
    {64, 10, 4, &mlp_kernel_b3<64, 10, 4, 8, 3>, 3},
    {64, 6, 4, &mlp_kernel_b3<64, 6, 4, 8, 3>, 3},
};
static const B3Plan* find_b3_plan(int H, int FX, int FD) {
    for (const B3Plan& p : g_b3_plans)
        if (p.H == H && p.FX == FX && p.FD == FD) return &p;
    return nullptr;
}
bool has_b3_kernel(int H, int FX, int FD) { return find_b3_plan(H, FX, FD) != nullptr; }

// A tuned plan when one is instantiated for exactly this shape (and the input itself is part of both encodings, which the
// tuned kernels' identity k-step assumes is laid out -- its weights may still be zero); otherwise the narrowest class of
// the generic family that holds the network; null only beyond the family's limits (mlp_api.hip says which).
const MlpPlan* find_mlp_plan(int H, int FX, int FD) {
    for (const MlpPlan& p : all_plans())
        if (!p.generic_nt && p.H == H && p.FX == FX && p.FD == FD) return &p;
    return nullptr;
}

// the narrowest class of the generic family that holds hidden_size H and whose LDS image (weight ring + every bias of an L-layer
// network + heads + tables) fits a CU; `long_encoding`: an encoding of more than G_ENC_STEPS k-steps (16 -- 31 functions) -- the
// instantiations with two-part encoding stages.  Null if there is none (the caller then takes the layer-wise path).
const MlpPlan* find_generic_plan(int H, int L, bool long_encoding) {
    const int want = long_encoding ? G_LONG_VARIANT : 0;
    for (const MlpPlan& p : all_plans())
        if (p.generic_nt && p.variant == want && p.H >= H && forward_lds_bytes(p, H, L, 0) <= 160 * 1024) return &p;
    return nullptr;
}

int mlp_plan_info(const MlpPlan* p, int* nw) {
    *nw = p->NW;
    return p->generic_nt ? 1000 + p->generic_nt : p->variant;     // generic family: 1000 + width class
}

int forward_lds_bytes(const MlpPlan& p, int H, int L, int head_floats) {
    if (p.generic_nt)      // padded widths, both head layouts, the two argument tables (mlp_device_g.h)
        return g_lds_bytes(p.ring_bytes, p.generic_nt, L, p.variant == G_LONG_VARIANT ? G_ENC_PARTS : 1);
    return p.ring_bytes + tuned_cache_bytes(H, L, head_floats);
}

static bool ray_termination_enabled() {
    const char* e = std::getenv("NM_RAY_TERMINATION");
    return !(e && e[0] == '0' && e[1] == 0);
}

int launch_mlp(const nm_mlp* m, const MlpArgs& args_in, int density_only, hipStream_t stream) {
    const MlpPlan* p = m->plan;
    if (args_in.n <= 0) return 0;
    // The render path's skip of tiles without density (MlpArgs::skip_empty) exists as mlp_kernel3's SKIP instantiation only: every other
    // family -- mlp_kernel<64, ...>, the generic kernels, bf16x3, the use_viewdirs = 0 heads -- evaluates every sample in linear order.
    MlpArgs args = args_in;
    if (!(args.skip_empty && p->kernel_skip && density_only == 0 && m->precision == NM_PREC_F32)) args.skip_empty = 0;
    args.ray_tiles = args.skip_empty && (args.mode == MODE_RAYS || args.mode == MODE_VIEW) && args.samples % 16 == 0;
    if (args.ray_tiles && mlp_wg_iters(args, p->wg_samples) > INT32_MAX) args.ray_tiles = 0;   // the kernel splits `it` in 32 bits
    // the skipping kernel claims its tiles from a 32-bit counter of the handle's
    if (args.skip_empty && (!m->d_tile_queue || mlp_wg_iters(args, p->wg_samples) > INT32_MAX)) args.skip_empty = args.ray_tiles = 0;
    args.tile_queue = nullptr;
    if (!args.skip_empty) args.skip_count = nullptr;
    float* const att = args.ray_tiles ? args.att : nullptr;       // ray termination: decided below, where the grid is known
    args.att = nullptr;
    args.att_blocks = 0;
    DeviceGuard guard(m->device);
    const int L = m->desc.num_layers, H = m->desc.hidden_size;
    NM_REQUIRE(density_only != 2 || (m->precision == NM_PREC_F32 && p->kernel_flat), "no kernel for use_viewdirs=0 networks in this plan");
    auto kernel = density_only == 2 ? p->kernel_flat : (args.skip_empty ? p->kernel_skip : p->kernel);
    if (m->precision == NM_PREC_BF16X3) {
        const B3Plan* b = find_b3_plan(H, m->desc.num_encoding_fn_xyz, m->desc.num_encoding_fn_dir);
        NM_REQUIRE(b && m->d_stream_b3, "no bf16x3 kernel for this network");
        const int lds_bytes = 3 * b->chunk_units * B3_UNIT + tuned_cache_bytes(H, L, 3 * H / 2 + 32);   // + the two band tables
        NM_REQUIRE(lds_bytes <= 160 * 1024, "LDS budget exceeded (bf16x3 ring + bias cache): too many layers");
        if (int rc = ensure_dynamic_lds((const void*)b->kernel, lds_bytes)) return rc;
        MlpArgs a = args;
        a.wstream = static_cast<const char*>(m->d_stream_b3);
        const unsigned grid = persistent_grid((a.n + 127) / 128, m->num_cus);
        hipLaunchKernelGGL(b->kernel, dim3(grid), dim3(512), lds_bytes, stream, a, L, density_only);
        NM_HIP_CHECK(hipGetLastError());
        return 0;
    }
    // a use_viewdirs = 0 network (mode 2) keeps three H-wide fc_out rows where fc_rgb's three H/2-wide ones go
    const int lds_bytes = forward_lds_bytes(*p, H, L, density_only == 2 ? 3 * H : 3 * H / 2);
    NM_REQUIRE(lds_bytes <= 160 * 1024, "LDS budget exceeded (ring + bias cache)");
    if (int rc = ensure_dynamic_lds((const void*)kernel, lds_bytes)) return rc;
    const int64_t wg_iters = mlp_wg_iters(args, p->wg_samples);
    unsigned grid = persistent_grid(wg_iters, (int64_t)m->num_cus * p->wg_per_cu);
    if (args.skip_empty) {
        // Tiles of unequal cost, drawn from a queue: exactly the workgroups that are resident at once (mlp_kernel3's launch bounds
        // put two of the networks up to 128 wide on a CU), each running until the queue is empty.  The counter is zero when the
        // kernel starts: set in stream order, no allocation and no host synchronisation here.
        const int64_t resident = (int64_t)m->num_cus * p->wg_per_cu * (p->H <= 128 ? 2 : 1);
        grid = (unsigned)(wg_iters < resident ? wg_iters : resident);
        args.tile_queue = m->d_tile_queue + (size_t)(__atomic_fetch_add(&m->tile_queue_turn, 1u, __ATOMIC_RELAXED) % TILE_QUEUE_SLOTS) * TILE_QUEUE_STRIDE;
        NM_HIP_CHECK(hipMemsetAsync(args.tile_queue, 0, sizeof(uint32_t), stream));
        // Ray termination (mlp_device_r3.h): only where a ray block's tile of the slot before has long been evaluated when a tile is
        // claimed in slot-major order, that is with at least two ray blocks per resident workgroup; below that the launch is what it
        // was (block-major order, no table).  The 128-wide skip kernel does not have it (mlp_device_r3.h).  NM_RAY_TERMINATION=0
        // switches it off (A/B in one build).
        const int64_t depth_slots = args.samples / 16, ray_blocks = att ? wg_iters / depth_slots : 0;
        const int64_t table = depth_slots * ray_blocks * p->NW;
        if (att && p->H > 128 && ray_blocks >= 2 * (int64_t)grid && table <= args.att_floats && ray_termination_enabled()) {
            args.att = att;
            args.att_blocks = (uint32_t)ray_blocks;
            NM_HIP_CHECK(hipMemsetAsync(att, 0, (size_t)table * sizeof(float), stream));
        }
    }
    if (!args.att) args.dead_count = nullptr;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(p->NW * 64), lds_bytes, stream, args, (int)m->desc.num_layers, density_only);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace nm
