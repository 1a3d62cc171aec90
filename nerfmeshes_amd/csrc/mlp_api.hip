// C ABI for the fused MLP: weight packing (torch.nn.Linear layout -> MFMA A-operand stream),
// handle lifetime, and the three entry points that launch nerf_mlp.hip's kernel.
#include <cstring>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "nm_internal.h"
#include "mlp_device_g.h"
#include "nerf_layerwise.h"

namespace nm {

static thread_local std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }

int ensure_dynamic_lds(const void* kernel, int bytes) {
    NM_REQUIRE(bytes <= 160 * 1024, "LDS budget exceeded");
    static std::mutex lock;
    static std::map<std::pair<int, const void*>, int> have;
    int dev = 0;
    NM_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> guard(lock);
    int& cur = have[{dev, kernel}];
    if (cur < bytes) {
        NM_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        cur = bytes;
    }
    return 0;
}

const MlpPlan* find_mlp_plan(int H, int FX, int FD);
const MlpPlan* find_generic_plan(int H, int L, bool long_encoding);
bool has_b3_kernel(int H, int FX, int FD);
int mlp_plan_info(const MlpPlan* p, int* nw);
int launch_mlp(const nm_mlp* m, const MlpArgs& args, int density_only, hipStream_t stream);

// ---- layer-wise path (nerf_layerwise.hip): networks beyond the fused families' limits -----------------------------------
// A plan that launches nothing by itself: launch_mlp_timed / the training entry points route such a handle to the layer-wise
// evaluator.  nm_mlp_kernel_variant reports 2000.
static const MlpPlan g_layerwise_plan = {0, 0, 0, 8, 0, 2000, 0, nullptr, 0, 0, nullptr, 0, nullptr, nullptr};

// the per-argument table of one encoding (GEncArg: band, coordinate)
static void fill_enc_table(float* tab /* [parts * G_ENC_ARGS][2] */, int parts, int F, const float* bands) {
    for (int a = 0; a < parts * G_ENC_ARGS; ++a) {
        const bool real = F > 0 && a < 3 * F;
        const int32_t coord = real ? a / F : 0;
        tab[2 * a] = real ? bands[a % F] : 0.0f;
        memcpy(&tab[2 * a + 1], &coord, 4);
    }
}

// fp32 image [unit][lane][8] -> three planes of packed bf16 [unit][plane][lane][8]: x1 = bf16(x), x2 = bf16(x - x1), ...
__global__ void split_b3_kernel(const float* __restrict__ src, uint4* __restrict__ dst, int64_t units) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;     // (unit, lane)
    if (t >= units * 64) return;
    const int64_t unit = t >> 6;
    const int lane = (int)(t & 63);
    const float* v = src + t * 8;
    uint32_t p[3][4];
    for (int q = 0; q < 4; ++q) {
        const float x = v[2 * q], y = v[2 * q + 1];
        auto pack = [](float a, float b) {
            typedef float f2 __attribute__((ext_vector_type(2)));
            typedef __bf16 b2 __attribute__((ext_vector_type(2)));
            const f2 f = {a, b};
            return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, b2));
        };
        p[0][q] = pack(x, y);
        const float rx = x - __uint_as_float(p[0][q] << 16), ry = y - __uint_as_float(p[0][q] & 0xffff0000u);
        p[1][q] = pack(rx, ry);
        const float sx = rx - __uint_as_float(p[1][q] << 16), sy = ry - __uint_as_float(p[1][q] & 0xffff0000u);
        p[2][q] = pack(sx, sy);
    }
    for (int k = 0; k < 3; ++k) dst[(unit * 3 + k) * 64 + lane] = uint4{p[k][0], p[k][1], p[k][2], p[k][3]};
}

// blob[i] = parameter element index[i] names (or 0): the whole packing, on the device.  Every pass also folds what it read into
// a 64-bit checksum of the packed image (sum over i of bits(value_i) * (2 i + 1), integer arithmetic: order-free, so plain
// atomics keep it deterministic): WRITE = the gather itself, !WRITE = a verification pass over the caller's LIVE tensors that
// touches nothing (nm_mlp_weights_current: "is the packed copy still what these tensors hold?").
template <bool WRITE>
__global__ __launch_bounds__(256) void gather_parameters(const int32_t* __restrict__ index, WeightPtrs ptrs, float* __restrict__ blob,
                                                         int64_t count, unsigned long long* __restrict__ check) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long term = 0;
    if (i < count) {
        const int32_t s = index[i];
        const float v = s < 0 ? 0.0f : ptrs.p[s >> 24][s & 0xffffff];
        if (WRITE) blob[i] = v;
        term = (unsigned long long)__float_as_uint(v) * (unsigned long long)(2 * i + 1);
    }
    if (!check) return;
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)term, off), hi = __shfl_xor((unsigned)(term >> 32), off);
        term += ((unsigned long long)hi << 32) | lo;
    }
    __shared__ unsigned long long part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = term;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(check, (part[0] + part[1]) + (part[2] + part[3]));
}

// the inverse of the gather for one tensor: out[element] = blob[i] wherever index[i] names that tensor (a parameter element sits in
// the packed image at least once -- forward stream, transposed stream --, always with the same value)
__global__ __launch_bounds__(256) void scatter_tensor(const int32_t* __restrict__ index, const float* __restrict__ blob, int64_t count,
                                                      int tensor, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int32_t s = index[i];
    if (s >= 0 && (s >> 24) == tensor) out[s & 0xffffff] = blob[i];
}

// [layer1.weight | layer1.bias]^T out of the packed image: out[(j, i)] = W1[i][j] for j < dx, out[(dx, i)] = b1[i]; (dx + 1, H) row-major
__global__ __launch_bounds__(256) void scatter_layer1_t(const int32_t* __restrict__ index, const float* __restrict__ blob, int64_t count,
                                                        int H, int dx, float* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= count) return;
    const int32_t s = index[p];
    if (s < 0) return;
    const int tensor = s >> 24, e = s & 0xffffff;
    if (tensor == T_L1W) out[(int64_t)(e % dx) * H + e / dx] = blob[p];
    else if (tensor == T_L1B) out[(int64_t)dx * H + e] = blob[p];
}

// The caller's tensors behind the handle's network (the layer walk: mlp_pack.h); every one of them must be there.
static int weight_pointers(const nm_mlp_desc& d, const nm_mlp_weights& w, WeightPtrs& p, const char* who) {
    std::memset(&p, 0, sizeof(p));
    for (const Linear& l : network_layers(d))
        for (int t : {l.w, l.b}) {
            p.p[t] = weight_tensor(w, t);
            if (!p.p[t]) {
                set_error(std::string(who) + ": missing tensor [!used || ptrs.p[t]]");
                return 2;
            }
        }
    return 0;
}

static int launch_gather(nm_mlp* m, const WeightPtrs& ptrs, hipStream_t stream) {
    const int64_t n = (int64_t)m->blob_floats;
    if (m->d_check) NM_HIP_CHECK(hipMemsetAsync(m->d_check, 0, 8, stream));
    hipLaunchKernelGGL(gather_parameters<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, m->d_index, ptrs,
                       static_cast<float*>(m->d_blob), n, m->d_check);
    if (m->precision == NM_PREC_BF16X3) {
        const int64_t nb = (int64_t)m->b3_units * 512;
        hipLaunchKernelGGL(gather_parameters<true>, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, stream, m->d_index_b3, ptrs,
                           m->d_tmp_b3, nb, static_cast<unsigned long long*>(nullptr));
        hipLaunchKernelGGL(split_b3_kernel, dim3((unsigned)((m->b3_units * 64 + 255) / 256)), dim3(256), 0, stream,
                           m->d_tmp_b3, static_cast<uint4*>(m->d_stream_b3), (int64_t)m->b3_units);
    }
    NM_HIP_CHECK(hipGetLastError());
    ++m->refresh_count;
    return 0;
}

MlpArgs ray_mode_args(const nm_mlp* m, const float* d_origins, int origins_per_ray, const float* d_dirs, const float* d_t, int64_t rays,
                      int32_t samples, float* d_radiance) {
    MlpArgs a = m->base;
    a.mode = MODE_RAYS;
    a.a = d_origins; a.b = d_dirs; a.c = d_t;
    a.origins_per_ray = origins_per_ray; a.samples = samples;
    a.n = rays * samples; a.out = d_radiance;
    return a;
}

// ---- optional per-launch timing of the dominant kernel (bench.py's roofline leg) ---------------
// A launch that may skip the colour branch of tiles without density (MlpArgs::skip_empty) counts them in a device word of its own:
// `slot` indexes g_prof_skips (-1: the launch cannot skip), `skip_flops` is what one skipped tile did not execute.  Tiles that ray
// termination did not evaluate at all (MlpArgs::att) are counted in the word PROF_SKIP_SLOTS behind it; each is `dead_flops` less.
struct ProfRec { hipEvent_t start, stop; double flops; int slot, device; double skip_flops, dead_flops; };
static bool g_prof_on = false;
static std::vector<ProfRec> g_prof;
constexpr int PROF_SKIP_SLOTS = 1 << 20;          // skipping launches per device between two reads (4 MB of counters per device)
struct ProfSkips { uint32_t* d = nullptr; int used = 0; };
static std::vector<ProfSkips> g_prof_skips;       // one array per device, allocated (zeroed) by nm_mlp_profile_enable(1), never in a launch

// density_only: 0 full evaluation | 1 sigma only.  For a use_viewdirs = 0 handle the full evaluation is the kernels' mode 2:
// the trunk as in mode 1, then all four rows of fc_out (models.py:77-79).
static int launch_mlp_timed(const nm_mlp* m, const MlpArgs& a, int density_only, hipStream_t stream) {
    if (!density_only && !m->desc.use_viewdirs) density_only = 2;
    auto launch = [&]() { return m->lw ? layerwise_forward(const_cast<nm_mlp*>(m), a, density_only, stream) : launch_mlp(m, a, density_only, stream); };
    if (!g_prof_on || a.n <= 0) return launch();
    ProfRec r;
    NM_HIP_CHECK(hipEventCreate(&r.start));
    NM_HIP_CHECK(hipEventCreate(&r.stop));
    r.flops = (double)a.n * (double)(density_only == 1 ? m->flops_density : m->flops_full);
    r.slot = -1; r.device = -1; r.skip_flops = 0; r.dead_flops = 0;
    MlpArgs counted = a;
    if (a.skip_empty && !density_only && !m->lw) {
        ProfSkips* ps = m->device >= 0 && m->device < (int)g_prof_skips.size() ? &g_prof_skips[m->device] : nullptr;
        if (ps && ps->d && ps->used < PROF_SKIP_SLOTS) {
            r.slot = ps->used++; r.device = m->device;
            r.skip_flops = (double)m->plan->wg_samples * (double)(m->flops_full - m->flops_density);
            r.dead_flops = (double)m->plan->wg_samples * (double)m->flops_full;
            counted.skip_count = ps->d + r.slot;
            counted.dead_count = ps->d + PROF_SKIP_SLOTS + r.slot;
        } else {
            // more than PROF_SKIP_SLOTS skipping launches since the last read (documented in the public header): without a
            // counter the launch evaluates every tile, so that it executes every FLOP it is credited with
            counted.skip_empty = 0;
        }
    }
    NM_HIP_CHECK(hipEventRecord(r.start, stream));
    const int rc = m->lw ? launch() : launch_mlp(m, counted, density_only, stream);
    NM_HIP_CHECK(hipEventRecord(r.stop, stream));
    g_prof.push_back(r);
    return rc;
}

// ---- nm_mlp_create_ex, step by step ------------------------------------------------------------------------------------
static int validate_create(const nm_mlp_desc& d, const nm_mlp_weights* w, int precision, bool force_generic) {
    NM_REQUIRE(precision == NM_PREC_F32 || precision == NM_PREC_BF16X3, "unknown precision");
    NM_REQUIRE(!force_generic || precision == NM_PREC_F32, "NM_KERNEL_GENERIC goes with NM_PREC_F32");
    NM_REQUIRE(d.use_viewdirs == 0 || d.use_viewdirs == 1, "use_viewdirs is 0 or 1");
    const bool no_view = d.use_viewdirs == 0;      // models.py:77-79: trunk -> fc_out (4 rows), no view branch
    NM_REQUIRE(!no_view || precision == NM_PREC_F32, "use_viewdirs=0 networks run in fp32 only");
    NM_REQUIRE(d.num_layers >= 2 && d.num_layers <= 32, "num_layers out of range");
    NM_REQUIRE(d.skip_step >= 1, "skip_step must be >= 1");
    NM_REQUIRE(d.hidden_size >= 1 && d.num_encoding_fn_xyz >= 0 && d.num_encoding_fn_dir >= 0, "negative network dimension");
    NM_REQUIRE(no_view || d.hidden_size >= 2, "hidden_size = 1 with view directions: layers_dir[0] would have hidden_size // 2 = 0 rows");
    NM_REQUIRE(d.num_encoding_fn_xyz > 0 || d.include_input_xyz,
               "the xyz encoding is empty (num_encoding_fn_xyz = 0 without include_input_xyz): layer1 would have no input");
    // every tensor the packer will read, checked before anything dereferences one
    NM_REQUIRE(w->layer1_w && w->layer1_b && w->fc_alpha_w && w->fc_alpha_b && w->fc_rgb_w && w->fc_rgb_b, "missing weight tensor");
    NM_REQUIRE(no_view || (w->fc_feat_w && w->fc_feat_b && w->layers_dir0_w && w->layers_dir0_b), "missing view-branch weight tensor");
    NM_REQUIRE(w->layers_xyz_w && w->layers_xyz_b, "missing layers_xyz tensor tables");
    for (int i = 0; i < d.num_layers - 1; ++i)
        NM_REQUIRE(w->layers_xyz_w[i] && w->layers_xyz_b[i], "missing layers_xyz weight tensor");
    NM_REQUIRE(d.num_encoding_fn_xyz == 0 || w->freq_xyz, "missing xyz frequency bands");
    NM_REQUIRE(no_view || d.num_encoding_fn_dir == 0 || w->freq_dir, "missing direction frequency bands");
    return 0;
}

// A tuned plan for exactly this shape, else the generic family (mlp_device_g.h): every shape FlexibleNeRFModel's
// constructor accepts up to hidden_size 512 and 24 k-steps per encoding, else the layer-wise plan.  (A network without view
// directions has no direction encoding: any tuned kernel of that width / xyz encoding runs it.)
static int choose_plan(const nm_mlp_desc& d, int precision, bool force_generic, const MlpPlan** out) {
    static const char* const b3_shapes = "precision bf16x3 is instantiated for hidden_size 64 / 128 / 256 with 6 or 10 xyz / 4 direction frequencies only";
    const int H = d.hidden_size, L = d.num_layers, FX = d.num_encoding_fn_xyz, FD = d.num_encoding_fn_dir;
    const bool no_view = d.use_viewdirs == 0;
    const MlpPlan* plan = (!force_generic && FX <= MAX_FREQ_XYZ && (no_view || FD <= MAX_FREQ_DIR)) ? find_mlp_plan(H, FX, no_view ? 4 : FD) : nullptr;
    if (!plan) {
        const int steps_x = (3 * FX + 1) / 2 + (d.include_input_xyz ? 1 : 0), steps_d = (3 * FD + 1) / 2 + (d.include_input_dir ? 1 : 0);
        const int steps = (!no_view && steps_d > steps_x) ? steps_d : steps_x;
        const bool long_encoding = steps > G_ENC_PARTS * G_ENC_STEPS;      // beyond what the fused kernels take even in two parts
        plan = find_generic_plan(H, L, steps > G_ENC_STEPS);
        if (precision != NM_PREC_F32) {
            set_error(b3_shapes);
            return 3;
        }
        if (!plan || long_encoding) {
            // beyond the fused families -- hidden_size > 512 (half of a wider layer's activations does not fit the register file of
            // one wavefront), an encoding of more than 48 MFMA k-steps (31 functions), or so many layers that their biases no longer
            // fit the LDS next to the weight ring --: the layer-wise path (nerf_layerwise.hip)
            if (FX > LW_MAX_FREQ || (!no_view && FD > LW_MAX_FREQ)) {
                set_error("an encoding of " + std::to_string(FX) + " / " + std::to_string(FD) + " functions: the limit is " +
                          std::to_string(LW_MAX_FREQ) + " per input (frequency 2^31 is past fp32's integer range)");
                return 3;
            }
            if ((int64_t)H * (H + encoded_width(FX, d.include_input_xyz)) >= (1 << 24)) {
                set_error("hidden_size=" + std::to_string(H) + ": a weight matrix of more than 2^24 elements exceeds the packer's index map");
                return 3;
            }
            plan = &g_layerwise_plan;
        }
    }
    if (precision == NM_PREC_BF16X3 && !has_b3_kernel(H, FX, FD)) {
        set_error(b3_shapes);
        return 3;
    }
    *out = plan;
    return 0;
}

// the packed images as index maps (mlp_pack.h); `lw`: the layer-wise handle's description, filled here
struct PackedIndex { std::vector<int32_t> index, index_b3; BlobLayout lay; size_t plain_off; };

static void build_indices(const nm_mlp_desc& d, const MlpPlan& plan, int precision, LwNet* lw, PackedIndex& px) {
    px.lay = BlobLayout{};
    if (lw) build_index_layerwise(px.index, d, lw);
    else px.lay = build_index_f32(px.index, d, StreamGeometry{plan.generic_nt ? plan.generic_nt : d.hidden_size / 16, plan.KCH, plan.generic_nt == 0});
    if (precision == NM_PREC_BF16X3) build_index_b3(px.index_b3, d);         // opt-in: the same stages as units of (k-block, tile)
    px.plain_off = append_plain_copies(px.index, d);
}

static int upload_indices(nm_mlp* m, const PackedIndex& px) {
    m->plain_off = px.plain_off;
    m->blob_floats = px.index.size();
    m->blob_bytes = px.index.size() * 4;
    NM_HIP_CHECK(hipMalloc(&m->d_blob, m->blob_bytes));
    NM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&m->d_check), 16));
    NM_HIP_CHECK(hipMemset(m->d_check, 0, 16));
    if (m->plan->kernel_skip) NM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&m->d_tile_queue), TILE_QUEUE_SLOTS * TILE_QUEUE_STRIDE * sizeof(uint32_t)));
    NM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&m->d_index), m->blob_bytes));
    NM_HIP_CHECK(hipMemcpy(m->d_index, px.index.data(), m->blob_bytes, hipMemcpyHostToDevice));
    if (m->precision == NM_PREC_BF16X3) {
        const std::vector<int32_t>& index_b3 = px.index_b3;
        m->b3_units = index_b3.size() / 512;
        NM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&m->d_index_b3), index_b3.size() * 4));
        NM_HIP_CHECK(hipMemcpy(m->d_index_b3, index_b3.data(), index_b3.size() * 4, hipMemcpyHostToDevice));
        NM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&m->d_tmp_b3), index_b3.size() * 4));
        NM_HIP_CHECK(hipMalloc(&m->d_stream_b3, m->b3_units * 3072));
    }
    return 0;
}

// the weight-related fields of MlpArgs / MlpBwdArgs, and a generic plan's encoding table
static int fill_args(nm_mlp* m, const nm_mlp_weights* w, const BlobLayout& lay) {
    const nm_mlp_desc& d = m->desc;
    const int H = d.hidden_size, FX = d.num_encoding_fn_xyz, FD = d.num_encoding_fn_dir;
    const bool no_view = d.use_viewdirs == 0;
    const float* base = static_cast<const float*>(m->d_blob);
    MlpArgs& a = m->base;
    a.wstream = reinterpret_cast<const char*>(base);
    a.bias = base + lay.off_bias;
    a.walpha = base + lay.off_wa;
    a.wrgb = base + lay.off_wr;
    for (int f = 0; f < FX && f < MAX_FREQ_XYZ; ++f) a.bands_xyz[f] = w->freq_xyz[f];
    for (int f = 0; f < FD && f < MAX_FREQ_DIR && !no_view; ++f) a.bands_dir[f] = w->freq_dir[f];
    a.skip_mask = lay.skip_mask;
    if (m->plan->generic_nt) {      // the encodings' run-time description (mlp_device_g.h)
        const int parts = m->plan->variant == G_LONG_VARIANT ? G_ENC_PARTS : 1;     // [xyz, dir][parts][G_ENC_ARGS] (band, coordinate)
        float tab[2 * 2 * G_ENC_PARTS * G_ENC_ARGS];
        fill_enc_table(tab, parts, FX, w->freq_xyz);
        fill_enc_table(tab + 2 * parts * G_ENC_ARGS, parts, no_view ? 0 : FD, w->freq_dir);
        const size_t tab_bytes = sizeof(float) * 2 * 2 * parts * G_ENC_ARGS;
        NM_HIP_CHECK(hipMalloc(&m->d_enc_tab, tab_bytes));
        NM_HIP_CHECK(hipMemcpy(m->d_enc_tab, tab, tab_bytes, hipMemcpyHostToDevice));
        a.g_tab = m->d_enc_tab;
        a.g_nsx = (3 * FX + 1) / 2; a.g_idx = d.include_input_xyz ? 1 : 0; a.g_chx = lay.chx;
        a.g_nsd = no_view ? 0 : (3 * FD + 1) / 2; a.g_idd = (!no_view && d.include_input_dir) ? 1 : 0; a.g_chd = lay.chd;
        a.g_h = H; a.g_hd = H / 2;
        m->bwd.g_h = H; m->bwd.g_hd = H / 2;
    }
    m->bwd.wstream = reinterpret_cast<const char*>(base + lay.off_bwd);
    m->bwd.walpha = a.walpha;
    m->bwd.wrgb = a.wrgb;
    m->flops_full = 2 * mlp_macs(d, false);
    m->flops_density = 2 * mlp_macs(d, true);
    return 0;
}

// fill the blob from the host tensors: stage them on the device (*d_flat: the caller frees it) and run the same gather
// nm_mlp_refresh uses
static int stage_and_gather(nm_mlp* m, const nm_mlp_weights* w, float** d_flat) {
    const std::vector<Linear> layers = network_layers(m->desc);
    std::vector<float> flat;
    std::vector<size_t> offs(T_COUNT, 0);
    auto stage = [&](int t, size_t count) {
        const float* src = weight_tensor(*w, t);
        offs[t] = flat.size();
        flat.insert(flat.end(), src, src + count);
    };
    for (const Linear& l : layers) { stage(l.w, (size_t)l.out * l.in); stage(l.b, l.out); }
    NM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(d_flat), flat.size() * 4));
    NM_HIP_CHECK(hipMemcpy(*d_flat, flat.data(), flat.size() * 4, hipMemcpyHostToDevice));
    WeightPtrs ptrs;
    std::memset(&ptrs, 0, sizeof(ptrs));
    for (const Linear& l : layers) { ptrs.p[l.w] = *d_flat + offs[l.w]; ptrs.p[l.b] = *d_flat + offs[l.b]; }
    int rc = launch_gather(m, ptrs, nullptr);
    if (rc == 0 && hipStreamSynchronize(nullptr) != hipSuccess) { set_error("parameter gather failed"); rc = 1; }
    return rc;
}

}  // namespace nm

using namespace nm;

extern "C" {

const char* nm_last_error(void) { return g_error.c_str(); }
int nm_abi_version(void) { return NM_ABI_VERSION; }
int nm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return -1;
    return n;
}

int nm_mlp_profile_enable(int on) {
    if (on && g_prof_skips.empty()) {             // a handle may live on any device: counters on each of them
        int count = 0;
        NM_HIP_CHECK(hipGetDeviceCount(&count));
        std::vector<ProfSkips> slots(count);
        for (int dev = 0; dev < count; ++dev) {
            DeviceGuard guard(dev);
            NM_HIP_CHECK(hipMalloc(&slots[dev].d, 2 * PROF_SKIP_SLOTS * sizeof(uint32_t)));      // skipped | terminated
            NM_HIP_CHECK(hipMemset(slots[dev].d, 0, 2 * PROF_SKIP_SLOTS * sizeof(uint32_t)));
        }
        g_prof_skips.swap(slots);
    }
    g_prof_on = on != 0;
    return 0;
}

int nm_mlp_profile_read(int64_t* launches, double* total_ms, double* total_flops) {
    return nm_mlp_profile_read_tiles(launches, total_ms, total_flops, nullptr, nullptr);
}

int nm_mlp_profile_read_tiles(int64_t* launches, double* total_ms, double* total_flops, int64_t* skipped_tiles, int64_t* terminated_tiles) {
    double ms = 0, fl = 0;
    int64_t n_skipped = 0, n_dead = 0;
    std::vector<uint32_t> skips, deads;
    for (ProfRec& r : g_prof) {
        NM_HIP_CHECK(hipEventSynchronize(r.stop));
        float t = 0;
        NM_HIP_CHECK(hipEventElapsedTime(&t, r.start, r.stop));
        ms += t; fl += r.flops;
        (void)hipEventDestroy(r.start); (void)hipEventDestroy(r.stop);
    }
    for (int dev = 0; dev < (int)g_prof_skips.size(); ++dev) {   // every counted launch has finished: its stop event was waited for above
        ProfSkips& ps = g_prof_skips[dev];
        if (ps.used == 0) continue;
        DeviceGuard guard(dev);
        skips.resize(ps.used);
        NM_HIP_CHECK(hipMemcpy(skips.data(), ps.d, skips.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        NM_HIP_CHECK(hipMemset(ps.d, 0, skips.size() * sizeof(uint32_t)));
        deads.resize(ps.used);
        NM_HIP_CHECK(hipMemcpy(deads.data(), ps.d + PROF_SKIP_SLOTS, deads.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        NM_HIP_CHECK(hipMemset(ps.d + PROF_SKIP_SLOTS, 0, deads.size() * sizeof(uint32_t)));
        for (const ProfRec& r : g_prof)
            if (r.slot >= 0 && r.device == dev) {
                fl -= (double)skips[r.slot] * r.skip_flops + (double)deads[r.slot] * r.dead_flops;
                n_skipped += skips[r.slot];
                n_dead += deads[r.slot];
            }
        ps.used = 0;
    }
    if (skipped_tiles) *skipped_tiles = n_skipped;
    if (terminated_tiles) *terminated_tiles = n_dead;
    if (launches) *launches = (int64_t)g_prof.size();
    if (total_ms) *total_ms = ms;
    if (total_flops) *total_flops = fl;
    g_prof.clear();
    return 0;
}

int nm_mlp_create(const nm_mlp_desc* desc, const nm_mlp_weights* w, int device, nm_mlp** out) {
    return nm_mlp_create_ex(desc, w, device, NM_PREC_F32, out);
}

int nm_mlp_precision(const nm_mlp* m) { return m ? m->precision : -1; }

int nm_mlp_create_ex(const nm_mlp_desc* desc, const nm_mlp_weights* w, int device, int precision, nm_mlp** out) {
    NM_REQUIRE(desc && w && out, "null argument");
    const bool force_generic = (precision & NM_KERNEL_GENERIC) != 0;
    precision &= ~NM_KERNEL_GENERIC;
    const nm_mlp_desc& d = *desc;
    if (int rc = validate_create(d, w, precision, force_generic)) return rc;
    const MlpPlan* plan = nullptr;
    if (int rc = choose_plan(d, precision, force_generic, &plan)) return rc;
    LwNet* lw_net = nullptr;
    if (plan == &g_layerwise_plan) {
        lw_net = new LwNet();
        std::memset(lw_net, 0, sizeof(*lw_net));
    }
    PackedIndex px;
    build_indices(d, *plan, precision, lw_net, px);

    nm_mlp* m = new nm_mlp();
    std::memset(m, 0, sizeof(*m));
    m->desc = d;
    m->device = device;
    m->plan = plan;
    m->precision = precision;
    m->lw = lw_net;          // freed with the handle (also by the rollback below)
    if (lw_net) {
        for (int f = 0; f < d.num_encoding_fn_xyz; ++f) lw_net->bands_x[f] = w->freq_xyz[f];
        for (int f = 0; f < d.num_encoding_fn_dir && d.use_viewdirs; ++f) lw_net->bands_d[f] = w->freq_dir[f];
    }
    int prev_device = -1;
    (void)hipGetDevice(&prev_device);
    // every early return below (a failed hip call) gives back the half-built handle and the staging buffer and leaves the
    // caller's device current
    struct Rollback {
        nm_mlp* m; float* d_flat; int prev, dev; bool keep;
        ~Rollback() {
            if (d_flat) (void)hipFree(d_flat);
            if (!keep) nm_mlp_destroy(m);
            if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
        }
    } rollback{m, nullptr, prev_device, device, false};
    NM_HIP_CHECK(hipSetDevice(device));
    hipDeviceProp_t prop;
    NM_HIP_CHECK(hipGetDeviceProperties(&prop, device));
    m->num_cus = prop.multiProcessorCount;
    if (int rc = upload_indices(m, px)) return rc;
    if (int rc = fill_args(m, w, px.lay)) return rc;
    if (int rc = stage_and_gather(m, w, &rollback.d_flat)) return rc;
    rollback.keep = true;
    *out = m;
    return 0;
}

int nm_mlp_refresh(nm_mlp* m, const nm_mlp_weights* d_weights, void* stream) {
    NM_REQUIRE(m && d_weights, "null argument");
    WeightPtrs ptrs;
    if (int rc = weight_pointers(m->desc, *d_weights, ptrs, "nm_mlp_refresh")) return rc;
    return launch_gather(m, ptrs, static_cast<hipStream_t>(stream));
}

int64_t nm_mlp_refresh_count(const nm_mlp* m) { return m ? m->refresh_count : -1; }

// Both products of the linearity identities in one launch: with S = [sums (H, dx) | colsum (H)]
//     l1w[i][j] = sum_k W0[k][i] sums[k][j],   l1b[i] = sum_k W0[k][i] colsum[k],   x0w[o][i] = sum_j sums[o][j] W1[i][j] + colsum[o] b1[i]
// one thread per output element, fixed summation order; W0, W1^T, b1 are the plain copies behind the packed image (coalesced or
// broadcast reads, everything L2-resident).  8.4 M multiply-adds at 8x256: launch-sized work -- it replaces two exports, three
// copies and two weight-gradient launches with their reductions (about 90 us of launches in an eager iteration).
__global__ __launch_bounds__(256) void linear_layer1_finish_kernel(const float* __restrict__ w0, const float* __restrict__ w1t,
                                                                   const float* __restrict__ b1, const float* __restrict__ sums, int ld,
                                                                   const float* __restrict__ colsum, int H, int dx, float* __restrict__ l1w,
                                                                   float* __restrict__ l1b, float* __restrict__ x0w) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int n_x0 = H * H;
    if (t < n_x0) {                       // x0w: thread (o, i), i fastest: sums[o][j] is a broadcast, w1t[j][i] coalesced
        const int o = t / H, i = t - o * H;
        float s = 0.0f;
#pragma unroll 8
        for (int j = 0; j < dx; ++j) s = fmaf(sums[(int64_t)o * ld + j], w1t[j * H + i], s);
        x0w[t] = fmaf(colsum[o], b1[i], s);
    } else if (t < n_x0 + (dx + 1) * H) { // l1: thread (j, i), i fastest: w0[k][i] coalesced, sums[k][j] a broadcast
        const int e = t - n_x0, j = e / H, i = e - j * H;
        float s = 0.0f;
        if (j < dx) {
#pragma unroll 8
            for (int k = 0; k < H; ++k) s = fmaf(w0[k * H + i], sums[(int64_t)k * ld + j], s);
            l1w[i * dx + j] = s;
        } else {
#pragma unroll 8
            for (int k = 0; k < H; ++k) s = fmaf(w0[k * H + i], colsum[k], s);
            l1b[i] = s;
        }
    }
}

int nm_mlp_linear_layer1_finish(nm_mlp* m, const float* d_sums, int32_t ld, const float* d_colsum, float* d_l1w, float* d_l1b,
                                float* d_x0w, void* stream_) {
    NM_REQUIRE(m && d_sums && d_colsum && d_l1w && d_l1b && d_x0w, "null argument");
    NM_REQUIRE(m->plain_off, "this handle keeps no plain copy of layer1 / layers_xyz[0] (layer-wise path, or a one-layer network)");
    const int H = m->desc.hidden_size, dx = 6 * m->desc.num_encoding_fn_xyz + (m->desc.include_input_xyz ? 3 : 0);
    NM_REQUIRE(ld >= dx, "row stride of the sums is smaller than the encoding");
    const float* w0 = static_cast<const float*>(m->d_blob) + m->plain_off;
    const int threads = H * H + (dx + 1) * H;
    hipLaunchKernelGGL(linear_layer1_finish_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream_),
                       w0, w0 + (size_t)H * H, w0 + (size_t)H * H + (size_t)dx * H, d_sums, (int)ld, d_colsum, H, dx, d_l1w, d_l1b, d_x0w);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

int nm_mlp_export_layer1_transposed(nm_mlp* m, float* d_out, void* stream_) {
    NM_REQUIRE(m && d_out, "null argument");
    NM_REQUIRE(!m->lw, "the layer-wise path keeps no index map of its packed image");
    const int dx = 6 * m->desc.num_encoding_fn_xyz + (m->desc.include_input_xyz ? 3 : 0);
    const int64_t n = (int64_t)m->blob_floats;
    hipLaunchKernelGGL(scatter_layer1_t, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream_), m->d_index,
                       static_cast<const float*>(m->d_blob), n, (int)m->desc.hidden_size, dx, d_out);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

int nm_mlp_export_xyz_weight(nm_mlp* m, int32_t layer, float* d_out, void* stream_) {
    NM_REQUIRE(m && d_out, "null argument");
    NM_REQUIRE(!m->lw, "the layer-wise path keeps no index map of its packed image");
    NM_REQUIRE(layer >= 0 && layer <= m->desc.num_layers - 2, "no such layers_xyz");
    const int64_t n = (int64_t)m->blob_floats;        // (launched on the caller's stream, which belongs to the handle's device)
    hipLaunchKernelGGL(scatter_tensor, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream_), m->d_index,
                       static_cast<const float*>(m->d_blob), n, (int)(T_XYZ0 + 2 * layer), d_out);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

int nm_mlp_weights_current(nm_mlp* m, const nm_mlp_weights* d_weights, void* stream_, int32_t* differs) {
    NM_REQUIRE(m && d_weights && differs, "null argument");
    WeightPtrs ptrs;
    if (int rc = weight_pointers(m->desc, *d_weights, ptrs, "nm_mlp_weights_current")) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t n = (int64_t)m->blob_floats;
    NM_HIP_CHECK(hipMemsetAsync(m->d_check + 1, 0, 8, stream));
    hipLaunchKernelGGL(gather_parameters<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, m->d_index, ptrs,
                       static_cast<float*>(nullptr), n, m->d_check + 1);
    unsigned long long both[2];
    NM_HIP_CHECK(hipMemcpyAsync(both, m->d_check, 16, hipMemcpyDeviceToHost, stream));
    NM_HIP_CHECK(hipStreamSynchronize(stream));
    *differs = both[0] != both[1];
    return 0;
}

void nm_mlp_destroy(nm_mlp* m) {
    if (!m) return;
    if (m->d_blob) (void)hipFree(m->d_blob);
    if (m->d_index) (void)hipFree(m->d_index);
    if (m->d_check) (void)hipFree(m->d_check);
    if (m->d_tile_queue) (void)hipFree(m->d_tile_queue);
    if (m->d_index_b3) (void)hipFree(m->d_index_b3);
    if (m->d_tmp_b3) (void)hipFree(m->d_tmp_b3);
    if (m->d_stream_b3) (void)hipFree(m->d_stream_b3);
    if (m->d_enc_tab) (void)hipFree(m->d_enc_tab);
    layerwise_destroy(m);
    delete m;
}

int nm_mlp_kernel_variant(const nm_mlp* m, int* waves_per_workgroup) {
    int nw = 0;
    const int v = mlp_plan_info(m->plan, &nw);
    if (waves_per_workgroup) *waves_per_workgroup = nw;
    return v;
}

int64_t nm_mlp_flops_per_sample(const nm_mlp* m, int density_only) {
    return density_only ? m->flops_density : m->flops_full;
}

int nm_mlp_sample_points(nm_mlp* m, const float* d_points, const float* d_dirs, int64_t n, float* d_radiance,
                         void* stream) {
    NM_REQUIRE(m && d_points && d_dirs && d_radiance && n >= 0, "bad argument");
    MlpArgs a = m->base;
    a.mode = MODE_POINTS;
    a.a = d_points; a.b = d_dirs; a.c = nullptr;
    a.n = n; a.out = d_radiance;
    return launch_mlp_timed(m, a, 0, static_cast<hipStream_t>(stream));
}

// MODE_POINTS with density_only = 1: every family writes out[sample] = sigma in that mode.  The point doubles as the view
// direction (as in MODE_GRID); the density-only trunk never reads it.
int nm_mlp_sample_density(nm_mlp* m, const float* d_points, int64_t n, float* d_sigma, void* stream) {
    NM_REQUIRE(m && d_points && d_sigma && n >= 0, "bad argument");
    NM_REQUIRE(m->precision == NM_PREC_F32, "sample_density: geometry is fp32 by contract (bf16x3 handle)");
    MlpArgs a = m->base;
    a.mode = MODE_POINTS;
    a.a = d_points; a.b = d_points; a.c = nullptr;
    a.n = n; a.out = d_sigma;
    return launch_mlp_timed(m, a, 1, static_cast<hipStream_t>(stream));
}

int nm_mlp_eval_rays(nm_mlp* m, const float* d_origins, int origins_per_ray, const float* d_dirs, const float* d_t,
                     int64_t rays, int32_t samples, float* d_radiance, void* stream) {
    NM_REQUIRE(m && d_origins && d_dirs && d_t && d_radiance && rays >= 0 && samples > 0, "bad argument");
    return launch_mlp_timed(m, ray_mode_args(m, d_origins, origins_per_ray, d_dirs, d_t, rays, samples, d_radiance), 0, static_cast<hipStream_t>(stream));
}

}  // extern "C"

namespace nm {
int nm_mlp_eval_render_internal(nm_mlp* m, const RayGen* gen, const float* d_origins, int origins_per_ray, const float* d_dirs,
                                const float* d_t, int64_t rays, int32_t samples, float* d_radiance, float* d_att, int64_t att_floats,
                                hipStream_t stream) {
    NM_REQUIRE(m && (gen || (d_origins && d_dirs)) && d_t && d_radiance && rays >= 0 && samples > 0, "bad argument");
    MlpArgs a = ray_mode_args(m, d_origins, origins_per_ray, d_dirs, d_t, rays, samples, d_radiance);
    if (gen) {
        a.mode = MODE_VIEW;
        a.a = nullptr; a.b = nullptr;
        a.gen = *gen;
    }
    a.skip_empty = 1;
    a.att = d_att; a.att_floats = d_att ? att_floats : 0;
    return launch_mlp_timed(m, a, 0, stream);
}
}  // namespace nm

extern "C" {

int nm_mlp_grid_query(nm_mlp* m, const float* d_ax0, const float* d_ax1, const float* d_ax2, int32_t n0, int32_t n1,
                      int32_t n2, int64_t first, int64_t count, int32_t density_only, float* d_out, void* stream) {
    NM_REQUIRE(m && d_ax0 && d_ax1 && d_ax2 && d_out, "bad argument");
    NM_REQUIRE(n0 > 0 && n1 > 0 && n2 > 0 && first >= 0 && count >= 0 &&
               first + count <= (int64_t)n0 * n1 * n2, "grid range");
    MlpArgs a = m->base;
    a.mode = MODE_GRID;
    a.a = d_ax0; a.b = d_ax1; a.c = d_ax2;
    a.n1 = n1; a.n2 = n2; a.first = first;
    a.n = count; a.out = d_out;
    return launch_mlp_timed(m, a, density_only ? 1 : 0, static_cast<hipStream_t>(stream));
}

}  // extern "C"
