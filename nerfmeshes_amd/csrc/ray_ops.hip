// Per-ray primitives of the NeRF render path for gfx950: one 64-lane wavefront per ray, the
// sample axis lives in the wave (compositing: up to 512 samples in one pass, 8 per lane, and any
// count beyond that in segments of 512), scans and reductions are wavefront shuffles.
//
// Replaces (reference file:line under /root/reference/src):
//   nerf/nerf_helpers.py:226-277  get_ray_bundle
//   nerf/modules.py:157-186       RaySampleInterval.forward (deterministic branch)
//   nerf/modules.py:67-121        VolumeRenderer.forward    (+ nerf_helpers.py:199-223 cumprod_exclusive)
//   nerf/modules.py:197-248       SamplePDF.forward / sample_pdf (deterministic u)
//
// All of these are HBM-bound streaming kernels (a few bytes in, a few bytes out per sample) and are
// < 1 % of the time of the path; they are written for exact agreement with the torch CPU
// semantics: torch.cumprod/cumsum accumulate in fp64 and round every output to fp32, torch.norm
// is an fma chain, a*b+c is two roundings (this file is compiled with -ffp-contract=off).
#include "nm_internal.h"

namespace nm {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ double shfl_up_f64(double v, int delta) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_up(lo, delta);
    hi = __shfl_up(hi, delta);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double shfl_f64(double v, int src) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    return __hiloint2double(__shfl(hi, src), __shfl(lo, src));
}

// exclusive multiplicative / additive scan across the 64 lanes, fp64
template <bool MUL>
__device__ __forceinline__ double wave_exclusive_scan(double v, int lane) {
    double incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = shfl_up_f64(incl, off);
        if (lane >= off) incl = MUL ? incl * o : incl + o;
    }
    const double prev = shfl_up_f64(incl, 1);
    return lane == 0 ? (MUL ? 1.0 : 0.0) : prev;
}

__device__ __forceinline__ float torch_norm3(float x, float y, float z) { return nm_norm3(x, y, z); }

// ---- R0: pinhole rays -----------------------------------------------------------------------
// the rays of `gen`, materialised; out_o == nullptr: the directions only (get_ray_bundle: one origin for all rays)
__global__ void view_rays_kernel(const RayGen gen, int64_t rays, float* __restrict__ out_o, float* __restrict__ out_d) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rays) return;
    float o[3], d[3];
    nm_gen_ray(gen, i, o, d);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (out_o) out_o[3 * i + a] = o[a];
        out_d[3 * i + a] = d[a];
    }
}

// ndc_rays (nerf_helpers.py:280-307) over n rays; origins (1,3) shared or (n,3)
__global__ void ndc_rays_kernel(const float* __restrict__ origins, int origins_per_ray, const float* __restrict__ dirs,
                                int64_t n, float near32, float c_w, float c_h, float two_near, float m_two_near,
                                float* __restrict__ out_o, float* __restrict__ out_d) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* op = origins + (origins_per_ray ? 3 * i : 0);
    float o[3] = {op[0], op[1], op[2]}, d[3] = {dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]};
    nm_ndc_ray(near32, c_w, c_h, two_near, m_two_near, o, d);
#pragma unroll
    for (int a = 0; a < 3; ++a) { out_o[3 * i + a] = o[a]; out_d[3 * i + a] = d[a]; }
}

// PositionalEncoding.forward (modules.py:26-34) on (n, dim) rows: [x | sin(x_c * f_k) c-major | cos(...)]
struct BandArgs { float f[MAX_FREQ_XYZ]; };
__global__ void positional_encoding_kernel(const float* __restrict__ x, int64_t n, int dim, int nf, int include_input,
                                           BandArgs bands, float* __restrict__ out) {
    const int width = 2 * dim * nf + (include_input ? dim : 0);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * (int64_t)(dim * nf)) return;
    const int64_t row = i / (dim * nf);
    const int a = (int)(i - row * (dim * nf));       // a = coord * nf + freq
    const int c = a / nf, k = a - c * nf;
    const float v = x[row * dim + c];
    float* o = out + row * width;
    const float arg = bands.f[k] * v;
    float sv, cv;
    sincosf(arg, &sv, &cv);
    const int base = include_input ? dim : 0;
    o[base + a] = sv;
    o[base + dim * nf + a] = cv;
    if (include_input && k == 0) o[c] = v;
}

// ---- R1: coarse depth samples -----------------------------------------------------------------
__global__ void coarse_intervals_kernel(const float* __restrict__ u, const float* __restrict__ near_,
                                        const float* __restrict__ far_, int per_ray, int lindisp, int64_t rays,
                                        int samples, float* __restrict__ t) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rays * samples) return;
    const int64_t ray = i / samples;
    const int k = (int)(i - ray * samples);
    const float nr = near_[per_ray ? ray : 0], fr = far_[per_ray ? ray : 0];
    const float uk = u[k], om = 1.0f - uk;
    float v;
    if (!lindisp) {
        v = nr * om + fr * uk;
    } else {
        const float a = (1.0f / nr) * om, b = (1.0f / fr) * uk;
        v = 1.0f / (a + b);
    }
    t[i] = v;
}

// ---- R4: alpha compositing ----------------------------------------------------------------------
// One wave per ray; a lane owns PER consecutive samples of a segment of 64 * PER.  LONG = false: the ray is one segment
// (<= 512 samples).  LONG = true (PER = 8; no shipped config has such rays, modules.py:67-121 takes any count): segments of
// 512, the transmittance carried from segment to segment in fp64.
struct RayRows {             // one ray's rows of the inputs
    const float* t;
    const f32x4* rad;
    const float* noise;      // or null
    int samples;
    float norm;              // of the ray's direction
};

__device__ __forceinline__ RayRows ray_rows(const float* __restrict__ radiance, const float* __restrict__ t,
                                            const float* __restrict__ noise, int64_t ray, int samples, float norm) {
    return RayRows{t + ray * samples, reinterpret_cast<const f32x4*>(radiance) + ray * samples,
                   noise ? noise + ray * samples : nullptr, samples, norm};
}

// A lane's samples first .. first + PER - 1 (modules.py:82-93); past the ray's end a sample has alpha 0 and nothing is read.
template <int PER>
struct LaneSamples {
    float t[PER], dist[PER], raw[PER], decay[PER];       // raw = sigma + noise, decay = exp(-relu(raw) * dist)
    f32x4 rad[PER];
    __device__ __forceinline__ float alpha(int q) const { return 1.0f - decay[q]; }
    __device__ __forceinline__ float keep(int q) const { return (1.0f - alpha(q)) + 1e-10f; }
};

// Loads the lane's samples; returns the transmittance in front of the first of them: `carry` (the product of every keep() in
// front of the segment) times the fp64 exclusive product scan over the lanes.
template <int PER>
__device__ __forceinline__ double load_samples(const RayRows& in, int first, int lane, double carry, LaneSamples<PER>& L) {
    double local = 1.0;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int s = first + q;
        L.t[q] = 0.0f; L.dist[q] = 0.0f; L.raw[q] = 0.0f; L.decay[q] = 1.0f; L.rad[q] = f32x4{0, 0, 0, 0};
        if (s < in.samples) {
            L.t[q] = in.t[s];
            L.rad[q] = in.rad[s];
            float d = (s + 1 < in.samples) ? (in.t[s + 1] - L.t[q]) : 1e10f;
            d = d * in.norm;
            L.dist[q] = d;
            L.raw[q] = L.rad[q][3] + (in.noise ? in.noise[s] : 0.0f);
            L.decay[q] = expf(-fmaxf(L.raw[q], 0.0f) * d);      // d alpha / d (sigma * dist) too: autograd keeps exp's result
            local *= (double)L.keep(q);
        }
    }
    return carry * wave_exclusive_scan<true>(local, lane);
}

// One segment of the forward: weights and mask of its samples, their terms added to the lane's five sums {r, g, b, acc, depth}.
// Returns the lane's running product behind its last sample (lane 63: the transmittance in front of the next segment).
template <int PER>
__device__ __forceinline__ double composite_segment(const RayRows& in, int base, int lane, double carry, float thr,
                                                    float* __restrict__ weights, float* __restrict__ mask_weights,
                                                    float (&sum)[5]) {
    LaneSamples<PER> L;
    double run = load_samples<PER>(in, base + lane * PER, lane, carry, L);
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int s = base + lane * PER + q;
        if (s < in.samples) {
            const float T = (float)run;           // fp64 running product rounded per element, as torch.cumprod
            const float w = L.alpha(q) * T;
            if (weights) weights[s] = w;
            if (mask_weights) mask_weights[s] = T > thr ? 1.0f : 0.0f;
            sum[0] += w * L.rad[q][0]; sum[1] += w * L.rad[q][1]; sum[2] += w * L.rad[q][2];
            sum[3] += w;
            sum[4] += w * L.t[q];
            run *= (double)L.keep(q);
        }
    }
    return run;
}

// The transmittance behind the full segment at `base`, formed as composite_segment forms it (the same fp64 products in the same order)
template <int PER>
__device__ __forceinline__ double transmittance_segment(const RayRows& in, int base, int lane, double carry) {
    LaneSamples<PER> L;
    double run = load_samples<PER>(in, base + lane * PER, lane, carry, L);
#pragma unroll
    for (int q = 0; q < PER; ++q) run *= (double)L.keep(q);
    return run;
}

template <int PER, bool LONG>
__global__ __launch_bounds__(256) void composite_kernel(const float* __restrict__ radiance,
                                                        const float* __restrict__ t, const float* __restrict__ dirs,
                                                        const float* __restrict__ noise, int64_t rays, int samples,
                                                        float thr, int white_bg, int training, nm_bundle_out out,
                                                        const RayGen gen) {
    static_assert(!LONG || PER == 8, "rays of more than 512 samples are composited in segments of 512");
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (ray >= rays) return;
    float norm;
    if (gen.enabled) {       // rays generated from the pose: no direction buffer exists
        float go[3], gd[3];
        nm_gen_ray(gen, ray, go, gd);
        norm = torch_norm3(gd[0], gd[1], gd[2]);
    } else {
        norm = torch_norm3(dirs[3 * ray], dirs[3 * ray + 1], dirs[3 * ray + 2]);
    }
    const RayRows in = ray_rows(radiance, t, noise, ray, samples, norm);
    float* weights = out.d_weights ? out.d_weights + ray * samples : nullptr;
    float* mask_weights = out.d_mask_weights ? out.d_mask_weights + ray * samples : nullptr;
    float sum[5] = {0, 0, 0, 0, 0};
    if constexpr (LONG) {
        double carry = 1.0;                       // product of (1 - alpha + 1e-10) over every earlier segment
#pragma unroll 1
        for (int base = 0; base < samples; base += 64 * PER)     // lane 63 has walked to the end of the segment
            carry = shfl_f64(composite_segment<PER>(in, base, lane, carry, thr, weights, mask_weights, sum), 63);
    } else {
        composite_segment<PER>(in, 0, lane, 1.0, thr, weights, mask_weights, sum);
    }
    float r = wave_sum(sum[0]), g = wave_sum(sum[1]), b = wave_sum(sum[2]), acc = wave_sum(sum[3]), depth = wave_sum(sum[4]);
    if (lane == 0) {
        float disp = 1.0f / fmaxf(1e-10f, depth / acc);
        if (disp != disp || (depth / acc) != (depth / acc)) disp = 0.0f;  // NaN -> 0 (modules.py:107)
        if (!training && acc < 1.0f) depth = 0.0f;                        // modules.py:108-109
        if (white_bg) { const float bg = 1.0f - acc; r += bg; g += bg; b += bg; }
        if (out.d_rgb_map) { out.d_rgb_map[3 * ray] = r; out.d_rgb_map[3 * ray + 1] = g; out.d_rgb_map[3 * ray + 2] = b; }
        if (out.d_depth_map) out.d_depth_map[ray] = depth;
        if (out.d_acc_map) out.d_acc_map[ray] = acc;
        if (out.d_disp_map) out.d_disp_map[ray] = disp;
    }
}

// ---- R5: inverse-CDF resampling + merge -------------------------------------------------------------
// One wave per ray, its cdf / bins / merged depths in LDS: 3 * coarse + fine floats per wave, sized per launch (192-sample
// rays: 1.3 KB per wave; the limit is what four waves fit into a CU's 160 KB: 3 * num_coarse + num_fine <= 10 240).
constexpr int PDF_MAX_FLOATS_PER_WAVE = 10240;

__global__ __launch_bounds__(256) void sample_pdf_kernel(const float* __restrict__ t, const float* __restrict__ weights,
                                                         const float* __restrict__ u, int u_per_ray, int64_t rays,
                                                         int coarse, int fine, float* __restrict__ t_out) {
    extern __shared__ __attribute__((aligned(16))) float s_pdf[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t ray = (int64_t)blockIdx.x * 4 + wv;
    if (ray >= rays) return;  // wave-uniform; no block-level barriers below
    float* cdf = s_pdf + (size_t)wv * (3 * coarse + fine);
    float* bins = cdf + coarse;
    float* all = bins + coarse;
    const float* tr = t + ray * coarse;
    const float* wr = weights + ray * coarse;
    const int nb = coarse - 1;   // bins / cdf entries
    const int np = coarse - 2;   // pdf entries (weights[1:-1])

    // bins, pdf numerators, their sum
    float psum = 0.0f;
    for (int i = lane; i < coarse; i += 64) {
        const float ti = tr[i];
        all[i] = ti;
        if (i < nb) bins[i] = 0.5f * (tr[i + 1] + ti);
        if (i < np) psum += wr[i + 1] + 1e-5f;
    }
    psum = wave_sum(psum);
    // cdf = [0, cumsum(pdf)]: fp64 accumulation rounded per element (torch.cumsum on CPU)
    double carry = 0.0;
    for (int base = 0; base < np; base += 64) {
        const int i = base + lane;
        const double pdf = i < np ? (double)((wr[i + 1] + 1e-5f) / psum) : 0.0;
        double incl = pdf;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double o = shfl_up_f64(incl, off);
            if (lane >= off) incl += o;
        }
        incl += carry;
        if (i < np) cdf[i + 1] = (float)incl;
        int lo = __double2loint(incl), hi = __double2hiint(incl);
        carry = __hiloint2double(__shfl(hi, 63), __shfl(lo, 63));
    }
    if (lane == 0) cdf[0] = 0.0f;
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();

    // invert: idx = searchsorted(cdf, u, right=True)
    for (int j = lane; j < fine; j += 64) {
        const float uj = u[(u_per_ray ? ray * fine : 0) + j];   // modules.py:221-228: linspace, or rand per ray
        int lo = 0, hi = nb;             // first index with cdf[idx] > uj
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cdf[mid] <= uj) lo = mid + 1; else hi = mid;
        }
        const int below = lo - 1 > 0 ? lo - 1 : 0;
        const int above = lo < nb - 1 ? lo : nb - 1;
        const float cb = cdf[below], ca = cdf[above];
        float denom = ca - cb;
        if (denom < 1e-5f) denom = 1.0f;
        const float frac = (uj - cb) / denom;
        const float bb = bins[below], ba = bins[above];
        all[coarse + j] = bb + frac * (ba - bb);
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();

    // sort(cat(t, samples)): rank sort (any order of inputs, ties by index) -- 192 elements per ray
    const int total = coarse + fine;
    float* dst = t_out + ray * total;
    for (int e = lane; e < total; e += 64) {
        const float v = all[e];
        int rank = 0;
        for (int k = 0; k < total; ++k) {
            const float o = all[k];
            rank += (o < v || (o == v && k < e)) ? 1 : 0;
        }
        dst[rank] = v;
    }
}

// ---- training-mode pieces -----------------------------------------------------------
// Stratified jitter of the coarse depths (modules.py:171-184): lower + (upper - lower) * rand, with
// mids = 0.5 * (t[k+1] + t[k]); the random numbers are the caller's (torch.rand on the device).
__global__ void perturb_intervals_kernel(const float* __restrict__ t, const float* __restrict__ rnd, int64_t rays,
                                         int samples, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rays * samples) return;
    const int k = (int)(i % samples);
    const float tk = t[i];
    const float upper = k + 1 < samples ? 0.5f * (t[i + 1] + tk) : tk;
    const float lower = k > 0 ? 0.5f * (tk + t[i - 1]) : tk;
    const float span = upper - lower;
    const float step = span * rnd[i];
    out[i] = lower + step;
}

// Backward of VolumeRenderer.forward (modules.py:67-121) for the differentiable outputs the losses use:
//   w_k = alpha_k * T_k,  T_k = prod_{j<k} (1 - alpha_j + 1e-10),  alpha_k = 1 - exp(-relu(sigma_k + noise_k) * dist_k)
//   dL/dw_k = G_rgb . rgb_k + G_acc + G_depth * t_k + G_w[k] (- sum(G_rgb) with a white background)
//   dL/dalpha_k = dL/dw_k * T_k - (sum_{j>k} dL/dw_j * w_j) / (1 - alpha_k + 1e-10)
//   dL/dsigma_k = dL/dalpha_k * dist_k * exp(-relu(sigma_k + noise_k) * dist_k)   where sigma_k + noise_k > 0
// One wave per ray, the forward kernel's layout and segments: T_k from the same fp64 exclusive product scan as the forward, the
// suffix sums sum_{j>k} dL/dw_j * w_j from an fp64 suffix scan (reverse lane order) and a walk from the lane's last sample down.
// (Until round 5: one THREAD per ray, two sequential sweeps over its samples with T_k / alpha_k parked in the output rows --
// 2048 threads for a 2048-ray batch, 0.12 ms per call, 0.25 ms of every training iteration.)
struct RayGrads {            // one ray's upstream gradients
    float r, g, b, acc, depth;       // acc: G_acc - sum(G_rgb) with a white background
    const float* weights;            // the ray's row, or null
};

// One segment of the backward: `carry` is the transmittance in front of it, `behind` the sum of dL/dw_j * w_j over the samples
// behind it.  Writes the segment's rows of the radiance gradient; returns the lane's suffix sum in front of its first sample
// (lane 0: `behind` of the segment in front).
template <int PER>
__device__ __forceinline__ double composite_backward_segment(const RayRows& in, const RayGrads& G, int base, int lane, double carry,
                                                             double behind, f32x4* __restrict__ out) {
    LaneSamples<PER> L;
    double run = load_samples<PER>(in, base + lane * PER, lane, carry, L);
    float dw[PER], T[PER];
    double own = 0.0;                                          // sum of dL/dw_j * w_j over this lane's samples
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int s = base + lane * PER + q;
        dw[q] = 0.0f;
        if (s < in.samples) {
            dw[q] = (G.r * L.rad[q][0] + G.g * L.rad[q][1] + G.b * L.rad[q][2]) + G.acc + G.depth * L.t[q];
            if (G.weights) dw[q] += G.weights[s];
        }
        T[q] = (float)run;                                     // fp64 running product rounded per element, as the forward
        run *= (double)L.keep(q);
        own += (double)(dw[q] * (L.alpha(q) * T[q]));
    }
    // suffix over the lanes above this one: exclusive additive scan in reversed lane order.  Accumulated from the far end: total -
    // prefix in a near-to-far walk is the same number on paper; behind a surface, where the true sum is 1e-10 of the total or
    // less, it is the rounding error of the total.
    const double after = wave_exclusive_scan<false>(shfl_f64(own, 63 - lane), lane);
    double suffix = behind + shfl_f64(after, 63 - lane);
#pragma unroll
    for (int q = PER - 1; q >= 0; --q) {
        const int s = base + lane * PER + q;
        if (s < in.samples) {
            const float w = L.alpha(q) * T[q];
            const float dalpha = dw[q] * T[q] - (float)suffix / L.keep(q);
            suffix += (double)(dw[q] * w);
            // (decay, not 1 - alpha: the subtraction has lost exp's low bits, all of them from alpha == 1.0f on)
            const float dsigma = L.raw[q] > 0.0f ? dalpha * L.dist[q] * L.decay[q] : 0.0f;
            out[s] = f32x4{w * G.r, w * G.g, w * G.b, dsigma};
        }
    }
    return suffix;
}

// LONG: the segments from the far end to the near one.  The transmittance in front of a segment is the product over the segments
// before it, formed again for each: one more pass over the ray's depths and densities per segment in front.
template <int PER, bool LONG>
__global__ __launch_bounds__(256) void composite_backward_kernel(const float* __restrict__ radiance,
                                                                 const float* __restrict__ t,
                                                                 const float* __restrict__ dirs,
                                                                 const float* __restrict__ noise, int64_t rays, int samples,
                                                                 int white_bg, nm_bundle_grads g,
                                                                 float* __restrict__ grad_radiance) {
    static_assert(!LONG || PER == 8, "rays of more than 512 samples are composited in segments of 512");
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (ray >= rays) return;
    const RayRows in = ray_rows(radiance, t, noise, ray, samples, torch_norm3(dirs[3 * ray], dirs[3 * ray + 1], dirs[3 * ray + 2]));
    f32x4* out = reinterpret_cast<f32x4*>(grad_radiance) + ray * samples;
    float gr = 0.0f, gg = 0.0f, gb = 0.0f;
    if (g.d_rgb_map) { gr = g.d_rgb_map[3 * ray]; gg = g.d_rgb_map[3 * ray + 1]; gb = g.d_rgb_map[3 * ray + 2]; }
    const float gacc = (g.d_acc_map ? g.d_acc_map[ray] : 0.0f) - (white_bg ? (gr + gg + gb) : 0.0f);
    const RayGrads G{gr, gg, gb, gacc, g.d_depth_map ? g.d_depth_map[ray] : 0.0f, g.d_weights ? g.d_weights + ray * samples : nullptr};
    if constexpr (LONG) {
        double behind = 0.0;
#pragma unroll 1
        for (int base = (samples - 1) / (64 * PER) * (64 * PER); base >= 0; base -= 64 * PER) {
            double carry = 1.0;
#pragma unroll 1
            for (int b = 0; b < base; b += 64 * PER) carry = shfl_f64(transmittance_segment<PER>(in, b, lane, carry), 63);
            // lane 0 has walked down to the segment's first sample
            behind = shfl_f64(composite_backward_segment<PER>(in, G, base, lane, carry, behind, out), 0);
        }
    } else {
        composite_backward_segment<PER>(in, G, 0, lane, 1.0, 0.0, out);
    }
}

// ---- launchers ------------------------------------------------------------------------------------
// the pose and pixel grid of a RayGen (c2w: rows of 4 floats, 3 x 4 or 4 x 4); no NDC
static void set_pose(RayGen* g, const float* c2w, int height, int width, float focal, int64_t first) {
    memset(g, 0, sizeof(*g));
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) g->rot[3 * a + b] = c2w[4 * a + b];
        g->origin[a] = c2w[4 * a + 3];
    }
    g->height = height; g->width = width; g->focal = focal;
    g->enabled = 1; g->first = first;
}

// ndc_rays' python-float constants (nerf_helpers.py:288-303), computed in fp64 and rounded once, as torch does
static void set_ndc_constants(RayGen* g, int height, int width, double focal, double near_) {
    g->ndc_near = (float)near_;
    g->c_w = (float)(-1.0 / (width / (2.0 * focal)));
    g->c_h = (float)(-1.0 / (height / (2.0 * focal)));
    g->two_near = (float)(2.0 * near_);
    g->m_two_near = (float)(-2.0 * near_);
}

static int launch_view_rays(const RayGen& g, int64_t rays, float* d_origins, float* d_dirs, hipStream_t stream) {
    if (rays <= 0) return 0;
    hipLaunchKernelGGL(view_rays_kernel, dim3((unsigned)((rays + 255) / 256)), dim3(256), 0, stream, g, rays, d_origins, d_dirs);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_coarse_intervals(const float* d_u, const float* d_near, const float* d_far, int per_ray, int lindisp,
                            int64_t rays, int samples, float* d_t, hipStream_t stream) {
    const int64_t n = rays * samples;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(coarse_intervals_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_u, d_near,
                       d_far, per_ray, lindisp, rays, samples, d_t);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

// KERNEL<PER, LONG>(...) on `rays` rays of `samples` samples, one wave per ray: one pass with the smallest PER of 1, 2, 3, 4, 8 that
// holds the samples in 64 lanes, segments of 512 (PER = 8, LONG) beyond 512 samples
#define NM_LAUNCH_COMPOSITE(KERNEL, rays, samples, stream, ...)                                                               \
    do {                                                                                                                      \
        const int per_ = ((samples) + 63) / 64;                                                                               \
        auto* kernel_ = per_ == 1 ? KERNEL<1, false> : per_ == 2 ? KERNEL<2, false> : per_ == 3 ? KERNEL<3, false>            \
                      : per_ == 4 ? KERNEL<4, false> : per_ <= 8 ? KERNEL<8, false> : KERNEL<8, true>;                        \
        hipLaunchKernelGGL(kernel_, dim3((unsigned)(((rays) + 3) / 4)), dim3(256), 0, stream, __VA_ARGS__);                   \
        NM_HIP_CHECK(hipGetLastError());                                                                                      \
    } while (0)

int launch_composite(const float* d_radiance, const float* d_t, const float* d_dirs, const float* d_noise, int64_t rays,
                     int samples, float thr, int white_bg, int training, const nm_bundle_out& out, hipStream_t stream,
                     const RayGen* gen_ptr = nullptr) {
    if (rays <= 0) return 0;
    RayGen gen;
    if (gen_ptr) gen = *gen_ptr; else memset(&gen, 0, sizeof(gen));
    NM_REQUIRE(samples >= 1, "composite: samples per ray must be >= 1");
    NM_LAUNCH_COMPOSITE(composite_kernel, rays, samples, stream, d_radiance, d_t, d_dirs, d_noise, rays, samples, thr, white_bg, training, out,
                        gen);
    return 0;
}

int launch_sample_pdf(const float* d_t, const float* d_weights, const float* d_u, int u_per_ray, int64_t rays, int coarse,
                      int fine, float* d_t_out, hipStream_t stream) {
    if (rays <= 0) return 0;
    NM_REQUIRE(coarse >= 3 && fine >= 1, "sample_pdf: num_coarse must be >= 3 and num_fine >= 1");
    NM_REQUIRE(3 * (int64_t)coarse + fine <= PDF_MAX_FLOATS_PER_WAVE,
               "sample_pdf: 3 * num_coarse + num_fine must be <= 10240 (a ray's cdf, bins and merged depths live in LDS)");
    const int lds_bytes = 4 * (3 * coarse + fine) * 4;
    if (int rc = ensure_dynamic_lds((const void*)sample_pdf_kernel, lds_bytes)) return rc;
    hipLaunchKernelGGL(sample_pdf_kernel, dim3((unsigned)((rays + 3) / 4)), dim3(256), lds_bytes, stream, d_t, d_weights, d_u,
                       u_per_ray, rays, coarse, fine, d_t_out);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace nm

using namespace nm;

extern "C" {

int nm_ray_bundle(const float* h_c2w, int32_t height, int32_t width, float focal, int64_t first, int64_t count,
                  float* d_dirs, float* h_origin, void* stream) {
    NM_REQUIRE(h_c2w && d_dirs && height > 0 && width > 0, "bad argument");
    NM_REQUIRE(first >= 0 && count >= 0 && first + count <= (int64_t)height * width, "pixel range");
    if (h_origin)
        for (int a = 0; a < 3; ++a) h_origin[a] = h_c2w[4 * a + 3];
    RayGen g;
    set_pose(&g, h_c2w, height, width, focal, first);
    return launch_view_rays(g, count, nullptr, d_dirs, static_cast<hipStream_t>(stream));
}

int nm_coarse_intervals(const float* d_u, const float* d_near, const float* d_far, int bounds_per_ray, int lindisp,
                        int64_t rays, int32_t samples, float* d_t, void* stream) {
    NM_REQUIRE(d_u && d_near && d_far && d_t && samples > 0 && rays >= 0, "bad argument");
    return launch_coarse_intervals(d_u, d_near, d_far, bounds_per_ray, lindisp, rays, samples, d_t,
                                   static_cast<hipStream_t>(stream));
}

int nm_composite(const float* d_radiance, const float* d_t, const float* d_dirs, int64_t rays, int32_t samples,
                 float attenuation_threshold, int white_background, int training, const nm_bundle_out* out,
                 void* stream) {
    NM_REQUIRE(d_radiance && d_t && d_dirs && out && rays >= 0, "bad argument");
    return launch_composite(d_radiance, d_t, d_dirs, nullptr, rays, samples, attenuation_threshold, white_background,
                            training, *out, static_cast<hipStream_t>(stream));
}

int nm_sample_pdf(const float* d_t, const float* d_weights, const float* d_u, int64_t rays, int32_t coarse,
                  int32_t fine, float* d_t_out, void* stream) {
    NM_REQUIRE(d_t && d_weights && d_u && d_t_out && rays >= 0, "bad argument");
    return launch_sample_pdf(d_t, d_weights, d_u, 0, rays, coarse, fine, d_t_out, static_cast<hipStream_t>(stream));
}

int nm_perturb_intervals(const float* d_t, const float* d_rand, int64_t rays, int32_t samples, float* d_t_out,
                         void* stream) {
    NM_REQUIRE(d_t && d_rand && d_t_out && rays >= 0 && samples > 0, "bad argument");
    const int64_t n = rays * samples;
    if (n == 0) return 0;
    hipLaunchKernelGGL(perturb_intervals_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), d_t, d_rand, rays, samples, d_t_out);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

int nm_composite_train(const float* d_radiance, const float* d_t, const float* d_dirs, const float* d_noise,
                       int64_t rays, int32_t samples, float attenuation_threshold, int white_background,
                       const nm_bundle_out* out, void* stream) {
    NM_REQUIRE(d_radiance && d_t && d_dirs && out && rays >= 0, "bad argument");
    return launch_composite(d_radiance, d_t, d_dirs, d_noise, rays, samples, attenuation_threshold, white_background, 1,
                            *out, static_cast<hipStream_t>(stream));
}

int nm_composite_backward(const float* d_radiance, const float* d_t, const float* d_dirs, const float* d_noise,
                          int64_t rays, int32_t samples, int white_background, const nm_bundle_grads* grads,
                          float* d_grad_radiance, void* stream) {
    NM_REQUIRE(d_radiance && d_t && d_dirs && grads && d_grad_radiance && rays >= 0, "bad argument");
    NM_REQUIRE(samples >= 1, "composite: samples per ray must be >= 1");
    if (rays == 0) return 0;
    NM_LAUNCH_COMPOSITE(composite_backward_kernel, rays, samples, static_cast<hipStream_t>(stream), d_radiance, d_t, d_dirs, d_noise, rays,
                        samples, white_background, *grads, d_grad_radiance);
    return 0;
}

int nm_sample_pdf_rand(const float* d_t, const float* d_weights, const float* d_u, int64_t rays, int32_t coarse,
                       int32_t fine, float* d_t_out, void* stream) {
    NM_REQUIRE(d_t && d_weights && d_u && d_t_out && rays >= 0, "bad argument");
    return launch_sample_pdf(d_t, d_weights, d_u, 1, rays, coarse, fine, d_t_out, static_cast<hipStream_t>(stream));
}

static inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// The ray-termination table of the network launches (MlpArgs::att): one float per 16-sample depth slot and ray, the rays padded to
// whole ray blocks (at most 16 rays: a tuned kernel has at most 16 waves), for the longer of the two passes.
static inline size_t att_table_floats(int64_t rays, int32_t samples) { return (size_t)((rays + 15) / 16 * 16) * (size_t)((samples + 15) / 16); }

int64_t nm_render_workspace_bytes(int64_t rays, int32_t num_coarse, int32_t num_fine) {
    const size_t sc = (size_t)num_coarse, sf = (size_t)(num_coarse + (num_fine > 0 ? num_fine : 0));
    size_t b = 0;
    b += align256(rays * sc * 4);        // t coarse
    b += align256(rays * sc * 16);       // radiance coarse
    b += align256(rays * sc * 4);        // weights coarse (when the caller does not ask for them)
    if (num_fine > 0) {
        b += align256(rays * sf * 4);    // t fine
        b += align256(rays * sf * 16);   // radiance fine
    }
    b += align256(att_table_floats(rays, (int32_t)sf) * 4);     // ray termination table (both passes use it in turn)
    return (int64_t)b;
}

// NeRFModel.forward (model_nerf.py:37-78); `gen` != nullptr: the rays come from the pose (no origin / direction buffers)
static int render_impl(nm_mlp* coarse, nm_mlp* fine, const nm_render_cfg* cfg, const float* d_origins, int origins_per_ray,
                       const float* d_dirs, const RayGen* gen, const float* d_near, const float* d_far,
                       int bounds_per_ray, const float* d_u_coarse, const float* d_u_fine, int64_t rays,
                       void* d_workspace, const nm_bundle_out* coarse_out, const nm_bundle_out* fine_out,
                       hipStream_t stream) {
    if (rays <= 0) return 0;
    const int sc = cfg->num_coarse, sf = cfg->num_coarse + cfg->num_fine;
    char* ws = static_cast<char*>(d_workspace);
    float* t_c = reinterpret_cast<float*>(ws); ws += align256(rays * (size_t)sc * 4);
    float* rad_c = reinterpret_cast<float*>(ws); ws += align256(rays * (size_t)sc * 16);
    float* w_c = reinterpret_cast<float*>(ws); ws += align256(rays * (size_t)sc * 4);
    // the ray-termination table: behind everything else this call uses of the workspace
    const size_t att_floats = att_table_floats(rays, fine ? sf : sc);
    float* att = reinterpret_cast<float*>(ws + (fine ? align256(rays * (size_t)sf * 4) + align256(rays * (size_t)sf * 16) : 0));
    int rc;
    auto mlp = [&](nm_mlp* m, const float* t, int samples, float* rad) -> int {
        // `rad` is workspace only the compositor below reads, and no noise is added to sigma: tiles without density skip the colour branch
        return nm_mlp_eval_render_internal(m, gen, d_origins, origins_per_ray, d_dirs, t, rays, samples, rad, att, (int64_t)att_floats, stream);
    };
    // RaySampleInterval -> intervals_to_ray_points -> model_coarse -> volume_renderer (model_nerf.py:52-62)
    if ((rc = launch_coarse_intervals(d_u_coarse, d_near, d_far, bounds_per_ray, cfg->lindisp, rays, sc, t_c, stream))) return rc;
    if ((rc = mlp(coarse, t_c, sc, rad_c))) return rc;
    nm_bundle_out co = *coarse_out;
    if (!co.d_weights) co.d_weights = w_c;
    if ((rc = launch_composite(rad_c, t_c, d_dirs, nullptr, rays, sc, cfg->attenuation_threshold, cfg->white_background,
                               cfg->training, co, stream, gen))) return rc;
    if (!fine) return 0;
    // sample_pdf -> intervals_to_ray_points -> model_fine -> volume_renderer (model_nerf.py:65-76)
    float* t_f = reinterpret_cast<float*>(ws); ws += align256(rays * (size_t)sf * 4);
    float* rad_f = reinterpret_cast<float*>(ws);
    if ((rc = launch_sample_pdf(t_c, co.d_weights, d_u_fine, 0, rays, sc, cfg->num_fine, t_f, stream))) return rc;
    if ((rc = mlp(fine, t_f, sf, rad_f))) return rc;
    return launch_composite(rad_f, t_f, d_dirs, nullptr, rays, sf, cfg->attenuation_threshold, cfg->white_background,
                            cfg->training, *fine_out, stream, gen);
}

int nm_render_rays(nm_mlp* coarse, nm_mlp* fine, const nm_render_cfg* cfg, const float* d_origins, int origins_per_ray,
                   const float* d_dirs, const float* d_near, const float* d_far, int bounds_per_ray,
                   const float* d_u_coarse, const float* d_u_fine, int64_t rays, void* d_workspace,
                   const nm_bundle_out* coarse_out, const nm_bundle_out* fine_out, void* stream_) {
    NM_REQUIRE(coarse && cfg && d_origins && d_dirs && d_near && d_far && d_u_coarse && d_workspace && coarse_out,
               "bad argument");
    NM_REQUIRE(!fine || (d_u_fine && fine_out && cfg->num_fine > 0), "fine network needs u_fine / fine_out / num_fine");
    return render_impl(coarse, fine, cfg, d_origins, origins_per_ray, d_dirs, nullptr, d_near, d_far, bounds_per_ray,
                       d_u_coarse, d_u_fine, rays, d_workspace, coarse_out, fine_out, static_cast<hipStream_t>(stream_));
}

static int make_raygen(const nm_view* v, int64_t first, RayGen* g) {
    NM_REQUIRE(v && v->height > 0 && v->width > 0 && v->focal > 0.0, "bad view");
    set_pose(g, v->c2w, v->height, v->width, (float)v->focal, first);
    g->ndc = v->use_ndc ? 1 : 0;
    set_ndc_constants(g, v->height, v->width, v->focal, v->ndc_near);
    return 0;
}

int nm_render_view(nm_mlp* coarse, nm_mlp* fine, const nm_render_cfg* cfg, const nm_view* view, int64_t first_pixel,
                   int64_t rays, const float* d_near, const float* d_far, int bounds_per_ray, const float* d_u_coarse,
                   const float* d_u_fine, void* d_workspace, const nm_bundle_out* coarse_out,
                   const nm_bundle_out* fine_out, void* stream_) {
    NM_REQUIRE(coarse && cfg && view && d_near && d_far && d_u_coarse && d_workspace && coarse_out, "bad argument");
    NM_REQUIRE(!fine || (d_u_fine && fine_out && cfg->num_fine > 0), "fine network needs u_fine / fine_out / num_fine");
    NM_REQUIRE(first_pixel >= 0 && rays >= 0 && first_pixel + rays <= (int64_t)view->height * view->width, "pixel range");
    RayGen g;
    int rc = make_raygen(view, first_pixel, &g);
    if (rc) return rc;
    return render_impl(coarse, fine, cfg, nullptr, 0, nullptr, &g, d_near, d_far, bounds_per_ray, d_u_coarse, d_u_fine,
                       rays, d_workspace, coarse_out, fine_out, static_cast<hipStream_t>(stream_));
}

int nm_view_rays(const nm_view* view, int64_t first_pixel, int64_t rays, float* d_origins, float* d_dirs, void* stream_) {
    NM_REQUIRE(view && d_origins && d_dirs, "bad argument");
    NM_REQUIRE(first_pixel >= 0 && rays >= 0 && first_pixel + rays <= (int64_t)view->height * view->width, "pixel range");
    RayGen g;
    int rc = make_raygen(view, first_pixel, &g);
    if (rc) return rc;
    return launch_view_rays(g, rays, d_origins, d_dirs, static_cast<hipStream_t>(stream_));
}

int nm_ndc_rays(int32_t height, int32_t width, double focal, double near_, const float* d_origins, int origins_per_ray,
                const float* d_dirs, int64_t n, float* d_out_origins, float* d_out_dirs, void* stream_) {
    NM_REQUIRE(d_origins && d_dirs && d_out_origins && d_out_dirs && height > 0 && width > 0 && focal > 0.0 && n >= 0,
               "bad argument");
    if (n == 0) return 0;
    RayGen g;
    set_ndc_constants(&g, height, width, focal, near_);
    hipLaunchKernelGGL(ndc_rays_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream_),
                       d_origins, origins_per_ray, d_dirs, n, g.ndc_near, g.c_w, g.c_h, g.two_near, g.m_two_near, d_out_origins,
                       d_out_dirs);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

int nm_positional_encoding(const float* d_x, int64_t n, int32_t dim, const float* h_bands, int32_t num_bands,
                           int32_t include_input, float* d_out, void* stream_) {
    NM_REQUIRE(d_x && h_bands && d_out && n >= 0 && dim >= 1, "bad argument");
    NM_REQUIRE(num_bands >= 0 && num_bands <= MAX_FREQ_XYZ, "positional_encoding: at most 16 frequency bands");
    if (n == 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int width = 2 * dim * num_bands + (include_input ? dim : 0);
    if (num_bands == 0) {   // encoding = the input itself (or nothing)
        if (include_input) NM_HIP_CHECK(hipMemcpyAsync(d_out, d_x, (size_t)n * dim * 4, hipMemcpyDeviceToDevice, stream));
        (void)width;
        return 0;
    }
    BandArgs b;
    for (int k = 0; k < MAX_FREQ_XYZ; ++k) b.f[k] = k < num_bands ? h_bands[k] : 0.0f;
    const int64_t work = n * (int64_t)(dim * num_bands);
    hipLaunchKernelGGL(positional_encoding_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, stream, d_x, n,
                       dim, num_bands, include_input, b, d_out);
    NM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
