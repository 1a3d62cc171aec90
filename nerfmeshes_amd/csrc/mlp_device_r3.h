// Round-2 inference kernel: the same dataflow as mlp_device.h's mlp_kernel (register-resident activations, weights
// as the only streamed operand, bit-identical results) with the two stalls the round-1 ablations located removed:
//
//   * 3-slot LDS ring, weight DMA TWO chunks ahead.  In the 2-slot kernel the chunk that is read next only becomes
//     visible at the barrier that ends the current chunk, so the first A-operand ds_read of every chunk is issued AFTER
//     the barrier and BOTH waves of a SIMD -- released together -- expose its latency together (plus the DMA issue
//     sequence in front of it): ~300 idle matrix-pipe cycles per 8192-cycle chunk.  With the chunk after next in
//     flight, the next chunk is already resident while the current one is consumed, and the operand prefetch runs
//     ACROSS chunk and stage boundaries (`carry`): after a barrier the first MFMA issues immediately.
//   * the DMA issue of the two waves sharing a SIMD is staggered (waves 0..NW/2-1 at k-step 0, the others half a chunk
//     later): one wave's scalar/VMEM issue sequence runs under its partner's MFMAs instead of next to the partner's
//     identical sequence.
// Measured (profiles/r02_mlp_variants.json): on their own these two are worth +0.1 % -- the stall that mattered was
// the address-VGPR read of the DMA instruction itself (see stream_to_lds in mlp_device.h).
#pragma once
#include "mlp_device.h"

namespace nm {

struct NextChunks {          // the first two chunks of whatever stage runs next (bytes 0: nothing follows)
    const char* s0; int b0;
    const char* s1; int b1;
};

// A chunk is consumed as a stream of "blocks": block j = one ds_read_b128 per lane (the A operands of 4 consecutive
// output tiles of k-step j / NB) feeding 4 MFMAs; blocks are contiguous in the chunk image (offset j * 1 KiB).  The
// operands of block j + 2 are fetched while block j runs (8 MFMAs = 256 matrix-pipe cycles of cover, 3 live operand
// quads instead of round 1's 8), and the stream simply continues into the next chunk / the next stage: `carry` holds
// blocks 0 and 1 of whatever comes next.
// Waves 0..NW/2-1 issue their DMA pieces at block 0 of a chunk, the others half a chunk later.
template <int NT, int KS1, int KS2, int NW, int LDSBUF, int KCH>
__device__ __forceinline__ void gemm_stage3(f32x4 (&acc)[NT], const float (&b1)[KS1],
                                            const float (&b2)[(KS2 > 0 ? KS2 : 1)], const char* gw,
                                            const NextChunks nx, char* lds, int& slot, f32x4 (&carry)[2],
                                            int wave, int lane) {
    constexpr int KS = KS1 + KS2;
    constexpr int NCH = (KS + KCH - 1) / KCH;
    constexpr int NB = NT / 4;
    constexpr int STEP_BYTES = NT * 256;
    static_assert(NT % 4 == 0 && NB >= 1, "tile count");
    static_assert(NCH >= 2, "every stage must span at least two chunks (DMA runs two chunks ahead)");
    f32x4 ab[3];
    ab[0] = carry[0];
    ab[1] = carry[1];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int steps = (KS - c * KCH) < KCH ? (KS - c * KCH) : KCH;
        const int nblk = steps * NB;
        const int slot1 = slot == 2 ? 0 : slot + 1;
        const int slot2 = slot1 == 2 ? 0 : slot1 + 1;
        const char* src;
        int bytes;
        if (c + 2 < NCH) {
            const int nsteps = (KS - (c + 2) * KCH) < KCH ? (KS - (c + 2) * KCH) : KCH;
            src = gw + (c + 2) * KCH * STEP_BYTES; bytes = nsteps * STEP_BYTES;
        } else if (c + 2 == NCH) { src = nx.s0; bytes = nx.b0; }
        else { src = nx.s1; bytes = nx.b1; }
        char* dst = lds + slot2 * LDSBUF;
        const char* buf = lds + slot * LDSBUF + lane * 16;
        const char* nbuf = lds + slot1 * LDSBUF + lane * 16;
#pragma unroll
        for (int j = 0; j < nblk; ++j) {
            if (j == 0 && wave < NW / 2) stream_to_lds<NW>(src, dst, bytes, wave, lane);
            if (j == nblk / 2 && wave >= NW / 2) stream_to_lds<NW>(src, dst, bytes, wave, lane);
            const int ks = j / NB, blk = j % NB;
            const int s = c * KCH + ks;
            const float b = s < KS1 ? b1[s < KS1 ? s : 0] : b2[s >= KS1 ? s - KS1 : 0];
            // the chunk after this one is resident since the last barrier: the stream runs straight into it
            const char* from = (j + 2 < nblk) ? buf + (j + 2) * 1024 : nbuf + (j + 2 - nblk) * 1024;
            const int r0 = (c * KCH * NB + j) % 3;           // ring position of block j (static: loops are unrolled)
            ab[(r0 + 2) % 3] = *reinterpret_cast<const f32x4*>(from);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                acc[blk * 4 + q] = __builtin_amdgcn_mfma_f32_16x16x4f32(ab[r0][q], b, acc[blk * 4 + q], 0, 0, 0);
        }
        __syncthreads();   // this wave's DMA pieces have landed (vmcnt(0)); after it the chunk after next is visible to all
        slot = slot1;
    }
    constexpr int TOTAL = KS * NB;                           // blocks consumed: the two in flight sit at TOTAL, TOTAL + 1
    carry[0] = ab[TOTAL % 3];
    carry[1] = ab[(TOTAL + 1) % 3];
}

// Inference only.  The taping forward on this dataflow was built, wrote the same tape bit for bit and measured 4.7 % SLOWER than
// the 2-slot taping kernel (3.54 vs 3.38 ms per 393 216 samples of the 8x256 network, profiles/r04_train_three_slot.json; source
// last present in 94bb324): the training kernels stay on mlp_device.h's dataflow.
// SKIP: the render path's instantiation (MlpArgs::skip_empty): a tile on which no sample has density writes
// {0, 0, 0, sigma} and skips fc_feat, the view layer and fc_rgb; in ray modes with samples % 16 == 0 a tile is NW adjacent rays x
// 16 consecutive samples (MlpArgs::ray_tiles).  A separate instantiation so that every other entry point runs the kernel it ran.
// Its tiles cost unequal time (an empty one about 0.83 of a full one), and in ray-tile order a static stride hands a workgroup the
// same few depth slots for its whole life -- the slots in front of the object are nearly all empty --, so SKIP draws its tiles from
// a queue instead (MlpArgs::tile_queue): the first is blockIdx.x, every further one gridDim.x + the value one lane's
// atomicAdd returned.  The tile after this one is claimed early in this one (behind layer1) and handed to the other waves through
// LDS under the trunk's barriers, so the round trip is hidden and `has_next` is known before the last stage, which needs it.  A
// workgroup makes one claim per tile it runs and stops at the first one past the end: no workgroup waits for another, and a launch
// makes exactly wg_iters claims.
// Ray termination (MlpArgs::att; ray-tile launches of at least two ray blocks per resident workgroup): the queue runs
// slot-major (tile `it` = depth slot it / ray_blocks of ray block it % ray_blocks), every wave adds an upper bound of log2 of its
// ray's transmittance factors over the tile to the ray's entry of the slot before and stores it, and the claiming wave reads the 8
// entries of the slot in front of the tile it claimed: where all are below -160 the compositor's fp32 transmittance is 0 on the
// whole tile, which is then not evaluated at all -- it writes zeros (top of the tile loop).  The verdict travels in the top bit of
// the claim word.  The table is read and written at agent scope (the XCDs' L2s are not coherent); an entry that is missing when
// it is read only loses a verdict.
template <int H, int FX, int FD, int NW, int KCH, bool FLAT = false, bool SKIP = false>   // FLAT: see mlp_kernel
// Occupancy: networks up to 128 wide are compiled for FOUR waves per SIMD (128 registers: two 8-wave workgroups per CU; the
// 128-wide instances spill 9 -- 17 registers outside the k-step loops for it).  With VALU issue time adding to matrix time on
// narrow networks two more waves per SIMD are worth +2.7 points at 8x128 (0.875 -> 0.902, same bits).
__global__ __launch_bounds__(NW * 64, H <= 128 ? 4 : 2) void mlp_kernel3(const MlpArgs args, const int num_layers,
                                                          const int density_only) {
    using N = Net<H, FX, FD, KCH>;
    static_assert(!(FLAT && SKIP), "the use_viewdirs = 0 heads have no colour branch to skip");
    static_assert(N::EX > KCH && N::KH >= 2 * KCH, "stages must span two chunks");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    float* lds_bias = reinterpret_cast<float*>(lds + 3 * N::LDSBUF);
    const int nbias = H * (1 + num_layers) + H / 2 + 4;
    float* lds_walpha = lds_bias + nbias;
    float* lds_wrgb = lds_walpha + H;
    // SKIP's vote word, behind fc_rgb's rows (the cache is 4 H (L + 4) + 16 bytes rounded up to 256: 240 bytes are spare; the
    // FLAT heads' wider rows never meet SKIP).  It holds the stamp of the last iteration on which some wave saw density.
    int* lds_vote = reinterpret_cast<int*>(lds_wrgb + 3 * H / 2);
    // ... and behind it the two words through which lane 0 publishes its claims, alternating (the next claim is written while
    // the last one may still be unread by a slower wave of the iteration before)
    uint32_t* lds_claim = reinterpret_cast<uint32_t*>(lds_vote + 1);
    if (SKIP && threadIdx.x == 0) *lds_vote = 0;
    for (int i = threadIdx.x; i < nbias; i += NW * 64) lds_bias[i] = args.bias[i];
    for (int i = threadIdx.x; i < H; i += NW * 64) lds_walpha[i] = args.walpha[i];
    for (int i = threadIdx.x; i < ((FLAT && density_only == 2) ? 3 * H : 3 * H / 2); i += NW * 64) lds_wrgb[i] = args.wrgb[i];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, col = lane & 15;
    const float* tail_bias = lds_bias + nbias - 4;

    const int64_t wg_iters = mlp_wg_iters(args, NW * 16);
    auto hidden_next = [](const char* p) {
        return NextChunks{p, KCH * N::STEP, p + KCH * N::STEP, (N::KH - KCH < KCH ? N::KH - KCH : KCH) * N::STEP};
    };
    auto enc_next = [](const char* p, bool on) {
        return NextChunks{p, on ? KCH * N::STEP : 0, p + KCH * N::STEP,
                          on ? (N::EX - KCH < KCH ? N::EX - KCH : KCH) * N::STEP : 0};
    };
    auto dir_next = [](const char* p) { return NextChunks{p, KCH * N::STEPD, p + KCH * N::STEPD, KCH * N::STEPD}; };

    int slot = 0;
    f32x4 carry[2];
    if ((int64_t)blockIdx.x < wg_iters) {
        const NextChunks first = enc_next(args.wstream, true);
        stream_to_lds<NW>(first.s0, lds, first.b0, wave, lane);
        stream_to_lds<NW>(first.s1, lds + N::LDSBUF, first.b1, wave, lane);
    }
    __syncthreads();
    carry[0] = *reinterpret_cast<const f32x4*>(lds + lane * 16);
    carry[1] = *reinterpret_cast<const f32x4*>(lds + lane * 16 + 1024);

    int64_t next_it = 0;     // SKIP: the tile claimed for the iteration after this one
    int turn = 0;
    // Ray termination is compiled into the 256-wide instances only: in the 128-wide one, held to 128 registers for four waves per
    // SIMD, it spilled 38 registers (156 B of scratch) where the kernel spills 16; that instance is the code it was.
    constexpr bool TERM = SKIP && H > 128;
    const bool term = TERM && args.att != nullptr;      // launch_mlp: ray tiles, slot-major order
    // this wave's entry of the table for tile `t` (slot-major: t = k * ray_blocks + block; a row is ray_blocks * NW rays)
    auto att_entry = [&](int64_t t, uint32_t& k) -> float* {
        k = (uint32_t)t / args.att_blocks;
        return args.att + ((size_t)(uint32_t)t * NW + wave);     // (k * ray_blocks + block) * NW + wave
    };
    bool dead = false;       // the verdict on tile `it` (a workgroup's first tile is evaluated)
    // wave 0: claim a tile and start the loads of its rays' entries of the slot before (lanes 0 .. NW-1 one ray each).  An entry
    // that is not loaded (first slot, past the end) counts as alive.
    auto claim_tile = [&](float& pre) -> uint32_t {
        uint32_t c = 0;
        if (lane == 0) c = atomicAdd(args.tile_queue, 1u);
        c = (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
        pre = 0.0f;
        if (term) {
            const int64_t nx = (int64_t)gridDim.x + c;
            if (nx < wg_iters && nx >= (int64_t)args.att_blocks && lane < NW)      // not the first slot: the row before, NW entries
                pre = __hip_atomic_load(args.att + ((size_t)((uint32_t)nx - args.att_blocks) * NW + lane), __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT);
        }
        return c;
    };
    auto claim_word = [&](uint32_t c, float pre) -> uint32_t {     // all NW entries below -160: the tile is dead
        const bool all_dead = term && __ballot(lane < NW && !(pre < -160.0f)) == 0;
        return c | (all_dead ? 0x80000000u : 0u);
    };
    for (int64_t it = blockIdx.x; it < wg_iters; it = SKIP ? next_it : it + gridDim.x) {
        bool has_next = !SKIP && it + gridDim.x < wg_iters;     // SKIP: known once the claim is read (before fc_feat)
        // linear order: wave w of iteration `it` owns 16 consecutive samples; ray_tiles: ray NW * block + w, depth slot k
        int64_t sample = (it * NW + wave) * 16 + col;
        bool valid = sample < args.n;
        if (SKIP && args.ray_tiles) {   // (32-bit split: launch_mlp keeps wg_iters below 2^31 in this mode; the 64-bit division costs registers)
            const uint32_t depth_slots = (uint32_t)args.samples >> 4;
            // block-major: it = block * depth_slots + k | ray termination, slot-major: it = k * ray_blocks + block
            const uint32_t div = term ? args.att_blocks : depth_slots;       // (!TERM: the division by depth_slots alone, as it was)
            const uint32_t q = (uint32_t)it / div, r = (uint32_t)it - q * div;
            const uint32_t block = term ? r : q;
            const int64_t ray_first = ((int64_t)block * NW + wave) * args.samples;
            sample = ray_first + ((term ? q : r) << 4) + col;
            valid = ray_first < args.n;
        }
        if (TERM && dead) {
            // Every ray of the tile has transmittance 0 in front of it: whatever the network gives here has weight alpha * 0 = +0, so
            // the tile is written as zeros (finite, and sigma 0 keeps T at 0) and nothing is evaluated.  Dead is absorbing.  The
            // weight ring is not touched: it holds layer1's first two chunks from the last tile's wrap-around DMA.
            if (valid && g == 0) {
                f32x4 o4 = {0.0f, 0.0f, 0.0f, 0.0f};
                *reinterpret_cast<f32x4*>(args.out + 4 * sample) = o4;
            }
            uint32_t k;
            float* const entry = att_entry(it, k);
            if (lane == 0) __hip_atomic_store(entry, -1e30f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (args.dead_count && threadIdx.x == 0) atomicAdd(args.dead_count, 1u);
            if (wave == 0) {
                float pre;
                const uint32_t c = claim_tile(pre);
                const uint32_t word = claim_word(c, pre);
                if (lane == 0) lds_claim[turn] = word;
            }
            __syncthreads();
            const uint32_t word = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_claim[turn]);
            turn ^= 1;
            next_it = (int64_t)gridDim.x + (word & 0x7fffffffu);
            dead = (word >> 31) != 0;
            continue;
        }
        const int64_t sidx = valid ? sample : args.n - 1;
        const SamplePD smp = fetch_sample(args, sidx);
        const float p[3] = {smp.px, smp.py, smp.pz}, d[3] = {smp.dx, smp.dy, smp.dz};
        const float dummy[1] = {0.0f};
        float encx[N::EX];
        encode<FX, N::EX>(encx, p, args.bands_xyz, g);
        NextChunks wrap = enc_next(args.wstream, has_next);

        f32x4 acc[N::NT];
        float in[N::KH];
        const char* gw = args.wstream;
        // ---- layer1: xyz_enc -> H, no activation (models.py:62)
        load_bias<N::NT>(acc, lds_bias, g);
        gemm_stage3<N::NT, N::EX, 0, NW, N::LDSBUF, KCH>(acc, encx, dummy, gw, hidden_next(gw + N::EX * N::STEP), lds, slot, carry, wave, lane);
        gw += N::EX * N::STEP;
        acc_to_operand<N::NT, false>(acc, in);
        // The claim of the tile after this one.  The compiler waits for the returned value where the atomic is issued, so it is
        // issued here and not in the prologue: in front of the trunk's stages this wave's wait runs under its SIMD partner's MFMAs.
        // With ray termination the claimed tile is judged here as well (a second round trip of wave 0 alone; holding the entries in
        // a register across the trunk's first stage instead, whose barriers wait for every load anyway, measured 0.2 % slower).
        if constexpr (TERM) {
            if (wave == 0) {
                float pre;
                const uint32_t claimed = claim_tile(pre);
                const uint32_t word = claim_word(claimed, pre);
                if (lane == 0) lds_claim[turn] = word;
            }
        } else if (SKIP && threadIdx.x == 0) lds_claim[turn] = atomicAdd(args.tile_queue, 1u);

        // ---- layers_xyz[0 .. L-2], then (full evaluation only) fc_feat as iteration L-1 (models.py:63-70)
        float sigma = 0.0f;
        bool empty_tile = false;
        const int trunk_iters = density_only ? num_layers - 1 : num_layers;
#pragma unroll 1
        for (int i = 0; i < trunk_iters; ++i) {
            const bool is_feat = i == num_layers - 1;
            // ray termination: the sample's interval and the ray's entry of the slot before, asked for in front of the density head
            float t_here = 0.0f, t_after = 0.0f, att_before = 0.0f;
            float* entry = nullptr;
            bool last_of_ray = false;
            if (term && is_feat) {
                uint32_t k;
                entry = att_entry(it, k);
                last_of_ray = (k << 4) + col + 1 == (uint32_t)args.samples;
                if (valid) {
                    t_here = args.c[sample];
                    if (!last_of_ray) t_after = args.c[sample + 1];
                    if (lane == 0 && k > 0)
                        att_before = __hip_atomic_load(entry - (size_t)args.att_blocks * NW, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            if (is_feat) sigma = alpha_gemv<H>(in, lds_walpha, g) + tail_bias[0];
            if (term && is_feat) {
                // The compositor's factor of this sample, (1 - alpha) + 1e-10f, as an upper bound of its log2: + 2^-23 for a quantum of
                // difference in 1 - alpha (where alpha rounds to 1 that moves log2 by whole units), + 2^-8 for expf, the norm and the sum.
                // A NaN sigma is no density to the compositor either (fmaxf).  Padding rays are dead.
                const float dist = (last_of_ray ? 1e10f : t_after - t_here) * nm_norm3(d[0], d[1], d[2]);
                const float a = 1.0f - expf(-(fmaxf(sigma, 0.0f) * dist));
                float c = log2f(((1.0f - a) + 1e-10f) + 0x1p-23f) + 0x1p-8f;
#pragma unroll
                for (int m = 1; m < 16; m <<= 1) c += __shfl_xor(c, m);
                if (lane == 0)
                    __hip_atomic_store(entry, valid ? att_before + c : -1e30f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (SKIP && is_feat) {
                // Workgroup-uniform vote (the stages below hold barriers: every wave must take the same branch): a wave on which some
                // valid sample has density -- or a NaN sigma, which must keep propagating -- stamps this iteration's number.
                const int epoch = (int)it + 1;      // never 0, and different on consecutive iterations of a workgroup
                const bool dense = valid && !(sigma <= 0.0f);
                if (dense) *lds_vote = epoch;
                __syncthreads();
                empty_tile = __builtin_amdgcn_readfirstlane(*lds_vote) != epoch;
                // the same barrier (and every one of the trunk before it) published the claim; nothing up to here issues the wrap-around DMA
                const uint32_t word = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_claim[turn]);
                next_it = (int64_t)gridDim.x + (word & 0x7fffffffu);
                dead = (word >> 31) != 0;
                turn ^= 1;
                has_next = next_it < wg_iters;
                wrap = enc_next(args.wstream, has_next);
                if (empty_tile) break;
            }
            const bool skip = !is_feat && ((args.skip_mask >> i) & 1u);
            const bool last_density = density_only && i == num_layers - 2;
            load_bias<N::NT>(acc, lds_bias + H * (1 + i), g);
            {
                const char* after = gw + N::KH * N::STEP;
                NextChunks nx = hidden_next(after);
                if (skip) nx = enc_next(after, true);
                else if (is_feat) nx = dir_next(after);
                else if (last_density) nx = wrap;
                gemm_stage3<N::NT, N::KH, 0, NW, N::LDSBUF, KCH>(acc, in, dummy, gw, nx, lds, slot, carry, wave, lane);
                gw = after;
            }
            if (skip) {  // cat(hidden, xyz_enc): the encoding columns of layers_xyz[i] (models.py:64-65)
                const char* after = gw + N::EX * N::STEP;
                const NextChunks nx = last_density ? wrap : hidden_next(after);
                gemm_stage3<N::NT, N::EX, 0, NW, N::LDSBUF, KCH>(acc, encx, dummy, gw, nx, lds, slot, carry, wave, lane);
                gw = after;
            }
            acc_to_operand<N::NT, true>(acc, in);
        }

        if (empty_tile) {
            // No sample of the tile has density: alpha and weight are exactly 0 for all of them, so their colour never reaches a map.
            // It is written as zeros (finite: 0 * rgb must stay 0 in the compositor); fc_feat, the view layer and fc_rgb are skipped.
            if (valid && g == 0) {
                f32x4 o4 = {0.0f, 0.0f, 0.0f, sigma};
                *reinterpret_cast<f32x4*>(args.out + 4 * sample) = o4;
            }
            if (args.skip_count && threadIdx.x == 0) atomicAdd(args.skip_count, 1u);
            // The ring holds fc_feat's first two chunks and `carry` its first two blocks.  Restart the stream as the prologue does:
            // layer1's chunks 0 and 1 into the two slots after `slot` (every read of the ring completed before the vote's barrier),
            // one barrier, `carry` from the first of them, which becomes `slot`.
            if (has_next) {
                const int slot1 = slot == 2 ? 0 : slot + 1;
                const int slot2 = slot1 == 2 ? 0 : slot1 + 1;
                stream_to_lds<NW>(wrap.s0, lds + slot1 * N::LDSBUF, wrap.b0, wave, lane);
                stream_to_lds<NW>(wrap.s1, lds + slot2 * N::LDSBUF, wrap.b1, wave, lane);
                __syncthreads();
                slot = slot1;
                carry[0] = *reinterpret_cast<const f32x4*>(lds + slot * N::LDSBUF + lane * 16);
                carry[1] = *reinterpret_cast<const f32x4*>(lds + slot * N::LDSBUF + lane * 16 + 1024);
            }
            continue;
        }

        if (density_only) {
            sigma = alpha_gemv<H>(in, lds_walpha, g) + tail_bias[0];
            if (FLAT && density_only == 2) flat_head<H>(args, in, lds_wrgb, tail_bias, sigma, sample, valid, g);   // use_viewdirs = 0
            else if (valid && g == 0) args.out[sample] = sigma;
            continue;
        }

        // ---- layers_dir[0]: cat(feat, dir_enc) -> H/2, relu (models.py:72-74)
        f32x4 accd[N::NTD];
        float v[N::KD];
        load_bias<N::NTD>(accd, lds_bias + H * (1 + num_layers), g);
        float encd[N::ED];
        encode<FD, N::ED>(encd, d, args.bands_dir, g);
        gemm_stage3<N::NTD, N::KH, N::ED, NW, N::LDSBUF, KCH>(accd, in, encd, gw, wrap, lds, slot, carry, wave, lane);
        acc_to_operand<N::NTD, true>(accd, v);

        // ---- fc_rgb + sigmoid (models.py:75), 3-row GEMV on the VALU
        float rgb[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float part = 0.0f;
            const float* wr = lds_wrgb + (ch * 4 + g) * N::KD;
#pragma unroll
            for (int s = 0; s < N::KD; s += 4) {
                const f32x4 w4 = *reinterpret_cast<const f32x4*>(wr + s);
#pragma unroll
                for (int q = 0; q < 4; ++q) part = fmaf(v[s + q], w4[q], part);
            }
            const float x = group_sum(part) + tail_bias[1 + ch];
            rgb[ch] = 1.0f / (1.0f + expf(-x));
        }
        if (valid && g == 0) {
            f32x4 o4 = {rgb[0], rgb[1], rgb[2], sigma};
            *reinterpret_cast<f32x4*>(args.out + 4 * sample) = o4;
        }
    }
}

}  // namespace nm
