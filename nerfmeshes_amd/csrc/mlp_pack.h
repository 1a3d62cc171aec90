// The fused MLP's weight packer: every packed image as an INDEX MAP (entry = tensor id << 24 | element of that tensor, -1 = 0.0f)
// that one gather kernel (mlp_api.hip) turns into device memory.  Pure host arithmetic over the C++ standard library -- no HIP --
// so that tests/test_mlp_pack.py checks it without a GPU (tests/tools/mlp_pack_dump.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <array>
#include <vector>

#include "../../include/nerfmeshes_hip.h"

namespace nm {

// Flat addressing of the trainable tensors
enum TensorId : int {
    T_L1W = 0, T_L1B = 1, T_XYZ0 = 2 /* + 2i weight, + 2i + 1 bias */, T_FEATW = 66, T_FEATB, T_ALPHAW, T_ALPHAB,
    T_DIRW, T_DIRB, T_RGBW, T_RGBB, T_COUNT
};

inline bool is_skip(const nm_mlp_desc& d, int i) {   // models.py:37,63
    return i % d.skip_step == 0 && i > 0 && i != d.num_layers - 1;
}

inline int encoded_width(int F, int include_input) { return 6 * F + (include_input ? 3 : 0); }   // modules.py:26-34

// ---- the layer walk: every torch.nn.Linear of FlexibleNeRFModel (models.py:60-80), in the order
// layer1, layers_xyz[0 .. L-2], fc_alpha, [fc_feat, layers_dir[0],] fc_rgb (use_viewdirs = 0: rows 0..2 of fc_out).
// A trunk layer's input is [the hidden activation (`hidden_in` columns) | an encoding]; the heads are GEMV rows.
enum Encoding : int { ENC_NONE = 0, ENC_XYZ, ENC_DIR };
struct Linear {
    enum Kind : int { LAYER1, XYZ, ALPHA, FEAT, DIR, RGB } kind;
    int index;            // XYZ: i of layers_xyz[i]
    int w, b;             // tensor ids of weight (out x in, row-major) and bias (out)
    int out, in;
    int hidden_in;        // leading input columns that are a hidden activation
    Encoding enc;         // what the remaining in - hidden_in columns are
    bool head() const { return kind == ALPHA || kind == RGB; }
};

inline std::vector<Linear> network_layers(const nm_mlp_desc& d) {
    const int H = d.hidden_size, dx = encoded_width(d.num_encoding_fn_xyz, d.include_input_xyz);
    const int dd = encoded_width(d.num_encoding_fn_dir, d.include_input_dir);
    std::vector<Linear> v;
    v.push_back({Linear::LAYER1, 0, T_L1W, T_L1B, H, dx, 0, ENC_XYZ});
    for (int i = 0; i < d.num_layers - 1; ++i) {
        const bool skip = is_skip(d, i);       // cat(hidden, xyz): models.py:65
        v.push_back({Linear::XYZ, i, T_XYZ0 + 2 * i, T_XYZ0 + 2 * i + 1, H, H + (skip ? dx : 0), H, skip ? ENC_XYZ : ENC_NONE});
    }
    v.push_back({Linear::ALPHA, 0, T_ALPHAW, T_ALPHAB, 1, H, H, ENC_NONE});
    if (d.use_viewdirs) {
        v.push_back({Linear::FEAT, 0, T_FEATW, T_FEATB, H, H, H, ENC_NONE});
        v.push_back({Linear::DIR, 0, T_DIRW, T_DIRB, H / 2, H + dd, H, ENC_DIR});      // cat(feat, view): models.py:72
        v.push_back({Linear::RGB, 0, T_RGBW, T_RGBB, 3, H / 2, H / 2, ENC_NONE});
    } else {
        v.push_back({Linear::RGB, 0, T_RGBW, T_RGBB, 3, H, H, ENC_NONE});
    }
    return v;
}

// the caller's tensor behind a tensor id
inline const float* weight_tensor(const nm_mlp_weights& w, int t) {
    switch (t) {
        case T_L1W: return w.layer1_w;
        case T_L1B: return w.layer1_b;
        case T_FEATW: return w.fc_feat_w;
        case T_FEATB: return w.fc_feat_b;
        case T_ALPHAW: return w.fc_alpha_w;
        case T_ALPHAB: return w.fc_alpha_b;
        case T_DIRW: return w.layers_dir0_w;
        case T_DIRB: return w.layers_dir0_b;
        case T_RGBW: return w.fc_rgb_w;
        case T_RGBB: return w.fc_rgb_b;
        default: return ((t - T_XYZ0) & 1) ? w.layers_xyz_b[(t - T_XYZ0) / 2] : w.layers_xyz_w[(t - T_XYZ0) / 2];
    }
}

inline int64_t mlp_macs(const nm_mlp_desc& d, bool density_only) {
    int64_t macs = 0;
    for (const Linear& l : network_layers(d)) {
        macs += (int64_t)l.out * l.in;
        if (density_only && l.kind == Linear::ALPHA) break;      // (use_viewdirs = 0: row 3 of fc_out)
    }
    return macs;
}

// ---- pieces of an index map ------------------------------------------------------------------------------------------
inline void pack_range(std::vector<int32_t>& out, int tensor, int count, int padded = 0) {
    for (int i = 0; i < (padded > count ? padded : count); ++i) out.push_back(i < count ? ((tensor << 24) | i) : -1);
}

inline void pad_to(std::vector<int32_t>& v, size_t multiple) {
    while (v.size() % multiple) v.push_back(-1);
}

// ---- fp32 stream (mlp_device.h, mlp_device_r3.h: the tuned kernels; mlp_device_g.h, mlp_device_gs.h: the generic family) ------
// The two families stream the same image; what differs is the geometry:
//                          tuned (exactly H = 16 nt)                      generic (H <= 16 nt, zero padded)
//   encoding stage         argument k-steps + the identity k-step,        argument k-steps, the identity k-step only when the input
//                          always                                         is included, zero k-steps up to whole chunks of kch
//   1 KiB operand block    min(4, tiles) tiles                            4 tiles (those beyond the layer's are zeros)
//   behind a stream        1024 zero entries (DMA granularity, 4 KiB)     8192 (a tail fetch may run one 32 KiB chunk past it)
struct StreamGeometry {
    int nt;         // width class: the hidden activation is nt MFMA tiles of 16 features
    int kch;        // k-steps per LDS chunk (generic only)
    bool tuned;
    int block_tiles(int ntiles) const { return tuned && ntiles < 4 ? ntiles : 4; }
    size_t tail() const { return tuned ? 1024 : 8192; }
};

// Source column (input feature) of the weight matrix that lane group g consumes at k-step s.
using StepCols = std::array<int, 4>;  // -1 = zero padding

// hidden activation of `width` features in nt MFMA tiles: k-step s = 4*tile + reg, group g holds feature 16*tile + 4*g + reg
// (see nerf_mlp.hip header); columns beyond the real width are zero weights
inline void hidden_steps(std::vector<StepCols>& out, int nt, int width, int col_offset) {
    for (int s = 0; s < 4 * nt; ++s) {
        StepCols c;
        for (int g = 0; g < 4; ++g) {
            const int k = 16 * (s >> 2) + 4 * g + (s & 3);
            c[g] = k < width ? col_offset + k : -1;
        }
        out.push_back(c);
    }
}

// positional encoding [x(3) | sin(3F) | cos(3F)], coordinate-major (modules.py:26-34): k-step s carries arguments a0=2s
// (groups 0,1 = sin,cos) and a1=2s+1 (groups 2,3); then the identity step.  Returns the chunk count (generic; 0 for tuned).
inline int encoding_stage(std::vector<StepCols>& out, const StreamGeometry& geo, int F, bool include_input, int col_offset) {
    const int base = col_offset + (include_input ? 3 : 0);
    int n = 0;
    for (int s = 0; s < (3 * F + 1) / 2; ++s, ++n) {
        StepCols c;
        for (int g = 0; g < 4; ++g) {
            const int a = 2 * s + (g >> 1);
            c[g] = a < 3 * F ? base + ((g & 1) ? 3 * F : 0) + a : -1;
        }
        out.push_back(c);
    }
    if (include_input || geo.tuned) {
        StepCols id;
        for (int g = 0; g < 4; ++g) id[g] = (include_input && g < 3) ? col_offset + g : -1;
        out.push_back(id);
        ++n;
    }
    if (geo.tuned) return 0;
    for (; n % geo.kch; ++n) out.push_back(StepCols{-1, -1, -1, -1});
    return n / geo.kch;
}

// Append the A-operand stream of one GEMM: for k-step s, block b of VW tiles, lane l, slot q:
// W[16*(VW*b+q) + (l&15)][cols[s][l>>4]]; `transposed` addresses W^T (the backward stream: output row n is an input column of
// the stored nn.Linear weight).  Tiles beyond ntiles and rows beyond `rows` are zeros.
inline void pack_gemm(std::vector<int32_t>& out, const StreamGeometry& geo, int tensor, int ld, int rows, int ntiles,
                      const std::vector<StepCols>& steps, bool transposed = false) {
    const int vw = geo.block_tiles(ntiles), nb = (ntiles + vw - 1) / vw;
    for (const StepCols& c : steps)
        for (int b = 0; b < nb; ++b)
            for (int l = 0; l < 64; ++l)
                for (int q = 0; q < vw; ++q) {
                    const int n = 16 * (vw * b + q) + (l & 15);
                    const int k = c[l >> 4];
                    const int64_t off = transposed ? (int64_t)k * ld + n : (int64_t)n * ld + k;
                    out.push_back((vw * b + q < ntiles && n < rows && k >= 0) ? (int32_t)((tensor << 24) | (int32_t)off) : -1);
                }
}

// GEMV operand of a head row over a D-layout activation of nt tiles (fc_alpha's layout): [4 lane groups][4 nt]
inline void pack_head_row(std::vector<int32_t>& out, int tensor, int row_offset, int nt, int width) {
    for (int g = 0; g < 4; ++g)
        for (int s = 0; s < 4 * nt; ++s) {
            const int k = 16 * (s >> 2) + 4 * g + (s & 3);
            out.push_back(k < width ? ((tensor << 24) | (row_offset + k)) : -1);
        }
}

struct BlobLayout { size_t off_bias, off_wa, off_wr, off_bwd; uint32_t skip_mask; int chx, chd; };

// The whole blob of a fused plan as an index map: forward stream | biases | fc_alpha | fc_rgb (or fc_out's colour rows) |
// backward stream (the transposed layers in reverse order, hidden columns only).
inline BlobLayout build_index_f32(std::vector<int32_t>& index, const nm_mlp_desc& d, const StreamGeometry& geo) {
    const int H = d.hidden_size, NT = geo.nt, NTD = geo.tuned ? NT / 2 : (NT + 1) / 2;
    const bool no_view = d.use_viewdirs == 0;
    const std::vector<Linear> layers = network_layers(d);
    auto tiles = [&](int width) { return width == H ? NT : NTD; };       // a layer is H or H / 2 wide
    BlobLayout lay{};
    std::vector<StepCols> enc_x, skip_enc, dir_enc, hid, hid_half;
    lay.chx = encoding_stage(enc_x, geo, d.num_encoding_fn_xyz, d.include_input_xyz != 0, 0);
    encoding_stage(skip_enc, geo, d.num_encoding_fn_xyz, d.include_input_xyz != 0, H);
    lay.chd = no_view ? 0 : encoding_stage(dir_enc, geo, d.num_encoding_fn_dir, d.include_input_dir != 0, H);
    hidden_steps(hid, NT, H, 0);
    hidden_steps(hid_half, NTD, H / 2, 0);
    for (const Linear& l : layers) {
        if (l.head()) continue;
        if (l.hidden_in) pack_gemm(index, geo, l.w, l.in, l.out, tiles(l.out), hid);
        if (l.enc) pack_gemm(index, geo, l.w, l.in, l.out, tiles(l.out), l.enc == ENC_DIR ? dir_enc : l.hidden_in ? skip_enc : enc_x);
        if (l.kind == Linear::XYZ && l.enc) lay.skip_mask |= 1u << l.index;
    }
    index.resize(index.size() + geo.tail(), -1);
    pad_to(index, 64);
    lay.off_bias = index.size();
    for (const Linear& l : layers)
        if (!l.head()) pack_range(index, l.b, l.out, 16 * tiles(l.out));
    if (no_view) index.resize(index.size() + 16 * NT + 16 * NTD, -1);      // the kernels' bias layout is the same for both kinds
    pack_range(index, T_ALPHAB, 1);
    pack_range(index, T_RGBB, 3);
    pad_to(index, 64);
    lay.off_wa = index.size();
    pack_head_row(index, T_ALPHAW, 0, NT, H);
    pad_to(index, 64);
    lay.off_wr = index.size();
    const Linear& rgb = layers.back();                                      // over the trunk output, or over layers_dir[0]'s
    for (int c = 0; c < 3; ++c) pack_head_row(index, T_RGBW, c * rgb.in, tiles(rgb.in), rgb.in);
    pad_to(index, 64);
    lay.off_bwd = index.size();
    for (size_t i = layers.size(); i-- > 1;) {                              // delta at a layer's output -> delta at its hidden input
        const Linear& l = layers[i];
        if (!l.head()) pack_gemm(index, geo, l.w, l.in, H, NT, l.out == H ? hid : hid_half, true);
    }
    index.resize(index.size() + geo.tail(), -1);
    pad_to(index, 64);
    return lay;
}

// behind everything the kernels stream: PLAIN copies of the three tensors nm_mlp_linear_layer1_finish multiplies with, filled by
// the same gather -- layers_xyz[0].weight (H, H) row-major, layer1.weight TRANSPOSED (dx, H), layer1.bias (H).  Returns their offset.
inline size_t append_plain_copies(std::vector<int32_t>& index, const nm_mlp_desc& d) {
    const int H = d.hidden_size, dx = encoded_width(d.num_encoding_fn_xyz, d.include_input_xyz);
    pad_to(index, 64);
    const size_t off = index.size();
    pack_range(index, T_XYZ0, H * H);
    for (int j = 0; j < dx; ++j)
        for (int i = 0; i < H; ++i) index.push_back((T_L1W << 24) | (i * dx + j));
    pack_range(index, T_L1B, H);
    return off;
}

// ---- bf16x3 stream (mlp_device_b3.h): per (k-block m, tile nt) unit the fp32 image [lane][j = 0..7] =
// W[16 nt + (l & 15)][column of slot (m, l >> 4, j)]; a device kernel splits it into the three bf16 planes.
using SlotCols = std::array<int, 32>;   // source column of slot 8 g + j of one k-block (-1 = zero)

inline void hidden_blocks(std::vector<SlotCols>& out, int width, int col_offset) {
    for (int m = 0; m < width / 32; ++m) {
        SlotCols c;
        for (int g = 0; g < 4; ++g)
            for (int j = 0; j < 8; ++j) c[8 * g + j] = col_offset + 16 * (2 * m + j / 4) + 4 * g + (j % 4);
        out.push_back(c);
    }
}

// slots 2a, 2a+1 = sin, cos of argument a < 3F (reference columns base + a, base + 3F + a); then the identity coordinates
inline void encoding_blocks(std::vector<SlotCols>& out, int F, bool include_input, int col_offset, int blocks) {
    const int base = col_offset + (include_input ? 3 : 0);
    for (int m = 0; m < blocks; ++m) {
        SlotCols c;
        for (int q = 0; q < 32; ++q) {
            const int s = 32 * m + q;
            if (s < 6 * F) c[q] = base + ((s & 1) ? 3 * F : 0) + s / 2;
            else if (include_input && s - 6 * F < 3) c[q] = col_offset + (s - 6 * F);
            else c[q] = -1;
        }
        out.push_back(c);
    }
}

inline void pack_gemm_b3(std::vector<int32_t>& out, int tensor, int ld, int rows, int ntiles, const std::vector<SlotCols>& blocks) {
    for (const SlotCols& c : blocks)
        for (int nt = 0; nt < ntiles; ++nt)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int n = 16 * nt + (l & 15), k = c[8 * (l >> 4) + j];
                    out.push_back((n < rows && k >= 0) ? (int32_t)((tensor << 24) | (int32_t)((int64_t)n * ld + k)) : -1);
                }
}

// the forward stages of the fp32 stream as units of (k-block, tile); view-dependent networks of the tuned shapes only
inline void build_index_b3(std::vector<int32_t>& index, const nm_mlp_desc& d) {
    const int H = d.hidden_size;
    std::vector<SlotCols> bx, bskip, bdir, bh;
    encoding_blocks(bx, d.num_encoding_fn_xyz, d.include_input_xyz != 0, 0, 2);
    encoding_blocks(bskip, d.num_encoding_fn_xyz, d.include_input_xyz != 0, H, 2);
    encoding_blocks(bdir, d.num_encoding_fn_dir, d.include_input_dir != 0, H, 1);
    hidden_blocks(bh, H, 0);
    for (const Linear& l : network_layers(d)) {
        if (l.head()) continue;
        if (l.hidden_in) pack_gemm_b3(index, l.w, l.in, l.out, l.out / 16, bh);
        if (l.enc) pack_gemm_b3(index, l.w, l.in, l.out, l.out / 16, l.enc == ENC_DIR ? bdir : l.hidden_in ? bskip : bx);
    }
    index.resize(index.size() + 16 * 512, -1);      // DMA granularity / chunk padding
}

// ---- layer-wise path (nerf_layerwise.hip): networks beyond the fused families' limits -----------------------------------
constexpr int LW_MAX_FREQ = 32;     // encoding functions per input the layer-wise path takes (2^31 is past fp32's integer range anyway)

// one torch.nn.Linear (out x in) inside the handle's blob (offsets in floats): W^T (in x out) for the forward products,
// W (out x in) for the delta chain, the bias
struct LwLinear { size_t wt, w, b; int out, in; };

struct LwNet {
    LwLinear layer1, xyz[32], feat, dir, alpha, rgb;     // rgb: fc_rgb (3 x H/2), or rows 0..2 of fc_out (3 x H) without view directions
    int L, H, H2, dx, dd, flat;
    uint32_t skip_mask;                                  // bit i: layers_xyz[i] consumes cat(hidden, xyz encoding)
    int fx, fd, inc_x, inc_d;
    float bands_x[LW_MAX_FREQ], bands_d[LW_MAX_FREQ];
    float* ws;                                           // activation planes of one batch (grow-only)
    size_t ws_floats;
};

// The blob of a layer-wise handle as an index map: per Linear its transpose (in x out: the forward products' A operand), the
// matrix itself (out x in: the delta chain's), its bias; every piece 256-byte aligned (16-byte DMA pieces need it).
inline void build_index_layerwise(std::vector<int32_t>& index, const nm_mlp_desc& d, LwNet* net) {
    const bool no_view = d.use_viewdirs == 0;
    net->L = d.num_layers; net->H = d.hidden_size; net->H2 = d.hidden_size / 2; net->flat = no_view ? 1 : 0;
    net->dx = encoded_width(d.num_encoding_fn_xyz, d.include_input_xyz);
    net->dd = no_view ? 0 : encoded_width(d.num_encoding_fn_dir, d.include_input_dir);
    net->fx = d.num_encoding_fn_xyz; net->fd = no_view ? 0 : d.num_encoding_fn_dir;
    net->inc_x = d.include_input_xyz ? 1 : 0; net->inc_d = d.include_input_dir ? 1 : 0;
    net->skip_mask = 0;
    for (const Linear& l : network_layers(d)) {
        LwLinear* const slot[] = {&net->layer1, &net->xyz[l.index], &net->alpha, &net->feat, &net->dir, &net->rgb};
        LwLinear& p = *slot[l.kind];
        p.out = l.out; p.in = l.in;
        pad_to(index, 64); p.wt = index.size();
        for (int k = 0; k < l.in; ++k)
            for (int o = 0; o < l.out; ++o) index.push_back((l.w << 24) | (o * l.in + k));
        pad_to(index, 64); p.w = index.size();
        pack_range(index, l.w, l.out * l.in);
        pad_to(index, 64); p.b = index.size();
        pack_range(index, l.b, l.out);
        if (l.kind == Linear::XYZ && l.enc) net->skip_mask |= 1u << l.index;
    }
    index.resize(index.size() + 1024, -1);                       // what a piece's rounding may read past the last matrix
}

}  // namespace nm
