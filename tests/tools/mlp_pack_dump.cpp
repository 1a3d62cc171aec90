// Fingerprints of the weight packer's index maps (nerfmeshes_amd/csrc/mlp_pack.h) over a fixed matrix of network
// descriptions, as one JSON document on stdout.  Host only: tests/test_mlp_pack.py compiles this with g++ and compares the
// output with tests/golden/mlp_pack_fingerprints.json.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mlp_pack.h"

using namespace nm;

static uint64_t fnv1a(const std::vector<int32_t>& v, uint64_t h = 1469598103934665603ull) {
    for (int32_t e : v)
        for (int b = 0; b < 4; ++b) {        // little-endian bytes
            h ^= ((uint32_t)e >> (8 * b)) & 0xffu;
            h *= 1099511628211ull;
        }
    return h;
}

static bool g_first = true;
static void open_case(const char* family, const nm_mlp_desc& d, const std::string& extra) {
    printf("%s\n\"%s H%d L%d s%d FX%d FD%d in%d%d v%d%s\": {", g_first ? "" : ",", family, d.hidden_size, d.num_layers, d.skip_step,
           d.num_encoding_fn_xyz, d.num_encoding_fn_dir, d.include_input_xyz, d.include_input_dir, d.use_viewdirs, extra.c_str());
    g_first = false;
}

static nm_mlp_desc desc(int H, int L, int skip, int FX, int FD, int inc_x, int inc_d, int view) {
    nm_mlp_desc d;
    d.num_layers = L; d.hidden_size = H; d.skip_step = skip; d.num_encoding_fn_xyz = FX; d.num_encoding_fn_dir = FD;
    d.include_input_xyz = inc_x; d.include_input_dir = inc_d; d.use_viewdirs = view;
    return d;
}

// the fp32 stream of a fused plan: before and with the plain-copy tail
static void dump_f32(const char* family, const nm_mlp_desc& d, const StreamGeometry& geo, bool with_b3 = false) {
    std::vector<int32_t> index;
    const BlobLayout lay = build_index_f32(index, d, geo);
    open_case(family, d, geo.tuned ? "" : " nt" + std::to_string(geo.nt) + " kch" + std::to_string(geo.kch));
    printf("\"n\": %zu, \"off\": [%zu, %zu, %zu, %zu], \"skip_mask\": %u, \"ch\": [%d, %d], \"fnv\": \"%016llx\"", index.size(), lay.off_bias,
           lay.off_wa, lay.off_wr, lay.off_bwd, lay.skip_mask, lay.chx, lay.chd, (unsigned long long)fnv1a(index));
    const size_t plain_off = append_plain_copies(index, d);
    printf(", \"plain_off\": %zu, \"n_tail\": %zu, \"fnv_tail\": \"%016llx\"", plain_off, index.size(), (unsigned long long)fnv1a(index));
    if (with_b3) {
        std::vector<int32_t> b3;
        build_index_b3(b3, d);
        printf(", \"b3_n\": %zu, \"b3_fnv\": \"%016llx\"", b3.size(), (unsigned long long)fnv1a(b3));
    }
    printf("}");
}

static void dump_layerwise(const nm_mlp_desc& d) {
    std::vector<int32_t> index;
    LwNet net;
    memset(&net, 0, sizeof(net));
    build_index_layerwise(index, d, &net);
    open_case("layerwise", d, "");
    printf("\"n\": %zu, \"skip_mask\": %u, \"fnv\": \"%016llx\", \"dims\": [%d, %d, %d, %d, %d, %d, %d, %d, %d, %d], \"linears\": [", index.size(),
           net.skip_mask, (unsigned long long)fnv1a(index), net.L, net.H, net.H2, net.dx, net.dd, net.flat, net.fx, net.fd, net.inc_x, net.inc_d);
    std::vector<const LwLinear*> all = {&net.layer1};
    for (int i = 0; i < d.num_layers - 1; ++i) all.push_back(&net.xyz[i]);
    all.push_back(&net.alpha); all.push_back(&net.feat); all.push_back(&net.dir); all.push_back(&net.rgb);
    for (size_t i = 0; i < all.size(); ++i)
        printf("%s[%zu, %zu, %zu, %d, %d]", i ? ", " : "", all[i]->wt, all[i]->w, all[i]->b, all[i]->out, all[i]->in);
    printf("]");
    append_plain_copies(index, d);
    printf(", \"n_tail\": %zu, \"fnv_tail\": \"%016llx\"}", index.size(), (unsigned long long)fnv1a(index));
}

int main() {
    printf("{");
    const int inc[3][2] = {{1, 1}, {0, 1}, {1, 0}};
    // tuned family: the shipped shapes
    for (int H : {64, 128, 256})
        for (int FX : {6, 10})
            for (int L : {2, 3, 4, 8})
                for (int skip : {1, 2, 4})
                    for (int view : {0, 1})
                        for (const auto& in : inc) dump_f32("tuned", desc(H, L, skip, FX, 4, in[0], in[1], view), StreamGeometry{H / 16, 8, true});
    // generic family: (nt, kch) given directly (the plan table is not visible from here)
    const int widths[] = {7, 16, 40, 100, 144, 256, 320, 400, 512};
    int n = 0;
    for (int H : widths) {
        const int nt0 = (H + 15) / 16;
        for (int nt : {nt0, nt0 + 2}) {
            const int kch = nt <= 24 ? 8 : 4;
            // every encoding pair (single- and two-part stages); depth, skip, view and the include flags vary along
            for (int FX : {0, 3, 10, 15, 20, 31})
                for (int FD : {0, 4, 16}) {
                    const int Ls[] = {2, 5, 8}, L = Ls[n % 3], skip = (n / 3) % 2 ? 4 : 2, view = (n / 2) % 2;
                    const int inc_x = FX == 0 ? 1 : (n / 5) % 2, inc_d = FD == 0 ? 1 : (n / 7) % 2;
                    dump_f32("generic", desc(H, L, skip, FX, FD, inc_x, inc_d, view), StreamGeometry{nt, kch, false});
                    ++n;
                }
        }
        // depth x skip x view at one encoding
        for (int L : {2, 5, 8})
            for (int skip : {2, 4})
                for (int view : {0, 1}) dump_f32("generic", desc(H, L, skip, 10, 4, 1, 1, view), StreamGeometry{nt0, nt0 <= 24 ? 8 : 4, false});
    }
    // bf16x3: the six instantiated shapes
    for (int H : {64, 128, 256})
        for (int FX : {6, 10})
            for (int L : {4, 8}) dump_f32("bf16x3", desc(H, L, 4, FX, 4, 1, 1, 1), StreamGeometry{H / 16, 8, true}, true);
    // layer-wise path
    for (int H : {600, 1024})
        for (int FX : {10, 32})
            for (int view : {0, 1}) dump_layerwise(desc(H, 8, 4, FX, view ? 4 : 0, 1, 1, view));
    printf("\n}\n");
    return 0;
}
