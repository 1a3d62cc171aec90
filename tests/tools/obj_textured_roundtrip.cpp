// Stand-alone host program for the sanitizers: writes a small textured OBJ with nm_export_obj_textured (and the plain one with
// nm_export_obj), reads both back with a reader of its own and compares every number and index; then the argument errors.
// Host code only -- no device is touched.  Build and run on the CPU:
//
//     hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//           tests/tools/obj_textured_roundtrip.cpp nerfmeshes_amd/csrc/obj_writer.cpp -o obj_textured_roundtrip
//     ./obj_textured_roundtrip [directory]
//
// Prints OBJ_TEXTURED_ROUNDTRIP_OK and returns 0 when everything agrees.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/nerfmeshes_hip.h"

namespace nm {
static std::string last_error;
void set_error(const std::string& msg) { last_error = msg; }     // the library's own lives in a HIP unit
}  // namespace nm

struct Obj {
    std::vector<float> v, c, vn, vt;
    std::vector<int64_t> fv, ft, fn;
    std::string mtllib, material;
    std::vector<std::string> v_lines;                            // the `v` and `vn` lines as written
};

static bool read_obj(const std::string& path, Obj& o) {
    std::ifstream in(path);
    if (!in) return false;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string tag;
        ss >> tag;
        if (tag == "v") {
            float x[6];
            int n = 0;
            std::string word;
            while (n < 6 && ss >> word) x[n++] = std::strtof(word.c_str(), nullptr);
            if (n != 3 && n != 6) return false;
            o.v.insert(o.v.end(), x, x + 3);
            if (n == 6) o.c.insert(o.c.end(), x + 3, x + 6);
            o.v_lines.push_back(line);
        } else if (tag == "vn" || tag == "vt") {
            std::string word;
            std::vector<float>& into = tag == "vn" ? o.vn : o.vt;
            int n = 0;
            while (ss >> word) { into.push_back(std::strtof(word.c_str(), nullptr)); ++n; }
            if (n != (tag == "vn" ? 3 : 2)) return false;
            if (tag == "vn") o.v_lines.push_back(line);
        } else if (tag == "f") {
            std::string entry;
            int n = 0;
            while (ss >> entry) {
                const size_t a = entry.find('/'), b = entry.find('/', a + 1);
                if (a == std::string::npos || b == std::string::npos) return false;
                const std::string t = entry.substr(a + 1, b - a - 1);
                o.fv.push_back(std::atoll(entry.substr(0, a).c_str()));
                o.ft.push_back(t.empty() ? 0 : std::atoll(t.c_str()));
                o.fn.push_back(std::atoll(entry.substr(b + 1).c_str()));
                ++n;
            }
            if (n != 3) return false;
        } else if (tag == "mtllib") {
            ss >> o.mtllib;
        } else if (tag == "usemtl") {
            ss >> o.material;
        } else if (!tag.empty()) {
            return false;
        }
    }
    return true;
}

static bool same_bits(const std::vector<float>& got, const std::vector<float>& want) {
    return got.size() == want.size() && (got.empty() || std::memcmp(got.data(), want.data(), 4 * got.size()) == 0);
}

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            std::fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #cond, nm::last_error.c_str()); \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    const std::string textured = dir + "/roundtrip_textured.obj", plain = dir + "/roundtrip_plain.obj";
    const int64_t nv = 257, nf = 401;                            // more lines than writer threads, in uneven chunks
    std::vector<float> v(3 * nv), c(3 * nv), n(3 * nv), uv(6 * nf);
    std::vector<int32_t> f(3 * nf);
    uint32_t state = 12345u;
    auto next = [&] { state = state * 1664525u + 1013904223u; return state; };
    for (auto* a : {&v, &c, &n, &uv})
        for (float& x : *a) x = (float)((int32_t)next() / 65536) * std::ldexp(1.0f, (int)(next() % 40) - 30);
    v[0] = 1e-30f; v[1] = -0.0f; v[2] = 123456.789f; v[3] = 1e16f; v[4] = 9.999999e15f; v[5] = 1e-4f;
    uv[0] = 0.0f; uv[1] = 1.0f; uv[2] = 0.5f / 16384.0f; uv[3] = 32767.0f / 32768.0f;
    for (int32_t& i : f) i = (int32_t)(next() % nv);

    CHECK(nm_export_obj_textured(v.data(), nv, c.data(), nv, n.data(), nv, f.data(), nf, uv.data(), "roundtrip_textured.mtl",
                                 "material_0", textured.c_str()) == 0);
    CHECK(nm_export_obj(v.data(), nv, c.data(), nv, n.data(), nv, f.data(), nf, plain.c_str()) == 0);
    Obj a, b;
    CHECK(read_obj(textured, a) && read_obj(plain, b));
    CHECK(a.mtllib == "roundtrip_textured.mtl" && a.material == "material_0" && b.mtllib.empty() && b.material.empty());
    CHECK(same_bits(a.v, v) && same_bits(a.c, c) && same_bits(a.vn, n) && same_bits(a.vt, uv));
    CHECK(same_bits(b.v, v) && same_bits(b.c, c) && same_bits(b.vn, n) && b.vt.empty());
    CHECK(a.v_lines == b.v_lines && (int64_t)a.v_lines.size() == 2 * nv);
    CHECK((int64_t)a.fv.size() == 3 * nf && a.fv == b.fv && a.fn == b.fn && a.fv == a.fn);
    for (int64_t i = 0; i < 3 * nf; ++i) CHECK(a.fv[i] == f[i] + 1 && a.ft[i] == i + 1 && b.ft[i] == 0);

    // colours only while they last, no normals, no faces, nothing at all
    CHECK(nm_export_obj_textured(v.data(), nv, c.data(), 5, nullptr, 0, f.data(), nf, uv.data(), "m.mtl", "m", textured.c_str()) == 0);
    Obj few;
    CHECK(read_obj(textured, few) && (int64_t)few.c.size() == 15 && few.vn.empty() && same_bits(few.vt, uv));
    CHECK(nm_export_obj_textured(nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, uv.data(), "m.mtl", "m", textured.c_str()) == 0);
    Obj none;
    CHECK(read_obj(textured, none) && none.v.empty() && none.vt.empty() && none.fv.empty() && none.mtllib == "m.mtl");

    // argument errors: status 2 and a message, nothing written through a null pointer
    CHECK(nm_export_obj_textured(v.data(), nv, nullptr, 0, nullptr, 0, f.data(), nf, nullptr, "m.mtl", "m", textured.c_str()) == 2);
    CHECK(nm_export_obj_textured(nullptr, nv, nullptr, 0, nullptr, 0, f.data(), nf, uv.data(), "m.mtl", "m", textured.c_str()) == 2);
    CHECK(nm_export_obj_textured(v.data(), nv, nullptr, 0, nullptr, 0, f.data(), nf, uv.data(), nullptr, "m", textured.c_str()) == 2);
    CHECK(nm_export_obj_textured(v.data(), nv, nullptr, 0, nullptr, 0, f.data(), nf, uv.data(), "two words", "m", textured.c_str()) == 2);
    CHECK(nm_export_obj_textured(v.data(), nv, nullptr, 0, nullptr, 0, f.data(), nf, uv.data(), "m.mtl", "", textured.c_str()) == 2);
    CHECK(nm_export_obj_textured(v.data(), nv, nullptr, 0, nullptr, 0, f.data(), nf, uv.data(), "m.mtl", "m", nullptr) == 2);
    CHECK(nm_export_obj_textured(v.data(), -1, nullptr, 0, nullptr, 0, f.data(), nf, uv.data(), "m.mtl", "m", textured.c_str()) == 2);
    CHECK(nm_export_obj_textured(v.data(), nv, nullptr, 0, nullptr, 0, f.data(), nf, uv.data(), "m.mtl", "m",
                                 (dir + "/no/such/directory/x.obj").c_str()) == 6);
    std::remove(textured.c_str());
    std::remove(plain.c_str());
    std::puts("OBJ_TEXTURED_ROUNDTRIP_OK");
    return 0;
}
