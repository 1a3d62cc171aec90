// OBJ text writer (host code): the byte-for-byte output of the reference's export_obj
// (/root/reference/src/nerf/nerf_helpers.py:86-111) --
//     v x y z [r g b]      one line per vertex; colours only while the diffuse array lasts
//     vn x y z
//     f a//a b//b c//c     1-based
// and, for a textured mesh (nm_export_obj_textured: an addition), `mtllib`, `vt u v` and `usemtl` lines around the same `v` and
// `vn` lines, with `f a/t/a b/t/b c/t/c` --
// with every number printed the way Python's "{}".format(tensor_element) prints it: repr() of the fp32 value widened
// to a double (shortest round-trip digits; fixed notation for 1e-4 <= |x| < 1e16 with a trailing ".0" on integral
// values, otherwise d[.ddd]e+XX; nm_text.h).  Once marching cubes runs on the GPU (0.8 ms) the per-element Python writer is the
// bottleneck of mesh_nerf (10.6 s for the 480^3 mesh, 209 MB of text); here the lines are formatted by all host
// threads into per-chunk buffers and written in order.
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "nm_internal.h"
#include "nm_text.h"


using namespace nm;

// One writer for both entries: h_face_uv null -> the plain file; else `mtllib`, the `vt` lines, `usemtl` and `f a/t/a` entries
// around the same `v` and `vn` lines
static int write_obj(const float* h_vertices, int64_t num_vertices, const float* h_diffuse, int64_t num_diffuse,
                     const float* h_normals, int64_t num_normals, const int32_t* h_triangles, int64_t num_triangles,
                     const float* h_face_uv, const char* mtllib, const char* material, const char* path) {
    NM_REQUIRE(path && num_vertices >= 0 && num_diffuse >= 0 && num_normals >= 0 && num_triangles >= 0, "bad argument");
    NM_REQUIRE((h_vertices || !num_vertices) && (h_diffuse || !num_diffuse) && (h_normals || !num_normals) &&
               (h_triangles || !num_triangles), "null array");
    FILE* f = std::fopen(path, "wb");
    if (!f) { set_error(std::string("cannot open ") + path); return 6; }
    const int threads = writer_threads();
    std::vector<std::string> bufs;
    bool ok = true;
    auto flush = [&] { for (const std::string& b : bufs) ok = ok && std::fwrite(b.data(), 1, b.size(), f) == b.size(); };
    auto line = [&](const std::string& text) { bufs.assign(1, text); flush(); };

    if (mtllib) line(std::string("mtllib ") + mtllib + "\n");

    parallel_chunks(num_vertices, threads, bufs, [&](std::string& out, int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            out += "v ";
            append_triple(out, h_vertices + 3 * i);
            if (i < num_diffuse) { out += ' '; append_triple(out, h_diffuse + 3 * i); }
            out += '\n';
        }
    });
    flush();
    parallel_chunks(num_normals, threads, bufs, [&](std::string& out, int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) { out += "vn "; append_triple(out, h_normals + 3 * i); out += '\n'; }
    });
    flush();
    if (h_face_uv) {
        parallel_chunks(3 * num_triangles, threads, bufs, [&](std::string& out, int64_t lo, int64_t hi) {
            for (int64_t i = lo; i < hi; ++i) {
                out += "vt ";
                append_repr(out, h_face_uv[2 * i]); out += ' '; append_repr(out, h_face_uv[2 * i + 1]);
                out += '\n';
            }
        });
        flush();
        line(std::string("usemtl ") + material + "\n");
    }
    parallel_chunks(num_triangles, threads, bufs, [&](std::string& out, int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            out += 'f';
            for (int k = 0; k < 3; ++k) {
                const std::string id = std::to_string(static_cast<int64_t>(h_triangles[3 * i + k]) + 1);
                out += ' '; out += id; out += '/';
                if (h_face_uv) out += std::to_string(3 * i + k + 1);
                out += '/'; out += id;
            }
            out += '\n';
        }
    });
    flush();
    ok = std::fclose(f) == 0 && ok;
    if (!ok) { set_error(std::string("short write to ") + path); return 6; }
    return 0;
}

extern "C" int nm_export_obj(const float* h_vertices, int64_t num_vertices, const float* h_diffuse, int64_t num_diffuse,
                             const float* h_normals, int64_t num_normals, const int32_t* h_triangles,
                             int64_t num_triangles, const char* path) {
    return write_obj(h_vertices, num_vertices, h_diffuse, num_diffuse, h_normals, num_normals, h_triangles, num_triangles, nullptr,
                     nullptr, nullptr, path);
}

static bool plain_name(const char* s) {        // what a `mtllib` / `usemtl` line can carry: one word, no line break
    if (!s || !*s) return false;
    for (; *s; ++s)
        if (*s == '\n' || *s == '\r' || *s == ' ' || *s == '\t') return false;
    return true;
}

extern "C" int nm_export_obj_textured(const float* h_vertices, int64_t num_vertices, const float* h_diffuse, int64_t num_diffuse,
                                      const float* h_normals, int64_t num_normals, const int32_t* h_triangles,
                                      int64_t num_triangles, const float* h_face_uv, const char* mtllib, const char* material,
                                      const char* path) {
    NM_REQUIRE(plain_name(mtllib) && plain_name(material), "textured OBJ: mtllib and material must be names without blanks");
    NM_REQUIRE(h_face_uv != nullptr, "textured OBJ: no texture coordinates");
    return write_obj(h_vertices, num_vertices, h_diffuse, num_diffuse, h_normals, num_normals, h_triangles, num_triangles, h_face_uv,
                     mtllib, material, path);
}
