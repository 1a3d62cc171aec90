// PLY writer (host code) of the surface point cloud: one `vertex` element with the property names of the reference's
// export_ply (src/mesh_surface_ray.py:46-58) --
//     x y z nx ny nz      float
//     red green blue      uchar
// ascii (the reference's `text = True`): one vertex per line, the floats printed as the OBJ writer prints them (repr of the
// fp32 value widened to a double: reads back to the same fp32; nm_text.h), the colours as decimal integers.  Binary:
// binary_little_endian 1.0, 27 bytes per vertex.  The reference writes through the `plyfile` package; this is the same
// element and property layout, not a claim of byte equality with that package's output.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "nm_internal.h"
#include "nm_text.h"

using namespace nm;

extern "C" int nm_export_ply(const float* h_points, const float* h_normals, const uint8_t* h_colors_u8, int64_t n,
                             int binary, const char* path) {
    NM_REQUIRE(path && n >= 0, "bad argument");
    NM_REQUIRE((h_points && h_normals && h_colors_u8) || n == 0, "null array");
    FILE* f = std::fopen(path, "wb");
    if (!f) { set_error(std::string("cannot open ") + path); return 6; }
    std::string head = "ply\nformat ";
    head += binary ? "binary_little_endian" : "ascii";
    head += " 1.0\nelement vertex " + std::to_string(n) + "\n";
    for (const char* name : {"x", "y", "z", "nx", "ny", "nz"}) head += std::string("property float ") + name + "\n";
    for (const char* name : {"red", "green", "blue"}) head += std::string("property uchar ") + name + "\n";
    head += "end_header\n";
    bool ok = std::fwrite(head.data(), 1, head.size(), f) == head.size();
    std::vector<std::string> bufs;
    parallel_chunks(n, writer_threads(), bufs, [&](std::string& out, int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            if (binary) {                                  // the host is little-endian (x86-64), as the device is
                out.append(reinterpret_cast<const char*>(h_points + 3 * i), 12);
                out.append(reinterpret_cast<const char*>(h_normals + 3 * i), 12);
                out.append(reinterpret_cast<const char*>(h_colors_u8 + 3 * i), 3);
            } else {
                append_triple(out, h_points + 3 * i); out += ' ';
                append_triple(out, h_normals + 3 * i);
                for (int k = 0; k < 3; ++k) { out += ' '; out += std::to_string(static_cast<int>(h_colors_u8[3 * i + k])); }
                out += '\n';
            }
        }
    });
    for (const std::string& b : bufs) ok = ok && std::fwrite(b.data(), 1, b.size(), f) == b.size();
    ok = std::fclose(f) == 0 && ok;
    if (!ok) { set_error(std::string("short write to ") + path); return 6; }
    return 0;
}
