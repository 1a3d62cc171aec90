// Text formatting shared by the host-side file writers (obj_writer.cpp, ply_writer.cpp): a number printed the way Python's
// "{}".format(tensor_element) prints it -- repr() of the fp32 value widened to a double (shortest round-trip digits; fixed
// notation for 1e-4 <= |x| < 1e16 with a trailing ".0" on integral values, otherwise d[.ddd]e+XX), which reads back to the
// same fp32 -- and the split of n lines over the host threads into per-chunk buffers that are written in order.
#pragma once
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

namespace nm {

// repr(float(x)) appended to out
inline void append_repr(std::string& out, float x32) {
    const double x = static_cast<double>(x32);
    if (std::isnan(x)) { out += "nan"; return; }
    if (std::isinf(x)) { out += x < 0 ? "-inf" : "inf"; return; }
    char buf[64];
    const auto res = std::to_chars(buf, buf + sizeof(buf) - 1, x, std::chars_format::scientific);   // shortest digits
    *res.ptr = '\0';
    const char* p = buf;
    const char* end = res.ptr;
    if (*p == '-') { out += '-'; ++p; }
    char digits[32];
    int nd = 0;
    const char* e = p;
    for (; e < end && *e != 'e'; ++e)
        if (*e != '.') digits[nd++] = *e;
    const int exp10 = std::atoi(e + 1);
    const int decpt = exp10 + 1;                      // value = 0.d1d2... * 10^decpt
    if (x == 0.0) { out += "0.0"; return; }
    if (decpt <= -4 || decpt > 16) {                  // float_repr_style 'short', format code 'r'
        out += digits[0];
        if (nd > 1) { out += '.'; out.append(digits + 1, nd - 1); }
        const int ex = decpt - 1;
        out += 'e';
        out += ex < 0 ? '-' : '+';
        const int a = ex < 0 ? -ex : ex;
        if (a < 10) out += '0';
        out += std::to_string(a);
    } else if (decpt <= 0) {
        out += "0.";
        out.append(static_cast<size_t>(-decpt), '0');
        out.append(digits, nd);
    } else if (decpt >= nd) {
        out.append(digits, nd);
        out.append(static_cast<size_t>(decpt - nd), '0');
        out += ".0";
    } else {
        out.append(digits, decpt);
        out += '.';
        out.append(digits + decpt, nd - decpt);
    }
}

inline void append_triple(std::string& out, const float* v) {
    append_repr(out, v[0]); out += ' ';
    append_repr(out, v[1]); out += ' ';
    append_repr(out, v[2]);
}

template <typename F>
void parallel_chunks(int64_t n, int threads, std::vector<std::string>& bufs, F&& format_range) {
    const int64_t per = (n + threads - 1) / threads;
    bufs.assign(threads, std::string());
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t) {
        const int64_t lo = t * per, hi = lo + per < n ? lo + per : n;
        if (lo >= hi) break;
        pool.emplace_back([&, t, lo, hi] { bufs[t].reserve(static_cast<size_t>(hi - lo) * 64); format_range(bufs[t], lo, hi); });
    }
    for (auto& th : pool) th.join();
}

}  // namespace nm

namespace nm {

inline int writer_threads() {
    const unsigned hw = std::thread::hardware_concurrency();
    return hw == 0 ? 4 : (hw > 32 ? 32 : static_cast<int>(hw));
}

}  // namespace nm
