// What the host-API test programs (tests/cpp/test_*.cpp, linked against libicebin_hip.so) share: the host API itself, REQUIRE,
// the length-prefixed array files that tests/cpp_programs.py reads back, and the no-GPU report the Python side matches on.
// Templates and inline functions only: a program that uses some of them compiles without an unused-function warning.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../icebin_amd/host/icebin_hip.hpp"

// for main() and for functions that return an exit status
#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

// <int64 n><n values>
template <class T>
bool dump(std::string const &path, std::vector<T> const &v) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const int64_t n = (int64_t)v.size();
    bool ok = std::fwrite(&n, sizeof(n), 1, f) == 1 && std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    return std::fclose(f) == 0 && ok;
}

// a matrix as <name>.row/.col (int32), .val/.wM/.Mw (f64), .dim0/.dim1 (int64)
inline bool dump_matrix(std::string const &out, std::string const &name, icebin::linear::Weighted const &w) {
    std::vector<int> r, c;
    std::vector<double> v;
    w.M_coo(r, c, v);
    std::vector<int64_t> d0, d1;
    for (long x : w.dim_to_sparse(0)) d0.push_back(x);
    for (long x : w.dim_to_sparse(1)) d1.push_back(x);
    return dump(out + "/" + name + ".row", r) && dump(out + "/" + name + ".col", c) && dump(out + "/" + name + ".val", v) &&
           dump(out + "/" + name + ".wM", w.wM()) && dump(out + "/" + name + ".Mw", w.Mw()) && dump(out + "/" + name + ".dim0", d0) &&
           dump(out + "/" + name + ".dim1", d1);
}

// true, after saying so, when `e` is the library's refusal to run without a device: the caller returns 3
inline bool no_gpu(icebin::Exception const &e) {
    if (e.code != IBH_ENODEVICE) return false;
    std::printf("no GPU: %s (no CPU fallback)\n", e.what());
    return true;
}
