// planetile.h -- what the units that read the 1' int16 planes share on the device and around a launch (globalec.hip, etopo1.hip,
// topoo.hip): eight cells at a time, a double from one lane to all, the sort of a tile's 32-bit keys in LDS, and the host's checks
// of a call's plane arguments.  The split of a run at 16-byte boundaries is plane_split.h's.
#pragma once
#include <vector>

#include "common.h"
#include "plane_split.h"

namespace ibh {

typedef short short8 __attribute__((ext_vector_type(8)));

// Eight cells from p.  vec: p is 16-byte aligned -- a plane that is not aligned where FOCEAN (the plane the split was made for)
// is goes cell by cell.
__device__ __forceinline__ short8 load8(const int16_t *p, bool vec) {
    if (vec) return *reinterpret_cast<const short8 *>(p);
    short8 v;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = p[k];
    return v;
}
__device__ __forceinline__ void store8(int16_t *p, short8 v, bool vec) {
    if (vec) { *reinterpret_cast<short8 *>(p) = v; return; }
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = v[k];
}

// lane `lane`'s v in every lane (lane is uniform)
__device__ __forceinline__ double lane_bcast(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// R compare-exchange steps of the bitonic stage k (distances j, j / 2, ..., jl = j >> (R - 1)) on 2^R keys held in registers: the
// keys whose indices differ in those R bits only.  One trip through LDS and one barrier in place of R.  T threads.
template <int T, int R>
__device__ __forceinline__ void bitonic_pass(uint32_t *s, int n2, int k, int j, int tid) {
    constexpr int E = 1 << R;
    const int jl = j >> (R - 1);
    for (int t = tid; t < (n2 >> R); t += T) {
        const int base = ((t & ~(jl - 1)) << R) | (t & (jl - 1));       // t with R zero bits put in at jl
        const bool asc = (base & k) == 0;       // (k > j: the direction bit is none of the R)
        uint32_t e[E];
#pragma unroll
        for (int m = 0; m < E; ++m) e[m] = s[base + m * jl];
#pragma unroll
        for (int d = E >> 1; d > 0; d >>= 1) {
#pragma unroll
            for (int m = 0; m < E; ++m) {
                if (m & d) continue;
                const uint32_t a = e[m], b = e[m | d];
                if ((a > b) == asc) { e[m] = b; e[m | d] = a; }
            }
        }
#pragma unroll
        for (int m = 0; m < E; ++m) s[base + m * jl] = e[m];
    }
}

// The n keys s[0, n) of a workgroup of T threads, ascending: padded with ~0 to a power of two (no key is ~0) and sorted by the
// bitonic network, three of its steps to a trip through LDS.  The caller's barrier has made the n keys visible; the last trip's
// barrier has made the sorted keys visible.
template <int T>
__device__ __forceinline__ void lds_sort_keys(uint32_t *s, int n, int tid) {
    const int n2 = pow2_ceil(n);
    for (int c = n + tid; c < n2; c += T) s[c] = 0xFFFFFFFFu;
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0;) {
            if (j >= 4) { bitonic_pass<T, 3>(s, n2, k, j, tid); j >>= 3; }
            else if (j == 2) { bitonic_pass<T, 2>(s, n2, k, j, tid); j = 0; }
            else { bitonic_pass<T, 1>(s, n2, k, j, tid); j = 0; }
            __syncthreads();
        }
    }
}

// ---- the host's checks of a call's planes, all before a device is touched ---------------------------------------------------------
struct PlaneArg {
    const void *p;
    size_t bytes;
    const char *name;
    int align;          // 2: int16, 8: double
    bool out;
    bool optional;      // may be null
};
// Over all arguments in turn: no NULL plane (but an optional one), every plane aligned, no output over an argument before it.
// overlap_fmt words the last for the unit: it takes the unit, the output's name and the other argument's.
inline void check_plane_args(const char *unit, const PlaneArg *a, int n, const char *overlap_fmt = "%s: the output %s overlaps %s") {
    for (int k = 0; k < n; ++k) IBH_CHECK(a[k].p || a[k].optional, "%s: %s is null", unit, a[k].name);
    for (int k = 0; k < n; ++k)
        IBH_CHECK(((uintptr_t)a[k].p & (uintptr_t)(a[k].align - 1)) == 0, "%s: %s is not aligned to %s", unit, a[k].name,
                  a[k].align == 8 ? "double" : "int16");
    for (int o = 0; o < n; ++o) {
        if (!a[o].out || !a[o].p) continue;
        for (int k = 0; k < o; ++k)
            if (a[k].p && overlap(a[o].p, a[o].bytes, a[k].p, a[k].bytes)) fail(IBH_EINVAL, overlap_fmt, unit, a[o].name, a[k].name);
    }
}

// the row areas of an (im, jm) grid (make_dxyp with a 0-based row), for a handle to upload
inline std::vector<double> dxyp_rows(int32_t im, int32_t jm) {
    std::vector<double> d((size_t)jm);
    rethrow(ibh_hntr_dxyp(im, jm, d.data()));
    return d;
}

}  // namespace ibh
