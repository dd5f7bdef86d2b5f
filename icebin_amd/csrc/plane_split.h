// plane_split.h -- how a run of int16 cells is cut at 16-byte boundaries, and the few integer helpers the units that read the 1'
// planes share (globalec.hip, etopo1.hip, topoo.hip; the device side: planetile.h).  Plain arithmetic, on the host and in kernels:
// no HIP (tests/cpp/test_plane_split.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define IBH_PS_HD __host__ __device__
#else
#define IBH_PS_HD
#endif

namespace ibh {

// A run of n int16 cells that starts at address p: a head of fewer than 8 cells up to the first 16-byte boundary, npiece whole
// pieces of 8 cells (16 bytes each, aligned), and a tail of fewer than 8 cells from tail0() on.  The head and the tail are the
// LOOSE cells, nloose(n) of them, which go one a thread: loose index g is cell cell(g), the head first.  Piece k starts at cell
// piece(k).  A run that ends before the boundary is all head.
struct PlaneSplit {
    unsigned head, npiece;
    IBH_PS_HD unsigned tail0() const { return head + npiece * 8u; }
    IBH_PS_HD unsigned nloose(unsigned n) const { return head + (n - tail0()); }
    IBH_PS_HD unsigned cell(unsigned g) const { return g < head ? g : tail0() + (g - head); }
    IBH_PS_HD unsigned piece(unsigned k) const { return head + k * 8u; }
};
IBH_PS_HD inline PlaneSplit plane_split(const void *p, unsigned n) {
    const unsigned to_boundary = (unsigned)(((16 - ((uintptr_t)p & 15)) & 15) >> 1);
    const unsigned head = to_boundary < n ? to_boundary : n;
    return PlaneSplit{head, (n - head) >> 3};
}

// [a, a + na) and [b, b + nb) share a byte (ranges that merely touch do not)
IBH_PS_HD inline bool overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t A = (uintptr_t)a, B = (uintptr_t)b;
    return A < B + nb && B < A + na;
}
IBH_PS_HD inline long cdiv(long a, long b) { return (a + b - 1) / b; }
// the least power of two >= n (1 for n <= 1): the keys of an LDS sort are padded to it
IBH_PS_HD inline int pow2_ceil(int n) {
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    return n2;
}

}  // namespace ibh
#undef IBH_PS_HD
