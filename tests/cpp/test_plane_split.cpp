// The 16-byte split of a run of int16 cells and the integer helpers beside it (icebin_amd/csrc/plane_split.h), which the int16-plane
// units use on the host and in their kernels: every start address within a 16-byte block against every length 0..40, and overlap on
// touching, nested and disjoint ranges.  Host code only: the header alone, no HIP.
#include "../../icebin_amd/csrc/plane_split.h"

#include <cstdio>

using namespace ibh;
static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (k=%d n=%d)\n", __LINE__, #c, g_k, g_n); ++g_failed; } } while (0)
static int g_k = -1, g_n = -1;

static void test_split() {
    const uintptr_t base = 0x7f0000001000ull;       // 16-byte aligned; the split reads the address only
    for (g_k = 0; g_k < 8; ++g_k) {
        for (g_n = 0; g_n <= 40; ++g_n) {
            const unsigned n = (unsigned)g_n;
            const uintptr_t p = base + 2 * (uintptr_t)g_k;
            const PlaneSplit S = plane_split((const void *)p, n);
            const unsigned tail = n - S.tail0();
            CHECK(S.head < 8);
            CHECK(S.tail0() <= n && tail < 8);
            CHECK(S.head + 8 * S.npiece + tail == n);
            CHECK(S.tail0() == S.head + 8 * S.npiece);
            CHECK(S.nloose(n) == S.head + tail);
            // the head ends at the boundary, or with the run when that ends first
            const unsigned to_boundary = (unsigned)((8 - g_k) % 8);
            CHECK(S.head == (to_boundary < n ? to_boundary : n));
            if (n <= to_boundary) CHECK(S.head == n && S.npiece == 0 && tail == 0);
            if (S.npiece > 0) CHECK(((p + 2 * (uintptr_t)S.head) & 15) == 0);
            for (unsigned k = 0; k < S.npiece; ++k) {
                CHECK(S.piece(k) == S.head + 8 * k);
                CHECK(((p + 2 * (uintptr_t)S.piece(k)) & 15) == 0);
            }
            // the loose-index map: every head and tail cell once, no piece cell
            int hits[40] = {0};
            for (unsigned g = 0; g < S.nloose(n); ++g) {
                const unsigned c = S.cell(g);
                CHECK(c < n);
                if (c < n) ++hits[c];
            }
            for (unsigned c = 0; c < n; ++c) {
                const bool loose = c < S.head || c >= S.tail0();
                CHECK(hits[c] == (loose ? 1 : 0));
            }
            // in order: the head first, then the tail
            for (unsigned g = 0; g + 1 < S.nloose(n); ++g) CHECK(S.cell(g) < S.cell(g + 1));
        }
    }
    g_k = g_n = -1;
}

static void test_overlap() {
    const char *b = (const char *)(uintptr_t)0x1000;
    CHECK(!overlap(b, 16, b + 16, 16));         // touching
    CHECK(!overlap(b + 16, 16, b, 16));
    CHECK(overlap(b, 17, b + 16, 16));          // one byte shared
    CHECK(overlap(b + 16, 16, b, 17));
    CHECK(overlap(b, 64, b + 16, 8));           // nested
    CHECK(overlap(b + 16, 8, b, 64));
    CHECK(overlap(b, 64, b, 64));               // the same range
    CHECK(overlap(b, 64, b + 63, 1));
    CHECK(!overlap(b, 64, b + 64, 1));
    CHECK(!overlap(b, 16, b + 1024, 16));       // disjoint
    CHECK(!overlap(b + 1024, 16, b, 16));
    CHECK(!overlap(b, 0, b + 8, 0));            // empty
    CHECK(!overlap(b, 16, b, 0));               // an empty range at another's start shares no byte
}

static void test_helpers() {
    CHECK(cdiv(0, 256) == 0 && cdiv(1, 256) == 1 && cdiv(256, 256) == 1 && cdiv(257, 256) == 2);
    CHECK(cdiv((1l << 31) + 1, 256) == (1l << 23) + 1);
    CHECK(pow2_ceil(0) == 1 && pow2_ceil(1) == 1 && pow2_ceil(2) == 2 && pow2_ceil(3) == 4 && pow2_ceil(4) == 4 && pow2_ceil(5) == 8);
    CHECK(pow2_ceil(4096) == 4096 && pow2_ceil(4097) == 8192 && pow2_ceil(65535) == 65536);
}

int main() {
    test_split();
    test_overlap();
    test_helpers();
    if (g_failed) { printf("%d checks FAILED\n", g_failed); return 1; }
    printf("all checks passed\n");
    return 0;
}
