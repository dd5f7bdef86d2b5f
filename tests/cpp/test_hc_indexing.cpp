// HcIndexing (icebin_amd/csrc/common.h), the one definition of indexingHC: split(index(iA, ihc)) == (iA, ihc) and with_nhc for
// both orders, the class slowest (1, nA) and the class fastest (nhc, 1).  Host code only: nothing here touches a device.
#include "../../icebin_amd/csrc/common.h"

#include <cstdio>

using ibh::HcIndexing;
static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++g_failed; } } while (0)

int main() {
    const int64_t nAs[] = {1, 2, 5}, nhcs[] = {1, 3};
    for (int64_t nA : nAs)
        for (int64_t nhc : nhcs) {
            const HcIndexing orders[] = {{1, nA}, {nhc, 1}};
            for (int o = 0; o < 2; ++o) {
                const HcIndexing &hc = orders[o];
                // One class in the class-fastest order is the stride pair (1, 1), which is also the class-slowest order of one
                // cell: the strides alone do not say which.  The decode reads it as the latter (sHC >= sA), as every unit
                // always has, so with nA > 1 it returns (0, iE) there and no function of the strides could round-trip both.
                const bool ambiguous = o == 1 && nhc == 1 && nA > 1;
                bool seen[15] = {false};
                for (int64_t iA = 0; iA < nA; ++iA)
                    for (int64_t ihc = 0; ihc < nhc; ++ihc) {
                        const int64_t iE = hc.index(iA, ihc);
                        CHECK(iE >= 0 && iE < nA * nhc && !seen[iE]);      // a bijection onto [0, nA * nhc)
                        seen[iE] = true;
                        int64_t a = -1, h = -1;
                        hc.split(iE, a, h);
                        if (ambiguous) CHECK(a == 0 && h == iE);
                        else CHECK(a == iA && h == ihc);
                    }
            }
            // with_nhc: the class-slowest order keeps its strides, the class-fastest one takes the new class count (the
            // ambiguous pair (1, 1) is kept, again as the class-slowest order)
            const HcIndexing slow = HcIndexing{1, nA}.with_nhc(nhc + 4), fast = HcIndexing{nhc, 1}.with_nhc(nhc + 4);
            CHECK(slow.sA == 1 && slow.sHC == nA);
            if (nhc == 1) CHECK(fast.sA == 1 && fast.sHC == 1);
            else CHECK(fast.sA == nhc + 4 && fast.sHC == 1);
        }
    // the two orders number the same pair differently once there is more than one of each
    CHECK((HcIndexing{1, 5}.index(2, 1)) == 7 && (HcIndexing{3, 1}.index(2, 1)) == 7 && (HcIndexing{1, 5}.index(1, 2)) == 11 &&
          (HcIndexing{3, 1}.index(1, 2)) == 5);
    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("all checks passed\n");
    return 0;
}
