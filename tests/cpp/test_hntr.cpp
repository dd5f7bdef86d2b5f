// C++ test of icebin::modele::Hntr in icebin_amd/host/icebin_hip.hpp, used the way the reference's topography tools use
// modele::Hntr (slib/icebin/modele/topo.cpp): construct from two HntrSpecs, regrid host arrays.  The result must be
// bitwise the reference's loop (hntr.hpp:260-296 matrix + RegridAccum :322-338, mean_polar :404-423), restated below
// over the partition that ibh_hntr_partition returns.
// Exit code 0 = pass, 3 = no GPU (the no-fallback error path was verified instead).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host_test.h"

using namespace icebin;
using icebin::modele::Hntr;
using icebin::modele::HntrSpec;

static std::vector<double> serial_regrid(HntrSpec const &B, HntrSpec const &A, double DATMIS, std::vector<double> const &WTA,
                                         std::vector<double> const &Av, bool mean_polar, double wtm, double wtb) {
    std::vector<double> SINA(A.jm + 1), SINB(B.jm + 1), FMIN(B.im), FMAX(B.im), GMIN(B.jm), GMAX(B.jm);
    std::vector<int32_t> IMIN(B.im), IMAX(B.im), JMIN(B.jm), JMAX(B.jm);
    check(ibh_hntr_partition(A.im, A.jm, A.offi, A.dlat, B.im, B.jm, B.offi, B.dlat, SINA.data(), SINB.data(), IMIN.data(), IMAX.data(),
                             FMIN.data(), FMAX.data(), JMIN.data(), JMAX.data(), GMIN.data(), GMAX.data()));
    std::vector<double> out((size_t)B.size());
    for (int JB = 1; JB <= B.jm; ++JB)
        for (int IB = 1; IB <= B.im; ++IB) {
            double VALUE = 0, WEIGHT = 0;
            for (int JA = JMIN[JB - 1]; JA <= JMAX[JB - 1]; ++JA) {
                double G = SINA[JA] - SINA[JA - 1];
                if (JA == JMIN[JB - 1]) G -= GMIN[JB - 1];
                if (JA == JMAX[JB - 1]) G -= GMAX[JB - 1];
                for (int IAREV = IMIN[IB - 1]; IAREV <= IMAX[IB - 1]; ++IAREV) {
                    const int IA = 1 + ((IAREV - 1) % A.im);
                    const int IJA = IA + A.im * (JA - 1);
                    double F = 1;
                    if (IAREV == IMIN[IB - 1]) F -= FMIN[IB - 1];
                    if (IAREV == IMAX[IB - 1]) F -= FMAX[IB - 1];
                    const double FG = F * G;
                    const double wta = wtm * WTA[IJA - 1] + wtb;
                    const double wt = FG * wta;
                    WEIGHT += wt;
                    VALUE += wt * Av[IJA - 1];
                }
            }
            out[(size_t)(IB + B.im * (JB - 1) - 1)] = WEIGHT == 0 ? DATMIS : VALUE / WEIGHT;
        }
    if (mean_polar)
        for (int JB = 1; JB <= B.jm; JB += B.jm - 1) {
            double BMEAN = DATMIS, WEIGHT = 0, VALUE = 0;
            for (int IB = 1;; ++IB) {
                if (IB > B.im) { if (WEIGHT != 0) BMEAN = VALUE / WEIGHT; break; }
                const double b = out[(size_t)(IB + B.im * (JB - 1) - 1)];
                if (b == DATMIS) break;
                WEIGHT += 1;
                VALUE += b;
            }
            for (int IB = 1; IB <= B.im; ++IB) out[(size_t)(IB + B.im * (JB - 1) - 1)] = BMEAN;
        }
    return out;
}

static bool same_bits(std::vector<double> const &a, std::vector<double> const &b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

int main() {
    // 1-degree field onto a ModelE-like 72 x 46 grid with half-height polar cells (dlat 240'), windows wrapping the date line
    const HntrSpec gA(360, 180, 0., 60.), gB(72, 46, 0.5, 240.);
    const double DATMIS = -1e30;
    std::vector<double> WTA((size_t)gA.size()), A((size_t)gA.size());
    for (int j = 0; j < gA.jm; ++j)
        for (int i = 0; i < gA.im; ++i) {
            const size_t ij = (size_t)i + (size_t)gA.im * j;
            A[ij] = std::sin(0.05 * i) * std::cos(0.07 * j) + 1e-3 * (double)((i * 131 + j * 71) % 97);
            WTA[ij] = (i >= 100 && i < 140 && j >= 20 && j < 160) ? 0.0 : 0.25 + 0.5 * (double)((i * 7 + j * 13) % 5);
        }
    try {
        Hntr hntr(17.17, gB, gA, DATMIS);
        REQUIRE(hntr.Agrid.spec.size() == gA.size() && hntr.Bgrid.spec.im == 72 && hntr.DATMIS == DATMIS);
        // the reference's regrid(WTA, A, B, mean_polar) and regrid(WTA, A, mean_polar)
        std::vector<double> B((size_t)gB.size(), 0.0);
        hntr.regrid(ArrayView<const double>(WTA), ArrayView<const double>(A), ArrayView<double>(B.data(), (long)B.size()), false);
        REQUIRE(same_bits(B, serial_regrid(gB, gA, DATMIS, WTA, A, false, 1.0, 0.0)));
        std::vector<double> Bm = hntr.regrid(ArrayView<const double>(WTA), ArrayView<const double>(A), true);
        REQUIRE(same_bits(Bm, serial_regrid(gB, gA, DATMIS, WTA, A, true, 1.0, 0.0)));
        // wtm/wtb: weight 1 - WTA
        hntr.regrid(ArrayView<const double>(WTA), ArrayView<const double>(A), ArrayView<double>(B.data(), (long)B.size()), false, -1.0, 1.0);
        REQUIRE(same_bits(B, serial_regrid(gB, gA, DATMIS, WTA, A, false, -1.0, 1.0)));
        int ndatmis = 0;
        for (double b : serial_regrid(gB, gA, DATMIS, WTA, A, false, 1.0, 0.0)) ndatmis += b == DATMIS;
        REQUIRE(ndatmis > 0);
        // the reference's dimension check
        bool threw = false;
        try {
            hntr.regrid(ArrayView<const double>(WTA.data(), 10), ArrayView<const double>(A), ArrayView<double>(B.data(), (long)B.size()));
        } catch (Exception const &e) {
            threw = e.code == IBH_EINVAL && std::string(e.what()).find("Error in dimensions") != std::string::npos;
        }
        REQUIRE(threw);
        // mean_polar on a one-row B grid is refused (the reference never terminates)
        Hntr one(17.17, HntrSpec(8, 1, 0., 10800.), gA, DATMIS);
        std::vector<double> B1(8);
        threw = false;
        try {
            one.regrid(ArrayView<const double>(WTA), ArrayView<const double>(A), ArrayView<double>(B1.data(), 8), true);
        } catch (Exception const &e) {
            threw = e.code == IBH_EINVAL;
        }
        REQUIRE(threw);
    } catch (Exception const &e) {
        if (e.code == IBH_ENODEVICE) {
            std::printf("%s\n", e.what());
            return 3;
        }
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
