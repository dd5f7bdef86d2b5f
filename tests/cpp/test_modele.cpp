// C++ test of the ModelE regridder in icebin_amd/host/icebin_hip.hpp, used the way modele/GCMCoupler_ModelE.cpp:956-968 uses
// it: a GCMRegridder_Standard on the ocean grid wrapped in GCMRegridder_ModelE / GCMRegridder_WrapE, the four coupler matrices
// through matrix_d with a shared dimE.  The results go to <outdir>/*.bin, which tests/test_cpp_modele.py compares bitwise with
// the Python surface (GCMRegridder.to_modele).
// Exit code 0 = pass, 3 = no GPU (the no-fallback error path was verified instead).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "host_test.h"

using namespace icebin;
using icebin::modele::HntrSpec;

int main(int argc, char **argv) {
    const std::string out = argc > 1 ? argv[1] : ".";
    const HntrSpec hspecO(8, 6, 0., 1800.), hspecI(48, 36, 0.5, 300.);
    const double eq_rad = 6371000.;
    // the inputs the Python side rebuilds: no ice where (i*7) % 5 == 0, else i % 3000 m; ModelE ocean on every 5th O cell, a
    // fractional ice-model ocean on every 5th + 1
    std::vector<double> elevmaskI((size_t)hspecI.size());
    for (int i = 0; i < hspecI.size(); ++i)
        elevmaskI[(size_t)i] = (i * 7) % 5 == 0 ? std::numeric_limits<double>::quiet_NaN() : (double)(i % 3000);
    std::vector<double> foceanOp((size_t)hspecO.size(), 0.), foceanOm((size_t)hspecO.size(), 0.);
    for (int i = 0; i < hspecO.size(); ++i) {
        if (i % 5 == 0) foceanOp[(size_t)i] = foceanOm[(size_t)i] = 1.;
        if (i % 5 == 1) foceanOp[(size_t)i] = 0.25;
    }
    try {
        REQUIRE(modele::make_hntrA(hspecO).im == 4 && modele::make_hntrA(hspecO).jm == 3 && modele::make_hntrA(hspecO).dlat == 3600.);
        std::shared_ptr<GCMRegridder_Standard> gcmO(
            modele::new_gcmA_standard(hspecO, hspecI, ArrayView<const double>(elevmaskI), {0., 1500., 3000.}, true, eq_rad).release());
        std::unique_ptr<modele::GCMRegridder_ModelE> gcmA(new modele::GCMRegridder_ModelE("", gcmO, hspecO, eq_rad));
        REQUIRE(gcmA->nA() == 12 && gcmA->nhc() == 3 && gcmA->nE() == 36);
        std::vector<int64_t> dimA;
        for (long x : gcmA->agridA_dim(0)) dimA.push_back(x);
        REQUIRE(dump(out + "/agridA.dim", dimA));
        modele::GCMRegridder_WrapE wrap(std::move(gcmA), foceanOp, foceanOm);
        REQUIRE(wrap.nA() == 12 && wrap.nE() == 36 && wrap.foceanOm.size() == 48);

        auto rm = wrap.regrid_matrices(0, ArrayView<const double>(elevmaskI));
        SparseSetT dimE;
        RegridParams scaled(true, false, {{0., 0., 0.}}), unscaled(false, false, {{0., 0., 0.}});
        auto EvI = rm->matrix_d("EvI", {{&dimE, nullptr}}, scaled);
        REQUIRE(!EvI->conservative && EvI->scaled && dimE.dense_extent() == EvI->shape_d()[0]);
        REQUIRE(dump_matrix(out, "EvI", *EvI));
        auto AvI = rm->matrix("AvI");
        REQUIRE(dump_matrix(out, "AvI", *AvI));
        const int nE = dimE.dense_extent();
        auto IvE = rm->matrix_d("IvE", {{nullptr, &dimE}}, unscaled);
        REQUIRE(dimE.dense_extent() == nE && IvE->shape_d()[1] == nE && !IvE->scaled);
        REQUIRE(dump_matrix(out, "IvE", *IvE));
        auto XvE = rm->matrix_d("XvE", {{nullptr, &dimE}}, unscaled);
        REQUIRE(dump_matrix(out, "XvE", *XvE));
        // an unknown name, and a ModelE ocean that is neither 0 nor 1 on a cell with ice
        try { rm->matrix("AvE"); REQUIRE(false); } catch (Exception const &e) { REQUIRE(e.code == IBH_ENOKEY); }
        wrap.foceanOm[7] = 0.5;
        try {
            wrap.regrid_matrices(0, ArrayView<const double>(elevmaskI))->matrix("AvI");
            REQUIRE(false);
        } catch (Exception const &e) {
            REQUIRE(e.code == IBH_EINVAL && std::string(e.what()).find("fcont_m[7]") != std::string::npos);
        }
    } catch (Exception const &e) {
        if (no_gpu(e)) return 3;
        std::printf("FAILED: exception %d: %s\n", e.code, e.what());
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
