// C++ test of global_ec in icebin_amd/host/icebin_hip.hpp, used the way modele/global_ec.cpp uses it: new_gcmA_standard from
// two HntrSpecs and an ice mask, AvI and IvE through RegridMatrices_Dynamic::matrix_d with shared dims, make_I2vX onto a
// plottable grid, check_negative on each.  The results go to <outdir>/*.bin, which tests/test_cpp_global_ec.py compares
// bitwise with the Python surface (icebin_amd.global_ec).
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
    const HntrSpec hspecA(72, 46, 0., 240.), hspecI(360, 180, 0., 60.), hspecI2(144, 90, 0., 120.);
    const double eq_rad = 6371000.;
    // the mask the Python side rebuilds: NaN where (i*7) % 3 == 0, else i % 3000
    std::vector<double> elevmaskI((size_t)hspecI.size());
    for (int i = 0; i < hspecI.size(); ++i)
        elevmaskI[(size_t)i] = (i * 7) % 3 == 0 ? std::numeric_limits<double>::quiet_NaN() : (double)(i % 3000);
    try {
        std::vector<double> hcdefs = modele::make_hcdefs(0., 3000., 500.);
        REQUIRE(hcdefs.size() == 7 && hcdefs[6] == 3000.);
        SparseSetT _dimA, _dimI;
        auto gcmA = modele::new_gcmA_standard(hspecA, hspecI, ArrayView<const double>(elevmaskI), hcdefs, true, eq_rad,
                                              InterpStyle::Z_INTERP, &_dimA, &_dimI);
        REQUIRE(gcmA->nA() == (unsigned long)hspecA.size() && gcmA->nhc() == 7);
        REQUIRE(gcmA->ice_regridder(0)->name() == "globalI" && gcmA->ice_regridder(0)->nI() == (size_t)hspecI.size());
        REQUIRE(_dimA.dense_extent() == (int)gcmA->agridA->dim_to_sparse.size() && _dimI.dense_extent() > 0);
        std::vector<int64_t> a2s(gcmA->agridA->dim_to_sparse.begin(), gcmA->agridA->dim_to_sparse.end());
        REQUIRE(dump(out + "/agridA.dim", a2s) && dump(out + "/agridA.native_area", gcmA->agridA->native_area));
        REQUIRE(dump(out + "/wA", gcmA->wA("globalI", true)));

        auto rm = gcmA->regrid_matrices(0, ArrayView<const double>(elevmaskI));
        RegridParams params(false, true, {{0., 0., 0.}});
        SparseSetT dimA, dimI, dimE, dimI2(hspecI2.size());
        auto AvI = rm->matrix_d("AvI", {{&dimA, &dimI}}, params);
        modele::check_negative(*AvI, "AvI");
        REQUIRE(dump_matrix(out, "AvI", *AvI));
        auto IvE = rm->matrix_d("IvE", {{&dimI, &dimE}}, params);
        modele::check_negative(*IvE, "IvE");
        REQUIRE(dump_matrix(out, "IvE", *IvE));
        auto I2vE = modele::make_I2vX(*IvE, hspecI, hspecI2, ArrayView<const double>(elevmaskI), dimI2, eq_rad);
        modele::check_negative(*I2vE, "I2vE");
        REQUIRE(I2vE->shape_d()[0] == dimI2.dense_extent() && I2vE->shape_d()[1] == dimE.dense_extent());
        REQUIRE(dump_matrix(out, "I2vE", *I2vE));
    } catch (Exception const &e) {
        if (no_gpu(e)) return 3;
        std::printf("FAILED: exception %d: %s\n", e.code, e.what());
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
