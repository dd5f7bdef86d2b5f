// C++ test of global_AvE in icebin_amd/host/icebin_hip.hpp (namespace icebin::modele): two ice sheets in one
// GCMRegridder_Standard on an 8 x 6 ocean grid, a base ice matrix with a duplicated entry, compute_EOpvAOp_merged with and
// without squash_ECs, _compute_AAmvEAm and GCMRegridder_ModelE::global_AvE.  The results go to <outdir>/*.bin, which
// tests/test_cpp_global_ave.py compares bitwise with the Python surface.
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

// dump_matrix's files and .extent (int64[2])
static bool dump_matrix_extent(std::string const &out, std::string const &name, linear::Weighted const &w) {
    std::vector<int64_t> ext = {w.shape()[0], w.shape()[1]};
    return dump_matrix(out, name, w) && dump(out + "/" + name + ".extent", ext);
}

static bool dump_classes(std::string const &out, std::string const &name, modele::EOpvAOpResult const &eo) {
    std::vector<int64_t> meta = {eo.offsetE, eo.indexingHC_strides[0], eo.indexingHC_strides[1], eo.indexingHC_extents[0],
                                 eo.indexingHC_extents[1]};
    return dump(out + "/" + name + ".hcdefs", eo.hcdefs) && dump(out + "/" + name + ".underice", eo.underice_hc) &&
           dump(out + "/" + name + ".meta", meta);
}

int main(int argc, char **argv) {
    const std::string out = argc > 1 ? argv[1] : ".";
    const HntrSpec hspecO(8, 6, 0., 1800.);
    const HntrSpec hspecI[2] = {HntrSpec(48, 36, 0.5, 300.), HntrSpec(24, 18, 0.25, 600.)};
    const double eq_rad = 6371000., nan = std::numeric_limits<double>::quiet_NaN();
    const long nO = hspecO.size();
    // the inputs the Python side rebuilds
    std::vector<double> em[2];
    for (int i = 0; i < hspecI[0].size(); ++i) em[0].push_back((i * 7) % 5 == 0 ? nan : (double)(i % 3000));
    for (int i = 0; i < hspecI[1].size(); ++i) em[1].push_back((i * 3) % 4 == 0 ? nan : (double)((i * 5) % 3000));
    std::vector<double> foceanOp((size_t)nO, 0.), foceanOm((size_t)nO, 0.);
    for (long i = 0; i < nO; ++i) {
        if (i % 5 == 0) foceanOp[(size_t)i] = foceanOm[(size_t)i] = 1.;
        if (i % 5 == 1) foceanOp[(size_t)i] = 0.25;
    }
    modele::EOpvAOpBase base;
    base.hcdefs = {1500., 4000.};
    base.shape = {{2 * nO, nO}};
    for (long c = 1; c < nO; c += 4) { base.iE.push_back(c + nO * (c % 3 == 0)); base.iO.push_back(c); base.val.push_back(1e9 * (double)(c + 1)); }
    base.iE.push_back(base.iE[2]); base.iO.push_back(base.iO[2]); base.val.push_back(2.5e9);       // one pair twice
    try {
        // two sheets in one regridder whose every O cell is realised; the exchange grids come from the Hntr builder
        std::shared_ptr<GCMRegridder_Standard> gcmO(new GCMRegridder_Standard);
        AbbrGrid agridO;
        agridO.sparse_extent = nO;
        for (long i = 0; i < nO; ++i) { agridO.dim_to_sparse.push_back(i); agridO.native_area.push_back(1.); }
        gcmO->init(std::move(agridO), {0., 1500., 3000.}, true);
        for (int k = 0; k < 2; ++k) {
            auto one = modele::new_gcmA_standard(hspecO, hspecI[k], ArrayView<const double>(em[k]), {0., 1500., 3000.}, true, eq_rad);
            int64_t nX = 0;
            check(ibh_regridder_exgrid(one->ice_regridder(0)->handle(), &nX, nullptr, nullptr));
            ExchangeGrid ex;
            ex.indices.resize(2 * (size_t)nX); ex.overlaps.resize((size_t)nX);
            check(ibh_regridder_exgrid(one->ice_regridder(0)->handle(), &nX, ex.indices.data(), ex.overlaps.data()));
            gcmO->add_sheet("sheet" + std::to_string(k), hspecI[k].size(), ex);
        }
        REQUIRE(gcmO->nsheets() == 2 && gcmO->indexingHC_strides()[1] == nO);
        std::vector<ArrayView<const double>> emIs = {ArrayView<const double>(em[0]), ArrayView<const double>(em[1])};

        SparseSetT dimAOp;
        modele::EOpvAOpResult eo = modele::compute_EOpvAOp_merged(dimAOp, base, gcmO.get(), emIs, true, true, false);
        REQUIRE(eo.offsetE == 3 * nO && eo.hcdefs.size() == 5 && eo.underice_hc[2] == modele::UI_LOCALICE && eo.underice_hc[3] == modele::UI_GLOBALICE);
        REQUIRE(eo.dimEOp->sparse_extent() == 5 * nO && dimAOp.sparse_extent() == nO && !eo.EOpvAOp->scaled);
        REQUIRE(dump_matrix_extent(out, "EOpvAOp", *eo.EOpvAOp) && dump_classes(out, "EOpvAOp", eo));
        SparseSetT dimAOp2;
        modele::EOpvAOpResult sq = modele::compute_EOpvAOp_merged(dimAOp2, base, gcmO.get(), emIs, true, true, true);
        REQUIRE(sq.hcdefs.size() == 4 && sq.dimEOp->sparse_extent() == 4 * nO);
        REQUIRE(dump_matrix_extent(out, "EOpvAOp_sq", *sq.EOpvAOp) && dump_classes(out, "EOpvAOp_sq", sq));

        auto AvE_s = modele::_compute_AAmvEAm(true, eq_rad, hspecO, ArrayView<const double>(foceanOp), ArrayView<const double>(foceanOm), eo, dimAOp);
        REQUIRE(!AvE_s->conservative && AvE_s->scaled && AvE_s->shape()[0] == 12 && AvE_s->shape()[1] == 60);
        REQUIRE(dump_matrix_extent(out, "AvE_s", *AvE_s));
        SparseSetT dimAAm, dimEAm;
        auto AvE_sq = modele::_compute_AAmvEAm_EIGEN({{&dimAAm, &dimEAm}}, false, eq_rad, hspecO, sq.indexingHC_strides, {{1, 12}}, 4,
                                                    ArrayView<const double>(foceanOp), ArrayView<const double>(foceanOm), *sq.EOpvAOp,
                                                    *sq.dimEOp, dimAOp2);
        REQUIRE(dimAAm.dense_extent() == AvE_sq->shape_d()[0] && dimEAm.sparse_extent() == 48 && !AvE_sq->scaled);
        REQUIRE(dump_matrix_extent(out, "AvE_sq", *AvE_sq));

        modele::GCMRegridder_ModelE gcmA(base, gcmO, hspecO, eq_rad);
        REQUIRE(gcmA.hcdefs().size() == 5 && gcmA.hcdefs()[3] == 1500. && gcmA.underice(2) == modele::UI_LOCALICE &&
                gcmA.underice(3) == modele::UI_GLOBALICE);
        long offsetE = -1;
        auto AvE_u = gcmA.global_AvE({}, emIs, ArrayView<const double>(foceanOp), ArrayView<const double>(foceanOm), false, offsetE);
        REQUIRE(offsetE == 3 * nO && !AvE_u->scaled);
        REQUIRE(dump_matrix_extent(out, "AvE_u", *AvE_u));

        // a base index outside its shape; a ModelE ocean that is neither 0 nor 1 on a cell with ice
        modele::EOpvAOpBase bad = base;
        bad.iE[1] = 2 * nO;
        SparseSetT dimAOp3;
        try {
            modele::compute_EOpvAOp_merged(dimAOp3, bad, gcmO.get(), emIs, true, true, false);
            REQUIRE(false);
        } catch (Exception const &e) {
            REQUIRE(e.code == IBH_EINVAL && std::string(e.what()).find("base entry 1") != std::string::npos && dimAOp3.dense_extent() == 0);
        }
        foceanOm[7] = 0.5;
        try {
            modele::_compute_AAmvEAm(true, eq_rad, hspecO, ArrayView<const double>(foceanOp), ArrayView<const double>(foceanOm), eo, dimAOp);
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
