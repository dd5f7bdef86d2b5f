// C++ test of the smoothed IvE / IvA through the ModelE regridder of icebin_amd/host/icebin_hip.hpp, the coupler's call
// rm->matrix_d("IvE", {&dimI, &dimE}, RegridParams(true, true, sigma)) (IceCoupler.cpp:461-463).  The grid (with the ice grid's
// centroids), the mask and the two ocean fractions come from <indir>/*.bin, written by tests/test_cpp_modele_smoothed.py; the
// matrices go to <outdir>/*.bin, which that test compares bitwise with the Python surface.
// Exit code 0 = pass, 3 = no GPU (the no-fallback error path was verified instead).
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "host_test.h"

using namespace icebin;
using icebin::modele::HntrSpec;

// dump()'s format read back: <int64 n><n values>
template <class T>
static std::vector<T> load(std::string const &path) {
    std::vector<T> v;
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) throw Exception(IBH_EINVAL, "cannot open " + path);
    int64_t n = 0;
    if (std::fread(&n, sizeof(n), 1, f) == 1 && n >= 0) {
        v.resize((size_t)n);
        if (std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) v.clear();
    }
    std::fclose(f);
    return v;
}

int main(int argc, char **argv) {
    if (argc < 3) { std::printf("usage: test_modele_smoothed <indir> <outdir>\n"); return 2; }
    const std::string in = argv[1], out = argv[2];
    const double eq_rad = 6371000.;
    try {
        // sizes: nA, nI, imO, jmO;  hspec: offiO, dlatO;  sigma: three
        std::vector<int64_t> sizes = load<int64_t>(in + "/sizes.bin");
        std::vector<double> hspec = load<double>(in + "/hspec.bin"), sg = load<double>(in + "/sigma.bin");
        REQUIRE(sizes.size() == 4 && hspec.size() == 2 && sg.size() == 3);
        const HntrSpec hspecO((int)sizes[2], (int)sizes[3], hspec[0], hspec[1]);
        AbbrGrid a;
        a.sparse_extent = (long)sizes[0];
        for (int64_t s : load<int64_t>(in + "/A_to_sparse.bin")) a.dim_to_sparse.push_back((long)s);
        a.native_area = load<double>(in + "/A_native_area.bin");
        a.name = "gridA";
        ExchangeGrid ex;
        ex.indices = load<int>(in + "/ex_indices.bin");
        ex.overlaps = load<double>(in + "/ex_area.bin");
        std::vector<double> elevmaskI = load<double>(in + "/elevmaskI.bin"), foceanOp = load<double>(in + "/foceanOp.bin"),
                            foceanOm = load<double>(in + "/foceanOm.bin");
        REQUIRE((int64_t)elevmaskI.size() == sizes[1] && (int64_t)foceanOp.size() == sizes[0] && foceanOm.size() == foceanOp.size());
        std::shared_ptr<GCMRegridder_Standard> gcmO(new GCMRegridder_Standard);
        gcmO->init(std::move(a), load<double>(in + "/hcdefs.bin"), true);
        gcmO->add_sheet("greenland", (long)sizes[1], ex, load<double>(in + "/A_proj_area.bin"), InterpStyle::Z_INTERP,
                        load<double>(in + "/I_centroid_xy.bin"));
        modele::GCMRegridder_WrapE wrap(
            std::unique_ptr<modele::GCMRegridder_ModelE>(new modele::GCMRegridder_ModelE("", gcmO, hspecO, eq_rad)), foceanOp, foceanOm);

        const std::array<double, 3> sigma = {{sg[0], sg[1], sg[2]}};
        const RegridParams smoothed(true, true, sigma), plain(true, true, {{0., 0., 0.}});
        // the object is made with the default params; sigma comes per matrix_d, as in the coupler
        auto rm = wrap.regrid_matrices(0, ArrayView<const double>(elevmaskI));
        SparseSetT dimE;
        auto EvI = rm->matrix_d("EvI", {{&dimE, nullptr}}, smoothed);       // (compute_XAmvGp never reads sigma)
        const int nE = dimE.dense_extent();
        REQUIRE(dump_matrix(out, "EvI", *EvI));
        auto IvE = rm->matrix_d("IvE", {{nullptr, &dimE}}, smoothed);
        REQUIRE(dimE.dense_extent() == nE && IvE->shape_d()[1] == nE && IvE->scaled && !IvE->conservative);
        REQUIRE(dump_matrix(out, "IvE", *IvE));
        auto IvE0 = rm->matrix_d("IvE", {{nullptr, &dimE}}, plain);
        REQUIRE(IvE->nnz() > IvE0->nnz());
        auto IvA = rm->matrix_d("IvA", {{nullptr, nullptr}}, smoothed);
        REQUIRE(dump_matrix(out, "IvA", *IvA));
        // an object made WITH sigma hands it to matrix(name), and its O-grid matrices are unsmoothed
        auto rmS = wrap.regrid_matrices(0, ArrayView<const double>(elevmaskI), smoothed);
        auto viaMatrix = rmS->matrix("IvA");
        REQUIRE(dump_matrix(out, "IvA_matrix", *viaMatrix));
        // rows on the exchange grid cannot be smoothed: the O-grid's own refusal, and the set stays as it was
        try { rm->matrix_d("XvE", {{nullptr, &dimE}}, smoothed); REQUIRE(false); } catch (Exception const &e) { REQUIRE(e.code == IBH_ENOTIMPL); }
        REQUIRE(dimE.dense_extent() == nE);
    } catch (Exception const &e) {
        if (no_gpu(e)) return 3;
        std::printf("FAILED: exception %d: %s\n", e.code, e.what());
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
