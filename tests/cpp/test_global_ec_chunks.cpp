// C++ test of the chunked global_ec in icebin_amd/host/icebin_hip.hpp (icebin::modele::global_ec), used the way
// modele/global_ec.cpp's main() and combine_global_ec.cpp use their parts: IceScan over two int16 planes, the chunk plan, one
// mask and one regridder per chunk, AvI and EvA unscaled, combine_chunks.  The results go to <outdir>/*.bin, which
// tests/test_cpp_global_ec_chunks.py compares bitwise with the Python surface (icebin_amd.global_ec).
// Exit code 0 = pass, 3 = no GPU (the no-fallback error path was verified instead).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "host_test.h"

using namespace icebin;
using icebin::modele::HntrSpec;
namespace gec = icebin::modele::global_ec;

// everything one chunk keeps alive: the sets outlive the matrices that borrow them
struct ChunkRun {
    std::vector<double> mask;
    std::unique_ptr<GCMRegridder_Standard> gcm;
    std::unique_ptr<RegridMatrices_Dynamic> rm;
    SparseSetT dimA, dimI, dimE;
    std::unique_ptr<linear::Weighted_Eigen> AvI, EvA;
};

int main(int argc, char **argv) {
    const std::string out = argc > 1 ? argv[1] : ".";
    const HntrSpec hspecO(8, 4, 0., 2700.), hspecI(32, 16, 0., 675.);
    const double eq_rad = 6371000., ec_skip = 500.;
    // the planes the Python side rebuilds
    std::vector<int16_t> fg((size_t)hspecI.size()), el((size_t)hspecI.size());
    for (int x = 0; x < hspecI.size(); ++x) {
        fg[(size_t)x] = (int16_t)((x * 7 + x / 13) % 3 == 0 ? 0 : 1 + x % 2);
        el[(size_t)x] = (int16_t)((x * 37) % 3000 - 200);
    }
    try {
        // the errors that need no device
        try {
            gec::IceScan bad(hspecO, HntrSpec(36, 16, 0., 675.), ArrayView<const int16_t>(fg.data(), 576), ArrayView<const int16_t>(el.data(), 576));
            REQUIRE(!"a grid that does not nest was accepted");
        } catch (Exception const &e) {
            REQUIRE(e.code == IBH_EINVAL && std::string(e.what()).find("must be an even multiple of (8x4)") != std::string::npos);
        }
        gec::IceScan scan(hspecO, hspecI, ArrayView<const int16_t>(fg), ArrayView<const int16_t>(el));
        REQUIRE(scan.mult_i() == 4 && scan.mult_j() == 4);
        std::vector<int> nice = scan.nice();
        for (int k = 0; k < hspecO.size(); ++k) {       // the tile counts, by the definition
            int n = 0;
            for (int j = 0; j < 4; ++j)
                for (int i = 0; i < 4; ++i) n += fg[(size_t)(((k / 8) * 4 + j) * 32 + (k % 8) * 4 + i)] != 0;
            REQUIRE(nice[(size_t)k] == n);
        }
        const std::array<double, 2> ec = scan.ec_range(ec_skip);
        REQUIRE(scan.elevI_range()[0] >= -200 && scan.elevI_range()[1] <= 2799 && ec[0] == -500. && ec[1] == 3000.);
        try {
            gec::chunk_plan(scan, 16);
            REQUIRE(!"a chunk size one cell can reach was accepted");
        } catch (Exception const &e) {
            REQUIRE(e.code == IBH_EINVAL && std::string(e.what()).find("chunk_size") != std::string::npos);
        }
        const gec::ChunkPlan plan = gec::chunk_plan(scan, 70);
        REQUIRE(plan.chunks.size() >= 3 && plan.chunks.front()[1] == 0 && plan.chunks.front()[2] == 0 && plan.chunks.back()[3] == hspecO.jm &&
                plan.chunks.back()[4] == 0);
        std::vector<int> flat;
        for (gec::Chunk const &c : plan.chunks) flat.insert(flat.end(), c.begin(), c.end());
        REQUIRE(dump(out + "/chunks", flat) && dump(out + "/chunks.nice", plan.nice) && dump(out + "/fgiceO", scan.fgiceO()));

        std::vector<double> hcdefs = modele::make_hcdefs(ec[0], ec[1], ec_skip);
        RegridParams params(false, true, {{0., 0., 0.}});
        std::vector<std::unique_ptr<ChunkRun>> runs;
        std::vector<linear::Weighted const *> AvIs, EvAs;
        for (gec::Chunk const &c : plan.chunks) {
            std::unique_ptr<ChunkRun> r(new ChunkRun);
            r->mask = gec::chunk_mask(scan, c);
            REQUIRE(dump(out + "/mask" + std::to_string(c[0]), r->mask));
            r->gcm = modele::new_gcmA_standard(hspecO, hspecI, ArrayView<const double>(r->mask), hcdefs, true, eq_rad);
            r->rm = r->gcm->regrid_matrices(0, ArrayView<const double>(r->mask));
            r->AvI = r->rm->matrix_d("AvI", {{&r->dimA, &r->dimI}}, params);
            r->EvA = r->rm->matrix_d("EvA", {{&r->dimE, &r->dimA}}, params);
            AvIs.push_back(r->AvI.get());
            EvAs.push_back(r->EvA.get());
            runs.push_back(std::move(r));
        }
        gec::CombinedChunks AvI = gec::combine_chunks(AvIs, false), EvA = gec::combine_chunks(EvAs, false), EvAs_ = gec::combine_chunks(EvAs, true);
        REQUIRE(!AvI.M->scaled && EvAs_.M->scaled && AvI.iB.size() == AvI.val.size() && (long)AvI.val.size() >= AvI.M->nnz());
        REQUIRE(dump_matrix(out, "AvI", *AvI.M) && dump_matrix(out, "EvA", *EvA.M) && dump_matrix(out, "EvA_scaled", *EvAs_.M));
        REQUIRE(dump(out + "/EvA.iB", EvA.iB) && dump(out + "/EvA.iA", EvA.iA) && dump(out + "/EvA.stream", EvA.val));
        REQUIRE(dump(out + "/EvA_scaled.stream", EvAs_.val));
    } catch (Exception const &e) {
        if (no_gpu(e)) return 3;
        std::printf("FAILED: exception %d: %s\n", e.code, e.what());
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
