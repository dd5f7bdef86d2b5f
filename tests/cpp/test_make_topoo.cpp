// C++ test of make_topoO in icebin_amd/host/icebin_hip.hpp (icebin::modele::make_topoO), used the way modele/topo_base.cpp's
// MakeTopoO uses _make_topoO: the four 1' planes and FLAKES in, the bundle's planes out.  The results go to <outdir>/*, which
// tests/test_cpp_make_topoo.py compares bitwise with the Python surface (icebin_amd.topoo).
// Exit code 0 = pass, 3 = no GPU (the no-fallback error path was verified instead).
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "host_test.h"

using namespace icebin;
using icebin::modele::HntrSpec;

int main(int argc, char **argv) {
    const std::string out = argc > 1 ? argv[1] : ".";
    const HntrSpec hspecO(12, 12, 0., 900.), hspecI(48, 48, 0., 225.), hspecS(18, 9, 0., 1200.);
    // the planes the Python side rebuilds
    std::vector<int16_t> fg((size_t)hspecI.size()), zt(fg.size()), zs(fg.size()), fo(fg.size());
    for (int x = 0; x < hspecI.size(); ++x) {
        fo[(size_t)x] = (int16_t)(((x * 7 + x / 13) % 5) < 2);
        fg[(size_t)x] = (int16_t)(((x * 5 + x / 7) % 3) == 0);
        zt[(size_t)x] = (int16_t)(((x * 37) % 7) * 100 - 300);
        zs[(size_t)x] = (int16_t)(zt[(size_t)x] - ((x % 48) < 24 ? (x * 11) % 100 : 0));
    }
    std::vector<double> fl((size_t)hspecS.size());
    for (int k = 0; k < hspecS.size(); ++k) fl[(size_t)k] = k % 4 == 0 ? 0. : (k % 9) / 16.0;
    modele::TopoOCells cells;
    cells.set_to_land = {{3, 4}};
    cells.set_to_ocean = {{7, 6}};
    cells.resets = {{5, 5, -30.}, {6, 7, 53.}};
    const ArrayView<const int16_t> vfg(fg), vzt(zt), vzs(zs), vfo(fo);
    const ArrayView<const double> vfl(fl);
    try {
        // the errors that need no device
        try {
            modele::make_topoO(HntrSpec(50, 48, 0., 225.), hspecO, ArrayView<const int16_t>(fg.data(), 2400), ArrayView<const int16_t>(zt.data(), 2400),
                               ArrayView<const int16_t>(zs.data(), 2400), ArrayView<const int16_t>(fo.data(), 2400), hspecS, vfl);
            REQUIRE(!"a grid that does not nest was accepted");
        } catch (Exception const &e) {
            REQUIRE(e.code == IBH_EINVAL && std::string(e.what()).find("(50x48)") != std::string::npos &&
                    std::string(e.what()).find("(12x12)") != std::string::npos);
        }
        try {
            modele::make_topoO(hspecI, hspecO, vfg, vzt, ArrayView<const int16_t>(zs.data(), 100), vfo, hspecS, vfl);
            REQUIRE(!"a short plane was accepted");
        } catch (Exception const &e) {
            REQUIRE(e.code == IBH_EINVAL);
        }
        try {
            modele::TopoOCells bad;
            bad.set_to_land = {{13, 1}};
            modele::make_topoO(hspecI, hspecO, vfg, vzt, vzs, vfo, hspecS, vfl, bad);
            REQUIRE(!"a cell outside the ocean grid was accepted");
        } catch (Exception const &e) {
            REQUIRE(e.code == IBH_EINVAL && std::string(e.what()).find("set_to_land") != std::string::npos);
        }
        const modele::BaseTopoO r = modele::make_topoO(hspecI, hspecO, vfg, vzt, vzs, vfo, hspecS, vfl, cells);
        REQUIRE(r.planes.size() == IBH_MAKE_TOPOO_NPLANE);
        const size_t nO = (size_t)hspecO.size();
        for (size_t x = 0; x < nO; ++x) {
            const double focean = r.at("FOCEAN")[x];
            REQUIRE(focean == 0. || focean == 1.);
            REQUIRE(r.at("ZLAND_MIN")[x] == 0. && r.at("ZLAND_MAX")[x] == 0. && r.at("FGICE_greenland")[x] == 0.);
            REQUIRE(r.at("ZSOLDG")[x] == r.at("ZSOLDG")[x]);        // no NaN
            if (x < 12) REQUIRE(focean == 0. && r.at("FGICE")[x] == 1. && r.at("FGICEF")[x] == 1.);     // :498-502
        }
        REQUIRE(r.at("FOCEAN")[3 * 12 + 2] == 0. && r.at("FOCEAN")[5 * 12 + 6] == 1.);      // SET_TO
        REQUIRE(r.at("ZLAKE")[4 * 12 + 4] == -30. && r.at("ZATMO")[6 * 12 + 5] == 53.);     // the resets
        for (int k = 0; k < IBH_MAKE_TOPOO_NPLANE; ++k) REQUIRE(dump(out + "/" + modele::BaseTopoO::names()[k], r.planes[(size_t)k]));
        std::vector<double> counts = {(double)r.counts.FGICE_low, (double)r.counts.FGICE_high, (double)r.counts.FLAKE_reduced,
                                      (double)r.counts.FGRND_range, (double)r.counts.dZOCEN_nonpositive, (double)r.counts.FLAKE_one};
        REQUIRE(dump(out + "/counts", counts));
        const modele::TopoO t = modele::topoo(r);       // what update_topo takes
        REQUIRE(t.FOCEANF == r.at("FOCEANF") && t.ZLAKE == r.at("ZLAKE") && t.mergemask.empty());
        // a continental cell without land: the reference's message
        try {
            std::vector<int16_t> sea(fo);
            for (int x = 0; x < 48 * 4; ++x) sea[(size_t)x] = 1;
            modele::make_topoO(hspecI, hspecO, vfg, vzt, vzs, ArrayView<const int16_t>(sea), hspecS, vfl, cells);
            REQUIRE(!"a south pole without land was accepted");
        } catch (Exception const &e) {
            REQUIRE(std::string(e.what()) == "Continental cell (1,1) has no continental area on 2-minute grid. (1-48, 1-4)");
        }
    } catch (Exception const &e) {
        if (no_gpu(e)) return 3;
        std::printf("FAILED: exception %d: %s\n", e.code, e.what());
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
