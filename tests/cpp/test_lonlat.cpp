// C++ test of the path from grid specs in icebin_amd/host/icebin_hip.hpp: a 6 x 4 lon/lat spec with a north cap under SeaRISE's
// northern projection, a 24 x 30 ice grid of 20 km cells -> regridder_from_specs.  Prints the regridder's sizes and the
// exchange-cell count for tests/test_cpp_lonlat.py to compare with the Python path.
// Exit code 0 = pass, 3 = no GPU (the no-fallback error path was verified instead).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host_test.h"

using namespace icebin;

int main() {
    const std::string sproj = "+proj=stere +lon_0=-39 +lat_0=90 +lat_ts=71.0 +ellps=WGS84";
    GridSpec_LonLat spec;
    for (int i = 0; i <= 6; ++i) spec.lonb.push_back(-99. + 10.5 * i);
    spec.latb = {48., 58.5, 68., 79., 88.};
    spec.north_pole = true; spec.points_in_side = 2;
    std::vector<long> realised;
    for (int j = 0; j < 4; ++j) for (int i = 0; i < 6; ++i) realised.push_back(j * 6 + i);
    realised.push_back((long)spec.nlat() * 6 + 5);
    std::vector<double> xe, ye;
    for (int k = 0; k <= 24; ++k) xe.push_back(-0.24e6 + 2e4 * k);
    for (int k = 0; k <= 30; ++k) ye.push_back(-0.7e6 + 2e4 * k);
    // the parser names what it does not know, GPU or not
    try { parse_sproj("+proj=stere +lat_0=90 +towgs84=0,0,0"); REQUIRE(false); }
    catch (std::exception const &e) { REQUIRE(std::strstr(e.what(), "'towgs84'") != nullptr); }
    ibh_stere_params p = parse_sproj(sproj);
    REQUIRE(p.a == 6378137.0 && p.lat_0 == 90. && p.lon_0 == -39. && p.has_lat_ts == 1 && p.lat_ts == 71.);
    try {
        auto gcm = regridder_from_specs(spec, realised, xe, ye, false, sproj, {0., 500., 1500., 3000.});
        LonLatCells cells(spec, realised, sproj);
        ExchangeGrid ex = make_exchange_grid_lonlat(cells, xe, ye, false);
        REQUIRE(cells.ncell() == 25 && cells.nA() == 6 * 6);
        REQUIRE((long)gcm->nA() == cells.nA() && (long)gcm->nE() == 4 * cells.nA());
        std::printf("sizes nA=%ld nE=%ld nI=%ld nX=%ld ncell=%ld\n", (long)gcm->nA(), (long)gcm->nE(), 24l * 30l, (long)ex.overlaps.size(), cells.ncell());
        std::vector<long> unsorted{5, 3};
        try { LonLatCells bad(spec, unsorted, sproj); REQUIRE(false); }
        catch (std::exception const &e) { REQUIRE(std::strstr(e.what(), "ascending") != nullptr); }
    } catch (std::exception const &e) {
        if (std::strstr(e.what(), "no CPU fallback")) { std::printf("no GPU: %s\n", e.what()); return 3; }
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
