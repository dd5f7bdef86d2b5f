// C++ test of etopo1_ice in icebin_amd/host/icebin_hip.hpp (icebin::modele::etopo1_ice), used the way modele/etopo1_ice.cpp's
// main() uses it: the three ETOPO1 planes and the coarse ice fractions in, the four fine planes and the four h planes out, with
// and without Greenland.  The results go to <outdir>/*, which tests/test_cpp_etopo1_ice.py compares bitwise with the Python
// surface (icebin_amd.etopo1).
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
    const HntrSpec hspecC(8, 4, 0., 2700.), hspecI(32, 16, 0., 675.), hspecH(16, 8, 0., 1350.);
    // the planes the Python side rebuilds
    std::vector<int16_t> fo((size_t)hspecI.size()), zt(fo.size()), zs(fo.size());
    for (int x = 0; x < hspecI.size(); ++x) {
        fo[(size_t)x] = (int16_t)((x * 7 + x / 13) % 4);
        zt[(size_t)x] = (int16_t)(((x * 37) % 7) * 100 - 300);
        zs[(size_t)x] = (int16_t)(zt[(size_t)x] - (x * 11) % 100);
    }
    std::vector<double> fC((size_t)hspecC.size());
    for (int k = 0; k < hspecC.size(); ++k) fC[(size_t)k] = k % 3 == 0 ? 0. : (k % 7) / 6.0;
    const ArrayView<const int16_t> vfo(fo), vzt(zt), vzs(zs);
    const ArrayView<const double> vfC(fC);
    try {
        // the errors that need no device
        try {
            modele::etopo1_ice(HntrSpec(36, 16, 0., 675.), hspecC, ArrayView<const int16_t>(fo.data(), 576), ArrayView<const int16_t>(zt.data(), 576),
                               ArrayView<const int16_t>(zs.data(), 576), vfC);
            REQUIRE(!"a grid that does not nest was accepted");
        } catch (Exception const &e) {
            REQUIRE(e.code == IBH_EINVAL && std::string(e.what()).find("(36x16)") != std::string::npos &&
                    std::string(e.what()).find("(8x4)") != std::string::npos);
        }
        try {
            modele::etopo1_ice(hspecI, hspecC, vfo, vzt, ArrayView<const int16_t>(zs.data(), 100), vfC);
            REQUIRE(!"a short plane was accepted");
        } catch (Exception const &e) {
            REQUIRE(e.code == IBH_EINVAL);
        }
        for (int incl = 0; incl < 2; ++incl) {
            const modele::Etopo1Ice r = modele::etopo1_ice(hspecI, hspecC, vfo, vzt, vzs, vfC, incl != 0, &hspecH);
            REQUIRE(r.FGICE1m.size() == fo.size() && r.FGICEh.size() == (size_t)hspecH.size());
            long nice = 0;
            for (size_t x = 0; x < fo.size(); ++x) {
                REQUIRE(r.FGICE1m[x] == 0 || r.FGICE1m[x] == 1);
                REQUIRE(r.FGICE1m[x] == 0 || r.FOCEAN1m[x] == 0);        // no ice on the sea
                const bool greenland = fo[x] == 2 && x / 32 >= 8;
                REQUIRE(r.FOCEAN1m[x] == (greenland ? (incl ? 0 : 1) : fo[x]));
                REQUIRE(r.ZICETOP1m[x] == (greenland && !incl ? -300 : zt[x]) && r.ZSOLG1m[x] == (greenland && !incl ? -300 : zs[x]));
                nice += r.FGICE1m[x];
            }
            REQUIRE(nice > 0);
            const std::string tag = out + (incl ? "/g1." : "/g0.");
            REQUIRE(dump(tag + "FOCEAN1m", r.FOCEAN1m) && dump(tag + "FGICE1m", r.FGICE1m) && dump(tag + "ZICETOP1m", r.ZICETOP1m) &&
                    dump(tag + "ZSOLG1m", r.ZSOLG1m) && dump(tag + "FOCEANh", r.FOCEANh) && dump(tag + "FGICEh", r.FGICEh) &&
                    dump(tag + "ZICETOPh", r.ZICETOPh) && dump(tag + "ZSOLGh", r.ZSOLGh));
        }
        const modele::Etopo1Ice plain = modele::etopo1_ice(hspecI, hspecC, vfo, vzt, vzs, vfC);
        REQUIRE(plain.FOCEANh.empty() && plain.FGICE1m.size() == fo.size());
    } catch (Exception const &e) {
        if (no_gpu(e)) return 3;
        std::printf("FAILED: exception %d: %s\n", e.code, e.what());
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
