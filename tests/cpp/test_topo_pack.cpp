// C++ test of update_topo's packing in icebin_amd/host/icebin_hip.hpp: VectorMultivec::append_planes / affine and
// icebin::modele::TopoPacker over two coupling steps (initialisation, then a step after the ice has retreated from the eastern
// half of both sheets) on the inputs of tests/cpp/test_topo.cpp.  The vectors go to <outdir>/step<k>.*, which
// tests/test_cpp_topo_pack.py compares with the Python surface, bitwise.
// Exit code 0 = pass, 3 = no GPU (the no-fallback error path was verified instead).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "host_test.h"

using namespace icebin;
using icebin::modele::HntrSpec;

static bool dump_vec(std::string const &prefix, VectorMultivec const &v) {
    std::vector<long> ix = v.index();
    return dump(prefix + ".index", std::vector<int64_t>(ix.begin(), ix.end())) && dump(prefix + ".weights", v.weights()) &&
           dump(prefix + ".vals", v.vals());
}

static bool same_bits(std::vector<double> const &a, std::vector<double> const &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0);
}

int main(int argc, char **argv) {
    const std::string out = argc > 1 ? argv[1] : ".";
    const HntrSpec hspecO(8, 6, 0., 1800.);
    const HntrSpec hspecI[2] = {HntrSpec(48, 36, 0.5, 300.), HntrSpec(24, 18, 0.25, 600.)};
    const double eq_rad = 6371000., nan = std::numeric_limits<double>::quiet_NaN();
    const long nO = hspecO.size();
    // the inputs of tests/cpp/test_topo.cpp; step 2: no land and no ice in the ice-grid columns >= im / 2
    std::vector<double> land[2][2], ice[2][2];
    for (int i = 0; i < hspecI[0].size(); ++i) land[0][0].push_back((i * 7) % 5 == 0 ? nan : (double)(i % 3000) - 100.);
    for (int i = 0; i < hspecI[1].size(); ++i) land[0][1].push_back((i * 3) % 4 == 0 ? nan : (double)((i * 5) % 3000) + 200.);
    for (int k = 0; k < 2; ++k) {
        for (size_t i = 0; i < land[0][k].size(); ++i)
            ice[0][k].push_back(i % 3 == 0 || !(land[0][k][i] >= 0. && land[0][k][i] <= 3000.) ? nan : land[0][k][i]);
        land[1][k] = land[0][k];
        ice[1][k] = ice[0][k];
        for (size_t i = 0; i < land[1][k].size(); ++i)
            if ((int)(i % (size_t)hspecI[k].im) >= hspecI[k].im / 2) land[1][k][i] = ice[1][k][i] = nan;
    }
    modele::TopoO topoo;
    for (long i = 0; i < nO; ++i) {
        const bool ocean = i % 5 == 0;
        const double op = ocean ? 1. : (i % 5 == 1 ? 0.25 : 0.);
        topoo.FOCEAN.push_back(ocean ? 1. : 0.); topoo.FOCEANF.push_back(op);
        topoo.FGICE.push_back(ocean ? 0. : 0.25); topoo.FLAKE.push_back(ocean ? 0. : 0.125); topoo.FGRND.push_back(ocean ? 0. : 0.625);
        topoo.FGICEF.push_back(ocean ? 0. : 0.25 * (1. - op));
        topoo.ZATMO.push_back(ocean ? 0. : 100. + (double)i); topoo.ZATMOF.push_back(ocean ? 0. : (100. + (double)i) * (1. - op));
        topoo.ZICETOP.push_back(ocean ? 0. : 150. + (double)i); topoo.ZLAKE.push_back(ocean ? 0. : 5.);
    }
    modele::EOpvAOpBase base;
    base.hcdefs = {1500., 4000.};
    base.shape = {{2 * nO, nO}};
    for (long c = 17; c < 32; c += 3) { base.iE.push_back(c + nO * (c % 2 == 0)); base.iO.push_back(c); base.val.push_back(1e9 * (double)(c + 1)); }
    const std::vector<std::string> varsA = {"focean", "flake", "fgrnd", "fgice", "zatmo", "hlake"}, varsE = {"fhc", "elevE", "underice_d"};
    const std::vector<double> mmA = {1., 1., 1., 1., 9.80665, 1.}, bbA = {0., 0., 0., 0., -3.5, 0.}, mmE = {1., 2., 1.}, bbE = {0., .5, 0.};
    try {
        std::shared_ptr<GCMRegridder_Standard> gcmO(new GCMRegridder_Standard);
        AbbrGrid agridO;
        agridO.sparse_extent = nO;
        for (long i = 0; i < nO; ++i) { agridO.dim_to_sparse.push_back(i); agridO.native_area.push_back(1.e13); }
        gcmO->init(std::move(agridO), {0., 1500., 3000.}, true);
        for (int k = 0; k < 2; ++k) {       // the exchange grid holds every cell of the first step's LAND mask
            auto one = modele::new_gcmA_standard(hspecO, hspecI[k], ArrayView<const double>(land[0][k]), {0., 1500., 3000.}, true, eq_rad);
            int64_t nX = 0;
            check(ibh_regridder_exgrid(one->ice_regridder(0)->handle(), &nX, nullptr, nullptr));
            ExchangeGrid ex;
            ex.indices.resize(2 * (size_t)nX); ex.overlaps.resize((size_t)nX);
            check(ibh_regridder_exgrid(one->ice_regridder(0)->handle(), &nX, ex.indices.data(), ex.overlaps.data()));
            gcmO->add_sheet("sheet" + std::to_string(k), hspecI[k].size(), ex);
        }
        modele::GCMRegridder_ModelE gcmA(base, gcmO, hspecO, eq_rad);
        const HntrSpec hspecA = gcmA.hspecA();
        const size_t nA = (size_t)hspecA.size(), nhc = gcmA.hcdefs().size(), n3 = nA * (nhc + 1);
        REQUIRE(nA == 12 && nhc == 5);

        // an unknown contract variable, as .at(name) throws
        for (int which = 0; which < 2; ++which) {
            try {
                modele::TopoPacker bad(which ? varsA : std::vector<std::string>{"focean", "fland"},
                                       which ? std::vector<std::string>{"fhc", "underice"} : varsE, {{1, (long)nA}});
                REQUIRE(false);
            } catch (Exception const &e) {
                REQUIRE(e.code == IBH_ENOKEY && std::string(e.what()).find(which ? "'underice'" : "'fland'") != std::string::npos);
            }
        }

        modele::TopoPacker packer(varsA, varsE, {{1, (long)nA}}, mmA, bbA, mmE, bbE), packer_u(varsA, varsE, {{1, (long)nA}}, mmA, bbA, mmE, bbE);
        std::vector<int16_t> mask_before;
        for (int step = 0; step < 2; ++step) {
            std::vector<ArrayView<const double>> lands = {ArrayView<const double>(land[step][0]), ArrayView<const double>(land[step][1])};
            std::vector<ArrayView<const double>> ices = {ArrayView<const double>(ice[step][0]), ArrayView<const double>(ice[step][1])};
            const std::string name = out + "/step" + std::to_string(step + 1);
            // the planes: merge_topoO, global_AvE, make_topoA (whatever its sanity checks say: the packing does not read them)
            modele::TopoO m = topoo;
            m.ZLAND_MIN.assign((size_t)nO, 7.); m.ZLAND_MAX.assign((size_t)nO, 7.); m.mergemask.assign((size_t)nO, 7);
            std::vector<std::string> errors;
            modele::merge_topoO(m.FOCEANF.data(), m.FGICEF.data(), m.ZATMOF.data(), m.FOCEAN.data(), m.FLAKE.data(), m.FGRND.data(), m.FGICE.data(),
                                m.ZATMO.data(), m.ZICETOP.data(), m.ZLAND_MIN.data(), m.ZLAND_MAX.data(), m.mergemask.data(), gcmO.get(), hspecO,
                                RegridParams(false, true, {{0., 0., 0.}}), lands, ices, eq_rad, errors);
            long offsetE = -1;
            auto AvE = gcmA.global_AvE(lands, ices, ArrayView<const double>(m.FOCEANF), ArrayView<const double>(m.FOCEAN), true, offsetE);
            modele::TopoA a;
            for (std::vector<double> *p : {&a.focean, &a.flake, &a.fgrnd, &a.fgice, &a.zatmo, &a.hlake, &a.zicetop, &a.zland_min, &a.zland_max})
                p->assign(nA, 7.);
            a.mergemask.assign(nA, 7); a.fhc.assign(n3, 7.); a.elevE.assign(n3, 7.); a.underice.assign(n3, 7);
            std::vector<int16_t> ui;
            for (int ihc = 0; ihc < (int)nhc; ++ihc) ui.push_back((int16_t)gcmA.underice(ihc));
            std::vector<std::string> errors2 = modele::make_topoA(
                m.FOCEAN.data(), m.FLAKE.data(), m.FGRND.data(), m.FGICE.data(), m.ZATMO.data(), m.ZLAKE.data(), m.ZICETOP.data(), m.ZLAND_MIN.data(),
                m.ZLAND_MAX.data(), m.mergemask.data(), hspecO, hspecA, {{1, (long)nA}}, gcmA.hcdefs(), ui, *AvE, a.focean.data(), a.flake.data(),
                a.fgrnd.data(), a.fgice.data(), a.zatmo.data(), a.hlake.data(), a.zicetop.data(), a.zland_min.data(), a.zland_max.data(),
                a.mergemask.data(), a.fhc.data(), a.elevE.data(), a.underice.data());

            VectorMultivec A((int)varsA.size()), E((int)varsE.size());
            packer.pack(a, (int)nhc, step == 1, A, E);
            REQUIRE(packer.mergemaskA0() == a.mergemask);
            std::vector<long> kept;
            for (size_t c = 0; c < nA; ++c)
                if (a.mergemask[c] != 0 || (step == 1 && mask_before[c] != 0)) kept.push_back((long)c);
            REQUIRE(!kept.empty() && A.size() == kept.size() && E.size() == nhc * kept.size());
            REQUIRE(A.index() == kept);
            const std::vector<long> iE = E.index();
            const std::vector<double> vA = A.vals(), vE = E.vals(), wE = E.weights();
            for (size_t h = 0; h < nhc; ++h)
                for (size_t r = 0; r < kept.size(); ++r) {
                    const size_t e = h * kept.size() + r, src = h * nA + (size_t)kept[r];
                    REQUIRE(iE[e] == kept[r] + (long)(h * nA) && wE[e] == 1.0);
                    REQUIRE(vE[3 * e] == a.fhc[src] && vE[3 * e + 1] == a.elevE[src] * 2. + .5 && vE[3 * e + 2] == (double)a.underice[src]);
                }
            for (size_t r = 0; r < kept.size(); ++r)
                REQUIRE(vA[6 * r] == a.focean[(size_t)kept[r]] && vA[6 * r + 4] == a.zatmo[(size_t)kept[r]] * 9.80665 + -3.5);
            REQUIRE(dump_vec(name + ".A", A) && dump_vec(name + ".E", E) && dump(name + ".mergemask", a.mergemask));
            mask_before = a.mergemask;

            // the update_topo overload is the same calls; when make_topoA's checks fail it throws before it packs
            modele::TopoO u = topoo;
            VectorMultivec A2((int)varsA.size()), E2((int)varsE.size());
            try {
                gcmA.update_topo(u, lands, ices, step == 1, packer_u, A2, E2);
                REQUIRE(errors.empty() && errors2.empty());
                REQUIRE(A2.index() == A.index() && E2.index() == E.index() && same_bits(A2.vals(), vA) && same_bits(E2.vals(), vE));
                std::printf("step %d: update_topo packed %zu + %zu entries\n", step + 1, A2.size(), E2.size());
            } catch (Exception const &e) {
                if (e.code == IBH_ENODEVICE) throw;
                REQUIRE((!errors.empty() || !errors2.empty()) && std::string(e.what()).find("halting!") != std::string::npos);
                std::printf("step %d: update_topo halted on its sanity checks, TopoPacker::pack alone was compared\n", step + 1);
                packer_u.pack(a, (int)nhc, step == 1, A2, E2);      // keep its mergemaskA0 in step
            }
        }

        // append_planes on its own: an int16 plane among doubles, a vector that already holds an entry, the class-fastest index
        {
            const std::vector<double> p0 = {1.5, -0., 3.5, 4.5, 5.5, 6.5};
            const std::vector<int16_t> p1 = {-32768, 32767, 3, 4, 5, 6}, mask = {0, 7, 0}, mask0 = {-1, 0, 0};
            VectorMultivec v(2);
            const double first[2] = {9., 8.};
            v.add(41, first, .25);
            REQUIRE(v.append_planes({p0.data(), p1.data()}, {0, 1}, 3, 2, 3, mask.data(), mask0.data(), 2, 1) == 2);
            REQUIRE((v.index() == std::vector<long>{41, 0, 2, 1, 3}) && (v.weights() == std::vector<double>{.25, 1., 1., 1., 1.}));
            REQUIRE(same_bits(v.vals(), {9., 8., 1.5, -32768., -0., 32767., 4.5, 4., 5.5, 5.}));
            try {
                v.append_planes({p0.data(), nullptr}, {0, 1}, 3, 2, 3, mask.data(), nullptr, 2, 1);
                REQUIRE(false);
            } catch (Exception const &e) {
                REQUIRE(e.code == IBH_EINVAL && std::string(e.what()).find("plane 1 is null") != std::string::npos && v.size() == 5);
            }
        }
    } catch (Exception const &e) {
        if (no_gpu(e)) return 3;
        std::printf("FAILED: exception %d: %s\n", e.code, e.what());
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
