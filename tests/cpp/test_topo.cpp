// C++ test of update_topo's field handling in icebin_amd/host/icebin_hip.hpp (namespace icebin::modele): merge_topoO, make_topoA
// and GCMRegridder_ModelE::update_topo on two ice sheets in one GCMRegridder_Standard on an 8 x 6 ocean grid with a base ice
// matrix.  The results go to <outdir>/*.bin and the sanity-check strings to <outdir>/*.txt, which tests/test_cpp_topo.py compares
// with the Python surface, bitwise.
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

static bool dump_text(std::string const &path, std::vector<std::string> const &lines) {
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) return false;
    for (std::string const &l : lines) std::fprintf(f, "%s\n", l.c_str());
    return std::fclose(f) == 0;
}

static bool dump_topoo(std::string const &out, std::string const &name, modele::TopoO const &t) {
    const std::string p = out + "/" + name + ".";
    return dump(p + "FOCEANF", t.FOCEANF) && dump(p + "FGICEF", t.FGICEF) && dump(p + "ZATMOF", t.ZATMOF) && dump(p + "FOCEAN", t.FOCEAN) &&
           dump(p + "FLAKE", t.FLAKE) && dump(p + "FGRND", t.FGRND) && dump(p + "FGICE", t.FGICE) && dump(p + "ZATMO", t.ZATMO) &&
           dump(p + "ZICETOP", t.ZICETOP) && dump(p + "ZLAND_MIN", t.ZLAND_MIN) && dump(p + "ZLAND_MAX", t.ZLAND_MAX) &&
           dump(p + "mergemask", t.mergemask);
}

static bool dump_topoa(std::string const &out, std::string const &name, modele::TopoA const &a) {
    const std::string p = out + "/" + name + ".";
    return dump(p + "focean", a.focean) && dump(p + "flake", a.flake) && dump(p + "fgrnd", a.fgrnd) && dump(p + "fgice", a.fgice) &&
           dump(p + "zatmo", a.zatmo) && dump(p + "hlake", a.hlake) && dump(p + "zicetop", a.zicetop) && dump(p + "zland_min", a.zland_min) &&
           dump(p + "zland_max", a.zland_max) && dump(p + "mergemask", a.mergemask) && dump(p + "fhc", a.fhc) && dump(p + "elevE", a.elevE) &&
           dump(p + "underice", a.underice);
}

static void merge(modele::TopoO &t, GCMRegridder_Standard const *gcmO, HntrSpec const &O, std::vector<ArrayView<const double>> const &lands,
                  std::vector<ArrayView<const double>> const &ices, double eq_rad, std::vector<std::string> &errors) {
    t.ZLAND_MIN.assign(t.FOCEAN.size(), 7.); t.ZLAND_MAX.assign(t.FOCEAN.size(), 7.); t.mergemask.assign(t.FOCEAN.size(), 7);
    modele::merge_topoO(t.FOCEANF.data(), t.FGICEF.data(), t.ZATMOF.data(), t.FOCEAN.data(), t.FLAKE.data(), t.FGRND.data(), t.FGICE.data(),
                        t.ZATMO.data(), t.ZICETOP.data(), t.ZLAND_MIN.data(), t.ZLAND_MAX.data(), t.mergemask.data(), gcmO, O,
                        RegridParams(false, true, {{0., 0., 0.}}), lands, ices, eq_rad, errors);
}

int main(int argc, char **argv) {
    const std::string out = argc > 1 ? argv[1] : ".";
    const HntrSpec hspecO(8, 6, 0., 1800.);
    const HntrSpec hspecI[2] = {HntrSpec(48, 36, 0.5, 300.), HntrSpec(24, 18, 0.25, 600.)};
    const double eq_rad = 6371000., nan = std::numeric_limits<double>::quiet_NaN();
    const long nO = hspecO.size();
    // the inputs the Python side rebuilds: land masks, ice masks that are subsets of them, the TOPOO planes, the base ice
    std::vector<double> land[2], ice[2];
    for (int i = 0; i < hspecI[0].size(); ++i) land[0].push_back((i * 7) % 5 == 0 ? nan : (double)(i % 3000) - 100.);
    for (int i = 0; i < hspecI[1].size(); ++i) land[1].push_back((i * 3) % 4 == 0 ? nan : (double)((i * 5) % 3000) + 200.);
    for (int k = 0; k < 2; ++k)
        for (size_t i = 0; i < land[k].size(); ++i) ice[k].push_back(i % 3 == 0 || !(land[k][i] >= 0. && land[k][i] <= 3000.) ? nan : land[k][i]);
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
    try {
        std::shared_ptr<GCMRegridder_Standard> gcmO(new GCMRegridder_Standard);
        AbbrGrid agridO;
        agridO.sparse_extent = nO;
        for (long i = 0; i < nO; ++i) { agridO.dim_to_sparse.push_back(i); agridO.native_area.push_back(1.e13); }
        gcmO->init(std::move(agridO), {0., 1500., 3000.}, true);
        for (int k = 0; k < 2; ++k) {       // the exchange grid holds every cell of the LAND mask
            auto one = modele::new_gcmA_standard(hspecO, hspecI[k], ArrayView<const double>(land[k]), {0., 1500., 3000.}, true, eq_rad);
            int64_t nX = 0;
            check(ibh_regridder_exgrid(one->ice_regridder(0)->handle(), &nX, nullptr, nullptr));
            ExchangeGrid ex;
            ex.indices.resize(2 * (size_t)nX); ex.overlaps.resize((size_t)nX);
            check(ibh_regridder_exgrid(one->ice_regridder(0)->handle(), &nX, ex.indices.data(), ex.overlaps.data()));
            gcmO->add_sheet("sheet" + std::to_string(k), hspecI[k].size(), ex);
        }
        std::vector<ArrayView<const double>> lands = {ArrayView<const double>(land[0]), ArrayView<const double>(land[1])};
        std::vector<ArrayView<const double>> ices = {ArrayView<const double>(ice[0]), ArrayView<const double>(ice[1])};

        // merge_topoO, then make_topoA on its planes under global_AvE's matrix
        modele::TopoO m = topoo;
        std::vector<std::string> errors;
        merge(m, gcmO.get(), hspecO, lands, ices, eq_rad, errors);
        REQUIRE(errors.empty());
        int nmerged = 0;
        for (long i = 0; i < nO; ++i) {
            REQUIRE(m.mergemask[(size_t)i] == 0 || m.mergemask[(size_t)i] == 1);
            REQUIRE((m.mergemask[(size_t)i] == 0) == std::isnan(m.ZLAND_MIN[(size_t)i]));
            nmerged += m.mergemask[(size_t)i];
        }
        REQUIRE(nmerged >= 8);
        REQUIRE(dump_topoo(out, "merged", m));

        modele::GCMRegridder_ModelE gcmA(base, gcmO, hspecO, eq_rad);
        long offsetE = -1;
        auto AvE = gcmA.global_AvE(lands, ices, ArrayView<const double>(m.FOCEANF), ArrayView<const double>(m.FOCEAN), true, offsetE);
        const HntrSpec hspecA = gcmA.hspecA();
        const size_t nA = (size_t)hspecA.size(), nhc = gcmA.hcdefs().size(), n3 = nA * (nhc + 1);
        REQUIRE(nA == 12 && nhc == 5 && offsetE == 3 * nO);
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
        REQUIRE(dump_topoa(out, "topoa", a) && dump_text(out + "/topoa.errors.txt", errors2));
        for (size_t c = 0; c < nA; ++c) REQUIRE(a.elevE[nhc * nA + c] == a.zatmo[c] && a.elevE[c] == 0. && a.elevE[3 * nA + c] == 1500.);

        // update_topo is the three calls: the same planes, or (when make_topoA's checks fail) the same strings in what it throws
        modele::TopoO u = topoo;
        std::string thrown;
        try {
            modele::TopoA ua = gcmA.update_topo(u, lands, ices);
            REQUIRE(errors2.empty() && ua.offsetE == offsetE);
            REQUIRE(ua.fhc == a.fhc && ua.underice == a.underice && ua.mergemask == a.mergemask && ua.fgice == a.fgice && ua.zicetop == a.zicetop);
            REQUIRE(dump_topoa(out, "update", ua));
            std::vector<int64_t> kE;
            std::vector<double> wE;
            for (auto const &kv : ua.wEAm_base) { kE.push_back(kv.first); wE.push_back(kv.second); }
            REQUIRE(dump(out + "/update.wEAm_base.iE", kE) && dump(out + "/update.wEAm_base.w", wE));
        } catch (Exception const &e) {
            if (e.code == IBH_ENODEVICE) throw;
            thrown = e.what();
            REQUIRE(!errors2.empty() && thrown.find("halting!") != std::string::npos);
            for (std::string const &s : errors2) REQUIRE(thrown.find("ERROR: " + s) != std::string::npos);
        }
        REQUIRE(u.FOCEANF == m.FOCEANF && u.FOCEAN == m.FOCEAN && u.ZICETOP == m.ZICETOP && u.mergemask == m.mergemask);
        REQUIRE(dump_text(out + "/update.thrown.txt", {thrown.empty() ? std::string("-") : std::string("thrown")}));

        // NaN planted in an input and a land fraction off by 1e-10: the strings, check by check, then j, then i
        modele::TopoO bad = topoo;
        bad.ZATMOF[13] = nan; bad.ZATMOF[2] = nan; bad.FLAKE[30] = nan; bad.FGRND[11] += 1e-10;
        std::vector<std::string> berr;
        merge(bad, gcmO.get(), hspecO, lands, ices, eq_rad, berr);
        REQUIRE(berr.size() >= 6 && berr[0] == "(3, 1): zatmoOp2-0 is NaN" && berr[1] == "(6, 2): zatmoOp2-0 is NaN");
        REQUIRE(berr.back().find("(4, 2): FOCEAN(0) + FGRND(0.625) + FLAKE(0.125) + FGICE(0.25)  = 1") == 0);
        REQUIRE(dump_text(out + "/merged.errors.txt", berr) && dump_topoo(out, "bad", bad));
        try {
            gcmA.update_topo(bad = topoo, lands, {ices[0]});
            REQUIRE(false);
        } catch (Exception const &e) {
            if (e.code == IBH_ENODEVICE) throw;
            REQUIRE(e.code == IBH_EINVAL && std::string(e.what()).find("2 land masks and 1 ice masks for 2 sheets") != std::string::npos);
        }
    } catch (Exception const &e) {
        if (no_gpu(e)) return 3;
        std::printf("FAILED: exception %d: %s\n", e.code, e.what());
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
