// The decisions of a smoothed build (icebin_amd/csrc/smooth_plan.h): the bin geometry with its cap, the order of the device forms for
// every knob setting on both sides of the row threshold, the LDS layout of the tile kernel, and the split of a shared tile build among
// the ranks -- which otherwise runs only inside multi-process GPU tests at worlds 2 and 3.  Expected values are written out here: the
// bin geometry from its definition (grid_expected), the rest from smooth_matrix as it stood before the plan existed (the *_before
// functions are that code's arithmetic, line by line); the properties are what the kernels rely on.  Host code only: its own
// get_tuning, no HIP.
#include "../../icebin_amd/csrc/smooth_plan.h"

#include <cstdio>
#include <map>
#include <random>
#include <string>

static std::map<std::string, int> g_tuning;
static std::map<std::string, int> g_reads;
int ibh::get_tuning(const char *key, int dflt) {
    ++g_reads[key];
    auto it = g_tuning.find(key);
    return it == g_tuning.end() ? dflt : it->second;
}

using namespace ibh;
static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { if (g_failed < 50) printf("FAILED line %d: %s\n", __LINE__, #c); ++g_failed; } } while (0)

// ---- the bins ----------------------------------------------------------------------------------------------------------------------
// The expected geometry, written out: bins two sigmas wide over the bounding box, regrown to extent / 4096 where that is wider (the
// cap), and on either branch wider by the margin that keeps neighbours within one bin of each other (smooth_plan.h states the argument).
// Before the margin the widths were exactly 2 sigma, or extent / 4096 * (1 + 1e-12) when the uncapped count reached 4096 -- which on
// the cap's edge, an extent of [4095, 4096) bin widths, was up to 1/4096 NARROWER than two sigmas.
struct GridExpected { double x0, y0, bw, bh; int nbx, nby; };
static GridExpected grid_expected(const double cmin[2], const double cmax[2], const double sigma[3]) {
    const double ex = cmax[0] - cmin[0], ey = cmax[1] - cmin[1];
    GridExpected v{cmin[0], cmin[1], std::max(2.0 * sigma[0], ex / 4096.0) * (1.0 + 1e-9), std::max(2.0 * sigma[1], ey / 4096.0) * (1.0 + 1e-9), 1, 1};
    v.nbx = (int)std::min(4096.0, std::floor(ex / v.bw) + 1.0);
    v.nby = (int)std::min(4096.0, std::floor(ey / v.bh) + 1.0);
    return v;
}
// the unclamped bin of a coordinate, as smooth_bin forms it on the device
static int bin_of(double c, double c0, double width) { return (int)((c - c0) / width); }
static void check_grid(double x0, double y0, double ex, double ey, double sx, double sy, int want_nbx = 0, int want_nby = 0) {
    const double cmin[2] = {x0, y0}, cmax[2] = {x0 + ex, y0 + ey}, sigma[3] = {sx, sy, 100.0};
    const SmoothGrid g = smooth_grid(cmin, cmax, sigma);
    const GridExpected b = grid_expected(cmin, cmax, sigma);
    CHECK(g.x0 == b.x0 && g.y0 == b.y0 && g.bw == b.bw && g.bh == b.bh && g.nbx == b.nbx && g.nby == b.nby);
    CHECK(g.nbx >= 1 && g.nbx <= 4096 && g.nby >= 1 && g.nby <= 4096 && g.nbins() == (size_t)g.nbx * g.nby);
    // bins only grow, on every branch, so that 3 x 3 bins hold everything within two sigmas; and by no more than the margin or the cap
    CHECK(g.bw > 2.0 * sx && g.bh > 2.0 * sy);
    CHECK(g.bw <= std::max(2.0 * sx, (cmax[0] - cmin[0]) / 4096.0) * (1 + 2e-9) && g.bh <= std::max(2.0 * sy, (cmax[1] - cmin[1]) / 4096.0) * (1 + 2e-9));
    CHECK(bin_of(cmin[0], g.x0, g.bw) == 0 && bin_of(cmin[1], g.y0, g.bh) == 0);
    // the far corner falls inside the grid before clamping -- by construction where the cap is not active, by the (1 + 1e-12) where it is
    CHECK(bin_of(cmax[0], g.x0, g.bw) < g.nbx && bin_of(cmax[1], g.y0, g.bh) < g.nby);
    if (g.nbx < 4096) CHECK(bin_of(cmax[0], g.x0, g.bw) == g.nbx - 1);
    if (g.nby < 4096) CHECK(bin_of(cmax[1], g.y0, g.bh) == g.nby - 1);
    if (want_nbx) CHECK(g.nbx == want_nbx);
    if (want_nby) CHECK(g.nby == want_nby);
}
static void test_grid() {
    check_grid(0, 0, 0, 0, 50e3, 50e3, 1, 1);                       // zero extent
    check_grid(-3e5, 2e5, 99e3, 1e3, 50e3, 50e3, 1, 1);             // smaller than one bin
    check_grid(0, 0, 100e3, 300e3, 50e3, 50e3, 1, 3);               // exact multiples of two sigmas: the margin keeps the far edge in the last bin
    check_grid(0, 0, 100e3 + 1.0, 300e3 + 1.0, 50e3, 50e3, 2, 4);   // just beyond: it opens one
    check_grid(25e3, 25e3, 1450e3, 2750e3, 60e3, 60e3, 13, 23);     // the 50 km test grid
    check_grid(0, 0, 4095 * 100e3, 4094 * 100e3, 50e3, 50e3, 4095, 4094);      // the last sizes below the cap
    check_grid(0, 0, 4095.5 * 100e3, 4096 * 100e3, 50e3, 50e3, 4096, 4096);    // 4096 bins uncapped (two sigmas wide), and the cap's first size
    check_grid(0, 0, 4096 * 100e3, 10e3, 50e3, 50e3, 4096, 1);      // the cap in x only
    check_grid(0, 0, 10e3, 1e9, 50e3, 50e3, 1, 4096);               // in y only
    check_grid(-1e9, -1e9, 3e9, 5e9, 10.0, 20.0, 4096, 4096);       // in both
    check_grid(0, 0, 5000 * 100e3, 4097 * 100e3, 50e3, 50e3, 4096, 4096);
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    for (int k = 0; k < 20000; ++k) {
        const double ex = std::pow(10.0, 2.0 + 8.0 * u(rng)), ey = std::pow(10.0, 2.0 + 8.0 * u(rng));
        const double sx = std::pow(10.0, 1.0 + 5.0 * u(rng)), sy = std::pow(10.0, 1.0 + 5.0 * u(rng));
        check_grid((u(rng) - .5) * 1e7, (u(rng) - .5) * 1e7, ex, ey, sx, sy);
        check_grid(0, 0, std::floor(ex / (2 * sx)) * 2 * sx, std::floor(ey / (2 * sy)) * 2 * sy, sx, sy);      // multiples of the width
    }
}

// two coordinates the smoother takes for neighbours -- fl((b - a) / sigma) < 2 -- fall at most one bin apart: the pair that bins of exactly
// two sigmas put two apart, and pairs just under two sigmas apart a few ulps around every kind of bin edge, on grids far from the origin
static void test_neighbours_one_bin_apart() {
    {
        const double cmin[2] = {-1234500.0, 0}, cmax[2] = {215500.0, 1e5}, sigma[3] = {50e3, 50e3, 1e6};
        const double a = -234500.0000000001, b = -134500.00000000012;
        CHECK((b - a) / sigma[0] < 2.0);
        CHECK(bin_of(b, cmin[0], 2.0 * sigma[0]) - bin_of(a, cmin[0], 2.0 * sigma[0]) == 2);      // (the bins before the margin)
        const SmoothGrid g = smooth_grid(cmin, cmax, sigma);
        CHECK(bin_of(b, g.x0, g.bw) - bin_of(a, g.x0, g.bw) <= 1);
    }
    std::mt19937_64 rng(23);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    long tried = 0;
    for (int k = 0; k < 4000; ++k) {
        const double sx = std::pow(10.0, 1.0 + 4.0 * u(rng)), ext = sx * std::pow(10.0, 4.6 * u(rng));
        const double x0 = (u(rng) - .5) * std::pow(10.0, 3.0 + 7.0 * u(rng));
        const double cmin[2] = {x0, 0}, cmax[2] = {x0 + ext, 1.0}, sigma[3] = {sx, 1.0, 1.0};
        const SmoothGrid g = smooth_grid(cmin, cmax, sigma);
        for (int t = 0; t < 32; ++t) {
            const int e = 1 + (int)(rng() % (uint64_t)std::max(g.nbx, 2));
            double a = x0 + e * (rng() % 2 ? 2.0 * sx : g.bw);       // an edge of the old bins, or of the new ones
            for (int s = (int)(rng() % 5); s > 0; --s) a = std::nextafter(a, rng() % 2 ? -1e300 : 1e300);
            double b = a + std::nextafter(2.0 * sx, 0.0);
            for (int s = (int)(rng() % 3); s > 0; --s) b = std::nextafter(b, -1e300);
            if (a < x0 || b > x0 + ext || !((b - a) / sx < 2.0)) continue;
            ++tried;
            CHECK(bin_of(b, g.x0, g.bw) - bin_of(a, g.x0, g.bw) <= 1);
        }
    }
    CHECK(tried > 10000);
}

// ---- the forms ---------------------------------------------------------------------------------------------------------------------
static void check_plan(int nrow, int direct, int tile, int max_rows) {
    g_tuning.clear();
    if (direct != -2) g_tuning["smooth_direct"] = direct;
    if (tile != -2) g_tuning["smooth_tile"] = tile;
    if (max_rows >= 0) g_tuning["smooth_direct_max_rows"] = max_rows;
    g_reads.clear();
    const double cmin[2] = {0, 0}, cmax[2] = {1e6, 2e6}, sigma[3] = {50e3, 50e3, 100.0};
    const SmoothPlan p = plan_smooth(nrow, cmin, cmax, sigma);
    for (auto &kv : g_reads) CHECK(kv.second == 1);             // every knob once per build
    // smooth_matrix before: `if (tile > 0 || (tile < 0 && !take_direct)) {tiles}  if (take_direct) {direct}  triplets`
    const int d = direct == -2 ? -1 : direct, t = tile == -2 ? -1 : tile;
    const bool take_direct = d > 0 || (d < 0 && nrow <= (max_rows >= 0 ? max_rows : 16384));
    SmoothForm want[3];
    int n = 0;
    if (t > 0 || (t < 0 && !take_direct)) want[n++] = SMOOTH_TILE;
    if (take_direct) want[n++] = SMOOTH_DIRECT;
    want[n++] = SMOOTH_TRIPLET;
    CHECK(p.nform == n);
    for (int k = 0; k < n && k < p.nform; ++k) CHECK(p.form[k] == want[k]);
    CHECK(p.nform >= 1 && p.nform <= 3 && p.form[p.nform - 1] == SMOOTH_TRIPLET);
    for (int a = 0; a < p.nform; ++a)
        for (int b = a + 1; b < p.nform; ++b) CHECK(p.form[a] != p.form[b]);
    for (int f = SMOOTH_TRIPLET; f <= SMOOTH_TILE; ++f) CHECK(p.tries((SmoothForm)f) == (std::find(want, want + n, (SmoothForm)f) != want + n));
    CHECK(!p.tries(SMOOTH_NONE));
    const SmoothGrid g = smooth_grid(cmin, cmax, sigma);
    CHECK(p.grid.nbx == g.nbx && p.grid.nby == g.nby && p.grid.bw == g.bw && p.grid.bh == g.bh && p.grid.x0 == g.x0 && p.grid.y0 == g.y0);
}
static void test_plan() {
    for (int direct : {-2, -1, 0, 1})                           // (-2: the knob is not set)
        for (int tile : {-2, -1, 0, 1}) {
            for (int nrow : {1, 16384, 16385, 1 << 22}) check_plan(nrow, direct, tile, -1);
            for (int nrow : {1, 100, 101, 16384, 16385}) check_plan(nrow, direct, tile, 100);
            check_plan(5, direct, tile, 0);
        }
    g_tuning.clear();
    const double cmin[2] = {0, 0}, cmax[2] = {1e6, 2e6}, sigma[3] = {50e3, 50e3, 100.0};
    // the defaults, spelled out: small grids direct then triplets, larger ones tiles then triplets
    SmoothPlan p = plan_smooth(16384, cmin, cmax, sigma);
    CHECK(p.nform == 2 && p.form[0] == SMOOTH_DIRECT && p.form[1] == SMOOTH_TRIPLET);
    p = plan_smooth(16385, cmin, cmax, sigma);
    CHECK(p.nform == 2 && p.form[0] == SMOOTH_TILE && p.form[1] == SMOOTH_TRIPLET);
    g_tuning["smooth_direct"] = 1; g_tuning["smooth_tile"] = 1;
    p = plan_smooth(16385, cmin, cmax, sigma);
    CHECK(p.nform == 3 && p.form[0] == SMOOTH_TILE && p.form[1] == SMOOTH_DIRECT && p.form[2] == SMOOTH_TRIPLET);
    g_tuning["smooth_direct"] = 0; g_tuning["smooth_tile"] = 0;
    p = plan_smooth(10, cmin, cmax, sigma);
    CHECK(p.nform == 1 && p.form[0] == SMOOTH_TRIPLET);
    g_tuning.clear();
    CHECK(SMOOTH_NONE == 0 && SMOOTH_TRIPLET == 1 && SMOOTH_DIRECT == 2 && SMOOTH_TILE == 3);      // ibh_weighted_smoothed_by's values
}

// ---- the LDS of the tile kernel ----------------------------------------------------------------------------------------------------
static void test_lds() {
    CHECK(SMD_HASH == 256 && SMD_MAXCOL == 128 && SMD_HITS == 1024 && SMD_WAVES == 4 && SMT_KMAX == 128 && SMT_ROWMAX == 8 && SMT_HASH == 1024);
    CHECK(sizeof(SmtCand) == 32);
    for (int k = 1; k <= SMT_KMAX; ++k) {
        const SmtLds l = smt_lds(k);
        // the host's launch size before: kmax * 64 * 8 + 64 * sizeof(SmtCand) + 64 * SMT_ROWMAX * 8 + SMT_KMAX * 4 + 64 * SMT_ROWMAX + 64
        CHECK(l.total == (size_t)k * 64 * 8 + 64 * 32 + 64 * 8 * 8 + 128 * 4 + 64 * 8 + 64);
        // the kernel's carve-up before: acc [k][64] doubles, then SmtCand [64], double [64][ROWMAX], int [KMAX], bytes [64][ROWMAX], bytes [64]
        CHECK(l.acc == 0 && l.s_c == (size_t)k * 64 * 8 && l.s_val == l.s_c + 64 * 32 && l.s_cols == l.s_val + 64 * 8 * 8 &&
              l.s_slot == l.s_cols + 128 * 4 && l.s_ne == l.s_slot + 64 * 8 && l.total == l.s_ne + 64);
        CHECK(l.acc < l.s_c && l.s_c < l.s_val && l.s_val < l.s_cols && l.s_cols < l.s_slot && l.s_slot < l.s_ne && l.s_ne < l.total);
        CHECK(l.acc % alignof(double) == 0 && l.s_c % alignof(SmtCand) == 0 && l.s_val % alignof(double) == 0 && l.s_cols % alignof(int) == 0);
    }
    CHECK(smt_lds(SMT_KMAX).total <= 160 * 1024 && SMT_LDS_RAISED == 160 * 1024);
    CHECK(SMT_KMAX <= 256 && SMT_KMAX <= 128);                  // a slot is a byte; the presence mask of a row is two 64-bit words
    static_assert(smt_lds(1).total > 0, "smt_lds is a constant expression: the kernel and the host evaluate the same function");
}

// ---- the shares of a shared tile build ---------------------------------------------------------------------------------------------
struct ShareBefore { std::vector<int> bs; int b0, b1, m0, m1, w0, w1, c0, c1; };
static ShareBefore share_before(const std::vector<uint32_t> &hb, int nbx, int nby, int world, int rank) {
    ShareBefore o;
    const int nb = nbx * nby;
    const size_t nbins = (size_t)nb;
    std::vector<double> cw(nbins + 1, 0.0);
    for (int b = 0; b < nb; ++b) {
        const int bx = b % nbx, by = b / nbx;
        const int x0 = std::max(bx - 1, 0), x1 = std::min(bx + 1, nbx - 1);
        double ncand = 0;
        for (int yy = std::max(by - 1, 0); yy <= std::min(by + 1, nby - 1); ++yy)
            ncand += (double)(hb[(size_t)yy * nbx + x1 + 1] - hb[(size_t)yy * nbx + x0]);
        cw[(size_t)b + 1] = cw[(size_t)b] + (double)(hb[(size_t)b + 1] - hb[(size_t)b]) * ncand;
    }
    o.bs.assign((size_t)world + 1, nb);
    o.bs[0] = 0;
    for (int r = 1; r < world; ++r)
        o.bs[(size_t)r] = std::max(o.bs[(size_t)r - 1], (int)(std::lower_bound(cw.begin(), cw.end(), cw[nbins] * r / world) - cw.begin()));
    auto waves_before = [&](int bb) {
        uint32_t s = 0;
        for (int b = 0; b < bb; ++b) s += (hb[(size_t)b + 1] - hb[(size_t)b] + 63) / 64;
        return (int)s;
    };
    o.b0 = o.bs[(size_t)rank]; o.b1 = o.bs[(size_t)rank + 1];
    o.m0 = (int)hb[(size_t)o.b0]; o.m1 = (int)hb[(size_t)o.b1];
    o.w0 = waves_before(o.b0); o.w1 = waves_before(o.b1);
    o.c0 = (int)hb[(size_t)std::max(o.b0 - nbx - 1, 0)]; o.c1 = (int)hb[(size_t)std::min(o.b1 + nbx + 1, nb)];
    return o;
}
static long g_shares = 0;
static void check_shares(int nbx, int nby, const std::vector<uint32_t> &count, std::mt19937_64 &rng) {
    const int nb = nbx * nby;
    std::vector<uint32_t> hb((size_t)nb + 1, 0), wstart((size_t)nb + 1, 0);       // binstart, and the device's scan of the waves per bin
    for (int b = 0; b < nb; ++b) {
        hb[(size_t)b + 1] = hb[(size_t)b] + count[(size_t)b];
        wstart[(size_t)b + 1] = wstart[(size_t)b] + (count[(size_t)b] + 63) / 64;
    }
    const int nmem = (int)hb[(size_t)nb], nwaves = (int)wstart[(size_t)nb];
    // the smoothed rows the members produce: lengths up to SMT_KMAX, scanned in member order as mptr is on the device
    std::vector<uint32_t> mptr((size_t)nmem + 1, 0);
    for (int q = 0; q < nmem; ++q) mptr[(size_t)q + 1] = mptr[(size_t)q] + (uint32_t)(rng() % (SMT_KMAX + 1));
    const uint32_t nnz2 = mptr[(size_t)nmem];
    for (int world = 1; world <= 8; ++world) {
        const std::vector<int> bs = smt_split(hb, nbx, nby, world);
        CHECK((int)bs.size() == world + 1 && bs[0] == 0 && bs[(size_t)world] == nb);
        const std::vector<uint32_t> ms = smt_member_starts(hb, bs);
        const std::vector<int64_t> ol = smt_gather_offsets(ms, 4);
        std::vector<uint32_t> hp((size_t)world + 1);
        for (int r = 0; r <= world; ++r) hp[(size_t)r] = mptr[ms[(size_t)r]];
        const std::vector<int64_t> oc = smt_gather_offsets(hp, 4), ov = smt_gather_offsets(hp, 8);
        CHECK((int)ol.size() == world + 1 && (int)oc.size() == world + 1 && (int)ov.size() == world + 1);
        CHECK(ol[0] == 0 && oc[0] == 0 && ov[0] == 0);
        CHECK(ol[(size_t)world] == 4 * (int64_t)nmem && oc[(size_t)world] == 4 * (int64_t)nnz2 && ov[(size_t)world] == 8 * (int64_t)nnz2);
        SmtShare prev;
        for (int rank = 0; rank < world; ++rank, ++g_shares) {
            const SmtShare s = smt_share(hb, bs, rank, nbx);
            const ShareBefore o = share_before(hb, nbx, nby, world, rank);
            CHECK(bs == o.bs);
            CHECK(s.b0 == o.b0 && s.b1 == o.b1 && s.m0 == o.m0 && s.m1 == o.m1 && s.w0 == o.w0 && s.w1 == o.w1 && s.c0 == o.c0 && s.c1 == o.c1);
            // the before-code's gatherv tables: ol[r] = 4 * hb[bs[r]], oc / ov = 4 / 8 * mptr[hb[bs[r]]]
            CHECK(ol[(size_t)rank] == 4 * (int64_t)hb[(size_t)o.bs[(size_t)rank]] && oc[(size_t)rank] == 4 * (int64_t)mptr[hb[(size_t)o.bs[(size_t)rank]]] &&
                  ov[(size_t)rank] == 8 * (int64_t)mptr[hb[(size_t)o.bs[(size_t)rank]]]);
            // contiguous, monotone, covering
            CHECK(s.b0 <= s.b1 && s.m0 <= s.m1 && s.w0 <= s.w1 && s.c0 <= s.c1);
            if (rank == 0) CHECK(s.b0 == 0 && s.m0 == 0 && s.w0 == 0);
            else CHECK(s.b0 == prev.b1 && s.m0 == prev.m1 && s.w0 == prev.w1);
            if (rank == world - 1) CHECK(s.b1 == nb && s.m1 == nmem && s.w1 == nwaves);
            // the waves are the device's: k_smt_tile finds its bin through wstart
            CHECK(s.w0 == (int)wstart[(size_t)s.b0] && s.w1 == (int)wstart[(size_t)s.b1]);
            CHECK(s.m0 == (int)hb[(size_t)s.b0] && s.m1 == (int)hb[(size_t)s.b1]);
            // a rank reads only candidates it packed: every member position of the 3 x 3 neighbourhood of every bin it owns
            CHECK(s.c0 >= 0 && s.c1 <= nmem && s.c0 <= s.m0 && s.m1 <= s.c1);
            for (int b = s.b0; b < s.b1; ++b) {
                const int bx = b % nbx, by = b / nbx;
                const int x0 = std::max(bx - 1, 0), x1 = std::min(bx + 1, nbx - 1);
                for (int yy = std::max(by - 1, 0); yy <= std::min(by + 1, nby - 1); ++yy)
                    CHECK((int)hb[(size_t)yy * nbx + x0] >= s.c0 && (int)hb[(size_t)yy * nbx + x1 + 1] <= s.c1);
            }
            // what the gathervs move for this rank: its row lengths and its rows, nothing else
            CHECK(ol[(size_t)rank] == 4 * (int64_t)s.m0 && ol[(size_t)rank + 1] == 4 * (int64_t)s.m1);
            CHECK(ol[(size_t)rank] <= ol[(size_t)rank + 1] && oc[(size_t)rank] <= oc[(size_t)rank + 1] && ov[(size_t)rank] <= ov[(size_t)rank + 1]);
            CHECK(oc[(size_t)rank] == 4 * (int64_t)mptr[(size_t)s.m0] && oc[(size_t)rank + 1] == 4 * (int64_t)mptr[(size_t)s.m1]);
            CHECK(ov[(size_t)rank] == 2 * oc[(size_t)rank]);
            prev = s;
        }
        if (world == 1) {           // one rank: the whole range, as smt_whole gives it without the histogram
            const SmtShare s = smt_share(hb, bs, 0, nbx), a = smt_whole(nb, nmem, nwaves);
            CHECK(s.b0 == a.b0 && s.b1 == a.b1 && s.m0 == a.m0 && s.m1 == a.m1 && s.w0 == a.w0 && s.w1 == a.w1 && s.c0 == a.c0 && s.c1 == a.c1);
        }
    }
}
static void test_shares() {
    std::mt19937_64 rng(11);
    auto hist = [&](int nbx, int nby, std::initializer_list<std::pair<int, uint32_t>> bins) {
        std::vector<uint32_t> c((size_t)nbx * nby, 0);
        for (auto &p : bins) c[(size_t)p.first] = p.second;
        check_shares(nbx, nby, c, rng);
    };
    hist(3, 3, {});                                             // empty
    hist(1, 1, {});
    hist(1, 1, {{0, 100}});                                     // one bin
    hist(1, 1, {{0, 64}});
    hist(5, 4, {{7, 1000}});                                    // all members in one bin
    hist(5, 4, {{0, 1000}});
    hist(5, 4, {{19, 1000}});
    hist(4, 4, {{5, 10}, {10, 700}});                           // fewer non-empty bins than ranks
    hist(1, 7, {{0, 3}, {1, 64}, {2, 65}, {3, 0}, {4, 128}, {5, 129}, {6, 1}});     // nbx == 1
    hist(7, 1, {{0, 3}, {1, 64}, {2, 65}, {3, 0}, {4, 128}, {5, 129}, {6, 1}});     // nby == 1
    hist(3, 2, {{0, 64}, {1, 65}, {2, 64}, {3, 65}, {4, 63}, {5, 1}});              // bins of exactly 64 and 65 members
    hist(2, 2, {{0, 64}, {1, 64}, {2, 64}, {3, 64}});
    for (int k = 0; k < 3000; ++k) {
        const int nbx = 1 + (int)(rng() % 12), nby = 1 + (int)(rng() % 12);
        const int fill = (int)(rng() % 4);                      // dense, half, sparse, a few bins
        const uint32_t top = (uint32_t)(1 + rng() % 300);
        std::vector<uint32_t> c((size_t)nbx * nby, 0);
        for (auto &v : c) {
            const bool on = fill == 0 || (fill == 1 && rng() % 2) || (fill == 2 && rng() % 8 == 0) || (fill == 3 && rng() % 40 == 0);
            if (on) v = (uint32_t)(rng() % (top + 1));
            if (on && rng() % 16 == 0) v = 64 * (uint32_t)(1 + rng() % 3) + (uint32_t)(rng() % 2);        // 64, 65, 128, 129, ...
        }
        check_shares(nbx, nby, c, rng);
    }
}

int main() {
    test_grid();
    test_neighbours_one_bin_apart();
    test_plan();
    test_lds();
    test_shares();
    if (g_failed) { printf("%d checks FAILED\n", g_failed); return 1; }
    printf("%ld shares checked; all checks passed\n", g_shares);
    return 0;
}
