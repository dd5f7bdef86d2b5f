// smooth_plan.h -- how a smoothed build (sigma != 0, DESIGN K5) runs, decided once, as plain values: the bin geometry, the device
// forms in the order they are tried, the LDS layout of the tile kernel and the split of a shared tile build among the ranks
// (smooth.hip's smooth_matrix walks them).  Host arithmetic over the centroids' bounding box, the sigmas, the tuning map and a bin
// histogram: no HIP (tests/cpp/test_smooth_plan.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ibh {
int get_tuning(const char *key, int dflt);

// ---- the limits --------------------------------------------------------------------------------------------------------------------
// the direct form (k_smooth_direct): hash slots and columns of a row, hits parked in LDS, rows (waves) per workgroup
constexpr int SMD_HASH = 256, SMD_MAXCOL = 128, SMD_HITS = 1024, SMD_WAVES = 4;
// the tile form (k_smt_*): columns around a bin, entries of a member's row of M, hash slots of the column tables
constexpr int SMT_KMAX = 128, SMT_ROWMAX = 8, SMT_HASH = 1024;
constexpr int SMOOTH_MAX_BINS = 4096;       // per axis
struct SmtCand { double x, y, z, area; };   // a candidate as the tile kernel stages it

// ---- the bins: a margin wider than 2 sigma_x x 2 sigma_y over the centroids' bounding box, never finer than SMOOTH_MAX_BINS per
// axis.  Every form searches the 3 x 3 bins around a row, so two coordinates a, b that the smoother takes for neighbours must fall at
// most one bin apart.  Neighbours have fl((b - a) / sigma) < 2, hence b - a < 2 sigma exactly (2 sigma is a double and rounding is
// monotone).  A bin is t(c) = fl(fl(c - x0) / bw), truncated: both roundings are relative to their result, and the result is at most
// the number of bins, so |t(c) - (c - x0) / bw| <= 2.01 * 2^-53 * SMOOTH_MAX_BINS = 9.2e-13, however far the grid lies from the plane's
// origin.  With bw = 2 sigma (1 + m):  t(b) - t(a) < 1 / (1 + m) + 1.9e-12, which is below 1 -- truncation then separates the two by
// at most one bin -- once m > 1.9e-12.  With bins of exactly two sigmas (m = 0) it is not: a pair 2 sigma (1 - 4e-16) apart, astride
// a bin edge, was seen two bins apart and dropped.  m = 1e-9 leaves a factor of 500 and costs nothing; the width of the capped
// branch takes the same margin, so bins only grow on every branch (and the far corner, at SMOOTH_MAX_BINS / (1 + m), stays inside).
constexpr double SMOOTH_BIN_MARGIN = 1e-9;
struct SmoothGrid {
    double x0 = 0, y0 = 0, bw = 1, bh = 1;
    int nbx = 1, nby = 1;
    size_t nbins() const { return (size_t)nbx * nby; }
};
inline double smooth_bin_width(double extent, double sigma) {
    return std::max(2.0 * sigma, extent / (double)SMOOTH_MAX_BINS) * (1.0 + SMOOTH_BIN_MARGIN);
}
inline SmoothGrid smooth_grid(const double cmin[2], const double cmax[2], const double sigma[3]) {
    SmoothGrid g;
    g.x0 = cmin[0]; g.y0 = cmin[1];
    g.bw = smooth_bin_width(cmax[0] - cmin[0], sigma[0]); g.bh = smooth_bin_width(cmax[1] - cmin[1], sigma[1]);
    g.nbx = (int)std::min((double)SMOOTH_MAX_BINS, std::floor((cmax[0] - cmin[0]) / g.bw) + 1.0);
    g.nby = (int)std::min((double)SMOOTH_MAX_BINS, std::floor((cmax[1] - cmin[1]) / g.bh) + 1.0);
    return g;
}

// ---- the forms, as ibh_weighted_smoothed_by reports them -----------------------------------------------------------------------
enum SmoothForm { SMOOTH_NONE = 0, SMOOTH_TRIPLET = 1, SMOOTH_DIRECT = 2, SMOOTH_TILE = 3 };
struct SmoothPlan {
    SmoothGrid grid;
    // the forms in the order they are tried; a form whose tables overflow (its flag, read back with its first counters) leaves the
    // build to the next one.  The tile form: more than SMT_KMAX columns around a bin or a member row of M longer than SMT_ROWMAX;
    // the direct form: a row with more than SMD_MAXCOL columns.  The triplet pipeline has no limit and is always last.
    SmoothForm form[3] = {SMOOTH_TRIPLET, SMOOTH_NONE, SMOOTH_NONE};
    int nform = 0;
    bool tries(SmoothForm f) const { return std::find(form, form + nform, f) != form + nform; }
};
// (measured: the direct form is 2 x faster than the triplet pipeline at 20 km -- 0.50 against 1.08 ms, that one is launch-bound
// there -- but slower at 5 km, 13 against 12 ms: three passes of ~3600 candidate evaluations per row, each five gathers; the direct
// form is therefore taken for small problems only, the tiles beyond them.  `smooth_direct`, `smooth_tile`: 1 always, 0 never,
// -1 by size.)
inline SmoothPlan plan_smooth(int nrow, const double cmin[2], const double cmax[2], const double sigma[3]) {
    SmoothPlan p;
    p.grid = smooth_grid(cmin, cmax, sigma);
    const int direct = get_tuning("smooth_direct", -1);
    const bool take_direct = direct > 0 || (direct < 0 && nrow <= get_tuning("smooth_direct_max_rows", 16384));
    const int tile = get_tuning("smooth_tile", -1);
    if (tile > 0 || (tile < 0 && !take_direct)) p.form[p.nform++] = SMOOTH_TILE;
    if (take_direct) p.form[p.nform++] = SMOOTH_DIRECT;
    p.form[p.nform++] = SMOOTH_TRIPLET;
    return p;
}

// ---- the dynamic LDS of k_smt_tile: byte offsets for a column stride of kstride (the widest column table of the build) ---------
struct SmtLds {
    size_t acc, s_c, s_val, s_cols, s_slot, s_ne, total;
};
constexpr size_t SMT_LDS_RAISED = 160 * 1024;       // the kernel's dynamic-LDS limit once a build needs more than the default 64 KB
constexpr SmtLds smt_lds(int kstride) {
    SmtLds l{};
    l.acc = 0;                                              // double [kstride][64]
    l.s_c = l.acc + (size_t)kstride * 64 * sizeof(double);  // SmtCand [64]
    l.s_val = l.s_c + 64 * sizeof(SmtCand);                 // double [64][SMT_ROWMAX]
    l.s_cols = l.s_val + 64 * SMT_ROWMAX * sizeof(double);  // int [SMT_KMAX]
    l.s_slot = l.s_cols + SMT_KMAX * sizeof(int);           // unsigned char [64][SMT_ROWMAX]
    l.s_ne = l.s_slot + 64 * SMT_ROWMAX;                    // unsigned char [64]
    l.total = l.s_ne + 64;
    return l;
}

// ---- the tile form shared by the ranks of a communicator ---------------------------------------------------------------------------
// A rank's share: bins [b0, b1), their member positions [m0, m1) and waves [w0, w1) (a wave serves 64 members of one bin); and the
// candidates [c0, c1) it packs -- the members of every bin a 3 x 3 neighbourhood of its bins can reach.
struct SmtShare {
    int b0 = 0, b1 = 0, m0 = 0, m1 = 0, w0 = 0, w1 = 0, c0 = 0, c1 = 0;
};
// one rank: everything (nothing of the histogram is needed on the host)
inline SmtShare smt_whole(int nbins, int nmem, int nwaves) { return SmtShare{0, nbins, 0, nmem, 0, nwaves, 0, nmem}; }
// bs[r] = the first bin of rank r, bs[world] = nbins: contiguous bin ranges balanced by work -- a bin costs its members times the
// candidates of its 3 x 3 neighbourhood.  binstart: the exclusive scan of the bins' member counts, [nbx * nby + 1].
inline std::vector<int> smt_split(const std::vector<uint32_t> &binstart, int nbx, int nby, int world) {
    const int nb = nbx * nby;
    std::vector<double> cw((size_t)nb + 1, 0.0);
    for (int b = 0; b < nb; ++b) {
        const int bx = b % nbx, by = b / nbx;
        const int x0 = std::max(bx - 1, 0), x1 = std::min(bx + 1, nbx - 1);
        double ncand = 0;
        for (int yy = std::max(by - 1, 0); yy <= std::min(by + 1, nby - 1); ++yy)
            ncand += (double)(binstart[(size_t)yy * nbx + x1 + 1] - binstart[(size_t)yy * nbx + x0]);
        cw[(size_t)b + 1] = cw[(size_t)b] + (double)(binstart[(size_t)b + 1] - binstart[(size_t)b]) * ncand;
    }
    std::vector<int> bs((size_t)world + 1, nb);
    bs[0] = 0;
    for (int r = 1; r < world; ++r)
        bs[(size_t)r] = std::max(bs[(size_t)r - 1], (int)(std::lower_bound(cw.begin(), cw.end(), cw[(size_t)nb] * r / world) - cw.begin()));
    return bs;
}
inline SmtShare smt_share(const std::vector<uint32_t> &binstart, const std::vector<int> &bs, int rank, int nbx) {
    const int nb = (int)binstart.size() - 1;
    SmtShare s;
    s.b0 = bs[(size_t)rank]; s.b1 = bs[(size_t)rank + 1];
    s.m0 = (int)binstart[(size_t)s.b0]; s.m1 = (int)binstart[(size_t)s.b1];
    uint32_t waves = 0;         // the exclusive scan of ceil(members / 64) the device holds in wstart
    for (int b = 0; b < s.b1; ++b) {
        if (b == s.b0) s.w0 = (int)waves;
        waves += (binstart[(size_t)b + 1] - binstart[(size_t)b] + 63) / 64;
    }
    if (s.b0 == s.b1) s.w0 = (int)waves;
    s.w1 = (int)waves;
    s.c0 = (int)binstart[(size_t)std::max(s.b0 - nbx - 1, 0)]; s.c1 = (int)binstart[(size_t)std::min(s.b1 + nbx + 1, nb)];
    return s;
}
// the member position at which each rank's rows start, and their end: [world + 1]
inline std::vector<uint32_t> smt_member_starts(const std::vector<uint32_t> &binstart, const std::vector<int> &bs) {
    std::vector<uint32_t> ms(bs.size());
    for (size_t r = 0; r < bs.size(); ++r) ms[r] = binstart[(size_t)bs[r]];
    return ms;
}
// the byte offsets a gatherv takes: rank r owns [off[r], off[r + 1]) of an array of elem_bytes-sized elements, the element counts
// `at` being the ranks' member starts (the row lengths) or the row offsets found at them (the packed rows)
inline std::vector<int64_t> smt_gather_offsets(const std::vector<uint32_t> &at, int elem_bytes) {
    std::vector<int64_t> off(at.size());
    for (size_t r = 0; r < at.size(); ++r) off[r] = (int64_t)elem_bytes * (int64_t)at[r];
    return off;
}
}  // namespace ibh
