// apply_plan.h -- which kernel an apply launches, decided once, as a plain value (spmm.hip walks it: launch_plan).  Host arithmetic
// over a few integers of the handle and the tuning map: no HIP (tests/cpp/test_apply_plan.cpp).  The numbers beside a rule are why it exists.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#ifndef IBH_MAX_BATCH
#define IBH_MAX_BATCH 32
#endif

namespace ibh {
int get_tuning(const char *key, int dflt);
// the apply kernel families (spmm.hip), as ibh_weighted_set_kernel / ibh_weighted_last_kernel name them (capi.hip)
enum ApplyKernel { KERNEL_AUTO = 0, KERNEL_ROWBLOCK = 1, KERNEL_SHORTROW, KERNEL_ROWDUAL, KERNEL_COLSWEEP, KERNEL_ROWGROUP };
inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }
constexpr int IBH_GSLOTS = 32;      // most rows (elevation classes of one GCM cell) in a row group (spmm.hip rowgroup)
// tiles of a row group (spmm.hip grouptile): seg = items (distinct columns) of a tile, 256 or 128 by the matrix (RowGroups::Tiles::seg)
constexpr int ibh_gt_ecap(int seg) { return 2 * seg + 4 * IBH_GSLOTS; }   // entries of a tile: <= 2 per item, every slot's list padded to a multiple of 4
constexpr size_t grouptile_lds(int f, int seg) { return (size_t)f * (seg + 2) * 8 + ibh_gt_ecap(seg) * 10 + 256; }     // (+ slack: a batch reads a few steps past its run)
constexpr int SWEEP_CB = 64, SWEEP_NW = 4, SWEEP_TS = SWEEP_CB + 1;      // sweep_kernel.inl: columns per block, waves per workgroup, padded tile row
inline size_t sweep_lds_bytes(int nslot) { return ((size_t)64 * SWEEP_TS + (size_t)SWEEP_NW * nslot * 64 + 2 * SWEEP_CB) * 8; }
constexpr int SR_THREADS = 256, SR_STEP = SR_THREADS - 8;      // shortrow: rows of a workgroup; re-aligning ones advance by SR_STEP
// fields per lane group of the sweep, as a power of two: 64 (one batch per wave row) from 33 fields; below, the next power of
// two >= 8 so that 64 >> lg batches share the lanes
inline int sweep_lg(int nvar) { return nvar > 32 ? 6 : nvar > 16 ? 5 : nvar > 8 ? 4 : 3; }
// lanes of the sweep that carry a (batch, field) pair for nvar fields in launches of nbatch
inline int sweep_lanes(int nvar, int nbatch) { return nvar > 32 ? 64 : nvar * std::min(nbatch, 64 >> sweep_lg(nvar)); }
// partial sums of an apply.  Bands: [2: lower, upper][nbatch][nvar][ld]; sweep: [slices of 64 lanes, a lane = (batch, field)][nprow][ld]
inline long band_part_ld(int nrow) { return ((long)nrow + 63) & ~63l; }
inline size_t band_part_count(int nrow, int nvar, int nbatch) { return 2 * (size_t)nbatch * (size_t)((long)nvar * band_part_ld(nrow)); }
inline long sweep_part_ld(int nvar) { return sweep_lg(nvar) == 6 ? (long)ceil_div(nvar, 64) * 64 : 64; }
inline size_t sweep_part_count(int nprow, int nvar, int nbatch) {
    const int lg = sweep_lg(nvar);
    return (size_t)(lg == 6 ? nbatch : ceil_div(nbatch, 64 >> lg)) * (size_t)((long)nprow * sweep_part_ld(nvar));
}

// What the choice reads from a handle (ibh::facts_of, common.h).
struct MatrixFacts {
    int nrow = 0, ncol = 0;
    int64_t nnz = 0, bands_n = 0, napply = 0;
    ApplyKernel kernel_override = KERNEL_AUTO;
    bool band_eligible = false, conservative = true, bands_built = false, bands_tried = false, sweep_built = false, sweep_tried = false,
         groups_built = false, groups_tried = false, tiles_built = false;
    int groups_n = 0, groups_nslot = 0, tiles_seg = 0, sweep_ntask = 0, sweep_nprow = 0, sweep_nslot = 0, sweep_ident = 0;
};

// ---- the instantiations: one list per kernel, in the order the code object holds them ----------------------------------------------
struct Inst { int a[5]; const char *sig; };      // template arguments (true = 1) and the name as ibh_weighted_last_launch spells it
enum InstTable { T_GROUPTILE, T_SWEEP, T_ROWGROUP, T_ROWDUAL, T_ROWONE, T_ROWBLOCK, T_SHORTROW, T_COUNT };
// (rows per group, tile size) -> grouptile<F, NS, SEG, NW, PAIR>; 16 fields per workgroup (32 lost everywhere it was measured: 1 km 269
// against 218 us, the Antarctic sheet 3.67 against 3.62 ms, 5 km 22 against 18 us)
#define IBH_GT2(X, NS, SEG, NW) X(16, NS, SEG, NW, true) X(16, NS, SEG, NW, false)
#define IBH_GROUPTILE_INSTS(X) IBH_GT2(X, 16, 128, 4) IBH_GT2(X, 32, 128, 4) IBH_GT2(X, 16, 256, 8) IBH_GT2(X, 32, 256, 8)
#define IBH_SWEEP_INSTS(X) X(true, true) X(true, false) X(false, true) X(false, false)      // <FULL, IDENT, 0>
#define IBH_RG2(X, NW, U, TW) X(NW, U, TW, false) X(NW, U, TW, true)                          // <NW, U, TW, PAIR>
#define IBH_ROWGROUP_INSTS(X) IBH_RG2(X, 8, 8, 32) IBH_RG2(X, 8, 16, 32) IBH_RG2(X, 4, 4, 32) IBH_RG2(X, 4, 8, 32) \
    IBH_RG2(X, 8, 8, 64) IBH_RG2(X, 8, 16, 64) IBH_RG2(X, 4, 4, 64) IBH_RG2(X, 4, 8, 64) IBH_RG2(X, 4, 16, 64)
// rowblock<FPW, WK, UNROLL, NW, DUAL>.  (4 waves: a lane stages twice the entries of a segment, and 12..16 gathers no longer fit 64
// registers: they spill; so 12, 14, 16 exist with one field per wave of 8 only)
#define IBH_RB4(X, F, K, N, D) X(F, K, 1, N, D) X(F, K, 2, N, D) X(F, K, 8, N, D) X(F, K, 4, N, D)
#define IBH_ROWDUAL_INSTS(X) IBH_RB4(X, 4, 1, 4, true) IBH_RB4(X, 2, 1, 4, true) IBH_RB4(X, 1, 1, 4, true)
#define IBH_ROWONE_INSTS(X) X(4, 8) X(4, 12) X(4, 14) X(8, 8) X(8, 12) X(8, 14) X(8, 16)      // <NW, U>
#define IBH_ROWBLOCK_INSTS(X) X(1, 1, 1, 8, false) X(1, 1, 2, 8, false) X(1, 1, 8, 8, false) X(1, 1, 12, 8, false) X(1, 1, 14, 8, false) \
    X(1, 1, 16, 8, false) X(1, 1, 4, 8, false) IBH_RB4(X, 2, 1, 8, false) IBH_RB4(X, 4, 1, 8, false) IBH_RB4(X, 4, 1, 4, false) \
    IBH_RB4(X, 8, 1, 4, false) IBH_RB4(X, 2, 1, 4, false) IBH_RB4(X, 1, 1, 4, false) IBH_RB4(X, 4, 2, 4, false) IBH_RB4(X, 2, 2, 4, false) \
    IBH_RB4(X, 1, 2, 4, false) IBH_RB4(X, 2, 4, 4, false) IBH_RB4(X, 4, 4, 4, false) IBH_RB4(X, 1, 4, 4, false)
#define IBH_SR4(X, NT, G) X(NT, G, true, true) X(NT, G, true, false) X(NT, G, false, true) X(NT, G, false, false)    // <NT, G, REALIGN, XT>
#define IBH_SHORTROW_INSTS(X) IBH_SR4(X, true, 16) IBH_SR4(X, false, 16) IBH_SR4(X, true, 8) IBH_SR4(X, false, 8) IBH_SR4(X, true, 4) IBH_SR4(X, false, 4)
#define IBH_I_GT(a, b, c, d, e) {{a, b, c, d, e}, "spmm_grouptile_kernel<" #a ", " #b ", " #c ", " #d ", " #e ">"},
#define IBH_I_RB(a, b, c, d, e) {{a, b, c, d, e}, "spmm_rowblock_kernel<" #a ", " #b ", " #c ", " #d ", " #e ">"},
#define IBH_I_SW(a, b) {{a, b, 0, 0, 0}, "spmm_sweep_kernel<" #a ", " #b ", 0>"},
#define IBH_I_RG(a, b, c, d) {{a, b, c, d, 0}, "spmm_rowgroup_kernel<" #a ", " #b ", " #c ", " #d ">"},
#define IBH_I_R1(a, b) {{a, b, 0, 0, 0}, "spmm_rowone_kernel<" #a ", " #b ">"},
#define IBH_I_SR(a, b, c, d) {{a, b, c, d, 0}, "spmm_shortrow_kernel<" #a ", " #b ", " #c ", " #d ">"},
static const Inst INSTS_GROUPTILE[] = {IBH_GROUPTILE_INSTS(IBH_I_GT)}, INSTS_SWEEP[] = {IBH_SWEEP_INSTS(IBH_I_SW)},
                  INSTS_ROWGROUP[] = {IBH_ROWGROUP_INSTS(IBH_I_RG)}, INSTS_ROWDUAL[] = {IBH_ROWDUAL_INSTS(IBH_I_RB)},
                  INSTS_ROWONE[] = {IBH_ROWONE_INSTS(IBH_I_R1)}, INSTS_ROWBLOCK[] = {IBH_ROWBLOCK_INSTS(IBH_I_RB)},
                  INSTS_SHORTROW[] = {IBH_SHORTROW_INSTS(IBH_I_SR)};
#define IBH_LIST(T) {T, (int)(sizeof(T) / sizeof(T[0]))}
static const struct InstList { const Inst *v; int n; } INSTS[T_COUNT] = {IBH_LIST(INSTS_GROUPTILE), IBH_LIST(INSTS_SWEEP), IBH_LIST(INSTS_ROWGROUP), IBH_LIST(INSTS_ROWDUAL),
                                        IBH_LIST(INSTS_ROWONE), IBH_LIST(INSTS_ROWBLOCK), IBH_LIST(INSTS_SHORTROW)};
inline int find_inst(int table, int a, int b, int c = 0, int d = 0, int e = 0) {      // -1: no such instantiation
    const int want[5] = {a, b, c, d, e};
    for (int i = 0; i < INSTS[table].n; ++i)
        if (std::equal(want, want + 5, INSTS[table].v[i].a)) return i;
    return -1;
}

// ---- the rules, each threshold once -------------------------------------------------------------------------------------------
inline double mean_len(const MatrixFacts &f) { return f.nrow ? (double)f.nnz / (double)f.nrow : 0.0; }
// (round 4, the Antarctic sheet -- 17.6 / 35.2 M entries -- one apply per launch: AvI, 128 fields, sweep 3 131 against 3 654 us;
// EvI, 16 fields, row groups 641 against 812 (bands) / 747 (rows) / 1 994 us (sweep): scratch/kernel_choice.py)
inline bool huge(const MatrixFacts &f) { return f.nnz >= (1l << 24); }
inline bool sweep_enabled(int nvar, int nbatch) { return sweep_lanes(nvar, nbatch) >= get_tuning("sweep_min_nvar", 32) && get_tuning("sweep_auto", 1); }
// The long-row matrices that are no E-row matrices (AvI, AvX) take the sweep in batched launches only (1 km, 64 fields: 167
// against 173 us per apply 32 deep, but 193 against 183 us one launch per apply) -- or one launch of >= 128 fields of a huge one.
inline bool sweep_batched(const MatrixFacts &f, int nvar, int nbatch) { return nbatch >= get_tuning("sweep_min_batch", 4) || (huge(f) && nvar >= 128); }
inline bool sweep_ok(const MatrixFacts &f, int nvar, int nbatch) {
    return f.sweep_built && sweep_enabled(nvar, nbatch) && (f.band_eligible || sweep_batched(f, nvar, nbatch));
}
inline bool groups_enabled(int nvar) { return nvar >= 4 && get_tuning("rowgroup_auto", 1); }
inline bool rowdual_enabled(int nvar) { return nvar >= 4 && get_tuning("rowdual_auto", 1); }
inline bool sweep_work(const MatrixFacts &f, int lanes) { return (double)f.nnz * lanes >= (double)get_tuning("sweep_min_work", 64 << 20); }
inline bool sweep_sized(const MatrixFacts &f, int nvar, int nbatch) { return sweep_work(f, std::max(sweep_lanes(nvar, nbatch), std::min(nvar, 64))); }
// (round 5: on matrices of 2^24 entries and more the tiled row groups beat the sweep in batched launches of few fields too --
// the Antarctic EvI, 16 fields, batches of 4: bench.py 0.487 of peak through the sweep, measured again below)
inline bool tiles_win(const MatrixFacts &f) { return f.tiles_built && huge(f) && get_tuning("rowgroup_form", -1) != 0; }
// Which form of the row groups: the tiles (grouptile) for bandwidth-sized matrices -- measured, one apply per launch, tiles
// against LDS atomics: the Antarctic sheet (35 M entries) 16 fields 503 against 672 us, 128 fields 3.62 against 4.34 ms; 1 km
// Greenland (4 M entries) 64 fields 218 against 220 us, 16 fields 82 against 74; 5 km (166 k entries: latency-bound, three
// tiles in sequence per GCM cell) 12.4 against 7.6 and 18.1 against 17.4 us.  ibh_set_tuning("rowgroup_form", 0 / 1) forces one.
inline bool use_grouptile(const MatrixFacts &f, int nvar) {
    if (!f.tiles_built) return false;
    const int form = get_tuning("rowgroup_form", -1);
    if (form >= 0) return form == 1;
    return huge(f) || (f.nnz >= (1l << 21) && nvar >= 48);
}

// ---- lazily built apply structures (column sweep, bands, row groups) ---------------------------------------------------
// Which structure applies of (nvar fields, nbatch per launch) would use, by the rules of plan_family; `seen` = the matrix has
// been applied before (an apply builds on the SECOND call only: the coupler's one build : one apply must not pay for a
// structure it never reuses; ibh_weighted_prepare builds at once).
inline bool wants_sweep(const MatrixFacts &f, int nvar, int nbatch, bool seen) {
    if (f.sweep_tried || f.sweep_built) return false;
    if (f.kernel_override == KERNEL_COLSWEEP) return true;
    const bool long_rows = f.nrow > 0 && mean_len(f) >= 64.0 && f.nnz <= 2 * (int64_t)f.ncol;      // AvI, AvX
    const bool e_rows = f.band_eligible && (nvar < 32 || (f.groups_tried && !f.groups_built) || !get_tuning("rowgroup_auto", 1));
    return (e_rows || (long_rows && sweep_batched(f, nvar, nbatch))) && f.kernel_override == KERNEL_AUTO && seen && sweep_enabled(nvar, nbatch) &&
           sweep_work(f, sweep_lanes(nvar, nbatch));
}
// An E-row matrix that is applied again gets its band structure (every ice cell carries the weights of BOTH classes it lies
// between and is read once instead of twice), for bandwidth-sized work only (measured, 64 fields: 1 km EvI 292 -> 255 us; at 5 km
// the extra combine pass costs more than the halved traffic saves, 18.5 -> 21.9).
inline bool wants_bands(const MatrixFacts &f, int nvar, bool seen) {
    return f.band_eligible && !f.bands_tried && !f.bands_built && !f.sweep_built && seen && f.kernel_override == KERNEL_AUTO && rowdual_enabled(nvar) &&
           (double)f.nnz * nvar >= (double)get_tuning("rowdual_min_work", 128 << 20);
}
// Row groups of an E-row matrix: bandwidth-sized matrices applied to >= 32 fields get them like the sweep always got its
// structure -- on the SECOND apply, or at once in ibh_weighted_prepare; with fewer fields such a matrix takes the sweep (batches
// share its lanes; a single launch of a 2^24-entry matrix takes the groups from 4 fields on).  Small matrices (5 km: the sweep is
// latency-bound there) get them from ibh_weighted_prepare only: the structure costs about as much as the matrix build itself, and
// an apply that switched kernels on its own would change the rounding of later results against earlier ones
// (ibh_set_tuning("rowgroup_after", n) asks for exactly that, from the n-th apply on).
inline bool wants_groups(const MatrixFacts &f, int nvar, int nbatch, long seen, bool asked) {
    if (!f.band_eligible || f.groups_tried || f.groups_built) return false;
    if (asked || f.kernel_override == KERNEL_ROWGROUP) return true;
    if (f.kernel_override != KERNEL_AUTO || !groups_enabled(nvar)) return false;
    if (sweep_sized(f, nvar, nbatch)) return (nvar >= 32 || (nbatch < 4 && huge(f))) && seen >= 1;
    return seen >= get_tuning("rowgroup_after", 1 << 30);
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------
struct ApplyPlan {
    ApplyKernel family = KERNEL_AUTO;
    int table = 0, inst = -1;                   // the instantiation: INSTS[table].v[inst]
    int unroll = 0, qi = 1, xcd_mode = 0, nfc = 1, lpt = 0, per_launch = 0;      // (per_launch: batches per launch)
    unsigned grid[3] = {1, 1, 1};
    long nblocks = 0;                           // grid[0] before it was narrowed: the launcher checks it fits
    int fper = 0, g = 0, use_xt = 0, ldt = 0, realign = 0, nt = 0;     // shortrow (realign: by the result planes' alignment, align_shortrow)
    size_t lds = 0, band_part = 0, sweep_part = 0, xt = 0;      // dynamic LDS bytes; elements of scratch the launches need
};

// which family serves (f, nvar, nbatch); lda: the input's leading dimension (0: ncol)
inline ApplyKernel plan_family(const MatrixFacts &f, int nvar, int nbatch, int64_t lda) {
    ApplyKernel kernel = f.kernel_override;
    if (kernel == KERNEL_COLSWEEP && !f.sweep_built) kernel = KERNEL_AUTO;      // no column-sweep structure: the automatic choice
    if (kernel == KERNEL_AUTO) {
        // rowblock = one workgroup per (row, field chunk): for FEW LONG rows.  Many rows of 6..63 entries (a smoothed IvE:
        // 76 k rows of ~16) are thread-per-row work (measured, 5 km smoothed IvE, 16 fields: 220 us as rowblock)
        const bool few_rows = f.nrow <= get_tuning("rowblock_max_short_rows", 16384);
        kernel = (mean_len(f) >= 64.0 || (few_rows && mean_len(f) >= (double)get_tuning("rowblock_min_mean_nnz", 6))) ? KERNEL_ROWBLOCK : KERNEL_SHORTROW;
    }
    // E-row matrices (EvI, EvX), once the structure exists: the row groups (every X element gathered once per GCM cell; measured
    // against the sweep at 1 km, 64 fields: 221 against 247 us one launch per apply, 199 against 203-223 batched) -- except
    // batched launches of FEWER than 32 fields, where the batches share the lanes of the column sweep (1 km, 16 fields, 16 per
    // launch: 51 against 63 us per apply).
    if (kernel == KERNEL_ROWBLOCK && f.kernel_override == KERNEL_AUTO) {
        const bool sw = sweep_ok(f, nvar, nbatch);
        if (f.groups_built && groups_enabled(nvar) && (nvar >= 32 || !sw || tiles_win(f))) kernel = KERNEL_ROWGROUP;
        else if (sw) kernel = KERNEL_COLSWEEP;
    }
    if (kernel == KERNEL_ROWGROUP && !f.groups_built) kernel = KERNEL_ROWBLOCK;     // no row groups were built for this matrix
    if (kernel == KERNEL_ROWBLOCK && f.kernel_override == KERNEL_AUTO && f.bands_built && rowdual_enabled(nvar)) kernel = KERNEL_ROWDUAL;
    if (kernel == KERNEL_ROWDUAL && !f.bands_built) kernel = KERNEL_ROWBLOCK;       // no bands were built for this matrix
    // the column sweep addresses a wave's 16 field planes through one buffer descriptor (32-bit offsets)
    if (kernel == KERNEL_COLSWEEP && (uint64_t)16 * (uint64_t)std::max<int64_t>(lda, f.ncol) * 8 + (uint64_t)f.ncol * 8 >= (1ull << 32))
        kernel = f.bands_built ? KERNEL_ROWDUAL : KERNEL_ROWBLOCK;
    return kernel;
}

// one workgroup per (row, field chunk), the chunks of a row on one XCD: blocks of the grid
inline long rowblock_grid(int nrow, int nfc, int &xcd_mode) {
    const bool whole = nfc % 8 == 0 || nfc == 1 || nfc == 2 || nfc == 4;
    xcd_mode = get_tuning("rowblock_xcd_mode", whole ? 1 : 0);
    if (xcd_mode == 1 && !whole) xcd_mode = 0;
    if (xcd_mode != 1) return ((long)nrow * nfc + 7) & ~7l;
    if (nfc >= 8) return (long)nrow * nfc;      // nfc % 8 == 0
    const int m = 8 / nfc;                      // 8/nfc XCDs per chunk, each a row range of <= ceil(nrow/m) rows
    return 8l * ((nrow + m - 1) / m + 1);
}
// a shortrow plan's launch-time half: the result planes of nq batches are (mis)aligned
inline void align_shortrow(ApplyPlan &p, const MatrixFacts &f, int nvar, bool misaligned, int nq) {
    // planes of B that do not start on 64-byte lines are re-aligned through LDS (see the kernel); below 2^18 rows: latency-bound,
    // the two extra barriers cost more
    const int forced = get_tuning("shortrow_realign", -1);
    p.realign = forced >= 0 ? forced != 0 : misaligned && f.nrow >= (1 << 18);
    p.nblocks = (long)ceil_div(f.nrow, p.realign ? SR_STEP : SR_THREADS) * ceil_div(nvar, p.fper);
    p.grid[0] = (unsigned)p.nblocks; p.grid[1] = (unsigned)nq;
    p.inst = find_inst(T_SHORTROW, p.nt, p.g >= 16 ? 16 : p.g >= 8 ? 8 : 4, p.realign, p.use_xt != 0);
}
// a captured stream cannot grow the transposed-input scratch: as many batches per launch as fit the xt_granted bytes
inline void clamp_shortrow(ApplyPlan &p, const MatrixFacts &f, int nbatch, size_t xt_granted) {
    const size_t stride = (size_t)f.ncol * (size_t)p.ldt;
    if (p.per_launch > 1 && p.xt * sizeof(double) > xt_granted) p.per_launch = std::max(1, (int)(xt_granted / (stride * sizeof(double))));
    if (p.use_xt) p.xt = stride * (size_t)std::min(p.per_launch, nbatch);
}

// One launch of nbatch <= IBH_MAX_BATCH batches of nvar fields by `family` (pair: with a fused second matrix in the epilogue).
inline ApplyPlan plan_launch(const MatrixFacts &f, ApplyKernel family, int nvar, int nbatch, bool pair) {
    ApplyPlan p;
    p.family = family;
    p.per_launch = nbatch;
    const double mean = mean_len(f);
    const long pairs = (long)f.nrow * nvar;
    auto rows = [&](int nrows, int fb) {        // the (row, field chunk) grid of the row kernels
        p.nfc = ceil_div(nvar, fb);
        p.nblocks = rowblock_grid(nrows, p.nfc, p.xcd_mode);
        p.grid[0] = (unsigned)p.nblocks;
    };
    if (family == KERNEL_ROWGROUP && use_grouptile(f, nvar)) {
        p.table = T_GROUPTILE;
        const int seg = f.tiles_seg == 128 ? 128 : 256, ns = f.groups_nslot <= 16 ? 16 : 32;
        p.inst = find_inst(T_GROUPTILE, 16, ns, seg, seg == 128 ? 4 : 8, pair);
        rows(f.groups_n, 16);
        p.grid[1] = pair ? 1u : (unsigned)nbatch;
        p.lds = grouptile_lds(16, seg);
    } else if (family == KERNEL_ROWGROUP) {
        p.table = T_ROWGROUP;
        // 8 waves (fields) share a staged segment from 32 fields (5 km, 64 fields: 17.1 against 19.3 us with 4)
        const int u = get_tuning("rowgroup_unroll", 8), nw = get_tuning("rowgroup_waves", nvar >= 32 ? 8 : 4) == 8 ? 8 : 4;
        // class tables of half width (two lanes per entry) for the small matrices: all workgroups of a 5 km launch fit the LDS at
        // once -- 16 applies per launch 13.5 -> 12.3 us (64 fields), 3.96 -> 3.37 (16 fields), one launch unchanged (17.6 / 17.8);
        // at 1 km the doubled atomic instructions cost 223 -> 238 us.  By the matrix alone, so one apply and a batch agree bitwise.
        const int tw = get_tuning("rowgroup_tw", f.nnz < (1 << 20) ? 32 : 64) == 32 ? 32 : 64;
        p.unroll = nw == 8 ? (u <= 8 ? 8 : 16) : u <= 4 ? 4 : (u <= 8 || tw == 32) ? 8 : 16;
        p.inst = find_inst(T_ROWGROUP, nw, p.unroll, tw, pair);
        rows(f.groups_n, nw);
        p.grid[1] = pair ? 1u : (unsigned)nbatch;
        p.lds = (size_t)(3 * p.unroll * 64 + nw * f.groups_nslot * tw) * sizeof(double);
    } else if (family == KERNEL_COLSWEEP) {
        p.table = T_SWEEP;
        const int lg = sweep_lg(nvar), G = 64 >> lg;
        const bool full = lg == 6 ? nvar % 64 == 0 : (nvar == (1 << lg) && nbatch % G == 0);
        p.inst = find_inst(T_SWEEP, full, f.sweep_ident != 0);
        p.grid[0] = (unsigned)f.sweep_ntask; p.grid[1] = lg == 6 ? (unsigned)ceil_div(nvar, 64) : 1u; p.grid[2] = lg == 6 ? (unsigned)nbatch : (unsigned)ceil_div(nbatch, G);
        p.lds = sweep_lds_bytes(f.sweep_nslot);
        p.sweep_part = sweep_part_count(f.sweep_nprow, nvar, nbatch);
    } else if (family == KERNEL_ROWDUAL) {
        p.table = T_ROWDUAL;
        const int t = get_tuning("rowdual_fpw", pairs >= 4 * 8192 ? 4 : pairs >= 2 * 8192 ? 2 : 1), fpw = t >= 4 ? 4 : t == 2 ? 2 : 1;
        p.unroll = get_tuning("rowdual_unroll", 0);
        if (p.unroll <= 0) {
            const double m = f.nrow ? (double)f.bands_n / (double)f.nrow / 64.0 : 1.0;
            p.unroll = m > 4.0 ? 8 : m > 2.0 ? 4 : m > 1.0 ? 2 : 1;
        }
        if (p.unroll != 1 && p.unroll != 2 && p.unroll != 8) p.unroll = 4;
        p.inst = find_inst(T_ROWDUAL, fpw, 1, p.unroll, 4, true);
        rows(f.nrow, fpw * 4);
        p.grid[1] = (unsigned)nbatch;
        p.band_part = band_part_count(f.nrow, nvar, nbatch);
    } else if (family == KERNEL_ROWBLOCK) {
        int fpw = get_tuning(nbatch > 1 ? "rowblock_many_fpw" : "rowblock_fpw", 0), wk = get_tuning("rowblock_wk", 0);
        if (fpw == 0 || wk == 0) {
            // enough workgroups to give every CU ~8: small problems are latency-bound and want many
            // small tasks, big ones amortise the staged row segment over more fields
            if (nvar >= 16 && pairs >= 4 * 8192) { fpw = 4; wk = 1; }
            else if (nvar >= 8 && pairs >= 2 * 8192) { fpw = 2; wk = 1; }
            else if (nvar >= 4) { fpw = 1; wk = 1; }
            else if (nvar >= 2) { fpw = 1; wk = 2; }
            else { fpw = 1; wk = 4; }
        }
        // one apply per launch, >= 32 fields, rows of a few hundred entries: the lean kernel (same bits as rowblock with wk == 1)
        if (nbatch == 1 && wk == 1 && get_tuning("rowone", nvar >= 32 && mean >= 192.0 && mean <= 1024.0 ? 1 : 0)) {
            p.table = T_ROWONE;
            // (4 waves: a lane stages twice the entries, and 16 gathers no longer fit 64 registers: they spill; 14)
            const int u = get_tuning("rowone_unroll", mean > 768.0 ? 16 : 14), nw = get_tuning("rowone_waves", 8) == 4 ? 4 : 8;
            p.unroll = u <= 8 ? 8 : u <= 12 ? 12 : (u <= 14 || nw == 4) ? 14 : 16;
            p.inst = find_inst(T_ROWONE, nw, p.unroll);
            rows(f.nrow, nw);
            return p;
        }
        p.table = T_ROWBLOCK;
        // deep batched launches: 8 waves (8 fields) per workgroup halve the workgroup count per batch
        // (measured at the 5 km headline shape, depth 16: 7.36 against 7.51 us per apply)
        int nw = get_tuning("rowblock_waves", nbatch >= 8 && fpw == 1 && wk == 1 ? 8 : 4);
        if (nw == 8 && wk == 1) fpw = fpw == 1 || fpw == 2 ? fpw : 4;
        else {
            nw = 4;
            if (find_inst(T_ROWBLOCK, fpw, wk, 1, 4, false) < 0) { fpw = 1; wk = 4; }
        }
        // loads in flight per lane and field: enough 64-entry slots to cover a typical row in one batch
        p.unroll = get_tuning("rowblock_unroll", 0);
        if (p.unroll == 0) {
            const double m = f.nrow ? mean / (64.0 * wk) : 1.0;
            // (a row is one partly filled batch when the unroll overshoots it: 5 km EvI, 2.1 passes of 64 per row, 26.2 / 18.4 us
            // with four loads in flight, 23.6 / 16.6 with two)
            p.unroll = m > 6.0 ? 8 : m > 3.0 ? 4 : m > 1.5 ? 2 : 1;
            // one field per wave: the weights are read when the gathers land, a slot in flight holds two registers -> a row of up to
            // 896 entries in ONE batch of 14 gathers per lane (measured, 5 km AvI, 32 applies per launch: 7.31 -> 7.03 us per apply;
            // 12 or 16 are slower: 8.5 / 7.4)
            if (fpw == 1 && wk == 1 && nw == 8 && m > 8.0 && m <= 14.0) p.unroll = 14;
        }
        // one batch covers a whole row of <= 768 / 896 / 1024 entries: 12, 14, 16 (one field per wave of 8; of 4: 8)
        if (p.unroll > 8 && fpw == 1 && wk == 1) p.unroll = nw == 8 ? (p.unroll <= 12 ? 12 : p.unroll <= 14 ? 14 : 16) : 8;
        else if (p.unroll != 1 && p.unroll != 2 && p.unroll != 8) p.unroll = 4;
        p.inst = find_inst(T_ROWBLOCK, fpw, wk, p.unroll, nw, false);
        // batches per workgroup: the staged row segment and the prologue are shared by qi batches
        if (nbatch > 1) {
            p.qi = get_tuning("rowblock_many_qi", 0);
            if (p.qi <= 0) p.qi = nbatch >= 4 ? 2 : 1;       // measured at the 5 km headline shape: depth 16 7.5 (qi 2) / 8.2 (qi 1) / 8.0 us (qi 8)
            p.qi = std::min(p.qi, nbatch);
        }
        rows(f.nrow, fpw * (nw / wk));
        p.grid[1] = (unsigned)ceil_div(nbatch, p.qi);
        p.lpt = nbatch > 1 && get_tuning("rowblock_lpt", 0);
    } else {                                                    // KERNEL_SHORTROW
        p.table = T_SHORTROW;
        // fields per thread.  At 1 km (1.9 M rows) the stores dominate and 16-32 fields per thread amortise the row's CSR reads.
        // Small problems (5 km: 76 k rows): round-2 sweep with the batched kernel (scratch/one_matrix.py, us per 64-field apply,
        // one launch / 16 per launch): one entry per row (IvA) 8 fields x transposed input 12.1 / 7.0 (4 fields, field-major:
        // 13.2 / 9.7); 2-3 entries (IvE) 16 fields 16.5 / 9.9, 32 fields 19.2 / 9.5 -- more fields per thread pay in deep launches.
        const bool one_entry = (double)f.nnz <= 1.5 * (double)f.nrow, big = f.nrow >= (1 << 19);
        // (2-3 entries, one launch of <= 32 fields: 4 fields per thread, field-major 8.2 us against 14.2 through the transposed copy)
        // (32 fields: 13.7 against 16.0; rows of 2-3 entries only: a smoothed IvE -- ~16 entries per row -- needs the lines of the
        // transposed copy: 59.6 against 143 us at 16 fields)
        const bool few_fields_once = nbatch < 4 && nvar <= 32 && (double)f.nnz <= 4.0 * (double)f.nrow;
        const int small_multi = nbatch >= 4 ? 32 : few_fields_once ? 4 : 16;
        // (round 3, kernel durations by dispatch events instead of wall time: ONE launch of a one-entry matrix at 5 km is fastest
        // field-major with 4 fields per thread -- 64 fields 13.2 us against 15.8 through the transposed copy, whose second
        // launch costs more than its lines save; 16 fields 5.6 against 6.8; deep launches keep the transposed form: 7.0)
        const int small_one = f.nrow >= 16384 ? (nbatch >= 4 ? 8 : nvar >= 64 ? 16 : 4) : 4;
        // (round 4, the Antarctic sheet -- 17.2 M one-entry rows, results of 2.2 / 17.6 GB: groups of 4 fields and, from ~100 fields on,
        // 32 fields per thread: 16 fields 579 -> 546 us, 128 fields 4 761 -> 3 829 us = 0.45 -> 0.56 of 8 TB/s; scratch/tune_shortrow.py)
        const bool huge_rows = f.nrow >= (1 << 23);
        p.fper = std::max(1, get_tuning("shortrow_fper", big ? (one_entry ? (huge_rows && nvar >= 96 ? 32 : 16) : 32) : (one_entry ? small_one : small_multi)));
        p.g = std::min(p.fper, get_tuning("shortrow_group", big ? (one_entry ? (huge_rows ? 4 : 8) : 4) : (p.fper >= 8 ? 8 : 4)));
        // transposed input: the G fields of an entry are 8*G contiguous bytes per lane (one line per entry instead of one per
        // field): 5 km IvE 26.9 -> 18.5 us, 1 km IvE 302 -> 183 us, 1 km IvA 207 -> 176 us, 5 km IvA 13.2 -> 12.1 us
        p.use_xt = get_tuning("shortrow_xt", -1);
        // (one-entry matrices: the extra launch costs more than it saves for tiny matrices -- EvA: 4.9 -> 8.9 us -- and for a
        // single launch of few fields -- 5 km IvA, 16 fields: 7.5 -> 9.3 us)
        if (p.use_xt < 0) p.use_xt = ((!one_entry && !(few_fields_once && !big)) || big || (f.nrow >= 16384 && nbatch >= 4)) ? 1 : 0;
        if (p.fper % p.g != 0 || (p.g & 1)) p.use_xt = 0;
        p.ldt = (nvar + 15) & ~15;
        p.nt = get_tuning("shortrow_nt", 1) != 0;
        // GB-sized results: deep launches cost the L2 locality of the row slices (measured at 1 km: 148 us per apply alone,
        // 181 us sixteen deep); they go out a few batches at a time
        p.per_launch = std::max(1, get_tuning("shortrow_many", big ? 1 : IBH_MAX_BATCH));
        if (p.use_xt) p.xt = (size_t)f.ncol * (size_t)p.ldt * (size_t)std::min(p.per_launch, nbatch);
        align_shortrow(p, f, nvar, false, std::min(p.per_launch, nbatch));
    }
    return p;
}

// The single place where a launch is decided: the family by the whole call's nbatch, its launch for <= IBH_MAX_BATCH of them.
inline ApplyPlan plan_apply(const MatrixFacts &f, int nvar, int nbatch, bool pair, int64_t lda = 0) {
    return plan_launch(f, pair ? KERNEL_ROWGROUP : plan_family(f, nvar, nbatch, lda), nvar, std::min(nbatch, IBH_MAX_BATCH), pair);
}
}  // namespace ibh
