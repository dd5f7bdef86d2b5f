// asm_plan.h -- how a sorted-grid build runs, decided once, as a plain value (fastasm.inl / streamasm.inl walk it: fast_build).  Host
// arithmetic over a few integers of the matrix spec, the regridder, the static plan, the two sets and the tuning map: no HIP
// (tests/cpp/test_asm_plan.cpp).  The numbers beside a rule are why it exists.
#pragma once
#include <algorithm>
#include <cstdint>

namespace ibh {
int get_tuning(const char *key, int dflt);
enum { LIST_AP = 0, LIST_I = 1, LIST_EP = 2 };
enum { KEY_A = 0, KEY_I = 1, KEY_E = 2, KEY_X = 3 };
enum { FAM_AEVI = 0, FAM_IVAE = 1, FAM_EVA = 2 };

constexpr int FA_NC = 64;           // elevation classes per range (nhc <= 64)
constexpr int FA_T = 256;           // threads per workgroup of the per-element kernels (the per-range kernels: fa_range_shape)
// the chained scans of k_fa_count carry {new P keys, entries, classes} of the ranges before in one 64-bit word: bits per field
constexpr int FA_CH_NP = 21, FA_CH_NE = 22, FA_CH_NC = 15;
constexpr int SA_T = 256, SA_CPT = 4, SA_TILE = SA_T * SA_CPT;      // the streamed passes: threads, cells per thread, cells per workgroup
// straddling entries of one (range, class) segment sorted in LDS by k_sa_rows: tables of 128 (many short ranges: four waves of a
// workgroup hold 12 KB, the CU stays full) or 512 (long ranges: few segments, occupancy does not matter); more -> fastasm.inl
constexpr int SA_OLDSEG_S = 128, SA_OLDSEG_L = 512;
constexpr long EMIT_BLOCKS = 8192;  // most workgroups of the streamed emit pass (stream_emit_grid)
inline long asm_cdiv(long a, long b) { return (a + b - 1) / b; }

// ---- what a decision reads ---------------------------------------------------------------------------------------------------------
struct SetFacts {
    int64_t n = 0;                  // members
    bool identity = false;
    int64_t extent = 0;             // the sparse extent of the set's key
    bool fresh() const { return n == 0; }
    bool identity_complete() const { return identity && n == extent; }
};
struct BuildFacts {                 // (facts_of_build, assemble.hip)
    int family = FAM_AEVI, row_key = KEY_A, col_key = KEY_I, row_list = LIST_AP, col_list = LIST_I;     // the MatSpec
    long nX = 0, nI = 0;            // the regridder: exchange cells, ice cells, elevation classes
    int nhc = 0;
    bool plan_ok = false;           // the fast path is wanted (fast_path_wanted) and the sheet has a static plan (ensure_plan)
    int nAr = 0, nmulti = 0, nmulti3 = 0, npair = 0, maxrange = 0;
    bool tiny = false, icnt_pos = false, icnt_nz = false;
    SetFacts set[2];                // rows, columns
    bool same_set = false;          // both sides are one set object
    bool smooth = false, bands_wanted = false;
    bool shared = false;            // the call has a communicator, of `world` ranks
    int world = 1;
};

// E-row matrices over ice / exchange columns (EvI, EvX): the apply may build bands for them (ensure_bands)
inline bool band_eligible(int row_key, int col_key) { return row_key == KEY_E && (col_key == KEY_I || col_key == KEY_X); }
// The band structure at build time is opt-in (ibh_set_tuning("assemble_bands", 1)): it costs +25-35 % of the build and buys -16 % on a
// 1 km apply, nothing at 5 km -- right for a matrix that is applied to many field batches, wrong for the coupler's one build : one
// apply per step.
inline bool bands_at_build(int row_key, int col_key) { return band_eligible(row_key, col_key) && get_tuning("assemble_bands", 0); }
// smoothing and the band structure work on intermediates of the general pipeline; a SHARED smoothed build takes the unsmoothed matrix
// from the shared build and smooths it, shared as well
inline bool fast_path_wanted(const BuildFacts &f) { return (!f.smooth || f.shared) && !f.bands_wanted && get_tuning("assemble_fast", 1); }
// large grids: the streamed build (and the class bytes of the elevation mask it reads, made when the mask is set)
inline bool stream_default(long nX) { return get_tuning("assemble_stream", nX >= (1l << 20) ? 1 : 0) != 0; }

// ---- roles -------------------------------------------------------------------------------------------------------------------------
// The two sides of a matrix of the G/P builds (every family but EvA): G = the A / E side, counted and numbered by the ranges;
// P = the I / X side, an element of which sees at most a few exchange cells
struct Roles {
    bool g_is_row = false;          // AvI, EvI, AvX, EvX: G is the row side
    int gkey = KEY_A, glist = LIST_AP, pkey = KEY_I, plist = LIST_I;
    int64_t gext = 0, pext = 0;     // the sparse extents of the two keys
    int64_t g_n = 0;                // members of the G set before the build
    int pmode = -1;                 // the P set: 1 fresh, 0 the identity over the whole extent, -1 unsupported
    bool g_fresh = false;           // the G set is numbered by this build; else pre-populated (E columns)
    int merge = 0;                  // 1: neither side is X, entries of the same (G, P) pair merge
    bool EP = false;                // the matrix has elevation-class entries (LIST_EP on one side)
};
inline Roles roles_of(const BuildFacts &f) {
    Roles r;
    r.g_is_row = f.family == FAM_AEVI;
    const SetFacts &gs = f.set[r.g_is_row ? 0 : 1], &ps = f.set[r.g_is_row ? 1 : 0];
    r.gkey = r.g_is_row ? f.row_key : f.col_key; r.glist = r.g_is_row ? f.row_list : f.col_list;
    r.pkey = r.g_is_row ? f.col_key : f.row_key; r.plist = r.g_is_row ? f.col_list : f.row_list;
    r.gext = gs.extent; r.pext = ps.extent; r.g_n = gs.n;
    r.pmode = ps.fresh() ? 1 : ps.identity_complete() ? 0 : -1;
    r.g_fresh = gs.fresh();
    r.merge = (f.row_key != KEY_X && f.col_key != KEY_X) ? 1 : 0;
    r.EP = f.row_list == LIST_EP || f.col_list == LIST_EP;
    return r;
}
// a pre-populated G set the sorted-grid builds serve: E columns of an I/X-row matrix (the coupler's shared dimE), looked up through
// the set's sparse -> dense table
inline bool prepopulated_g_ok(const Roles &r, const SetFacts &gs) { return !gs.identity && r.gkey == KEY_E && !r.g_is_row; }

// ---- the per-range build (fastasm.inl) ---------------------------------------------------------------------------------------------
// Workgroup shape of the two per-range kernels, by the size of the ranges.  One workgroup owns one range; what bounds it is
// latency (staged load rounds, ranking barriers, the sequential sums of one wave per class), so the chip wants many small
// workgroups when there are many small ranges and few large ones otherwise.  Measured (ms per build, AvI / EvI):
//   Antarctica 1 km x 1/2 deg (49 771 ranges of ~780 cells): 256 x 4 cells 1.53 / 2.10, 256 x 2 1.40 / 1.92, 128 x 2 1.26 / 1.74,
//                                                            128 x 4 1.33 / 1.87, 64 x 4 1.32 / 2.12, 64 x 2 1.38 / 2.22
//   1 km (553 ranges of ~7 900 cells):                       128 x 2 0.30 / 0.44, 256 x 4 0.24 / 0.32, 1024 x 4 0.34 / 0.37
//   5 km (122 ranges of ~1 500: fewer workgroups than CUs):  128 x 2 0.096 / 0.142, 256 x 4 0.082 / 0.109, 1024 x 4 0.076 / 0.089
// Round 5, the synthetic 5 km grid of the tests (252 ranges of ~720 cells; us per build AvI / EvI / IvE / XvE): 256 x 4 64.8 / 94.3 /
// 115.0 / 89.8, 1024 x 4 58.6 / 75.8 / 97.9 / 74.2, 1024 x 1 54.6 / 68.8 / 92.6 / 69.5; 20 km (60 ranges of ~240): 256 x 4 46.0 / 68.2 /
// 84.1 / 63.4, 1024 x 4 54.5 / 69.5 / 88.0 / 68.0, 1024 x 1 46.2 / 62.5 / 80.3 / 60.1 -- with fewer workgroups than the chip holds, one
// cell per thread: the per-thread loops over the cells of a pass are what a range's workgroup spends its time in.
// shape 0: 128 threads x 2 cells, 1: 256 x 4, 2: 1024 x 4, 3: 1024 x 1 (tuning "assemble_range_shape" overrides; scratch/asm_shapes.py)
constexpr int FA_SHAPE_T[4] = {128, 256, 1024, 1024}, FA_SHAPE_CPT[4] = {2, 4, 4, 1};
inline int fa_range_shape(long nX, int nAr) {
    const int forced = get_tuning("assemble_range_shape", -1);
    if (forced >= 0 && forced <= 3) return forced;
    const long mean = nX / (nAr > 0 ? nAr : 1);
    if (mean <= 1024 && nAr <= 512) return 3;           // every workgroup resident at once (two of 1024 threads per CU): a cell per thread
    if (mean <= 1024 && nAr >= 2048) return 0;
    if (mean > 1024 && nAr <= 256) return 2;            // at most one workgroup per CU: make it a big one
    return 1;
}
// one-class matrices of large grids: cells streamed, counts by integer atomics (three launches, all short)
inline bool range_stream_count(const Roles &r, int NC, long nX) {
    return !r.EP && NC == 1 && r.g_fresh && get_tuning("assemble_stream_count", nX >= (1l << 20) ? 1 : 0);
}
// Small grids are bound by launches and synchronisations, not by bytes: their outputs are allocated by upper bounds (<= 2 entries per
// exchange cell, <= NC rows per range) so that the counters are read back ONCE, with the final synchronisation; large grids read
// them after the scans and allocate exactly.
inline bool range_optimistic(long nX) { return nX <= (1l << 20); }
// small grids: the scans ride in the counting kernel (FaChain: the classes of the ranges before in FA_CH_NC bits) and the counters
// come initialised from a ring of slots -- three launches fewer in a chain of seven to nine that is all a 5 km build costs
inline bool range_chained(bool optimistic, bool stream_count, long nrc) { return optimistic && !stream_count && nrc < (1l << FA_CH_NC); }
// the scans over the ranges when they do not ride in the counting kernel: few ranges, one workgroup in one launch (k_fa_rscan); many,
// three short launches for all channels (one workgroup adds up the sums of <= 1024 tiles of 1024 ranges); more, the
// device-wide scan channel by channel
enum ScanForm { SCAN_CHAINED, SCAN_ONE_WORKGROUP, SCAN_MANY, SCAN_DEVICE_WIDE };
inline ScanForm range_scan_form(bool chained, int nAr) {
    if (chained) return SCAN_CHAINED;
    if (nAr <= 4096) return SCAN_ONE_WORKGROUP;
    return asm_cdiv(nAr, 1024) <= 1024 ? SCAN_MANY : SCAN_DEVICE_WIDE;
}
// Mw of the ice cells that straddle ranges (a few %), A/E-row matrices on ice columns: few of them, eight lanes per ice cell --
// on small grids in extra workgroups of the range kernel's own launch, else k_fa_psums8; many, a thread per ice cell (k_fa_pelem<SUMS>)
enum SumsForm { SUMS_NONE, SUMS_IN_RANGE_LAUNCH, SUMS_PSUMS8, SUMS_PELEM };
inline SumsForm range_sums_form(const Roles &r, int nmulti, bool chained) {
    if (!r.g_is_row || r.pkey != KEY_I || !nmulti) return SUMS_NONE;
    if (nmulti > (1l << 20)) return SUMS_PELEM;
    return chained ? SUMS_IN_RANGE_LAUNCH : SUMS_PSUMS8;
}
// where the row pointer of the matrix comes from: the range kernel writes it with the rows (A/E rows); I/X rows: count -> scan per
// element, or -- chained builds -- from the counting launch: extra workgroups count and scan the static row lengths of the identity
// ice set, the ranges' own look-back scans the rows of an ice set numbered by this build or of the identity exchange-cell set
enum RowptrFrom { ROWPTR_RANGE_EMIT, ROWPTR_PELEM_COUNT, ROWPTR_COUNT_LAUNCH_IDENTITY_I, ROWPTR_COUNT_LAUNCH_FRESH_I, ROWPTR_RANGES_X };
enum CountClears { CLEAR_NONE, CLEAR_MW_P, CLEAR_ROWLEN };      // what the counting launch of a chained build clears for the later kernels
struct RangePlan {
    int shape = 1, threads = 256, cpt = 4;      // the per-range kernels' workgroup
    int NC = 1;                     // classes per range: 1 (A) or nhc (E)
    long nrc = 0;                   // nAr * NC
    bool static_count = false;      // the static entry counts per ice cell are used (tuning "assemble_static_count")
    bool stream_count = false, optimistic = false, chained = false;
    ScanForm scan = SCAN_ONE_WORKGROUP;
    RowptrFrom rowptr = ROWPTR_RANGE_EMIT;
    long rowptr_rows = 0;           // rows the counting launch's row pointer is allocated for (0: it writes none)
    int count_extra = 0;            // workgroups of k_fa_count that count row lengths
    long nstatus = 0;               // status words of the chained scans
    CountClears clears = CLEAR_NONE;
    long nclear = 0;                // 32-bit words of it
    long nclear_mw_g = 0;           // ... and of Mw over a pre-populated G column set (0: none)
    long nfill = 0;                 // entries of the fresh E set's sparse -> dense table, written as the set is numbered (0: not written early)
    long np_ub = 0, ng_ub = 0, nnz_ub = 0;      // optimistic: the bounds the outputs are allocated with
    SumsForm sums = SUMS_NONE;
    int range_extra = 0;            // workgroups of k_fa_range that add up the straddlers' Mw
    bool published = false;         // the build's last kernel hands the counters to the host
};
inline RangePlan plan_range(const BuildFacts &f, const Roles &r) {
    RangePlan p;
    p.shape = fa_range_shape(f.nX, f.nAr); p.threads = FA_SHAPE_T[p.shape]; p.cpt = FA_SHAPE_CPT[p.shape];
    p.NC = r.gkey == KEY_E ? f.nhc : 1;
    p.nrc = (long)f.nAr * p.NC;
    p.static_count = get_tuning("assemble_static_count", 1) && f.icnt_pos;
    p.stream_count = range_stream_count(r, p.NC, f.nX);
    p.optimistic = range_optimistic(f.nX);
    p.chained = range_chained(p.optimistic, p.stream_count, p.nrc);
    p.scan = range_scan_form(p.chained, f.nAr);
    p.sums = range_sums_form(r, f.nmulti, p.chained);
    if (p.sums == SUMS_IN_RANGE_LAUNCH) p.range_extra = (int)asm_cdiv(8 * (long)f.nmulti, p.threads);
    p.published = p.chained;        // (chained => optimistic: the counters are read once, at the end)
    const bool fresh = r.pmode == 1;
    p.rowptr = r.g_is_row ? ROWPTR_RANGE_EMIT : ROWPTR_PELEM_COUNT;
    p.np_ub = fresh ? (long)std::min<int64_t>(r.pext, f.nX) : (long)r.pext;
    p.ng_ub = p.nrc;
    p.nnz_ub = (r.EP ? 2 : 1) * f.nX;
    if (!p.chained) return p;
    if (!r.g_is_row && r.pkey == KEY_I && p.static_count) {
        p.rowptr = fresh ? ROWPTR_COUNT_LAUNCH_FRESH_I : ROWPTR_COUNT_LAUNCH_IDENTITY_I;
        p.rowptr_rows = fresh ? p.np_ub : (long)r.pext;
        if (!fresh) p.count_extra = (int)asm_cdiv((long)r.pext, p.threads);
    } else if (!r.g_is_row && r.pkey == KEY_X && !fresh && r.merge == 0) {
        p.rowptr = ROWPTR_RANGES_X;
        p.rowptr_rows = f.nX;
    }
    p.nstatus = (long)f.nAr + p.count_extra + (p.rowptr == ROWPTR_COUNT_LAUNCH_FRESH_I ? (long)f.nAr : 0);
    // (what k_fa_zero_identity did in a launch of its own)
    if (!r.g_is_row && !r.g_fresh && r.g_n > 0) p.nclear_mw_g = 2 * (long)r.g_n;
    // a fresh E set: the step's later builds (IvE, XvE on the dimE this EvI numbers: IceCoupler.cpp:361-377) look keys up in the
    // sparse -> dense table -- written here as the set is numbered instead of by two launches and a synchronisation later
    if (r.g_fresh && r.gkey == KEY_E && r.gext < (1l << 22)) p.nfill = (long)r.gext;
    if (r.g_is_row && !fresh && p.np_ub) { p.clears = CLEAR_MW_P; p.nclear = 2 * p.np_ub; }       // Mw of an identity P set: members without entries stay 0
    else if (!r.g_is_row && fresh) { p.clears = CLEAR_ROWLEN; p.nclear = p.np_ub + 1; }            // row lengths beyond the real number of rows
    return p;
}
// EvA / AvE: the class counts and the (range, class) sums of the per-range kernels, never chained
inline RangePlan plan_range_eva(const BuildFacts &f) {
    RangePlan p;
    p.shape = fa_range_shape(f.nX, f.nAr); p.threads = FA_SHAPE_T[p.shape]; p.cpt = FA_SHAPE_CPT[p.shape];
    p.NC = f.nhc;
    p.nrc = (long)f.nAr * p.NC;
    p.static_count = get_tuning("assemble_static_count", 1) && f.icnt_pos;
    p.scan = range_scan_form(false, f.nAr);
    return p;
}

// ---- the streamed build (streamasm.inl) --------------------------------------------------------------------------------------------
struct StreamKernels {              // which instantiations the passes take: by the grid, the same for every rank of a shared build
    bool rel32 = false;             // positions inside a range's block of entries need 32 bits
    int oldseg = SA_OLDSEG_S, wpr = 1;
    bool rowsl = false, rows4 = false;
    int emit_cpt = 1;
};
struct StreamPlan : StreamKernels {
    bool ok = false;                // statically eligible
    int world = 1;
    int NC = 1, nAr = 0;
    // an I-row matrix on an identity ice set (the coupler's IvE, IceCoupler.cpp:462): its rows lie in ice-cell order, not in
    // first-seen order -- row lengths are scattered by ice cell and scanned over the ice cells
    bool by_ice = false;
    bool ident_p = false, ident_x_rows = false, ident_i_rows = false, prepop_g = false;     // the shared build's special pieces (stream_build)
    bool pscan = false;             // the P keys are numbered (first-seen ranks)
};
inline bool stream_rel32(bool EP, int maxrange) { return (int64_t)(EP ? 2 : 1) * maxrange > 65535; }
// (straddlers of a range ~ its perimeter: a range of ~10^3 cells has a few dozen, one of 10^4 a few hundred)
inline int stream_oldseg(long mean) {
    const int forced = get_tuning("assemble_stream_oldseg", -1);
    return (forced == SA_OLDSEG_S || forced == SA_OLDSEG_L) ? forced : mean <= 2048 ? SA_OLDSEG_S : SA_OLDSEG_L;
}
// waves per range by the size of the ranges: one wave walks ~10^3 cells in a few round trips; longer ranges are cut
inline int stream_wpr(long mean) {
    const int forced = get_tuning("assemble_stream_wpr", -1);
    return (forced == 1 || forced == 4 || forced == 16) ? forced : mean <= 1024 ? 1 : mean <= 4096 ? 4 : 16;
}
// row kernel: a 16-lane row of a wave per segment.  One-class matrices: four consecutive ranges per wave; elevation classes: a
// wave per range and group of four classes.
// (measured on the Antarctic sheet, same box, four segments per wave against one: the column sums of the I/X-row matrices win
// -- IvA 0.902 / 0.939 ms, IvE 1.53 / 1.55, XvE 1.14 / 1.20; the rows of AvI are even, 0.684 / 0.686, but with 128 values of a
// segment in registers -- more cost occupancy: 146 VGPRs at 256 -- the scaling re-reads the rest: 264 against 176 MB fetched; EvI
// loses, 1.33 / 1.25: a range has two or three classes there, a quarter to half of the rows idle.  So: column sums only.)
inline bool stream_rows4(int oldseg, bool g_is_row) {
    const int forced = get_tuning("assemble_stream_rows4", -1);
    return oldseg == SA_OLDSEG_S && (forced >= 0 ? forced != 0 : !g_is_row);
}
// the lane-parallel row kernel (k_sa_oldsort + k_sa_rowsL), R ranges per wave.  Measured on the Antarctic sheet, same box, against
// the kernels above: the column sums of IvE 42 + 149 us against 231 (IvE 1.55 -> 1.43 ms, IvA 0.937 -> 0.910), the rows of AvI 25 +
// 143 against 138, of EvI 42 + 340 against 270 -- a wave with sixteen chains waits for its memory round trips with two waves per
// SIMD (66 KB of LDS per workgroup), and R = 4 beats 16: more waves matter more than full lanes.  1 km Greenland (1 143 long
// ranges) loses by 2 x.  So: column sums of grids with many ranges only.
inline bool stream_rowsl(bool g_is_row, int nAr) {       // (by the whole grid's ranges: every rank of a shared build takes the same kernel)
    const int forced = get_tuning("assemble_stream_rowsl", -1);
    return forced >= 0 ? forced != 0 : (!g_is_row && nAr >= 16384);
}
// the emit pass: one cell per thread (four with 32-bit offsets), at most EMIT_BLOCKS workgroups.  The pass is bound by instruction
// issue and latency, not by bandwidth (ablation on the Antarctic AvI: 129 us with every load of cell data, every term and every
// store removed; stores +95, the first-seen lookup of the straddlers +45 after the bitmask change, +115 before): a workgroup that
// walks several tiles has the code bytes of its next tile in flight while it works.  Measured (cells per thread x workgroups), a1h
// AvI / IvA / EvI / IvE ms, same box: 2 x full grid 0.645 / 0.915 / 1.216 / 1.604; 1 x full 0.704 / 0.919 / 1.228 / 1.555;
// 1 x 8192 0.636 / 0.878 / 1.135 / 1.470; 2 x 8192 0.642 / 0.926 / 1.183 / 1.574; 4 x full 0.709 / 1.063 / 1.274 / 1.711
inline unsigned stream_emit_grid(const StreamKernels &s, long ncell) { return (unsigned)std::min(asm_cdiv(ncell, (long)SA_T * s.emit_cpt), EMIT_BLOCKS); }

// world <= 1: the streamed build of one GPU; world > 1: the shared build of a communicator's ranks
inline StreamPlan plan_stream(const BuildFacts &f, const Roles &r, int world) {
    StreamPlan s;
    s.world = std::max(world, 1);
    s.NC = r.gkey == KEY_E ? f.nhc : 1; s.nAr = f.nAr;
    const bool sharded = s.world > 1;
    s.by_ice = !r.g_is_row && r.pkey == KEY_I && r.pmode == 0;
    // sharded: the pieces of a rank must be contiguous in every result array -- sets numbered by this build; at most 8 ranks (one
    // 256-byte read-back carries all counters), each with a range of its own.  Served too (stream_build says how): an A/E-row matrix
    // on an identity P set, an X-row matrix on the identity dimX, I rows on the identity dimI, a pre-populated G set.
    s.ident_p = sharded && r.pmode == 0 && r.g_is_row;
    s.ident_x_rows = sharded && r.pmode == 0 && !r.g_is_row && r.pkey == KEY_X;
    s.ident_i_rows = sharded && s.by_ice;
    s.prepop_g = sharded && !r.g_fresh;
    s.pscan = r.pmode == 1 || s.ident_p || s.ident_i_rows;
    if (!sharded && !stream_default(f.nX)) return s;
    if (r.EP && (f.tiny || !f.icnt_nz)) return s;       // classes are counted by the sign of the area here
    if (!f.icnt_pos) return s;
    if (sharded && ((r.pmode != 1 && !s.ident_p && !s.ident_x_rows && !s.ident_i_rows) || s.world > 8 || f.nAr < s.world)) return s;
    if (f.nhc > 64) return s;
    s.ok = true;
    return s;
}
inline StreamKernels stream_kernels(const BuildFacts &f, const Roles &r) {
    StreamKernels k;
    k.rel32 = stream_rel32(r.EP, f.maxrange);
    const long mean = f.nX / std::max(f.nAr, 1);
    k.oldseg = stream_oldseg(mean);
    if (r.EP) k.wpr = stream_wpr(mean);
    k.rows4 = stream_rows4(k.oldseg, r.g_is_row);
    k.rowsl = stream_rowsl(r.g_is_row, f.nAr);
    k.emit_cpt = k.rel32 ? 4 : 1;
    return k;
}
// The row kernels' grids, known after the mid-build read-back: ncls_slice = classes of this rank's nr ranges, ncls_grid = of the whole
// grid's (every rank of a shared build derives the same kernel from whole-grid numbers; only the grids are by the slice).
struct StreamRowsPlan {
    int avg_cls = 1, rows_R = 1;    // k_sa_rowsL: ranges per wave
    unsigned grid_rows4[2] = {1, 1}, grid_rows1[2] = {1, 1}, grid_rowsl = 1;
};
inline StreamRowsPlan plan_stream_rows(const StreamPlan &s, int nr, uint32_t ncls_slice, uint64_t ncls_grid) {
    StreamRowsPlan q;
    const int NC = s.NC, per_range = (int)(ncls_slice / (uint32_t)std::max(nr, 1));
    // rows4: y = the groups of four classes a range has on average, + 1 (the others loop)
    q.grid_rows4[0] = (unsigned)asm_cdiv(NC == 1 ? asm_cdiv(nr, 4) : nr, 4);
    q.grid_rows4[1] = NC == 1 ? 1u : (unsigned)std::max(1, std::min((std::min(NC, 16) + 3) / 4, (per_range + 2 + 3) / 4));
    // (long ranges: one wave per (range, class), y = the classes a range has on average, rounded up, + 1)
    q.grid_rows1[0] = (unsigned)asm_cdiv(nr, 4);
    q.grid_rows1[1] = NC == 1 ? 1u : (unsigned)std::max(1, std::min(std::min(NC, 16), per_range + 2));
    const uint64_t nA = (uint64_t)std::max(s.nAr, 1);
    q.avg_cls = NC == 1 ? 1 : std::max(1, (int)((ncls_grid + nA - 1) / nA));
    q.rows_R = std::max(1, std::min(16, get_tuning("assemble_stream_rowsl_r", std::min(4, 16 / q.avg_cls))));
    q.grid_rowsl = (unsigned)asm_cdiv(nr, 4 * q.rows_R);
    return q;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------------
// the paths, as ibh_weighted_built_fast reports them (EvA / AvE report the per-range build's code)
enum BuildPath { PATH_GENERAL = 0, PATH_RANGE = 1, PATH_STREAM = 2, PATH_STREAM_SHARED = 3, PATH_EVA = 4 };
struct BuildPlan {
    Roles roles;                    // (every family but EvA)
    // the statically eligible paths in the order they are tried; a build discarded at run time (fallback flags) moves to the next one
    BuildPath path[4] = {PATH_GENERAL, PATH_GENERAL, PATH_GENERAL, PATH_GENERAL};
    int npath = 0;
    bool prepop_table = false;      // a pre-populated G set is read through its sparse -> dense table (fast_prewarm makes it up front)
    RangePlan range;
    StreamPlan stream_shared, stream;
    bool tries(BuildPath p) const { return std::find(path, path + npath, p) != path + npath; }
};
inline BuildPlan plan_build(const BuildFacts &f) {
    BuildPlan b;
    auto general = [&]() -> BuildPlan & { b.path[b.npath++] = PATH_GENERAL; return b; };
    if (!f.plan_ok) return general();
    if (f.family == FAM_EVA) {      // both sets fresh; pre-populated ones: the general pipeline
        if (!get_tuning("assemble_fast_eva", 1) || !f.set[0].fresh() || !f.set[1].fresh() || f.same_set) return general();
        b.range = plan_range_eva(f);
        b.path[b.npath++] = PATH_EVA;
        return general();
    }
    b.roles = roles_of(f);
    const Roles &r = b.roles;
    const bool g_ok = r.g_fresh || prepopulated_g_ok(r, f.set[r.g_is_row ? 0 : 1]);
    b.prepop_table = !r.g_fresh && g_ok;
    if (r.pmode < 0 || !g_ok) return general();
    // the sharded build; when it does not apply (the same on every rank: static conditions, exchanged flags) the ranks go on to
    // build the matrix redundantly
    if (f.shared && f.world > 1) {
        b.stream_shared = plan_stream(f, r, f.world);
        if (b.stream_shared.ok) b.path[b.npath++] = PATH_STREAM_SHARED;
    }
    b.stream = plan_stream(f, r, 1);
    if (b.stream.ok) b.path[b.npath++] = PATH_STREAM;
    if (b.stream_shared.ok || b.stream.ok) static_cast<StreamKernels &>(b.stream_shared) = static_cast<StreamKernels &>(b.stream) = stream_kernels(f, r);
    b.range = plan_range(f, r);
    b.path[b.npath++] = PATH_RANGE;
    return general();
}
}  // namespace ibh
