// The decisions of the sorted-grid builds (icebin_amd/csrc/asm_plan.h) on both sides of every host-decided threshold of
// tests/assembly_limit_cases.py, every knob's override, the gate over matrix names x set states, and invariants over a sweep of
// facts -- at sizes no GPU test builds.  Expected values are written out here from the builders as they stood before the plan
// existed (range_before below is that code's arithmetic, line by line).  Host code only: its own get_tuning, no HIP.
#include "../../icebin_amd/csrc/asm_plan.h"

#include <climits>
#include <cstdio>
#include <cstring>
#include <map>
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
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++g_failed; } } while (0)

struct Spec { const char *name; int family, row_list, row_key, col_list, col_key; };
static const Spec SPECS[10] = {
    {"AvI", FAM_AEVI, LIST_AP, KEY_A, LIST_I, KEY_I},  {"EvI", FAM_AEVI, LIST_EP, KEY_E, LIST_I, KEY_I},
    {"AvX", FAM_AEVI, LIST_AP, KEY_A, LIST_AP, KEY_X}, {"EvX", FAM_AEVI, LIST_EP, KEY_E, LIST_EP, KEY_X},
    {"IvA", FAM_IVAE, LIST_I, KEY_I, LIST_AP, KEY_A},  {"IvE", FAM_IVAE, LIST_I, KEY_I, LIST_EP, KEY_E},
    {"XvA", FAM_IVAE, LIST_AP, KEY_X, LIST_AP, KEY_A}, {"XvE", FAM_IVAE, LIST_EP, KEY_X, LIST_EP, KEY_E},
    {"EvA", FAM_EVA, LIST_EP, KEY_E, LIST_AP, KEY_A},  {"AvE", FAM_EVA, LIST_AP, KEY_A, LIST_EP, KEY_E},
};
enum SetState { FRESH, IDENT_COMPLETE, IDENT_PARTIAL, PREPOP };
static int64_t extent_of(int key, long nX, long nI, long nA, int nhc) { return key == KEY_A ? nA : key == KEY_E ? nA * nhc : key == KEY_I ? nI : nX; }
static void set_state(SetFacts &s, SetState st) {
    s.n = st == FRESH ? 0 : st == IDENT_COMPLETE ? s.extent : s.extent / 2 + 1;
    s.identity = st == IDENT_COMPLETE || st == IDENT_PARTIAL;
}
// a sheet with a static plan: nAr ranges over nX exchange cells, one ice cell per exchange cell, nhc classes, both sets fresh
static BuildFacts facts(const char *name, long nX, int nAr, int nhc = 4) {
    BuildFacts f;
    for (const Spec &s : SPECS)
        if (!strcmp(s.name, name)) { f.family = s.family; f.row_key = s.row_key; f.col_key = s.col_key; f.row_list = s.row_list; f.col_list = s.col_list; }
    f.nX = nX; f.nI = nX; f.nhc = nhc;
    f.plan_ok = true; f.nAr = nAr; f.nmulti = 100; f.nmulti3 = 10; f.npair = 90; f.maxrange = (int)std::min<long>(2 * (nX / std::max(nAr, 1)), 30000);
    f.icnt_pos = f.icnt_nz = true;
    f.set[0].extent = extent_of(f.row_key, nX, f.nI, nAr, nhc); f.set[1].extent = extent_of(f.col_key, nX, f.nI, nAr, nhc);
    return f;
}
static BuildFacts facts_in(const char *name, long nX, int nAr, SetState rows, SetState cols, int nhc = 4) {
    BuildFacts f = facts(name, nX, nAr, nhc);
    set_state(f.set[0], rows); set_state(f.set[1], cols);
    return f;
}
static bool paths_are(const BuildPlan &b, std::initializer_list<BuildPath> want) {
    if (b.npath != (int)want.size()) return false;
    int k = 0;
    for (BuildPath p : want) if (b.path[k++] != p) return false;
    return true;
}

// ---- fast_build_gp's decisions as that function computed them while it allocated (the code before asm_plan.h, transcribed) ----
struct Before {
    bool stream_count, optimistic, chained, pc, ir, xr, zero2, fill_m1, zero_mw, zero_rowlen, pcount_done, in_range, psums8, pelem_sums, published;
    int fa_shape, count_extra, range_extra, scan;      // scan: 0 chained, 1 one workgroup, 2 many, 3 device-wide
    long nstatus, nzero, nzero2, nfill, np_ub;
};
static int shape_before(long nX, int nAr) {
    const int forced = get_tuning("assemble_range_shape", -1);
    if (forced >= 0 && forced <= 3) return forced;
    const long mean = nX / (nAr > 0 ? nAr : 1);
    if (mean <= 1024 && nAr <= 512) return 3;
    if (mean <= 1024 && nAr >= 2048) return 0;
    if (mean > 1024 && nAr <= 256) return 2;
    return 1;
}
static Before range_before(const BuildFacts &f) {
    Before o{};
    const bool g_is_row = f.family == FAM_AEVI;
    const SetFacts &gset = f.set[g_is_row ? 0 : 1], &pset = f.set[g_is_row ? 1 : 0];
    const int gkey = g_is_row ? f.row_key : f.col_key, pkey = g_is_row ? f.col_key : f.row_key;
    const int64_t gext = gset.extent, pext = pset.extent;
    const int p_fresh = pset.n == 0 ? 1 : 0;
    const bool g_fresh = gset.n == 0, EP = f.row_list == LIST_EP || f.col_list == LIST_EP;
    const int merge = (f.row_key != KEY_X && f.col_key != KEY_X) ? 1 : 0;
    const bool icnt_pos = get_tuning("assemble_static_count", 1) ? f.icnt_pos : false;
    const long nX = f.nX;
    const int nAr = f.nAr, NC = gkey == KEY_E ? f.nhc : 1;
    const size_t nrc = (size_t)nAr * NC;
    const bool tab = !g_fresh;
    o.stream_count = !EP && NC == 1 && !tab && get_tuning("assemble_stream_count", nX >= (1l << 20) ? 1 : 0);
    o.optimistic = nX <= (1l << 20);
    o.chained = o.optimistic && !o.stream_count && nrc < (1ul << 15);
    o.fa_shape = shape_before(nX, nAr);
    if (o.chained) {
        o.pc = !g_is_row && pkey == KEY_I && !p_fresh && icnt_pos;
        const long pc_rows = o.pc ? (long)pext : 0;
        const int tshape_c = o.fa_shape == 0 ? 128 : o.fa_shape == 1 ? 256 : 1024;
        o.count_extra = o.pc ? (int)((pc_rows + tshape_c - 1) / tshape_c) : 0;
        o.ir = !g_is_row && pkey == KEY_I && p_fresh && icnt_pos;
        o.nstatus = (long)((size_t)nAr + (size_t)o.count_extra + (o.ir ? (size_t)nAr : 0));
        o.xr = !g_is_row && pkey == KEY_X && !p_fresh && merge == 0;
        if (!g_is_row && !g_fresh && gset.n > 0) { o.zero2 = true; o.nzero2 = 2 * gset.n; }
        if (g_fresh && gkey == KEY_E && gext < (1l << 22)) { o.fill_m1 = true; o.nfill = gext; }
        o.np_ub = p_fresh ? (long)std::min<int64_t>(pext, nX) : (long)pext;
        if (g_is_row && !p_fresh && o.np_ub) { o.zero_mw = true; o.nzero = 2 * o.np_ub; }
        else if (!g_is_row && p_fresh) { o.zero_rowlen = true; o.nzero = o.np_ub + 1; }
    }
    o.pcount_done = o.count_extra > 0 || o.xr || o.ir;
    const int nb = (nAr + 1023) / 1024;
    o.scan = o.chained ? 0 : (nAr > 4096 && nb <= 1024) ? 2 : nAr > 4096 ? 3 : 1;
    if (g_is_row) {
        bool sums_after = pkey == KEY_I && f.nmulti;
        if (o.chained) o.published = true;
        if (sums_after && o.chained && f.nmulti <= (1l << 20)) {
            const int tshape = o.fa_shape == 0 ? 128 : o.fa_shape == 1 ? 256 : 1024;
            o.range_extra = (int)((8 * (long)f.nmulti + tshape - 1) / tshape);
            o.in_range = true;
            sums_after = false;
        }
        if (sums_after) { if (f.nmulti <= (1l << 20)) o.psums8 = true; else o.pelem_sums = true; }
    } else if (o.chained) o.published = true;
    return o;
}
static void check_same(const BuildFacts &f) {
    const Before o = range_before(f);
    const BuildPlan b = plan_build(f);
    const RangePlan &p = b.range;
    CHECK(b.tries(PATH_RANGE));
    CHECK(p.stream_count == o.stream_count && p.optimistic == o.optimistic && p.chained == o.chained && p.shape == o.fa_shape);
    CHECK(p.threads == (o.fa_shape == 0 ? 128 : o.fa_shape == 1 ? 256 : 1024) && p.cpt == (o.fa_shape == 0 ? 2 : o.fa_shape == 3 ? 1 : 4));
    CHECK(p.count_extra == o.count_extra && p.range_extra == o.range_extra && (int)p.scan == o.scan && p.published == o.published);
    CHECK((p.rowptr == ROWPTR_COUNT_LAUNCH_IDENTITY_I) == o.pc && (p.rowptr == ROWPTR_COUNT_LAUNCH_FRESH_I) == o.ir && (p.rowptr == ROWPTR_RANGES_X) == o.xr);
    CHECK((p.rowptr == ROWPTR_RANGE_EMIT) == b.roles.g_is_row);
    CHECK((p.rowptr != ROWPTR_PELEM_COUNT && p.rowptr != ROWPTR_RANGE_EMIT) == o.pcount_done);
    if (o.chained) CHECK(p.nstatus == o.nstatus && p.np_ub == o.np_ub);
    CHECK((p.nclear_mw_g > 0) == o.zero2 && p.nclear_mw_g == o.nzero2 && (p.nfill > 0) == o.fill_m1 && p.nfill == o.nfill);
    CHECK((p.clears == CLEAR_MW_P) == o.zero_mw && (p.clears == CLEAR_ROWLEN) == o.zero_rowlen && p.nclear == o.nzero);
    CHECK((p.sums == SUMS_IN_RANGE_LAUNCH) == o.in_range && (p.sums == SUMS_PSUMS8) == o.psums8 && (p.sums == SUMS_PELEM) == o.pelem_sums);
    // the invariants the builders rely on
    CHECK(!p.chained || p.optimistic);
    CHECK(p.count_extra == 0 || p.chained);
    CHECK(!p.published || p.chained);
    CHECK(p.nstatus == (p.chained ? (long)f.nAr + p.count_extra + (p.rowptr == ROWPTR_COUNT_LAUNCH_FRESH_I ? (long)f.nAr : 0) : 0));
    CHECK(p.nclear >= 0 && p.nclear <= (long)UINT_MAX && p.nclear_mw_g >= 0 && p.nclear_mw_g <= (long)UINT_MAX && p.nfill >= 0 && p.nfill <= (long)UINT_MAX);
    CHECK(p.rowptr_rows == (o.pc ? (long)b.roles.pext : o.ir ? o.np_ub : o.xr ? f.nX : 0));
}

int main() {
    const long NX20 = 1l << 20;
    {   // nhc 64 / 65: the streamed build's own limit (the static plan refuses 65 before: ensure_plan)
        g_tuning["assemble_stream"] = 1;
        CHECK(plan_build(facts("EvI", 5000, 50, 64)).stream.ok && plan_build(facts("AvI", 5000, 50, 64)).stream.ok);
        CHECK(!plan_build(facts("EvI", 5000, 50, 65)).stream.ok && !plan_build(facts("AvI", 5000, 50, 65)).stream.ok);
        CHECK(paths_are(plan_build(facts("EvI", 5000, 50, 65)), {PATH_RANGE, PATH_GENERAL}));
        g_tuning.clear();
    }
    {   // stream_default: from 2^20 exchange cells on the streamed build is tried first
        CHECK(paths_are(plan_build(facts("AvI", NX20 - 1, 16384)), {PATH_RANGE, PATH_GENERAL}));
        CHECK(paths_are(plan_build(facts("AvI", NX20, 16384)), {PATH_STREAM, PATH_RANGE, PATH_GENERAL}));
        CHECK(!stream_default(NX20 - 1) && stream_default(NX20));
        g_tuning["assemble_stream"] = 1;
        CHECK(paths_are(plan_build(facts("IvE", 5000, 50)), {PATH_STREAM, PATH_RANGE, PATH_GENERAL}));
        g_tuning["assemble_stream"] = 0;
        CHECK(paths_are(plan_build(facts("IvE", NX20, 16384)), {PATH_RANGE, PATH_GENERAL}));
        g_tuning.clear();
        // the streamed elevation-class builds count by the sign of the area: not for sheets with underflowing areas or without
        // static counts; no streamed build at all without the per-ice-cell counts
        BuildFacts f = facts("EvI", NX20, 16384);
        f.tiny = true;
        CHECK(!plan_build(f).stream.ok);
        f.family = FAM_AEVI; f.row_key = KEY_A; f.row_list = LIST_AP;       // AvI on the same sheet
        f.set[0].extent = f.nAr;
        CHECK(plan_build(f).stream.ok);
        f = facts("EvI", NX20, 16384); f.icnt_nz = false;
        CHECK(!plan_build(f).stream.ok);
        f = facts("AvI", NX20, 16384); f.icnt_pos = false;
        CHECK(!plan_build(f).stream.ok);
    }
    {   // optimistic: outputs by upper bounds and one read-back up to 2^20 exchange cells
        const RangePlan lo = plan_build(facts("EvI", NX20, 1000)).range, hi = plan_build(facts("EvI", NX20 + 1, 1000)).range;
        CHECK(lo.optimistic && lo.chained && lo.published && lo.scan == SCAN_CHAINED);
        CHECK(!hi.optimistic && !hi.chained && !hi.published && hi.scan == SCAN_ONE_WORKGROUP);
        CHECK(lo.nnz_ub == 2 * NX20 && lo.ng_ub == 4000 && lo.np_ub == NX20);
        CHECK(plan_build(facts("AvI", NX20, 1000)).range.nnz_ub == NX20);
    }
    {   // chained: nAr * NC < 2^15
        CHECK(plan_build(facts("AvI", 65534, 32767)).range.chained && !plan_build(facts("AvI", 65536, 32768)).range.chained);
        CHECK(plan_build(facts("EvI", 100000, 4681, 7)).range.chained);                 // 32767 (range, class) slots
        CHECK(!plan_build(facts("EvI", 100000, 4096, 8)).range.chained);                // 32768
        CHECK(plan_build(facts("IvE", 100000, 4681, 7)).range.chained && !plan_build(facts("IvE", 100000, 4096, 8)).range.chained);
        g_tuning["assemble_stream_count"] = 1;                                          // the streamed count has no chain
        CHECK(!plan_build(facts("AvI", 65534, 32767)).range.chained && plan_build(facts("AvI", 65534, 32767)).range.stream_count);
        CHECK(plan_build(facts("EvI", 100000, 4681, 7)).range.chained);                 // (elevation classes: never counted by streaming)
        g_tuning.clear();
        // stream_count by default: one-class matrices of >= 2^20 cells on a fresh G set
        CHECK(plan_build(facts("AvI", NX20, 1000)).range.stream_count && !plan_build(facts("AvI", NX20 - 1, 1000)).range.stream_count);
        CHECK(!plan_build(facts("EvI", NX20, 1000)).range.stream_count && plan_build(facts("XvA", NX20, 1000)).range.stream_count);
        g_tuning["assemble_stream_count"] = 0;
        CHECK(!plan_build(facts("AvI", NX20, 1000)).range.stream_count && plan_build(facts("AvI", NX20, 1000)).range.chained);
        g_tuning.clear();
    }
    {   // rscan_many: unchained builds scan <= 4096 ranges in one workgroup, up to 2^20 in three launches, more device-wide
        CHECK(plan_build(facts("EvI", 12288, 4096, 8)).range.scan == SCAN_ONE_WORKGROUP);
        CHECK(plan_build(facts("EvI", 12291, 4097, 8)).range.scan == SCAN_MANY);
        CHECK(plan_build(facts("AvI", 4 * NX20, 1 << 20)).range.scan == SCAN_MANY);
        CHECK(plan_build(facts("AvI", 4 * NX20, (1 << 20) + 1)).range.scan == SCAN_DEVICE_WIDE);
        CHECK(plan_build(facts("EvA", 12288, 4096, 8)).range.scan == SCAN_ONE_WORKGROUP && plan_build(facts("AvE", 12291, 4097, 8)).range.scan == SCAN_MANY);
        CHECK(plan_build(facts("EvA", 4 * NX20, (1 << 20) + 1)).range.scan == SCAN_DEVICE_WIDE);
        CHECK(range_scan_form(true, 5000) == SCAN_CHAINED);
    }
    {   // psums: the straddlers' column sums
        BuildFacts f = facts("AvI", 8 * NX20, 129);
        f.nmulti = 1 << 20;
        CHECK(plan_build(f).range.sums == SUMS_PSUMS8 && plan_build(f).range.range_extra == 0);
        f.nmulti = (1 << 20) + 1;
        CHECK(plan_build(f).range.sums == SUMS_PELEM);
        f = facts("EvI", 100000, 100);                   // chained: in extra workgroups of the range launch (shape 3: 1024 threads)
        f.nmulti = 1000;
        CHECK(plan_build(f).range.sums == SUMS_IN_RANGE_LAUNCH && plan_build(f).range.range_extra == 8 && plan_build(f).range.shape == 3);
        f.nmulti = 0;
        CHECK(plan_build(f).range.sums == SUMS_NONE);
        CHECK(plan_build(facts("EvX", 100000, 100)).range.sums == SUMS_NONE && plan_build(facts("IvA", 100000, 100)).range.sums == SUMS_NONE);
    }
    {   // rel32: positions inside a range's block of entries in 16 bits up to 65535
        g_tuning["assemble_stream"] = 1;
        BuildFacts f = facts("AvI", 70000, 4);
        f.maxrange = 65535; CHECK(!plan_build(f).stream.rel32 && plan_build(f).stream.emit_cpt == 1);
        f.maxrange = 65536; CHECK(plan_build(f).stream.rel32 && plan_build(f).stream.emit_cpt == 4);
        f = facts("EvI", 70000, 4);
        f.maxrange = 32767; CHECK(!plan_build(f).stream.rel32);
        f.maxrange = 32768; CHECK(plan_build(f).stream.rel32);
        CHECK(!stream_rel32(true, 32767) && stream_rel32(true, 32768) && !stream_rel32(false, 65535) && stream_rel32(false, 65536));
        g_tuning.clear();
    }
    {   // default_oldseg, default_wpr4 / 16, default_rowsl, rows4
        g_tuning["assemble_stream"] = 1;
        CHECK(plan_build(facts("EvI", 2048 * 10, 10)).stream.oldseg == 128 && plan_build(facts("EvI", 2049 * 10, 10)).stream.oldseg == 512);
        CHECK(plan_build(facts("EvI", 1024 * 10, 10)).stream.wpr == 1 && plan_build(facts("EvI", 1025 * 10, 10)).stream.wpr == 4);
        CHECK(plan_build(facts("IvE", 4096 * 10, 10)).stream.wpr == 4 && plan_build(facts("IvE", 4097 * 10, 10)).stream.wpr == 16);
        CHECK(plan_build(facts("AvI", 4097 * 10, 10)).stream.wpr == 1);                 // (one-class builds have no class-count pass)
        CHECK(!plan_build(facts("IvA", 65536, 16383)).stream.rowsl && plan_build(facts("IvA", 65536, 16384)).stream.rowsl);
        CHECK(plan_build(facts("XvE", 65536, 16384)).stream.rowsl && !plan_build(facts("AvI", 65536, 16384)).stream.rowsl && !plan_build(facts("EvI", 65536, 16384)).stream.rowsl);
        CHECK(plan_build(facts("IvA", 20480, 10)).stream.rows4 && !plan_build(facts("AvI", 20480, 10)).stream.rows4 && !plan_build(facts("IvA", 20490, 10)).stream.rows4);
        // the overrides, out-of-range values ignored
        g_tuning["assemble_stream_oldseg"] = 512; CHECK(plan_build(facts("EvI", 1000, 10)).stream.oldseg == 512);
        g_tuning["assemble_stream_oldseg"] = 128; CHECK(plan_build(facts("EvI", 2049 * 10, 10)).stream.oldseg == 128);
        g_tuning["assemble_stream_oldseg"] = 256; CHECK(plan_build(facts("EvI", 1000, 10)).stream.oldseg == 128 && plan_build(facts("EvI", 2049 * 10, 10)).stream.oldseg == 512);
        g_tuning.erase("assemble_stream_oldseg");
        for (int w : {1, 4, 16}) { g_tuning["assemble_stream_wpr"] = w; CHECK(plan_build(facts("EvI", 2000 * 10, 10)).stream.wpr == w); }
        for (int w : {0, 2, 8, 32}) { g_tuning["assemble_stream_wpr"] = w; CHECK(plan_build(facts("EvI", 2000 * 10, 10)).stream.wpr == 4); }
        g_tuning.erase("assemble_stream_wpr");
        g_tuning["assemble_stream_rows4"] = 1; CHECK(plan_build(facts("AvI", 20480, 10)).stream.rows4 && !plan_build(facts("AvI", 20490, 10)).stream.rows4);
        g_tuning["assemble_stream_rows4"] = 0; CHECK(!plan_build(facts("IvA", 20480, 10)).stream.rows4);
        g_tuning.erase("assemble_stream_rows4");
        g_tuning["assemble_stream_rowsl"] = 1; CHECK(plan_build(facts("AvI", 20480, 10)).stream.rowsl);
        g_tuning["assemble_stream_rowsl"] = 0; CHECK(!plan_build(facts("IvA", 65536, 16384)).stream.rowsl);
        g_tuning.clear();
    }
    {   // the emit grid: one cell per thread (four with 32-bit positions), at most 8192 workgroups
        StreamPlan s;
        CHECK(stream_emit_grid(s, 8191l * 256) == 8191 && stream_emit_grid(s, 8192l * 256) == 8192 && stream_emit_grid(s, 8192l * 256 + 1) == 8192);
        CHECK(stream_emit_grid(s, 1) == 1 && stream_emit_grid(s, 257) == 2);
        s.emit_cpt = 4;
        CHECK(stream_emit_grid(s, 8191l * 1024 + 1) == 8192 && stream_emit_grid(s, 8191l * 1024) == 8191 && stream_emit_grid(s, 129l * 65536) == 8192);
        CHECK(stream_emit_grid(s, (1l << 31) - 1) == 8192);
    }
    {   // the row kernels' grids after the read-back
        g_tuning["assemble_stream"] = 1;
        const StreamPlan one = plan_build(facts("IvA", 65536, 1000)).stream, ep = plan_build(facts("IvE", 65536, 1000, 20)).stream;
        StreamRowsPlan q = plan_stream_rows(one, 1000, 1000, 1000);
        CHECK(q.grid_rows4[0] == 63 && q.grid_rows4[1] == 1 && q.grid_rows1[0] == 250 && q.grid_rows1[1] == 1 && q.avg_cls == 1 && q.rows_R == 4 && q.grid_rowsl == 63);
        q = plan_stream_rows(ep, 500, 1500, 2500);       // three classes per range of the slice, 2.5 of the grid
        CHECK(q.grid_rows4[0] == 125 && q.grid_rows4[1] == 2 && q.grid_rows1[0] == 125 && q.grid_rows1[1] == 5 && q.avg_cls == 3 && q.rows_R == 4 && q.grid_rowsl == 32);
        q = plan_stream_rows(ep, 500, 500 * 20, 1000 * 20);     // every class everywhere: y capped at 16 classes
        CHECK(q.grid_rows4[1] == 4 && q.grid_rows1[1] == 16 && q.avg_cls == 20 && q.rows_R == 1 && q.grid_rowsl == 125);
        q = plan_stream_rows(ep, 0, 0, 0);
        CHECK(q.grid_rows4[0] == 0 && q.grid_rows4[1] == 1 && q.avg_cls == 1 && q.grid_rowsl == 0);
        g_tuning["assemble_stream_rowsl_r"] = 16; CHECK(plan_stream_rows(one, 1000, 1000, 1000).rows_R == 16 && plan_stream_rows(one, 1000, 1000, 1000).grid_rowsl == 16);
        g_tuning["assemble_stream_rowsl_r"] = 99; CHECK(plan_stream_rows(one, 1000, 1000, 1000).rows_R == 16);
        g_tuning["assemble_stream_rowsl_r"] = 0; CHECK(plan_stream_rows(one, 1000, 1000, 1000).rows_R == 1);
        g_tuning.clear();
    }
    {   // fa_range_shape: the four corners of the table, and its override
        CHECK(fa_range_shape(1024l * 512, 512) == 3 && fa_range_shape(1024l * 513, 513) == 1);
        CHECK(fa_range_shape(1024l * 2048, 2048) == 0 && fa_range_shape(1024l * 2047, 2047) == 1 && fa_range_shape(1025l * 2048, 2048) == 1);
        CHECK(fa_range_shape(1025l * 256, 256) == 2 && fa_range_shape(1025l * 257, 257) == 1 && fa_range_shape(1025l * 512, 512) == 1);
        CHECK(fa_range_shape(100, 0) == 3);
        for (int s = 0; s < 4; ++s) {
            g_tuning["assemble_range_shape"] = s;
            const RangePlan p = plan_build(facts("EvI", 100000, 100)).range;
            CHECK(p.shape == s && p.threads == (s == 0 ? 128 : s == 1 ? 256 : 1024) && p.cpt == (s == 0 ? 2 : s == 3 ? 1 : 4));
        }
        for (int s : {-1, 4, 100}) { g_tuning["assemble_range_shape"] = s; CHECK(plan_build(facts("EvI", 100000, 100)).range.shape == 3); }
        g_tuning.clear();
    }
    {   // the other knobs
        BuildFacts f = facts("EvI", 5000, 50);
        CHECK(fast_path_wanted(f));
        g_tuning["assemble_fast"] = 0; CHECK(!fast_path_wanted(f)); g_tuning.clear();
        f.smooth = true; CHECK(!fast_path_wanted(f)); f.shared = true; CHECK(fast_path_wanted(f));
        f.bands_wanted = true; CHECK(!fast_path_wanted(f));
        f = facts("EvI", 5000, 50); f.plan_ok = false;
        CHECK(paths_are(plan_build(f), {PATH_GENERAL}));
        CHECK(!bands_at_build(KEY_E, KEY_I));
        g_tuning["assemble_bands"] = 1;
        CHECK(bands_at_build(KEY_E, KEY_I) && bands_at_build(KEY_E, KEY_X) && !bands_at_build(KEY_A, KEY_I) && !bands_at_build(KEY_I, KEY_E) && !bands_at_build(KEY_E, KEY_A));
        g_tuning.clear();
        CHECK(paths_are(plan_build(facts("EvA", 5000, 50)), {PATH_EVA, PATH_GENERAL}));
        g_tuning["assemble_fast_eva"] = 0; CHECK(paths_are(plan_build(facts("EvA", 5000, 50)), {PATH_GENERAL})); g_tuning.clear();
        CHECK(plan_build(facts("IvE", 5000, 50)).range.static_count && plan_build(facts("IvE", 5000, 50)).range.rowptr == ROWPTR_COUNT_LAUNCH_FRESH_I);
        g_tuning["assemble_static_count"] = 0;
        CHECK(!plan_build(facts("IvE", 5000, 50)).range.static_count && plan_build(facts("IvE", 5000, 50)).range.rowptr == ROWPTR_PELEM_COUNT);
        g_tuning.clear();
        // every knob is read at most once per build
        g_tuning["assemble_stream"] = 1;
        g_reads.clear();
        BuildFacts s = facts("IvE", 5000, 50); s.shared = true; s.world = 2;
        (void)fast_path_wanted(s);
        const BuildPlan b = plan_build(s);
        CHECK(paths_are(b, {PATH_STREAM_SHARED, PATH_STREAM, PATH_RANGE, PATH_GENERAL}));
        (void)plan_stream_rows(b.stream_shared, 25, 60, 120);
        for (const auto &kv : g_reads) CHECK(kv.second == 1);
        CHECK(g_reads.count("assemble_fast") && g_reads.count("assemble_range_shape") && g_reads.count("assemble_stream_wpr"));
        g_tuning.clear();
    }
    {   // the gate: ten matrix names x the state of each set.  P side (I / X): fresh or the identity over the whole extent; G side
        // (A / E): fresh, or -- E columns of an I/X-row matrix only -- pre-populated and no identity; EvA / AvE: both fresh
        const SetState states[4] = {FRESH, IDENT_COMPLETE, IDENT_PARTIAL, PREPOP};
        for (const Spec &sp : SPECS)
            for (SetState rs : states)
                for (SetState cs : states) {
                    const BuildFacts f = facts_in(sp.name, 5000, 50, rs, cs);
                    const BuildPlan b = plan_build(f);
                    bool want;
                    if (sp.family == FAM_EVA) want = rs == FRESH && cs == FRESH;
                    else {
                        const bool g_rows = sp.family == FAM_AEVI;
                        const SetState gs = g_rows ? rs : cs, ps = g_rows ? cs : rs;
                        const bool e_cols = !strcmp(sp.name, "IvE") || !strcmp(sp.name, "XvE");
                        want = (ps == FRESH || ps == IDENT_COMPLETE) && (gs == FRESH || (gs == PREPOP && e_cols));
                        CHECK(b.prepop_table == (gs == PREPOP && e_cols));       // (whatever the P side: fast_prewarm)
                    }
                    CHECK(b.path[b.npath - 1] == PATH_GENERAL);
                    CHECK(want ? paths_are(b, {sp.family == FAM_EVA ? PATH_EVA : PATH_RANGE, PATH_GENERAL}) : paths_are(b, {PATH_GENERAL}));
                    if (want && sp.family != FAM_EVA) check_same(f);
                }
        BuildFacts f = facts("EvA", 5000, 50);
        f.same_set = true;
        CHECK(paths_are(plan_build(f), {PATH_GENERAL}));
        // roles
        const Roles r = plan_build(facts_in("XvE", 5000, 50, IDENT_COMPLETE, PREPOP)).roles;
        CHECK(!r.g_is_row && r.gkey == KEY_E && r.glist == LIST_EP && r.pkey == KEY_X && r.plist == LIST_EP && r.pmode == 0 && !r.g_fresh && r.merge == 0 && r.EP);
        CHECK(r.gext == 200 && r.pext == 5000 && r.g_n == 101);
        const Roles a = plan_build(facts("AvI", 5000, 50)).roles;
        CHECK(a.g_is_row && a.gkey == KEY_A && a.pkey == KEY_I && a.plist == LIST_I && a.pmode == 1 && a.g_fresh && a.merge == 1 && !a.EP);
    }
    {   // the sharded gate: 2 .. 8 ranks, a range for every rank; one rank or no communicator: not shared
        g_tuning["assemble_stream"] = 0;                // (the shared build does not ask the knob)
        for (int world : {1, 2, 8, 9}) {
            BuildFacts f = facts("EvI", 5000, 50);
            f.shared = true; f.world = world;
            CHECK((world >= 2 && world <= 8) ? paths_are(plan_build(f), {PATH_STREAM_SHARED, PATH_RANGE, PATH_GENERAL}) : paths_are(plan_build(f), {PATH_RANGE, PATH_GENERAL}));
            f.shared = false;
            CHECK(paths_are(plan_build(f), {PATH_RANGE, PATH_GENERAL}));
        }
        BuildFacts f = facts("EvI", 5000, 3);
        f.shared = true; f.world = 3; CHECK(plan_build(f).stream_shared.ok);
        f.world = 4; CHECK(!plan_build(f).stream_shared.ok);      // nAr < world
        // the special pieces of the shared build, by the sets
        struct { const char *name; SetState rs, cs; bool by_ice, ident_p, ident_x, ident_i, prepop, pscan; } T[] = {
            {"EvI", FRESH, FRESH, false, false, false, false, false, true},    {"EvI", FRESH, IDENT_COMPLETE, false, true, false, false, false, true},
            {"AvX", FRESH, IDENT_COMPLETE, false, true, false, false, false, true}, {"IvE", IDENT_COMPLETE, FRESH, true, false, false, true, false, true},
            {"IvE", IDENT_COMPLETE, PREPOP, true, false, false, true, true, true}, {"XvE", IDENT_COMPLETE, PREPOP, false, false, true, false, true, false},
            {"XvA", FRESH, FRESH, false, false, false, false, false, true},
        };
        for (const auto &t : T) {
            BuildFacts s = facts_in(t.name, 5000, 50, t.rs, t.cs);
            s.shared = true; s.world = 2;
            const BuildPlan b = plan_build(s);
            const StreamPlan &p = b.stream_shared;
            CHECK(p.ok && p.world == 2 && !b.stream.ok);
            CHECK(p.by_ice == t.by_ice && p.ident_p == t.ident_p && p.ident_x_rows == t.ident_x && p.ident_i_rows == t.ident_i && p.prepop_g == t.prepop && p.pscan == t.pscan);
            g_tuning["assemble_stream"] = 1;
            const StreamPlan u = plan_build(s).stream;           // the same matrix on one GPU: no shared pieces
            CHECK(u.ok && u.world == 1 && u.by_ice == t.by_ice && !u.ident_p && !u.ident_x_rows && !u.ident_i_rows && !u.prepop_g && u.pscan == (t.rs == FRESH || t.cs == FRESH ? (s.family == FAM_AEVI ? t.cs == FRESH : t.rs == FRESH) : false));
            g_tuning["assemble_stream"] = 0;
        }
        g_tuning.clear();
    }
    {   // a sweep of facts: the plan against the builders' own arithmetic (check_same), with its invariants
        const SetState states[4] = {FRESH, IDENT_COMPLETE, IDENT_PARTIAL, PREPOP};
        const long nXs[] = {1, 100, 5000, 65536, NX20 - 1, NX20, NX20 + 1, 8 * NX20};
        const int nArs[] = {1, 50, 256, 257, 512, 513, 2047, 2048, 4096, 4097, 8191, 8192, 32767, 32768, 1 << 20, (1 << 20) + 1};
        const int nmultis[] = {0, 1, 1000, 1 << 20, (1 << 20) + 1};
        const std::map<std::string, int> knobs[] = {{}, {{"assemble_stream_count", 1}}, {{"assemble_stream_count", 0}}, {{"assemble_static_count", 0}},
                                                    {{"assemble_range_shape", 0}}, {{"assemble_range_shape", 2}}};
        long n = 0;
        for (const auto &k : knobs) {
            g_tuning = k;
            for (int si = 0; si < 8; ++si)
                for (long nX : nXs)
                    for (int nAr : nArs)
                        for (int nhc : {1, 4, 8, 64})
                            for (SetState ps : {FRESH, IDENT_COMPLETE})
                                for (SetState gs : states) {
                                    if (nAr > nX) continue;
                                    const bool g_rows = SPECS[si].family == FAM_AEVI;
                                    BuildFacts f = facts_in(SPECS[si].name, nX, nAr, g_rows ? gs : ps, g_rows ? ps : gs, nhc);
                                    f.nmulti = nmultis[n % 5];
                                    f.nI = nX - nX / 3; f.set[g_rows ? 1 : 0].extent = extent_of(g_rows ? f.col_key : f.row_key, nX, f.nI, nAr, nhc);
                                    set_state(f.set[g_rows ? 1 : 0], ps);
                                    f.icnt_pos = n % 7 != 0;
                                    if (!plan_build(f).tries(PATH_RANGE)) continue;
                                    check_same(f);
                                    ++n;
                                }
        }
        g_tuning.clear();
        printf("sweep: %ld builds\n", n);
        CHECK(n > 20000);
    }
    {   // nX = 2^31 - 1, nAr = 2^24: nothing overflows
        const long NX = (1l << 31) - 1;
        for (const char *name : {"AvI", "EvI", "IvA", "IvE", "XvE", "EvX"}) {
            BuildFacts f = facts(name, NX, 1 << 24, 64);
            f.nmulti = INT_MAX; f.maxrange = INT_MAX;
            const BuildPlan b = plan_build(f);
            CHECK(paths_are(b, {PATH_STREAM, PATH_RANGE, PATH_GENERAL}));
            const bool E = b.roles.gkey == KEY_E;
            CHECK(b.range.nrc == (E ? 1l << 30 : 1l << 24) && b.range.ng_ub == b.range.nrc && b.range.nnz_ub == (b.roles.EP ? 2 : 1) * NX);
            CHECK(b.range.np_ub == NX && !b.range.optimistic && !b.range.chained && b.range.scan == SCAN_DEVICE_WIDE && b.range.shape == 0);
            CHECK(b.range.sums == (b.roles.g_is_row && b.roles.pkey == KEY_I ? SUMS_PELEM : SUMS_NONE) && b.range.nstatus == 0 && b.range.count_extra == 0);
            CHECK(b.stream.rel32 && b.stream.emit_cpt == 4 && b.stream.oldseg == 128 && stream_emit_grid(b.stream, NX) == 8192);
            const StreamRowsPlan q = plan_stream_rows(b.stream, 1 << 24, UINT_MAX, (uint64_t)UINT_MAX);
            CHECK(q.grid_rows1[0] == (1u << 22) && q.grid_rows1[1] == (E ? 16u : 1u) && q.avg_cls == (E ? 256 : 1) && q.rows_R == (E ? 1 : 4));
            check_same(f);
        }
        // the optimistic bounds at their largest: 2^20 cells, an identity ice set of 2^31 - 1 cells
        BuildFacts f = facts_in("EvI", NX20, 100, FRESH, IDENT_COMPLETE, 64);
        f.set[1].extent = f.set[1].n = INT_MAX;
        const RangePlan p = plan_build(f).range;
        CHECK(p.clears == CLEAR_MW_P && p.nclear == 2l * INT_MAX && p.nclear <= (long)UINT_MAX && p.np_ub == INT_MAX);
        check_same(f);
    }
    if (g_failed) { printf("%d checks FAILED\n", g_failed); return 1; }
    printf("all checks passed\n");
    return 0;
}
