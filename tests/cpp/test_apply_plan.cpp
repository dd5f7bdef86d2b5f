// The launch choice (icebin_amd/csrc/apply_plan.h) at the thresholds no small GPU matrix reaches: hand-written MatrixFacts on
// either side of 2^24 entries, 2^23 and 2^19 rows, the column sweep's 32-bit offset limit, the capture clamp of the shortrow
// batches and the scratch element counts.  Host code only: its own get_tuning, no HIP.
#include "../../icebin_amd/csrc/apply_plan.h"

#include <cstdio>
#include <cstring>
#include <map>
#include <string>

static std::map<std::string, int> g_tuning;
int ibh::get_tuning(const char *key, int dflt) {
    auto it = g_tuning.find(key);
    return it == g_tuning.end() ? dflt : it->second;
}

using namespace ibh;
static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++g_failed; } } while (0)

static MatrixFacts e_rows(int64_t nnz) {        // an E-row matrix with every structure built
    MatrixFacts f;
    f.nrow = 20480; f.ncol = 1 << 23; f.nnz = nnz; f.band_eligible = true;
    f.groups_built = f.tiles_built = f.sweep_built = true;
    f.groups_n = 4000; f.groups_nslot = 12; f.tiles_seg = 256; f.sweep_ntask = 1000; f.sweep_nprow = 50000; f.sweep_nslot = 40;
    return f;
}
static MatrixFacts one_entry(int nrow) {        // an I-row matrix of one entry per row
    MatrixFacts f;
    f.nrow = nrow; f.ncol = 20000; f.nnz = nrow;
    return f;
}
static const char *sig(const ApplyPlan &p) { return p.inst >= 0 ? INSTS[p.table].v[p.inst].sig : "none"; }

int main() {
    const int64_t HUGE = 1l << 24;
    {   // the lists: 128 instantiations, spelled as the code object spells them
        int n = 0;
        for (int t = 0; t < T_COUNT; ++t) n += INSTS[t].n;
        CHECK(n == 128);
        CHECK(!strcmp(INSTS[T_ROWBLOCK].v[find_inst(T_ROWBLOCK, 1, 1, 14, 8, 0)].sig, "spmm_rowblock_kernel<1, 1, 14, 8, false>"));
        CHECK(!strcmp(INSTS[T_SWEEP].v[find_inst(T_SWEEP, 1, 0)].sig, "spmm_sweep_kernel<true, false, 0>"));
        CHECK(find_inst(T_ROWBLOCK, 8, 2, 1, 4, 0) < 0);
    }
    {   // tiles_win: batched launches of few fields leave the sweep for the tiled row groups from 2^24 entries on
        ApplyPlan lo = plan_apply(e_rows(HUGE - 1), 16, 4, false), hi = plan_apply(e_rows(HUGE), 16, 4, false);
        CHECK(lo.family == KERNEL_COLSWEEP && lo.table == T_SWEEP);
        CHECK(hi.family == KERNEL_ROWGROUP && hi.table == T_GROUPTILE);
        CHECK(!strcmp(sig(hi), "spmm_grouptile_kernel<16, 16, 256, 8, false>"));
        g_tuning["rowgroup_form"] = 0;
        CHECK(plan_apply(e_rows(HUGE), 16, 4, false).family == KERNEL_COLSWEEP);
        g_tuning.clear();
    }
    {   // use_grouptile: below 48 fields the tiles serve from 2^24 entries on (from 2^21 with >= 48 fields)
        MatrixFacts lo = e_rows(HUGE - 1), hi = e_rows(HUGE);
        lo.sweep_built = hi.sweep_built = false;
        CHECK(plan_apply(lo, 32, 1, false).table == T_ROWGROUP && plan_apply(hi, 32, 1, false).table == T_GROUPTILE);
        CHECK(!strcmp(sig(plan_apply(lo, 32, 1, false)), "spmm_rowgroup_kernel<8, 8, 64, false>"));
        CHECK(plan_apply(lo, 48, 1, false).table == T_GROUPTILE && plan_apply(lo, 47, 1, false).table == T_ROWGROUP);
        lo.nnz = (1 << 21) - 1;
        CHECK(plan_apply(lo, 48, 1, false).table == T_ROWGROUP);
        CHECK(plan_apply(hi, 32, 1, true).table == T_GROUPTILE && plan_apply(hi, 32, 1, true).grid[1] == 1);
    }
    {   // huge && nvar >= 128: one launch of a long-row matrix that is no E-row matrix takes the sweep
        MatrixFacts lo = e_rows(HUGE - 1), hi = e_rows(HUGE);
        lo.band_eligible = hi.band_eligible = lo.groups_built = hi.groups_built = lo.tiles_built = hi.tiles_built = false;
        CHECK(plan_apply(lo, 128, 1, false).family == KERNEL_ROWBLOCK);
        CHECK(plan_apply(hi, 128, 1, false).family == KERNEL_COLSWEEP);
        CHECK(plan_apply(hi, 127, 1, false).family == KERNEL_ROWBLOCK);
        CHECK(plan_apply(lo, 127, 4, false).family == KERNEL_COLSWEEP);        // (batched: sweep_min_batch)
        // the structure is asked for by the same rule
        lo.sweep_built = hi.sweep_built = false;
        lo.nnz = 2l * lo.ncol - 1; hi.nnz = 2l * hi.ncol;
        CHECK(!wants_sweep(lo, 128, 1, true) && wants_sweep(hi, 128, 1, true) && !wants_sweep(hi, 127, 1, true) && !wants_sweep(hi, 128, 1, false));
        MatrixFacts e = e_rows(HUGE - 1);
        e.groups_built = e.tiles_built = e.sweep_built = false;
        CHECK(!wants_groups(e, 16, 1, 1, false));
        e.nnz = HUGE;
        CHECK(wants_groups(e, 16, 1, 1, false) && !wants_groups(e, 16, 4, 1, false) && wants_groups(e, 32, 4, 1, false) && !wants_groups(e, 16, 1, 0, false));
    }
    {   // 2^23 rows: 32 fields per thread from 96 fields, groups of 4
        ApplyPlan lo = plan_apply(one_entry((1 << 23) - 1), 96, 1, false), hi = plan_apply(one_entry(1 << 23), 96, 1, false);
        CHECK(lo.family == KERNEL_SHORTROW && lo.fper == 16 && lo.g == 8 && hi.fper == 32 && hi.g == 4);
        CHECK(plan_apply(one_entry(1 << 23), 95, 1, false).fper == 16 && plan_apply(one_entry(1 << 23), 95, 1, false).g == 4);
        CHECK(!strcmp(sig(hi), "spmm_shortrow_kernel<true, 4, false, true>") && !strcmp(sig(lo), "spmm_shortrow_kernel<true, 8, false, true>"));
    }
    {   // 2^19 rows: big -- 16 fields per thread, the transposed input, one batch per launch
        ApplyPlan lo = plan_apply(one_entry((1 << 19) - 1), 16, 8, false), hi = plan_apply(one_entry(1 << 19), 16, 8, false);
        CHECK(lo.fper == 8 && lo.per_launch == IBH_MAX_BATCH && lo.use_xt == 1 && lo.grid[1] == 8);
        CHECK(hi.fper == 16 && hi.g == 8 && hi.per_launch == 1 && hi.use_xt == 1 && hi.grid[1] == 1);
        CHECK(plan_apply(one_entry((1 << 19) - 1), 16, 1, false).use_xt == 0 && plan_apply(one_entry(1 << 19), 16, 1, false).use_xt == 1);
        CHECK(hi.xt == (size_t)20000 * 16 * 1 && lo.xt == (size_t)20000 * 16 * 8);
        CHECK(hi.grid[0] == (unsigned)((1 << 19) / 256));
        // re-aligned result planes from 2^18 rows on, in steps of 248 rows
        ApplyPlan a = plan_apply(one_entry(1 << 18), 4, 1, false), b = plan_apply(one_entry((1 << 18) - 1), 4, 1, false);
        align_shortrow(a, one_entry(1 << 18), 4, true, 1);
        align_shortrow(b, one_entry((1 << 18) - 1), 4, true, 1);
        CHECK(a.realign == 1 && a.grid[0] == (unsigned)(((1 << 18) + 247) / 248) && b.realign == 0 && b.grid[0] == 1024u);
        CHECK(!strcmp(sig(a), "spmm_shortrow_kernel<true, 4, true, false>"));
    }
    {   // the sweep's 32-bit offsets: 16 * lda * 8 + ncol * 8 < 2^32, else the bands, else the rows
        MatrixFacts f = e_rows(1 << 22);
        f.kernel_override = KERNEL_COLSWEEP;
        f.ncol = 31580641;      // 136 * ncol = 2^32 - 120
        CHECK(plan_apply(f, 64, 1, false).family == KERNEL_COLSWEEP);
        CHECK(plan_apply(f, 64, 1, false, f.ncol + 1).family == KERNEL_ROWBLOCK);      // (128 more bytes through lda)
        f.ncol = 31580642;
        CHECK(plan_apply(f, 64, 1, false).family == KERNEL_ROWBLOCK && plan_apply(f, 64, 1, false).table == T_ROWONE);
        f.bands_built = true; f.bands_n = f.nnz / 2;
        ApplyPlan p = plan_apply(f, 64, 1, false);
        CHECK(p.family == KERNEL_ROWDUAL && p.table == T_ROWDUAL && p.band_part == (size_t)2 * 64 * 20480);
    }
    {   // a captured stream: as many batches per launch as the transposed-input scratch holds
        MatrixFacts f = one_entry(50000);
        f.nnz = 3 * f.nrow; f.ncol = 1000;
        ApplyPlan p = plan_apply(f, 16, 8, false);
        CHECK(p.use_xt == 1 && p.fper == 32 && p.g == 8 && p.ldt == 16 && p.per_launch == 32 && p.xt == (size_t)1000 * 16 * 8);
        ApplyPlan q = p;
        clamp_shortrow(q, f, 8, 8 * 128000);
        CHECK(q.per_launch == 32 && q.xt == p.xt);      // (fits: nothing to clamp)
        clamp_shortrow(q, f, 8, 3 * 128000 + 5);
        CHECK(q.per_launch == 3 && q.xt == (size_t)1000 * 16 * 3);
        q = p;
        clamp_shortrow(q, f, 8, 10);
        CHECK(q.per_launch == 1 && q.xt == (size_t)1000 * 16);
    }
    {   // scratch element counts (Bands::part_count, Sweep::part_count, ncol * ldt * batches per launch)
        MatrixFacts f = e_rows(1 << 22);
        f.kernel_override = KERNEL_COLSWEEP;
        CHECK(plan_apply(f, 40, 3, false).sweep_part == (size_t)3 * 50000 * 64);
        CHECK(plan_apply(f, 130, 3, false).sweep_part == (size_t)3 * 50000 * 192);
        CHECK(plan_apply(f, 16, 5, false).sweep_part == (size_t)2 * 50000 * 64);       // (4 batches share a slice of 64 lanes)
        CHECK(plan_apply(f, 16, 5, false).grid[2] == 2 && plan_apply(f, 130, 3, false).grid[1] == 3);
        f.kernel_override = KERNEL_ROWDUAL; f.nrow = 40001; f.bands_built = true; f.bands_n = 1 << 21;
        CHECK(plan_apply(f, 7, 5, false).band_part == (size_t)2 * 5 * 7 * 40064);
        CHECK(plan_apply(f, 7, 5, false).sweep_part == 0 && plan_apply(f, 7, 5, false).xt == 0);
        MatrixFacts s = one_entry(100000);
        s.nnz = 3 * s.nrow;
        CHECK(plan_apply(s, 33, 40, false).xt == (size_t)20000 * 48 * 32);              // (launches of <= IBH_MAX_BATCH)
        g_tuning["shortrow_many"] = 5;
        CHECK(plan_apply(s, 33, 40, false).xt == (size_t)20000 * 48 * 5);
        g_tuning.clear();
    }
    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("all checks passed\n");
    return 0;
}
