// globalave.hip -- GCMRegridder_ModelE::global_AvE (slib/icebin/modele/GCMRegridder_ModelE.cpp:579-628) in its three library
// functions: compute_EOpvAOp_merged and squash_ECs (modele/merge_topo.cpp:375-527) and _compute_AAmvEAm_EIGEN
// (modele/topo.cpp:242-347); DESIGN.md 16.
//
// Where things live.  The merge keeps every index and value of every matrix in HBM: a sheet's EvA is visited by columns
// through transpose_csr and an emit kernel that writes 64-bit SPARSE keys from the two device to_sparse tables, the base
// matrix is uploaded once and shifted by offsetE there, and the first-seen numbering of the two key streams runs on the
// device as well (sparseset.h number_stream).  The composition behind it is
// modele_parts.h's (the keys of the GCM-grid-sized sets on the host) followed by two sparse products with the
// diagonal scalings between them, each operand rounded before it is used.
#include <algorithm>
#include <cmath>
#include <memory>

#include "assemble.h"
#include "common.h"
#include "csrbuild.h"
#include "csrops.h"
#include "modele_parts.h"
#include "prims.h"
#include "sparseset.h"

namespace ibh {
namespace {

constexpr int16_t UI_LOCALICE = 1, UI_GLOBALICE = 2;        // modele/grids.hpp:44-46

// ---- the merge's streams ------------------------------------------------------------------------------------------------------
// T = a sheet's EvA transposed: row c of T is column c of EvA with its rows ascending, so T's entries in storage order are
// begin(M)...end(M) of the column-major matrix.  One thread per column (an O cell: at most nhc entries).
__global__ void k_ga_emit_sheet(Csr T, const int64_t *__restrict__ tsE, const int64_t *__restrict__ tsA, int64_t *__restrict__ keyE,
                                int64_t *__restrict__ keyA, double *__restrict__ val) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= T.nrow) return;
    const int64_t a = tsA[c];
    for (int e = T.rowptr[c]; e < T.rowptr[c + 1]; ++e) { keyE[e] = tsE[T.colind[e]]; keyA[e] = a; val[e] = T.val[e]; }
}
__global__ void k_ga_add_offset(int64_t *__restrict__ key, long n, int64_t offset) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) key[i] = key[i] + offset;
}
// squash_ECs (:507-519): T = EOpvAOp0 transposed (the column-major visit).  A row key splits through the strides of
// indexingHC0 into (iO, ihc0) and becomes indexingHC1(iO, to_new[ihc0]); the column stays dense.  64-bit throughout (the
// reference computes these in int).  An ihc0 outside [0, nhc0) gives key -1, which number_stream refuses.
__global__ void k_ga_squash(Csr T, const int64_t *__restrict__ tsE0, HcIndexing s0, int32_t nhc0, const int32_t *__restrict__ to_new,
                            HcIndexing s1, int64_t *__restrict__ keyE, int32_t *__restrict__ col, double *__restrict__ val) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= T.nrow) return;
    for (int e = T.rowptr[c]; e < T.rowptr[c + 1]; ++e) {
        const int64_t k = tsE0[T.colind[e]];
        int64_t iO, ihc;
        s0.split(k, iO, ihc);
        keyE[e] = ihc >= 0 && ihc < nhc0 ? s1.index(iO, to_new[ihc]) : -1;
        col[e] = c; val[e] = T.val[e];
    }
}

struct MergeOut {
    int64_t offsetE = 0;
    HcIndexing hc{1, 0};
    std::vector<double> hcdefs;
    std::vector<int16_t> underice;
};

void merge_EOpvAOp(const ibh_regrid_matrices *const *rmOs, int nsheets, int64_t nO, int64_t base_nE, int64_t base_nO, int64_t base_nnz,
                   const int64_t *base_iE, const int64_t *base_iO, const double *base_val, const double *hcdefs_base, int32_t nhc_base,
                   HcIndexing sbase, bool use_global, bool use_local, bool squash, ibh_sparse_set *dimAOp, ibh_sparse_set *dimEOp,
                   ibh_weighted **out, MergeOut &mo) {
    hipStream_t st = hipStreamPerThread;
    const int T = 256;
    require_device();
    IBH_CHECK(nsheets >= 0 && nO > 0 && (nsheets == 0 || rmOs), "merge_EOpvAOp: bad arguments");
    IBH_CHECK(sbase.sA > 0 && sbase.sHC > 0, "merge_EOpvAOp: indexingHC strides (%ld,%ld) must be positive", (long)sbase.sA, (long)sbase.sHC);
    IBH_CHECK(dimEOp == nullptr || (dimEOp->n() == 0 && dimEOp != dimAOp), "merge_EOpvAOp: dimEOp must be a fresh set of its own");
    int32_t nhc_local = 0;
    const ibh_regridder *rg0 = nullptr;
    for (int k = 0; k < nsheets; ++k) {
        IBH_CHECK(rmOs[k] && rmOs[k]->rg, "merge_EOpvAOp: sheet %d is null", k);
        const ibh_regridder *rg = rmOs[k]->rg;
        check_current_device(rg->device, "regridder");
        IBH_CHECK(rg->nA == nO, "merge_EOpvAOp: sheet %d lives on an ocean grid of %lld cells, nO=%lld", k, (long long)rg->nA, (long long)nO);
        if (!rg0) rg0 = rg;
        IBH_CHECK(rg->nhc == rg0->nhc && rg->hc_stride_A == rg0->hc_stride_A && rg->hc_stride_HC == rg0->hc_stride_HC,
                  "merge_EOpvAOp: sheet %d has nhc=%d and indexingHC strides (%ld,%ld), sheet 0 nhc=%d and (%ld,%ld)", k, rg->nhc,
                  (long)rg->hc_stride_A, (long)rg->hc_stride_HC, rg0->nhc, (long)rg0->hc_stride_A, (long)rg0->hc_stride_HC);
        if (rmOs[k]->sigma[0] != 0) fail(IBH_EINVAL, "merge_EOpvAOp: sheet %d has a non-zero sigma", k);
    }
    if (rg0) nhc_local = rg0->nhc;
    if (use_global) {
        IBH_CHECK(base_nE >= 0 && base_nO >= 0 && base_nnz >= 0 && nhc_base >= 0, "merge_EOpvAOp: negative base shape");
        IBH_CHECK(base_nO == nO, "merge_EOpvAOp: the base matrix has %lld O cells, nO=%lld", (long long)base_nO, (long long)nO);
        IBH_CHECK(base_nnz == 0 || (base_iE && base_iO && base_val), "merge_EOpvAOp: null base arrays");
        IBH_CHECK(nhc_base == 0 || hcdefs_base, "merge_EOpvAOp: null hcdefs_base");
        for (int64_t p = 0; p < base_nnz; ++p)
            IBH_CHECK(base_iE[p] >= 0 && base_iE[p] < base_nE && base_iO[p] >= 0 && base_iO[p] < base_nO,
                      "merge_EOpvAOp: base entry %lld = (%lld, %lld) lies outside the shape (%lld, %lld)", (long long)p, (long long)base_iE[p],
                      (long long)base_iO[p], (long long)base_nE, (long long)base_nO);
    } else {
        base_nnz = 0;
    }
    // (:403, :434) and the decision of DESIGN.md 16: without global ice the extents are the local grid's, not 0
    mo.offsetE = use_global ? nO * nhc_local : 0;
    const int64_t extentE = use_global ? mo.offsetE + base_nE : nO * nhc_local, extentA = use_global ? base_nO : nO;
    if (use_local && rg0) {
        mo.hcdefs.insert(mo.hcdefs.end(), rg0->hcdefs_h.begin(), rg0->hcdefs_h.end());
        mo.underice.insert(mo.underice.end(), (size_t)nhc_local, UI_LOCALICE);
    }
    if (use_global) {
        mo.hcdefs.insert(mo.hcdefs.end(), hcdefs_base, hcdefs_base + nhc_base);
        mo.underice.insert(mo.underice.end(), (size_t)nhc_base, UI_GLOBALICE);
    }
    const int32_t nhc0 = (int32_t)mo.hcdefs.size();
    const HcIndexing s0 = sbase.with_nhc(nhc0);
    if (dimAOp) { dimAOp->check_extent(extentA, "merge_EOpvAOp: dimAOp"); dimAOp->check_entries_within(extentA, "dimAOp"); }
    // squash_ECs (:481-495): the sorted distinct elevations and the old class -> new class map
    std::vector<double> hc1(mo.hcdefs);
    std::sort(hc1.begin(), hc1.end());
    hc1.erase(std::unique(hc1.begin(), hc1.end()), hc1.end());
    std::vector<int32_t> to_new;
    for (double h : mo.hcdefs) to_new.push_back((int32_t)(std::lower_bound(hc1.begin(), hc1.end(), h) - hc1.begin()));
    const int32_t nhc1 = (int32_t)hc1.size();
    if (dimEOp) dimEOp->check_extent(squash ? extentA * nhc1 : extentE, "merge_EOpvAOp: dimEOp");

    // the sheets' EvA (scale = false, correctA = false, sigma = 0, fresh sets), in index order
    struct Sheet { ibh_sparse_set dE, dA; std::unique_ptr<ibh_weighted> EvA; };
    std::vector<Sheet> sheets((size_t)(use_local ? nsheets : 0));
    int64_t total = base_nnz;
    const double zero[3] = {0, 0, 0};
    for (size_t k = 0; k < sheets.size(); ++k) {
        ibh_weighted *w = nullptr;
        assemble_matrix(rmOs[k], "EvA", &sheets[k].dE, &sheets[k].dA, 0, 0, zero, &w);
        sheets[k].EvA.reset(w);
        total += w->nnz;
    }
    IBH_CHECK(total < (1ll << 31), "merge_EOpvAOp: %lld entries overflow int32", (long long)total);
    DevBuf<int64_t> keyE((size_t)total), keyA((size_t)total);
    DevBuf<double> val((size_t)total);
    DevBuf<int32_t> drow((size_t)total), dcol((size_t)total);
    int64_t off = 0;
    for (Sheet &sh : sheets) {
        const ibh_weighted &M = *sh.EvA;
        if (!M.nnz) continue;
        ibh_weighted Tm;
        transpose_csr(M, &Tm, st);          // (resets the arena)
        const int64_t *tsE = sh.dE.device_to_sparse(M.nrow, st), *tsA = sh.dA.device_to_sparse(M.ncol, st);
        hipLaunchKernelGGL(k_ga_emit_sheet, dim3(ceil_div(Tm.nrow, T)), dim3(T), 0, st, view(Tm), tsE, tsA, keyE.p + off, keyA.p + off, val.p + off);
        IBH_HIP(hipGetLastError());
        IBH_HIP(hipStreamSynchronize(st));  // Tm goes away
        off += M.nnz;
    }
    if (base_nnz) {
        IBH_HIP(hipMemcpyAsync(keyE.p + off, base_iE, sizeof(int64_t) * (size_t)base_nnz, hipMemcpyHostToDevice, st));
        IBH_HIP(hipMemcpyAsync(keyA.p + off, base_iO, sizeof(int64_t) * (size_t)base_nnz, hipMemcpyHostToDevice, st));
        IBH_HIP(hipMemcpyAsync(val.p + off, base_val, sizeof(double) * (size_t)base_nnz, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_ga_add_offset, dim3(ceil_div(base_nnz, T)), dim3(T), 0, st, keyE.p + off, (long)base_nnz, mo.offsetE);
        IBH_HIP(hipGetLastError());
    }
    sheets.clear();

    // {ADD_DENSE, ADD_DENSE} over {dimEOp (fresh), dimAOp (the caller's)}, then setFromTriplets with the weights (a stream
    // without entries gives the empty matrix over the sets as they are)
    WorkingSet wA(dimAOp), wE(dimEOp);
    ibh_sparse_set dimEOp0;                 // the unsquashed rows, when squash_ECs follows
    ibh_sparse_set &setE0 = squash ? dimEOp0 : *wE;
    arena().reset();
    number_stream(setE0, extentE, keyE.p, (long)total, drow.p, "merge_EOpvAOp: rows", st);
    number_stream(*wA, extentA, keyA.p, (long)total, dcol.p, "merge_EOpvAOp: columns", st);
    auto w = new_weighted();
    weighted_from_device_triplets(w.get(), setE0.n(), wA->n(), total, drow.p, dcol.p, val.p, st);
    mo.hc = s0;
    if (squash) {
        // squash_ECs (:497-523)
        const HcIndexing s1 = s0.with_nhc(nhc1);
        const int64_t nnz0 = w->nnz;
        DevBuf<int32_t> d_to_new;
        d_to_new.upload(to_new.data(), to_new.size(), st);
        auto w1 = new_weighted();
        if (nnz0) {
            ibh_weighted Tm;
            transpose_csr(*w, &Tm, st);
            const int64_t *tsE0 = dimEOp0.device_to_sparse(w->nrow, st);
            hipLaunchKernelGGL(k_ga_squash, dim3(ceil_div(Tm.nrow, T)), dim3(T), 0, st, view(Tm), tsE0, s0, nhc0, d_to_new.p, s1, keyE.p, dcol.p,
                               val.p);
            IBH_HIP(hipGetLastError());
            IBH_HIP(hipStreamSynchronize(st));
        }
        arena().reset();
        number_stream(*wE, extentA * nhc1, keyE.p, (long)nnz0, drow.p, "squash_ECs: rows", st);
        weighted_from_device_triplets(w1.get(), wE->n(), wA->n(), nnz0, drow.p, dcol.p, val.p, st);
        w = std::move(w1);
        mo.hcdefs = hc1;
        mo.underice.assign((size_t)nhc1, UI_GLOBALICE);
        mo.hc = s1;
    }
    w->conservative = 0; w->scaled = 0;
    IBH_HIP(hipStreamSynchronize(st));      // the caller's base arrays are free
    w->dims[0] = wE.commit();
    w->dims[1] = wA.commit();
    *out = w.release();
}

void check_set(const ibh_sparse_set *s, int64_t extent, const char *which) {
    if (!s) return;
    s->check_extent(extent, (std::string("AAmvEAm: ") + which).c_str());
    s->check_entries_within(extent, which);
}

// _compute_AAmvEAm_EIGEN (topo.cpp:242-347)
void compute_AAmvEAm(const ibh_weighted *EOpvAOp, const ibh_sparse_set *dimEOp, const ibh_sparse_set *dimAOp, int32_t imO, int32_t jmO,
                     double offiO, double dlatO, double eq_rad, int32_t nhc, int64_t sA_O, int64_t sHC_O, int64_t sA_A, int64_t sHC_A,
                     const double *foceanAOp, const double *foceanAOm, int64_t nO, int scale, ibh_sparse_set *dimAAm, ibh_sparse_set *dimEAm,
                     ibh_weighted **out) {
    hipStream_t st = hipStreamPerThread;
    IBH_CHECK(EOpvAOp && dimEOp && dimAOp && foceanAOp && foceanAOm && out, "null argument");
    check_current_device(EOpvAOp->device, "EOpvAOp");
    IBH_CHECK(imO > 0 && jmO > 0 && imO % 2 == 0 && jmO % 2 == 0,
              "Ocean grid must have even number of gridcells for im and jm (vs. %d %d)", imO, jmO);
    IBH_CHECK((int64_t)imO * jmO == nO, "the ocean HntrSpec has %lld cells, the focean arrays %lld", (long long)imO * jmO, (long long)nO);
    IBH_CHECK(nhc >= 0 && sA_O >= 0 && sHC_O >= 0 && sA_A >= 0 && sHC_A >= 0, "AAmvEAm: negative nhc or indexingHC stride");
    IBH_CHECK(EOpvAOp->nrow == dimEOp->n() && EOpvAOp->ncol == dimAOp->n(), "AAmvEAm: EOpvAOp is %d x %d, its sets hold %d and %d entries",
              EOpvAOp->nrow, EOpvAOp->ncol, dimEOp->n(), dimAOp->n());
    IBH_CHECK(dimAAm == nullptr || dimAAm != dimEAm, "dims[0] and dims[1] must be distinct sets");
    const int64_t nA = (int64_t)(imO / 2) * (jmO / 2);
    {
        const int64_t *ts = dimAOp->to_sparse_host();
        for (int d = 0; d < dimAOp->n(); ++d)
            IBH_CHECK(ts[d] >= 0 && ts[d] < nO, "AAmvEAm: dimAOp entry %lld outside the ocean grid of %lld cells", (long long)ts[d], (long long)nO);
    }
    check_set(dimAAm, nA, "dimAAm");
    check_set(dimEAm, nA * nhc, "dimEAm");
    ibh_hntr *hraw = nullptr;               // Hntr(17.17, hntrO, hntrA): B = O, A = make_hntrA(O) (hntr.cpp:232-241)
    rethrow(ibh_hntr_create(&hraw, imO / 2, jmO / 2, offiO * 0.5, dlatO * 2., imO, jmO, offiO, dlatO, 0.));
    std::unique_ptr<ibh_hntr, int (*)(ibh_hntr *)> hntr(hraw, ibh_hntr_destroy);

    WorkingSet work[2] = {WorkingSet(dimAAm), WorkingSet(dimEAm)};
    work[0]->set_sparse_extent(nA);
    work[1]->set_sparse_extent(nA * nhc);

    // wAOm (from wAOp = sum(EOpvAOp, 1, '+') = the matrix's Mw) and dimAOm (:277-279)
    ibh_sparse_set dimAOm, dimEOm;
    DevBuf<double> wAOm;
    std::vector<int32_t> aop2aom;
    compute_wAOm(foceanAOp, foceanAOm, nO, EOpvAOp->Mw.p, *dimAOp, dimAOm, aop2aom, wAOm, st);
    const int nAOm = dimAOm.n();
    std::vector<uint8_t> includeO((size_t)nO, 0);           // DimClip(&dimAOm)
    for (int k = 0; k < nAOm; ++k) includeO[(size_t)dimAOm.to_sparse_host()[k]] = 1;

    // AAmvAOm (:286-295), built by its columns: AOmvAAm by rows, numbering dimAAm in stream order
    std::unique_ptr<ibh_weighted> AOmvAAm;
    {
        ibh_weighted *h = nullptr;
        rethrow(ibh_hntr_matrix_d(hntr.get(), IBH_HNTR_OVERLAP, eq_rad, includeO.data(), &dimAOm, IBH_TO_DENSE_IGNORE_MISSING, work[0].get(),
                                  IBH_ADD_DENSE, 0, &h));
        AOmvAAm.reset(h);
    }
    const int nAAm = work[0]->n();
    IBH_CHECK(AOmvAAm->nrow == nAOm && AOmvAAm->ncol == nAAm, "internal: AOmvAAm shape disagrees with its sets");
    DevBuf<double> AAmvAOms, sAAmvAOm, wAAm, wEAm, lead;
    recip(AOmvAAm->wM.p, nAOm, AAmvAOms, st);               // sum(AAmvAOm, 1, '-')
    recip(AOmvAAm->Mw.p, nAAm, sAAmvAOm, st);               // sum(AAmvAOm, 0, '-')
    ibh_weighted AAmvAOm;
    transpose_csr(*AOmvAAm, &AAmvAOm, st);
    wAAm.alloc((size_t)nAAm);
    scaled_matvec(AAmvAOm, AAmvAOms.p, wAOm.p, wAAm.p, st);

    // EOmvAOm, its inverted column sums and wEOm from the GIVEN EOpvAOp (:298-306)
    ibh_weighted EOmvAOm;
    DevBuf<double> EOmvAOms, wEOm;
    std::vector<double> wEOm_h;
    compute_EOmvAOm_unscaled(*EOpvAOp, *dimEOp, *dimAOp, dimAOm, wAOm, dimEOp->sparse_extent(), dimEOm, &EOmvAOm, &EOmvAOms, wEOm, wEOm_h, st);
    const int nEOm = dimEOm.n();

    // EOmvEAm numbers dimEAm (:309-315); wEAm (:320-323)
    auto EOmvEAm = raw_EOvEA(hntr.get(), eq_rad, includeO, dimEOm, wEOm, wEOm_h, nhc, HcIndexing{sA_O, sHC_O}, HcIndexing{sA_A, sHC_A}, *work[1], st);
    const int nEAm = work[1]->n();
    IBH_CHECK(EOmvEAm->nrow == nEOm && EOmvEAm->ncol == nEAm && EOmvAOm.nrow == nEOm && EOmvAOm.ncol == nAOm,
              "internal: AAmvEAm matrix shapes disagree");
    DevBuf<double> EAmvEOms;
    recip(EOmvEAm->wM.p, nEOm, EAmvEOms, st);               // sum(EOmvEAm, 0, '-')
    ibh_weighted EAmvEOm;
    transpose_csr(*EOmvEAm, &EAmvEOm, st);
    wEAm.alloc((size_t)nEAm);
    scaled_matvec(EAmvEOm, EAmvEOms.p, wEOm.p, wEAm.p, st);

    // M = diag(lead) * AAmvAOm * diag(EOmvAOms) * AOmvEOm * diag(EAmvEOms) * EOmvEAm (:329-342), left-associated, each operand
    // rounded before it is used: X1 = diag(lead) * AAmvAOm, X2 = X1 * diag(EOmvAOms), P1 = X2 * AOmvEOm, P2 = P1 * diag(EAmvEOms)
    const double *ls = sAAmvAOm.p;
    if (!scale) {
        lead.alloc((size_t)nAAm);
        mul(wAAm.p, sAAmvAOm.p, nAAm, lead.p, st);
        ls = lead.p;
    }
    scale_rows(AAmvAOm.rowptr.p, nAAm, ls, AAmvAOm.val.p, st);
    scale_cols(AAmvAOm.colind.p, AAmvAOm.nnz, EOmvAOms.p, AAmvAOm.val.p, st);
    IBH_HIP(hipGetLastError());
    ibh_weighted AOmvEOm, P1;
    transpose_csr(EOmvAOm, &AOmvEOm, st);
    csr_product(AAmvAOm, AOmvEOm, &P1, st);
    scale_cols(P1.colind.p, P1.nnz, EAmvEOms.p, P1.val.p, st);
    IBH_HIP(hipGetLastError());
    auto w = new_weighted();
    csr_product(P1, *EOmvEAm, w.get(), st);
    w->wM = std::move(wAAm);
    w->Mw = std::move(wEAm);
    w->conservative = 0;
    w->scaled = scale ? 1 : 0;
    IBH_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < 2; ++k) w->dims[k] = work[k].commit();
    *out = w.release();
}

}  // namespace
}  // namespace ibh

using namespace ibh;
extern "C" {

int ibh_modele_merge_EOpvAOp(const ibh_regrid_matrices *const *rmOs, int nsheets, int64_t nO, int64_t base_nE, int64_t base_nO,
                             int64_t base_nnz, const int64_t *base_iE, const int64_t *base_iO, const double *base_val,
                             const double *hcdefs_base, int32_t nhc_base, int64_t base_stride_A, int64_t base_stride_HC, int use_global_ice,
                             int use_local_ice, int squash_ecs, ibh_sparse_set *dimAOp, ibh_sparse_set *dimEOp, ibh_weighted **EOpvAOp,
                             int64_t *offsetE, int32_t *nhc_out, double *hcdefs_out, int16_t *underice_out, int64_t *stride_A_out,
                             int64_t *stride_HC_out) {
    if (EOpvAOp) *EOpvAOp = nullptr;
    return guarded([&] {
        IBH_CHECK(EOpvAOp && offsetE && nhc_out && stride_A_out && stride_HC_out, "null argument");
        MergeOut mo;
        merge_EOpvAOp(rmOs, nsheets, nO, base_nE, base_nO, base_nnz, base_iE, base_iO, base_val, hcdefs_base, nhc_base,
                      HcIndexing{base_stride_A, base_stride_HC}, use_global_ice != 0, use_local_ice != 0, squash_ecs != 0, dimAOp, dimEOp,
                      EOpvAOp, mo);
        *offsetE = mo.offsetE; *nhc_out = (int32_t)mo.hcdefs.size();
        *stride_A_out = mo.hc.sA; *stride_HC_out = mo.hc.sHC;
        if (hcdefs_out) std::copy(mo.hcdefs.begin(), mo.hcdefs.end(), hcdefs_out);
        if (underice_out) std::copy(mo.underice.begin(), mo.underice.end(), underice_out);
    });
}

int ibh_modele_AAmvEAm(const ibh_weighted *EOpvAOp, const ibh_sparse_set *dimEOp, const ibh_sparse_set *dimAOp, int32_t imO, int32_t jmO,
                       double offiO, double dlatO, double eq_rad, int32_t nhc, int64_t sA_O, int64_t sHC_O, int64_t sA_A, int64_t sHC_A,
                       const double *foceanAOp, const double *foceanAOm, int64_t nO, int scale, ibh_sparse_set *dimAAm,
                       ibh_sparse_set *dimEAm, ibh_weighted **out) {
    if (out) *out = nullptr;
    return guarded([&] {
        compute_AAmvEAm(EOpvAOp, dimEOp, dimAOp, imO, jmO, offiO, dlatO, eq_rad, nhc, sA_O, sHC_O, sA_A, sHC_A, foceanAOp, foceanAOm, nO,
                        scale, dimAAm, dimEAm, out);
    });
}

}  // extern "C"
