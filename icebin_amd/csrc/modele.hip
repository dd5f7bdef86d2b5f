// modele.hip -- GCMRegridder_ModelE::regrid_matrices (slib/icebin/modele/GCMRegridder_ModelE.cpp:487-571) composed from the
// O-grid matrix builds (assemble.hip), Hntr's clipped overlap (hntr.hip) and ONE sparse product (csrops.h).
//
// Where things live.  Every matrix and every weight vector stays in HBM; the products, the re-numbered copies (crop_mvp) and
// the vector scalings are csrops.hip's, ModelE's two weight vectors kernels below.  The bookkeeping of the GCM-grid-sized SETS (dimAOp -> dimAOm, dimEOm, dimEAm: at
// most nO * nhc keys) runs on the host, where ibh_sparse_set keeps its keys: it reads the sets' keys, the INDICES of EOpvAOp
// (one entry per elevation class of an ice-bearing O cell) and, for raw_EOvEA's "weight != 0" test, the vector wEOm.  No
// entry of an ice-sized matrix travels to the host.  (So the add_dense_host loops below stay host loops, not sparseset.h's
// device numbering: moving them is a performance change of its own.)
#include <algorithm>
#include <cmath>
#include <memory>

#include "assemble.h"
#include "common.h"
#include "csrbuild.h"
#include "csrops.h"
#include "modele_parts.h"
#include "prims.h"

struct ibh_modele_matrices {
    const ibh_regrid_matrices *rmO = nullptr;
    ibh_hntr *hntr = nullptr;                   // Hntr(17.17, hntrO, hntrA): B = O, A = atmosphere
    int32_t nhc = 0;
    double eq_rad = 0;
    int64_t nO = 0, nA = 0;                     // cells of O and of A
    int64_t sA_O = 1, sHC_O = 0, sA_A = 1, sHC_A = 0;       // indexingHC of O and of A
    std::vector<double> foceanAOp, foceanAOm;
    ~ibh_modele_matrices() { ibh_hntr_destroy(hntr); }
};

namespace ibh {
namespace {

// ---- the small vectors --------------------------------------------------------------------------------------------------------
// compute_wAOm (topo.cpp:84-109): wAOm[k] = 0 + (1 / fcont_p) * wAOp[src[k]]; src[k] < 0 where fcont_p == 0 (no entry: 0)
__global__ void k_wAOm(const double *__restrict__ inv_fcont, const int32_t *__restrict__ src, const double *__restrict__ wAOp, int n,
                       double *__restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = src[k] >= 0 ? 0. + inv_fcont[k] * wAOp[src[k]] : 0.;
}
// wEOm, wXAm = (M * diag(d)) * w: y[r] = sum over the row's columns k ascending, from 0, of (M(r, k) * d[k]) * w[k]
__global__ void k_scaled_matvec(Csr M, const double *__restrict__ d, const double *__restrict__ w, double *__restrict__ y) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M.nrow) return;
    double s = 0.;
    for (int e = M.rowptr[r]; e < M.rowptr[r + 1]; ++e) {
        const int k = M.colind[e];
        s = s + (M.val[e] * d[k]) * w[k];
    }
    y[r] = s;
}
// a host vector into the arena (the caller keeps it alive until the stream is synchronised)
template <class T>
T *to_arena(const std::vector<T> &h, hipStream_t st) {
    T *d = arena().get<T>(h.size());
    if (!h.empty()) IBH_HIP(hipMemcpyAsync(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, st));
    return d;
}
template <class T>
void upload(DevBuf<T> &b, const std::vector<T> &h, hipStream_t st) { b.alloc(h.size()); b.upload(h.data(), h.size(), st); }

// sigma: only compute_GpvXAm's IpvXOp takes the caller's (RegridMatrices_Dynamic.cpp:404-409); every other build is unsmoothed
std::unique_ptr<ibh_weighted> o_matrix(const ibh_modele_matrices *mm, const char *name, ibh_sparse_set *d0, ibh_sparse_set *d1, int correctA,
                                       const double *sigma = nullptr) {
    const double zero[3] = {0, 0, 0};
    ibh_weighted *w = nullptr;
    assemble_matrix(mm->rmO, name, d0, d1, 0, correctA, sigma ? sigma : zero, &w);
    return std::unique_ptr<ibh_weighted>(w);
}
}  // namespace

// ---- the topo.cpp helpers (modele_parts.h): ComputeXAmvGp_Helper (:168-280) below and globalave.hip compose them -------------
HostTriplets hntr_overlap_triplets(const ibh_hntr *h, double eq_rad, const uint8_t *includeB) {
    HostTriplets t;
    int64_t ns = 0;
    rethrow(ibh_hntr_triplets(h, IBH_HNTR_OVERLAP, eq_rad, includeB, &ns, nullptr, nullptr, nullptr));
    t.iB.resize((size_t)ns); t.iA.resize((size_t)ns); t.v.resize((size_t)ns);
    if (ns) rethrow(ibh_hntr_triplets(h, IBH_HNTR_OVERLAP, eq_rad, includeB, &ns, t.iB.data(), t.iA.data(), t.v.data()));
    return t;
}

void scaled_matvec(const ibh_weighted &M, const double *d, const double *w, double *y, hipStream_t st) {
    if (M.nrow) hipLaunchKernelGGL(k_scaled_matvec, dim3(ceil_div(M.nrow, 256)), dim3(256), 0, st, view(M), d, w, y);
    IBH_HIP(hipGetLastError());
}

void compute_wAOm(const double *foceanAOp, const double *foceanAOm, int64_t nO, const double *d_wAOp, const ibh_sparse_set &dimAOp,
                  ibh_sparse_set &dimAOm, std::vector<int32_t> &aop2aom, DevBuf<double> &wAOm, hipStream_t st) {
    const int nAOp = dimAOp.n();
    const int64_t *ts = dimAOp.to_sparse_host();
    std::vector<int64_t> keys;
    std::vector<double> inv_fcont;
    std::vector<int32_t> src;
    aop2aom.assign((size_t)nAOp, -1);
    for (int d = 0; d < nAOp; ++d)          // dimAOm: the cells of dimAOp, in dense order, that ModelE calls land
        if (foceanAOm[(size_t)ts[d]] == 0) { aop2aom[(size_t)d] = (int32_t)keys.size(); keys.push_back(ts[d]); }
    inv_fcont.assign(keys.size(), 0.); src.assign(keys.size(), -1);
    for (int d = 0; d < nAOp; ++d) {        // scaled_AOmvAOp (topo.cpp:50-81)
        const double fcont_p = 1.0 - foceanAOp[(size_t)ts[d]], fcont_m = 1.0 - foceanAOm[(size_t)ts[d]];
        if (fcont_m == 0.0) continue;
        if (fcont_m != 1.0) fail(IBH_EINVAL, "fcont_m[%ld] = %g, must be 0 or 1", (long)ts[d], fcont_m);
        if (fcont_p == 0.0) continue;
        const int k = aop2aom[(size_t)d];
        if (k < 0) continue;                // (fcont_m == 1 means foceanAOm == 0: always in dimAOm)
        inv_fcont[(size_t)k] = 1. / fcont_p; src[(size_t)k] = d;
    }
    dimAOm.assign_host(nO, keys.data(), (int32_t)keys.size());
    arena().reset();
    const int nAOm = dimAOm.n();
    wAOm.alloc((size_t)nAOm);
    const double *d_inv = to_arena(inv_fcont, st);
    const int32_t *d_src = to_arena(src, st);
    if (nAOm) hipLaunchKernelGGL(k_wAOm, dim3(ceil_div(nAOm, 256)), dim3(256), 0, st, d_inv, d_src, d_wAOp, nAOm, wAOm.p);
    IBH_HIP(hipGetLastError());
    IBH_HIP(hipStreamSynchronize(st));      // the host vectors (and the caller's d_wAOp) may go away here
}

void compute_EOmvAOm_unscaled(const ibh_weighted &EOpvAOp, const ibh_sparse_set &dimEOp2, const ibh_sparse_set &dimAOp2,
                              const ibh_sparse_set &dimAOm, const DevBuf<double> &wAOm, int64_t extentEOm, ibh_sparse_set &dimEOm,
                              ibh_weighted *EOmvAOm_out, DevBuf<double> *EOmvAOms_out, DevBuf<double> &wEOm, std::vector<double> &wEOm_h,
                              hipStream_t st) {
    const int nE2 = EOpvAOp.nrow, nA2 = EOpvAOp.ncol, nAOm = dimAOm.n();
    const long nnz2 = (long)EOpvAOp.nnz;
    std::vector<int32_t> rp((size_t)nE2 + 1), ci((size_t)nnz2);
    EOpvAOp.rowptr.download(rp.data(), (size_t)nE2 + 1, st);
    EOpvAOp.colind.download(ci.data(), (size_t)nnz2, st);
    std::vector<int32_t> colptr((size_t)nA2 + 1, 0), by_col((size_t)nnz2), row_of((size_t)nnz2);
    for (long e = 0; e < nnz2; ++e) ++colptr[(size_t)ci[(size_t)e] + 1];
    for (int c = 0; c < nA2; ++c) colptr[(size_t)c + 1] += colptr[(size_t)c];
    {
        std::vector<int32_t> fill(colptr.begin(), colptr.end() - 1);
        for (int r = 0; r < nE2; ++r)
            for (int e = rp[(size_t)r]; e < rp[(size_t)r + 1]; ++e) { by_col[(size_t)fill[(size_t)ci[(size_t)e]]++] = e; row_of[(size_t)e] = r; }
    }
    dimEOm.set_sparse_extent(extentEOm);
    std::vector<int32_t> trow, tcol, tsrc;
    const int64_t *tsE2 = dimEOp2.to_sparse_host(), *tsA2 = dimAOp2.to_sparse_host();
    for (int c = 0; c < nA2; ++c) {
        const int kAOm = dimAOm.to_dense(tsA2[c]);
        if (kAOm < 0) continue;
        for (int q = colptr[(size_t)c]; q < colptr[(size_t)c + 1]; ++q) {
            const int e = by_col[(size_t)q];
            trow.push_back(dimEOm.add_dense_host(tsE2[row_of[(size_t)e]])); tcol.push_back(kAOm); tsrc.push_back(e);
        }
    }
    const int nEOm = dimEOm.n();
    const long nt = (long)trow.size();
    ibh_weighted local;
    DevBuf<double> local_s;
    ibh_weighted &EOmvAOm = EOmvAOm_out ? *EOmvAOm_out : local;
    DevBuf<double> &EOmvAOms = EOmvAOms_out ? *EOmvAOms_out : local_s;
    arena().reset();
    const int32_t *d_row = to_arena(trow, st), *d_col = to_arena(tcol, st), *d_src = to_arena(tsrc, st);
    double *d_val = arena().get<double>((size_t)nt);
    gather(EOpvAOp.val.p, d_src, nt, d_val, st);
    weighted_from_device_triplets(&EOmvAOm, nEOm, nAOm, nt, d_row, d_col, d_val, st);
    recip(EOmvAOm.Mw.p, nAOm, EOmvAOms, st);
    wEOm.alloc((size_t)nEOm);
    scaled_matvec(EOmvAOm, EOmvAOms.p, wAOm.p, wEOm.p, st);
    wEOm_h.resize((size_t)nEOm);
    wEOm.download(wEOm_h.data(), (size_t)nEOm, st);     // (synchronises: the host vectors and matrices above are free)
}

std::unique_ptr<ibh_weighted> raw_EOvEA(const ibh_hntr *hntr, double eq_rad, const std::vector<uint8_t> &includeO,
                                        const ibh_sparse_set &dimEOm, const DevBuf<double> &wEOm, const std::vector<double> &wEOm_h,
                                        int32_t nhc, HcIndexing hcO, HcIndexing hcA, ibh_sparse_set &dimEAm, hipStream_t st) {
    const HostTriplets s = hntr_overlap_triplets(hntr, eq_rad, includeO.data());
    std::vector<int32_t> trow, tcol;
    for (size_t p = 0; p < s.v.size(); ++p) {
        if (std::abs(s.v[p]) < 1e-8) fail(IBH_EINVAL, "Found a stray overlap; what should we do about it?");
        for (int ihc = 0; ihc < nhc; ++ihc) {
            const int dEO = dimEOm.to_dense(hcO.index(s.iB[p], ihc));
            if (dEO < 0 || wEOm_h[(size_t)dEO] == 0) continue;
            trow.push_back(dEO);
            tcol.push_back(dimEAm.add_dense_host(hcA.index(s.iA[p], ihc)));
        }
    }
    const long ne = (long)trow.size();
    std::unique_ptr<ibh_weighted> EOmvEAm(new ibh_weighted);
    arena().reset();
    const int32_t *d_row = to_arena(trow, st), *d_col = to_arena(tcol, st);
    double *d_val = arena().get<double>((size_t)ne);
    gather(wEOm.p, d_row, ne, d_val, st);
    weighted_from_device_triplets(EOmvEAm.get(), dimEOm.n(), dimEAm.n(), ne, d_row, d_col, d_val, st);
    IBH_HIP(hipStreamSynchronize(st));
    return EOmvEAm;
}

namespace {
// dimXAm, dimGp: the caller's sets (copies: the caller's own change only when the matrix is built).  XvG: true = XAmvGp.
// sigma (null: none): GpvXAm's smoothing, which goes to the one O-grid build of IpvXOp and to nothing else.
void modele_matrix(const ibh_modele_matrices *mm, char gridX, char gridG, bool XvG, int scale, const double *sigma, ibh_sparse_set &dimXAm,
                   ibh_sparse_set &dimGp, ibh_weighted *ret) {
    hipStream_t st = hipStreamPerThread;
    const char nameAvG[4] = {'A', 'v', gridG, 0}, nameXvG[4] = {gridX, 'v', gridG, 0}, nameGvX[4] = {gridG, 'v', gridX, 0};
    const int64_t nO = mm->nO;

    ibh_sparse_set dimAOp, dimAOm, dimEOp, dimEOm;
    DevBuf<double> wAOm;
    std::vector<int32_t> aop2aom;
    {   // AOpvIp with correctA numbers dimAOp (and dimGp); its wM is wAOp
        auto AOpvIp_c = o_matrix(mm, nameAvG, &dimAOp, &dimGp, 1);
        compute_wAOm(mm->foceanAOp.data(), mm->foceanAOm.data(), nO, AOpvIp_c->wM.p, dimAOp, dimAOm, aop2aom, wAOm, st);
    }
    const int nAOm = dimAOm.n();
    std::vector<uint8_t> includeO((size_t)nO, 0);           // DimClip(&dimAOm)
    for (int k = 0; k < nAOm; ++k) includeO[(size_t)dimAOm.to_sparse_host()[k]] = 1;

    dimXAm.set_sparse_extent(gridX == 'E' ? mm->nA * mm->nhc : mm->nA);

    std::unique_ptr<ibh_weighted> XOpvIp, XOmvXAm;          // XOmvXAm: the reference's XAmvXOm by its columns
    DevBuf<double> wEOm;
    const double *wXOm = wAOm.p;
    ibh_sparse_set *dimXOp = &dimAOp, *dimXOm = &dimAOm;
    if (gridX == 'E') {
        dimXOp = &dimEOp; dimXOm = &dimEOm;
        XOpvIp = o_matrix(mm, nameXvG, &dimEOp, &dimGp, 0);
        std::vector<double> wEOm_h;
        {
            ibh_sparse_set dimEOp2, dimAOp2;
            auto EOpvAOp = o_matrix(mm, "EvA", &dimEOp2, &dimAOp2, 0);
            compute_EOmvAOm_unscaled(*EOpvAOp, dimEOp2, dimAOp2, dimAOm, wAOm, nO * mm->nhc, dimEOm, nullptr, nullptr, wEOm, wEOm_h, st);
        }
        wXOm = wEOm.p;
        XOmvXAm = raw_EOvEA(mm->hntr, mm->eq_rad, includeO, dimEOm, wEOm, wEOm_h, mm->nhc, HcIndexing{mm->sA_O, mm->sHC_O},
                            HcIndexing{mm->sA_A, mm->sHC_A}, dimXAm, st);
    } else {
        XOpvIp = o_matrix(mm, nameXvG, &dimAOp, &dimGp, 0);
        IBH_HIP(hipStreamSynchronize(st));
        ibh_weighted *w = nullptr;      // AOmvAAm by rows: the reference's 'T' only swaps the output
        rethrow(ibh_hntr_matrix_d(mm->hntr, IBH_HNTR_OVERLAP, mm->eq_rad, includeO.data(), &dimAOm, IBH_TO_DENSE_IGNORE_MISSING, &dimXAm,
                                  IBH_ADD_DENSE, 0, &w));
        XOmvXAm.reset(w);
    }
    const int nXOm = dimXOm->n(), nXAm = dimXAm.n(), nXOp = dimXOp->n();
    IBH_CHECK(XOmvXAm->nrow == nXOm && XOmvXAm->ncol == nXAm && XOpvIp->nrow == nXOp, "internal: ModelE matrix shapes disagree");

    // XAmvXOms = sum(XAmvXOm, 1, '-'), sXAm = sum(XAmvXOm, 0, '-'): the row and column sums of XOmvXAm, inverted
    DevBuf<double> XAmvXOms, sXAm, wXAm, lscale;
    recip(XOmvXAm->wM.p, nXOm, XAmvXOms, st);
    recip(XOmvXAm->Mw.p, nXAm, sXAm, st);
    // wXAm = XAmvXOm * diag(XAmvXOms) * wXOm (:277-278)
    ibh_weighted XAmvXOm;
    transpose_csr(*XOmvXAm, &XAmvXOm, st);
    wXAm.alloc((size_t)nXAm);
    scaled_matvec(XAmvXOm, XAmvXOms.p, wXOm, wXAm.p, st);

    // dense XOp <-> dense XOm
    std::vector<int32_t> op2om((size_t)nXOp, -1), om2op((size_t)nXOm, -1);
    {
        const int64_t *ts = dimXOp->to_sparse_host();
        for (int d = 0; d < nXOp; ++d) {
            const int k = gridX == 'E' ? dimXOm->to_dense(ts[d]) : aop2aom[(size_t)d];
            op2om[(size_t)d] = k;
            if (k >= 0) om2op[(size_t)k] = d;
        }
    }
    DevBuf<int32_t> d_map;
    const int nG = dimGp.n();
    if (XvG) {
        // M = diag(scale ? sXAm : wXAm * sXAm) * XAmvXOm * crop_mvp(dimXOm, dimXOp, 0, diag(1 / XOpvIp.wM) * XOpvIp.M)   (:346-365)
        DevBuf<double> sXOpvIp;
        ibh_weighted cropped;
        recip(XOpvIp->wM.p, nXOp, sXOpvIp, st);
        upload(d_map, om2op, st);
        arena().reset();
        crop_rows(*XOpvIp, d_map.p, nXOm, sXOpvIp.p, &cropped, st);
        const double *ls = sXAm.p;
        if (!scale) {
            lscale.alloc((size_t)nXAm);
            mul(wXAm.p, sXAm.p, nXAm, lscale.p, st);
            ls = lscale.p;
        }
        scale_rows(XAmvXOm.rowptr.p, nXAm, ls, XAmvXOm.val.p, st);
        IBH_HIP(hipGetLastError());
        csr_product(XAmvXOm, cropped, ret, st);
        ret->composed_by = COMPOSED_PRODUCT;
        ret->wM = std::move(wXAm);
        ret->Mw.alloc((size_t)nG);
        if (nG) IBH_HIP(hipMemcpyAsync(ret->Mw.p, XOpvIp->Mw.p, sizeof(double) * (size_t)nG, hipMemcpyDeviceToDevice, st));
    } else {
        // M = crop_mvp(dimXOm, dimXOp, 1, [diag(1 / IpvXOp.wM) *] IpvXOp.M) * diag(XAmvXOms) * XOmvXAm   (:402-430)
        // (a smoothed IpvXOp keeps the rows and columns of the unsmoothed one: the smoother mixes rows of the same matrix)
        auto IpvXOp = o_matrix(mm, nameGvX, &dimGp, dimXOp, 0, sigma);
        IBH_CHECK(IpvXOp->ncol == nXOp && IpvXOp->nrow == nG, "internal: %s added cells to a set the O-grid builds had numbered", nameGvX);
        DevBuf<double> sIpvXOp;
        if (scale) recip(IpvXOp->wM.p, nG, sIpvXOp, st);
        upload(d_map, op2om, st);
        // every row of XOmvXAm holds at most one entry (an O cell lies in one A cell; raw_EOvEA emits one pair per class), so
        // the product is row-local; smoothed rows, tens of entries each, take that form (csrops.h)
        ret->composed_by = compose_cols(*IpvXOp, d_map.p, scale ? sIpvXOp.p : nullptr, XAmvXOms.p, *XOmvXAm,
                                        compose_rowlocal_wanted(sigma != nullptr), ret, st);
        ret->smoothed_by = IpvXOp->smoothed_by;
        ret->wM.alloc((size_t)nG);
        if (nG) IBH_HIP(hipMemcpyAsync(ret->wM.p, XOpvIp->Mw.p, sizeof(double) * (size_t)nG, hipMemcpyDeviceToDevice, st));
        ret->Mw = std::move(wXAm);
    }
    ret->conservative = 0;
    ret->scaled = scale;
    IBH_HIP(hipStreamSynchronize(st));
}

struct Parsed { int kind; char gridX, gridG; };        // kind 0: XAmvGp, 1: GpvXAm, 2: AOmvAAm, 3: AAmvAOm
Parsed parse_spec(const char *spec) {
    static const struct { const char *name; Parsed p; } table[] = {
        {"AvI", {0, 'A', 'I'}}, {"EvI", {0, 'E', 'I'}}, {"AvX", {0, 'A', 'X'}}, {"EvX", {0, 'E', 'X'}},
        {"AAmvIp", {0, 'A', 'I'}}, {"EAmvIp", {0, 'E', 'I'}},
        {"IvA", {1, 'A', 'I'}}, {"IvE", {1, 'E', 'I'}}, {"XvA", {1, 'A', 'X'}}, {"XvE", {1, 'E', 'X'}},
        {"IpvAAm", {1, 'A', 'I'}}, {"IpvEAm", {1, 'E', 'I'}},
        {"AOmvAAm", {2, 'A', 'A'}}, {"AAmvAOm", {3, 'A', 'A'}}};
    for (const auto &t : table)
        if (!std::strcmp(spec, t.name)) return t.p;
    fail(IBH_ENOKEY, "unknown ModelE matrix '%s'", spec);   // regrids.at(), RegridMatrices_Dynamic.cpp:419
}

void check_extent(const ibh_sparse_set *s, int64_t extent, const char *which) {
    if (!s) return;
    s->check_extent(extent, (std::string("ModelE matrix_d: ") + which).c_str());
    s->check_entries_within(extent, which);
}

void modele_matrix_d(const ibh_modele_matrices *mm, const char *spec, ibh_sparse_set *dim0, ibh_sparse_set *dim1, int scale,
                     const double *sigma, ibh_weighted **out) {
    const Parsed p = parse_spec(spec);
    // only compute_GpvXAm hands sigma on (RegridMatrices_Dynamic.cpp:404-409); compute_XAmvGp and compute_AOmvAAm never read it
    if (!(sigma && sigma[0] != 0 && p.kind == 1)) sigma = nullptr;
    const ibh_regridder *rg = mm->rmO->rg;
    check_current_device(rg->device, "regridder");
    IBH_CHECK(dim0 == nullptr || dim0 != dim1, "dims[0] and dims[1] must be distinct sets");
    ibh_sparse_set *dims[2] = {dim0, dim1};
    const int iX = p.kind == 0 ? 0 : 1, iG = 1 - iX;       // XAmvGp / GpvXAm: where the atmosphere set and the ice set stand
    if (p.kind >= 2) {
        check_extent(dim0, mm->nO, "dimAOm");
        check_extent(dim1, mm->nA, "dimAAm");
    } else {
        check_extent(dims[iX], p.gridX == 'E' ? mm->nA * mm->nhc : mm->nA, p.gridX == 'E' ? "dimEAm" : "dimAAm");
        check_extent(dims[iG], p.gridG == 'I' ? rg->nI : rg->nX, p.gridG == 'I' ? "dimIp" : "dimXp");
    }
    WorkingSet work[2] = {WorkingSet(dim0), WorkingSet(dim1)};
    std::unique_ptr<ibh_weighted> w;
    if (p.kind >= 2) {
        // compute_AOmvAAm (:92-121): dims {dimAOm, dimAAm} whichever way the matrix is stored; the clip is dimAOm as it comes
        std::vector<uint8_t> includeO((size_t)mm->nO, 0);
        for (int k = 0; k < work[0]->n(); ++k) includeO[(size_t)work[0]->to_sparse_host()[k]] = 1;
        ibh_weighted *h = nullptr;
        rethrow(ibh_hntr_matrix_d(mm->hntr, IBH_HNTR_OVERLAP, mm->eq_rad, includeO.data(), work[0].get(), IBH_TO_DENSE_IGNORE_MISSING,
                                  work[1].get(), IBH_ADD_DENSE, p.kind == 3, &h));
        w.reset(h);
    } else {
        w = new_weighted();
        modele_matrix(mm, p.gridX, p.gridG, p.kind == 0, scale, sigma, *work[iX], *work[iG], w.get());
    }
    // built: the caller's sets take the numbering, the result names them (or owns the fresh ones).  AAmvAOm is hntr's
    // transpose, stored {dimAAm, dimAOm}: its sets go to the other slot each.
    const bool swapped = p.kind == 3;
    for (int k = 0; k < 2; ++k) w->dims[swapped ? 1 - k : k] = work[k].commit();
    *out = w.release();
}

void modele_create(const ibh_regrid_matrices *rmO, int32_t imO, int32_t jmO, double offiO, double dlatO, double eq_rad,
                   const double *foceanAOp, const double *foceanAOm, int64_t nO, ibh_modele_matrices **out) {
    IBH_CHECK(rmO && foceanAOp && foceanAOm && out, "null argument");
    const ibh_regridder *rg = rmO->rg;
    // make_hntrA (hntr.cpp:232-241)
    IBH_CHECK(imO > 0 && jmO > 0 && imO % 2 == 0 && jmO % 2 == 0,
              "Ocean grid must have even number of gridcells for im and jm (vs. %d %d)", imO, jmO);
    IBH_CHECK((int64_t)imO * jmO == rg->nA, "the ocean HntrSpec has %lld cells, the regridder's grid nA=%lld", (long long)imO * jmO,
              (long long)rg->nA);
    IBH_CHECK(nO == rg->nA, "focean arrays have %lld elements, the ocean grid nA=%lld", (long long)nO, (long long)rg->nA);
    const bool hc_slowest = rg->hc_stride_A == 1 && rg->hc_stride_HC == nO, hc_fastest = rg->hc_stride_HC == 1 && rg->hc_stride_A == rg->nhc;
    IBH_CHECK(rg->nhc == 0 || hc_slowest || hc_fastest, "indexingHC strides (%ld,%ld) are neither (1,nO) nor (nhc,1)", (long)rg->hc_stride_A,
              (long)rg->hc_stride_HC);
    if (rmO->sigma[0] != 0) fail(IBH_ENOTIMPL, "smoothing (sigma != 0) through the ModelE regridder is not supported");
    check_current_device(rg->device, "regridder");
    std::unique_ptr<ibh_modele_matrices> mm(new ibh_modele_matrices);
    mm->rmO = rmO; mm->nhc = rg->nhc; mm->eq_rad = eq_rad;
    mm->nO = nO; mm->nA = (int64_t)(imO / 2) * (jmO / 2);
    mm->sA_O = rg->hc_stride_A; mm->sHC_O = rg->hc_stride_HC;
    mm->sA_A = hc_slowest ? 1 : rg->nhc; mm->sHC_A = hc_slowest ? mm->nA : 1;       // (:451-456)
    mm->foceanAOp.assign(foceanAOp, foceanAOp + nO);
    mm->foceanAOm.assign(foceanAOm, foceanAOm + nO);
    rethrow(ibh_hntr_create(&mm->hntr, imO / 2, jmO / 2, offiO * 0.5, dlatO * 2., imO, jmO, offiO, dlatO, 0.));
    *out = mm.release();
}

// make_agridA (:57-78)
void modele_agridA(const ibh_regridder *rg, int32_t imO, int32_t jmO, double offiO, double dlatO, int32_t *nA_dense, int64_t *to_sparse) {
    IBH_CHECK(rg && nA_dense, "null argument");
    IBH_CHECK(imO > 0 && jmO > 0 && imO % 2 == 0 && jmO % 2 == 0,
              "Ocean grid must have even number of gridcells for im and jm (vs. %d %d)", imO, jmO);
    IBH_CHECK((int64_t)imO * jmO == rg->nA, "the ocean HntrSpec has %lld cells, the regridder's grid nA=%lld", (long long)imO * jmO,
              (long long)rg->nA);
    std::vector<uint8_t> includeO((size_t)rg->nA, 0);
    for (int64_t s : rg->A_to_sparse) includeO[(size_t)s] = 1;
    ibh_hntr *h = nullptr;
    rethrow(ibh_hntr_create(&h, imO / 2, jmO / 2, offiO * 0.5, dlatO * 2., imO, jmO, offiO, dlatO, 0.));
    std::unique_ptr<ibh_hntr, int (*)(ibh_hntr *)> hold(h, ibh_hntr_destroy);
    const HostTriplets s = hntr_overlap_triplets(h, 1.0, includeO.data());
    ibh_sparse_set dimA((int64_t)(imO / 2) * (jmO / 2));
    for (int32_t iA : s.iA) dimA.add_dense_host(iA);
    *nA_dense = dimA.n();
    if (to_sparse && dimA.n()) std::copy(dimA.to_sparse_host(), dimA.to_sparse_host() + dimA.n(), to_sparse);
}

}  // namespace
}  // namespace ibh

using namespace ibh;
extern "C" {

int ibh_modele_matrices_create(const ibh_regrid_matrices *rmO, int32_t imO, int32_t jmO, double offiO, double dlatO, double eq_rad,
                               const double *foceanAOp, const double *foceanAOm, int64_t nO, ibh_modele_matrices **out) {
    if (out) *out = nullptr;
    return guarded([&] { modele_create(rmO, imO, jmO, offiO, dlatO, eq_rad, foceanAOp, foceanAOm, nO, out); });
}
int ibh_modele_matrices_matrix_d_sigma(const ibh_modele_matrices *mm, const char *spec, ibh_sparse_set *dim0, ibh_sparse_set *dim1, int scale,
                                       const double sigma[3], ibh_weighted **out) {
    if (out) *out = nullptr;
    return guarded([&] {
        IBH_CHECK(mm && spec && out, "null argument");
        modele_matrix_d(mm, spec, dim0, dim1, scale, sigma, out);
    });
}
int ibh_modele_matrices_matrix_d(const ibh_modele_matrices *mm, const char *spec, ibh_sparse_set *dim0, ibh_sparse_set *dim1, int scale,
                                 ibh_weighted **out) {
    return ibh_modele_matrices_matrix_d_sigma(mm, spec, dim0, dim1, scale, nullptr, out);
}
int ibh_modele_matrices_destroy(ibh_modele_matrices *mm) { delete mm; return IBH_OK; }
int ibh_modele_agridA(const ibh_regridder *rgO, int32_t imO, int32_t jmO, double offiO, double dlatO, int32_t *nA_dense,
                      int64_t *to_sparse) {
    return guarded([&] { modele_agridA(rgO, imO, jmO, offiO, dlatO, nA_dense, to_sparse); });
}

}  // extern "C"
