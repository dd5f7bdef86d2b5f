// topo.hip -- GCMCoupler_ModelE::update_topo's field handling (slib/icebin/modele/GCMCoupler_ModelE.cpp:972-1098): merge_topoO
// (modele/merge_topo.cpp:84-360) and make_topoA (modele/topo.cpp:538-888), with the row statistics of a Weighted that
// merge_topoO reads an OvI through; DESIGN.md 17.
//
// Where things live.  Every plane stays in HBM from the ice model's elevation masks to ModelE's arrays.  merge_topoO builds
// the four OvI of a sheet with the existing entry point (assemble_batch), reads each CSR once (k_topo_row_stats: the row sum
// and, for the land mask, the row's min / max of elevI in the same pass) and adds the sheet into six accumulator planes with
// one launch per sheet; the per-cell update, the single-cell-ocean pass and the sanity checks are one thread per O cell.
// make_topoA regrids with the existing Hntr kernel, gathers the mask and the land range over each A cell's window of O
// cells (no atomics), and walks AAmvEAm by its rows.  The sanity checks write one flag word per cell; the callers make the
// reference's strings from the flags and the planes.  Every multiply and add is one IEEE operation (-ffp-contract=off).
#include <cfloat>
#include <climits>
#include <cmath>
#include <memory>

#include "assemble.h"
#include "common.h"
#include "csrops.h"
#include "prims.h"

namespace ibh {
namespace {

constexpr int16_t UI_UNUSED = 0, UI_LOCALICE = 1, UI_VGHOST = 3, UI_SEALAND = 5;    // modele/grids.hpp:44-49
constexpr int T = 256;

// ---- row statistics of a Weighted -------------------------------------------------------------------------------------------
// One workgroup of WAVES waves per dense row.  The lanes stride the row, TOPO_UNROLL independent (column, value, x) loads in
// flight each, then one entry at a time; the partial results meet through wave shuffles and, between the waves, through LDS in
// wave order: the order of the sum is a function of the row's length alone.  Only stored entries are touched.
constexpr int TOPO_UNROLL = 4;
constexpr int TOPO_WAVES = 4, TOPO_WAVES_LONG = 16;
constexpr int64_t TOPO_LONG_ROWS = 16384;       // more entries per row than this on average: the 16-wave workgroup

__device__ __forceinline__ double topo_min(double a, double b) { return b < a ? b : a; }   // std::min(a, b), std::max(a, b)
__device__ __forceinline__ double topo_max(double a, double b) { return a < b ? b : a; }

template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_topo_row_stats(Csr M, const double *__restrict__ x, double *__restrict__ sum,
                                                               double *__restrict__ mn, double *__restrict__ mx) {
    constexpr int NT = WAVES * 64;
    __shared__ double part[3][WAVES];
    const int r = blockIdx.x;
    const long e = M.rowptr[r + 1];
    long k = (long)M.rowptr[r] + threadIdx.x;
    double s = 0., lo = DBL_MAX, hi = DBL_MIN;
    for (; k + (TOPO_UNROLL - 1) * NT < e; k += TOPO_UNROLL * NT) {
        int c[TOPO_UNROLL];
        double v[TOPO_UNROLL], xv[TOPO_UNROLL];
#pragma unroll
        for (int u = 0; u < TOPO_UNROLL; ++u) { c[u] = M.colind[k + u * NT]; v[u] = M.val[k + u * NT]; }
#pragma unroll
        for (int u = 0; u < TOPO_UNROLL; ++u) xv[u] = x[c[u]];
#pragma unroll
        for (int u = 0; u < TOPO_UNROLL; ++u) { s += v[u] * xv[u]; lo = topo_min(lo, xv[u]); hi = topo_max(hi, xv[u]); }
    }
    for (; k < e; k += NT) {
        const double xv = x[M.colind[k]];
        s += M.val[k] * xv; lo = topo_min(lo, xv); hi = topo_max(hi, xv);
    }
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        lo = topo_min(lo, __shfl_xor(lo, o, 64));
        hi = topo_max(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = s; part[1][threadIdx.x >> 6] = lo; part[2][threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < WAVES; ++w) { s += part[0][w]; lo = topo_min(lo, part[1][w]); hi = topo_max(hi, part[2][w]); }
        if (sum) sum[r] = s;
        if (mn) mn[r] = lo;
        if (mx) mx[r] = hi;
    }
}

void row_stats(const ibh_weighted &w, const double *x, double *sum, double *mn, double *mx, hipStream_t st) {
    if (w.nrow == 0 || (!sum && !mn && !mx)) return;
    if (w.nnz > TOPO_LONG_ROWS * (int64_t)w.nrow)
        hipLaunchKernelGGL(k_topo_row_stats<TOPO_WAVES_LONG>, dim3((unsigned)w.nrow), dim3(TOPO_WAVES_LONG * 64), 0, st, view(w), x, sum, mn, mx);
    else
        hipLaunchKernelGGL(k_topo_row_stats<TOPO_WAVES>, dim3((unsigned)w.nrow), dim3(TOPO_WAVES * 64), 0, st, view(w), x, sum, mn, mx);
    IBH_HIP(hipGetLastError());
}

// ---- merge_topoO ------------------------------------------------------------------------------------------------------------
// the nine in/out planes in the order of the argument list (:89-99), which is also the order of the sanity checks (:159-167)
enum { P_foceanOp, P_fgiceOp, P_zatmoOp, P_foceanOm, P_flakeOm, P_fgrndOm, P_fgiceOm, P_zatmoOm, P_zicetopO, NP_O, P_zland_minO = NP_O,
       P_zland_maxO, NP_MERGE };
struct PlanesO { double *p[NP_MERGE]; int16_t *mergemask; };
struct Accum { double *giceO, *zicetopO, *contO, *zatmoO, *zland_min, *zland_max; int16_t *mask; };

__global__ void k_topo_init(Accum a, long nO) {                 // (:142, :173-182)
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nO) return;
    a.giceO[i] = 0.; a.zicetopO[i] = 0.; a.contO[i] = 0.; a.zatmoO[i] = 0.;
    a.zland_min[i] = DBL_MAX; a.zland_max[i] = DBL_MIN; a.mask[i] = 0;
}

// One sheet (:192-250): its four builds -- ice raw, ice correctA, land raw, land correctA -- each over a dimO of its own.
// Inside one build a sparse index occurs once and the four builds write different planes (the ice build's mask apart,
// which only ever receives 1), so one launch adds a sheet without atomics; the sheets follow each other on the stream.
struct SheetParts {
    int n[4];
    const int64_t *ts[4];
    const double *elev_ice, *wM_ice, *elev_land, *min_land, *max_land, *wM_land;
};
__global__ void k_topo_add_sheet(SheetParts s, const double *__restrict__ native, long nO, Accum a) {
    int d = blockIdx.x * blockDim.x + threadIdx.x, part = 0;
    while (part < 4 && d >= s.n[part]) d -= s.n[part++];
    if (part == 4) return;
    const int64_t iO = s.ts[part][d];
    if (iO < 0 || iO >= nO) return;
    if (part == 0) {
        a.zicetopO[iO] += s.elev_ice[d] * native[iO];
        a.mask[iO] = 1;
    } else if (part == 1) {
        a.giceO[iO] += s.wM_ice[d];
    } else if (part == 2) {
        a.zatmoO[iO] += s.elev_land[d] * native[iO];
        a.zland_min[iO] = topo_min(a.zland_min[iO], s.min_land[d]);
        a.zland_max[iO] = topo_max(a.zland_max[iO], s.max_land[d]);
    } else {
        a.contO[iO] += s.wM_land[d];
    }
}

__device__ __forceinline__ uint32_t nan_flags(const PlanesO &P, long iO, int shift) {
    uint32_t f = 0;
#pragma unroll
    for (int k = 0; k < NP_O; ++k)
        if (isnan(P.p[k][iO])) f |= 1u << (shift + k);
    return f;
}

// the sanity checks of the inputs (:159-167) and the per-cell update (:255-284); foceanOm_snap: foceanOm as this pass leaves
// it, for the single-cell-ocean pass
__global__ void k_topo_cells(PlanesO P, Accum a, const double *__restrict__ native, long nO, uint32_t *__restrict__ flags,
                             double *__restrict__ foceanOm_snap) {
    const long iO = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (iO >= nO) return;
    flags[iO] = nan_flags(P, iO, 0);
    int16_t mask = a.mask[iO];
    double foceanOm = P.p[P_foceanOm][iO];
    if (!(a.contO[iO] == 0.)) {
        const double by_areaO = 1. / native[iO];
        const double fgiceOp0 = P.p[P_fgiceOp][iO];
        const double diff_fgiceOp = a.giceO[iO] * by_areaO;
        if (diff_fgiceOp != 0) mask = 1;
        const double fgiceOp = fgiceOp0 + diff_fgiceOp;
        const double foceanOp = P.p[P_foceanOp][iO] - a.contO[iO] * by_areaO;
        const double zatmoOp = P.p[P_zatmoOp][iO] + a.zatmoO[iO] * by_areaO;
        P.p[P_fgiceOp][iO] = fgiceOp; P.p[P_foceanOp][iO] = foceanOp; P.p[P_zatmoOp][iO] = zatmoOp;
        if (fgiceOp != 0)
            P.p[P_zicetopO][iO] = (P.p[P_zicetopO][iO] * fgiceOp0 + a.zicetopO[iO] * by_areaO * diff_fgiceOp) / fgiceOp;
        if ((foceanOp < 0.5) && (foceanOm == 1.0)) {
            const double fact = 1. / (1. - foceanOp);
            foceanOm = 0.0;
            const double fgiceOm = fgiceOp * fact;
            P.p[P_foceanOm][iO] = foceanOm; P.p[P_fgiceOm][iO] = fgiceOm;
            mask = 1;
            P.p[P_fgrndOm][iO] = 1.0 - fgiceOm - P.p[P_flakeOm][iO];
            P.p[P_zatmoOm][iO] = zatmoOp * fact;
        }
    }
    P.mergemask[iO] = mask;
    foceanOm_snap[iO] = foceanOm;
}

// the single-cell-ocean pass from the snapshot (:291-313; DESIGN.md 17 on why one parallel pass equals the sequential one), the
// sanity checks of the outputs (:317-326), the unset zland_* (:329-336) and the count of failing checks
__global__ void k_topo_finish(PlanesO P, Accum a, const double *__restrict__ snap, int IM, int JM, uint32_t *__restrict__ flags,
                              unsigned long long *__restrict__ nerr) {
    const long nO = (long)IM * JM;
    const long iO = (long)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t f = 0;
    if (iO < nO) {
        const int j = (int)(iO / IM), i = (int)(iO % IM);
        if (!((i == 0) || (i == IM - 1) || (j == 0) || (j == JM - 1))) {
            if (snap[iO - IM] == 0. && snap[iO + IM] == 0. && snap[iO - 1] == 0. && snap[iO + 1] == 0. && snap[iO] == 1. &&
                P.p[P_foceanOp][iO] != 1.) {
                const double denom = 1. - P.p[P_foceanOp][iO];
                const double fact = 1. / denom;
                P.p[P_foceanOm][iO] = 0.0;
                const double fgiceOm = P.p[P_fgiceOp][iO] * fact;
                P.p[P_fgiceOm][iO] = fgiceOm;
                P.p[P_fgrndOm][iO] = 1.0 - fgiceOm - P.p[P_flakeOm][iO];
                P.p[P_zatmoOm][iO] = P.p[P_zatmoOp][iO] * fact;
            }
        }
        f = flags[iO] | nan_flags(P, iO, NP_O);
        const double all_frac = P.p[P_foceanOm][iO] + P.p[P_fgrndOm][iO] + P.p[P_flakeOm][iO] + P.p[P_fgiceOm][iO];
        if (fabs(all_frac - 1.0) > 1.e-13) f |= 1u << (2 * NP_O);
        flags[iO] = f;
        const bool merged = P.mergemask[iO] != 0;
        P.p[P_zland_minO][iO] = merged ? a.zland_min[iO] : NAN;
        P.p[P_zland_maxO][iO] = merged ? a.zland_max[iO] : NAN;
    }
    add_to_launch_total((unsigned long long)__popc(f), nerr);
}

struct SheetBuild {
    ibh_sparse_set dimO[4], dimI;
    std::unique_ptr<ibh_weighted> w[4];
    DevBuf<double> elev_ice, elev_land, min_land, max_land;
};

void check_merge_args(const ibh_regrid_matrices *const *lands, int nlands, const ibh_regrid_matrices *const *ices, int nices, int32_t imO,
                      int32_t jmO, const ibh_regridder **rg0_out) {
    IBH_CHECK(nlands >= 0 && nices >= 0, "merge_topoO: negative sheet count");
    IBH_CHECK(nlands == nices, "merge_topoO: %d land masks (emI_lands) for %d ice masks (emI_ices)", nlands, nices);
    IBH_CHECK(nices == 0 || (lands && ices), "merge_topoO: null mask list");
    IBH_CHECK(imO > 0 && jmO > 0, "merge_topoO: the ocean grid is %d x %d", imO, jmO);
    const ibh_regridder *rg0 = nullptr;
    for (int k = 0; k < nices; ++k) {
        IBH_CHECK(lands[k] && lands[k]->rg && ices[k] && ices[k]->rg, "merge_topoO: sheet %d is null", k);
        const ibh_regridder *rg = ices[k]->rg;
        IBH_CHECK(lands[k]->rg == rg, "merge_topoO: sheet %d: emI_lands and emI_ices belong to different ice regridders", k);
        check_current_device(rg->device, "regridder");
        if (lands[k]->sigma[0] != 0 || lands[k]->sigma[1] != 0 || lands[k]->sigma[2] != 0 || ices[k]->sigma[0] != 0 || ices[k]->sigma[1] != 0 ||
            ices[k]->sigma[2] != 0)
            fail(IBH_EINVAL, "merge_topoO: sheet %d has a non-zero sigma", k);
        IBH_CHECK((int64_t)imO * jmO == rg->nA, "merge_topoO: sheet %d: imO*jmO = %lld but its ocean grid has nA=%lld cells", k,
                  (long long)imO * jmO, (long long)rg->nA);
        if (!rg0) rg0 = rg;
        IBH_CHECK(rg->nA == rg0->nA && rg->A_to_sparse == rg0->A_to_sparse && rg->A_native == rg0->A_native,
                  "merge_topoO: sheet %d lives on another ocean grid than sheet 0", k);
    }
    *rg0_out = rg0;
}

// planes: device pointers; flags: device [nO]; returns the number of failing checks
int64_t merge_topoO(const ibh_regrid_matrices *const *lands, const ibh_regrid_matrices *const *ices, int nsheets, const ibh_regridder *rg0,
                    int32_t imO, int32_t jmO, const PlanesO &P, uint32_t *flags, hipStream_t st) {
    const long nO = (long)imO * jmO;
    const dim3 grid((unsigned)ceil_div(nO, T));
    DevBuf<double> acc((size_t)nO * 7), native((size_t)nO);
    DevBuf<int16_t> mask((size_t)nO);
    DevBuf<unsigned long long> nerr(1);
    Accum a{acc.p, acc.p + nO, acc.p + 2 * nO, acc.p + 3 * nO, acc.p + 4 * nO, acc.p + 5 * nO, mask.p};
    double *snap = acc.p + 6 * nO;
    hipLaunchKernelGGL(k_topo_init, grid, dim3(T), 0, st, a, nO);
    IBH_HIP(hipGetLastError());
    IBH_HIP(hipMemsetAsync(nerr.p, 0, sizeof(unsigned long long), st));
    std::vector<double> native_h((size_t)nO, 0.);           // agridA->native_area(dim.to_dense(iO)), by sparse index
    if (rg0) {
        for (size_t d = 0; d < rg0->A_to_sparse.size(); ++d) {
            const int64_t iO = rg0->A_to_sparse[d];
            if (iO >= 0 && iO < nO) native_h[(size_t)iO] = rg0->A_native[d];
        }
    }
    native.upload(native_h.data(), (size_t)nO, st);
    const double zero[3] = {0, 0, 0};
    const char *const specs[2] = {"AvI", "AvI"};
    const int32_t scale[2] = {1, 0}, correctA[2] = {0, 1};  // paramsO_rawA, paramsO_correctA (:184-189)
    for (int k = 0; k < nsheets; ++k) {
        SheetBuild b;
        const ibh_regridder *rg = ices[k]->rg;
        b.dimI.make_identity(rg->nI);
        const ibh_regrid_matrices *rms[2] = {ices[k], lands[k]};
        for (int m = 0; m < 2; ++m) {
            ibh_sparse_set *d0[2] = {&b.dimO[2 * m], &b.dimO[2 * m + 1]}, *d1[2] = {&b.dimI, &b.dimI};
            ibh_weighted *out[2] = {nullptr, nullptr};
            assemble_batch(rms[m], 2, specs, d0, d1, scale, correctA, zero, out);
            b.w[2 * m].reset(out[0]); b.w[2 * m + 1].reset(out[1]);
        }
        if (st != hipStreamPerThread) IBH_HIP(hipStreamSynchronize(hipStreamPerThread));
        SheetParts s{};
        int total = 0;
        for (int q = 0; q < 4; ++q) {
            IBH_CHECK(b.w[q]->nrow == b.dimO[q].n() && b.w[q]->ncol == rg->nI, "internal: merge_topoO: an OvI disagrees with its sets");
            s.n[q] = b.w[q]->nrow;
            s.ts[q] = s.n[q] ? b.dimO[q].device_to_sparse(s.n[q], st) : nullptr;
            total += s.n[q];
        }
        b.elev_ice.alloc((size_t)s.n[0]); b.elev_land.alloc((size_t)s.n[2]); b.min_land.alloc((size_t)s.n[2]); b.max_land.alloc((size_t)s.n[2]);
        row_stats(*b.w[0], ices[k]->elevmaskI.p, b.elev_ice.p, nullptr, nullptr, st);
        row_stats(*b.w[2], lands[k]->elevmaskI.p, b.elev_land.p, b.min_land.p, b.max_land.p, st);
        s.elev_ice = b.elev_ice.p; s.wM_ice = b.w[1]->wM.p;
        s.elev_land = b.elev_land.p; s.min_land = b.min_land.p; s.max_land = b.max_land.p; s.wM_land = b.w[3]->wM.p;
        if (total) {
            hipLaunchKernelGGL(k_topo_add_sheet, dim3((unsigned)ceil_div(total, T)), dim3(T), 0, st, s, native.p, nO, a);
            IBH_HIP(hipGetLastError());
        }
        IBH_HIP(hipStreamSynchronize(st));      // the sheet's matrices and sets go away
    }
    hipLaunchKernelGGL(k_topo_cells, grid, dim3(T), 0, st, P, a, native.p, nO, flags, snap);
    hipLaunchKernelGGL(k_topo_finish, grid, dim3(T), 0, st, P, a, snap, (int)imO, (int)jmO, flags, nerr.p);
    IBH_HIP(hipGetLastError());
    unsigned long long n = 0;
    readback_sync(&n, nerr.p, sizeof(n), st);   // the call's own host wait; the temporaries go away
    return (int64_t)n;
}

// ---- make_topoA -------------------------------------------------------------------------------------------------------------
// the nine double planes in the order of the argument lists (:584-592, :605-613), which is TopoABundles' order
enum { A_focean, A_flake, A_fgrnd, A_fgice, A_zatmo, A_zlake, A_zicetop, A_zland_min, A_zland_max, NP_A };
struct PlanesA { double *p[NP_A]; int16_t *mergemask; };

// Fills a plane with one value.  make_topoA no longer launches it (its weight-1 regrids take Hntr's constant weight); it stays
// because tests/test_topo_kernels.py holds the kernel inventory of this unit.
__global__ void k_topo_fill(double *__restrict__ p, long n, double v) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// _RegridMinMax (:555-579) behind Hntr::scaled_regrid_matrix (hntr.hpp:205-244): a destination cell receives one add() per source
// cell of its window JMIN..JMAX x IMIN..IMAX (columns modulo the source grid), whatever the weight; OR / min / max are free of
// the order.  One thread per destination cell; then the conversion of the untouched cells (:651-655).
struct Windows { const int32_t *IMIN, *IMAX, *JMIN, *JMAX; int imS, jmS, imD, jmD; };
__global__ void k_topoa_window(Windows w, const double *__restrict__ zminO, const double *__restrict__ zmaxO, const int16_t *__restrict__ maskO,
                               double *__restrict__ zminA, double *__restrict__ zmaxA, int16_t *__restrict__ maskA) {
    const long ij = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (ij >= (long)w.imD * w.jmD) return;
    const int JB = (int)(ij / w.imD), IB = (int)(ij % w.imD);
    double lo = DBL_MAX, hi = DBL_MIN;
    int16_t m = 0;
    for (int JA = w.JMIN[JB]; JA <= w.JMAX[JB]; ++JA) {
        if (JA < 1 || JA > w.jmS) continue;
        for (int IAREV = w.IMIN[IB]; IAREV <= w.IMAX[IB]; ++IAREV) {
            const int IA = ((IAREV - 1) % w.imS + w.imS) % w.imS;
            const long iO = IA + (long)w.imS * (JA - 1);
            if (maskO[iO]) {
                m = 1;
                lo = topo_min(lo, zminO[iO]);
                hi = topo_max(hi, zmaxO[iO]);
            }
        }
    }
    maskA[ij] = m;
    zminA[ij] = lo == DBL_MAX ? NAN : lo;
    zmaxA[ij] = hi == DBL_MIN ? NAN : hi;
}

// merge_poles (:538-550) on the nine planes: one lane per plane takes the first row, then the last, summing over ascending i
__global__ void k_topoa_poles(PlanesA P, int im, int jm) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= NP_A) return;
    double *var = P.p[k];
    for (int q = 0; q < 2; ++q) {
        double *row = var + (long)(q == 0 ? 0 : jm - 1) * im;
        double sum = 0;
        for (int i = 0; i < im; ++i) sum += row[i];
        const double mean = sum / (double)im;
        for (int i = 0; i < im; ++i) row[i] = mean;
    }
}

__global__ void k_topoa_init3(double *__restrict__ fhc, double *__restrict__ elevE, int16_t *__restrict__ underice, long n) {    // (:696-698)
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fhc[i] = 0; elevE[i] = NAN; underice[i] = UI_UNUSED;
}

// Segment 0 (:706-731): one thread per row of AAmvEAm (an A cell: at most nhc entries).  An entry of the matrix is unique,
// so its cell of fhc receives one add onto 0.  A bad entry is not written anywhere; the smallest bad entry is reported.
__global__ void k_topoa_classes(Csr M, const int64_t *__restrict__ tsA, const int64_t *__restrict__ tsE, HcIndexing s, int32_t nhc, int64_t nA,
                                const int16_t *__restrict__ underice_hc, double *__restrict__ fhc, int16_t *__restrict__ underice,
                                uint32_t *__restrict__ bad) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M.nrow) return;
    const int64_t iA = tsA[r];
    for (int e = M.rowptr[r]; e < M.rowptr[r + 1]; ++e) {
        const int64_t iE = tsE[M.colind[e]];
        int64_t iA2, ihc;
        s.split(iE, iA2, ihc);
        if (iA2 != iA || ihc < 0 || ihc >= nhc || iA < 0 || iA >= nA) { atomicMin(bad, (uint32_t)e); continue; }
        fhc[ihc * nA + iA] += M.val[e];
        underice[ihc * nA + iA] = underice_hc[ihc];
    }
}

// the south-pole mean of fhc (:735-740): one lane per class
__global__ void k_topoa_fhc_pole(double *__restrict__ fhc, int32_t nhc, long nA, int im) {
    const int ihc = blockIdx.x * blockDim.x + threadIdx.x;
    if (ihc >= nhc) return;
    double *row = fhc + ihc * nA;
    double fhc_sum = 0;
    for (int i = 0; i < im; ++i) fhc_sum += row[i];
    const double fhc_mean = fhc_sum / (double)im;
    for (int i = 0; i < im; ++i) row[i] = fhc_mean;
}

// class levels and vertical ghosts (:744-792), the sea-land segment (:834-846) and the two sanity checks (:857-888): one
// thread per A cell
__global__ void k_topoa_levels(PlanesA P, const double *__restrict__ hcdefs, int32_t nhc, int32_t nhc_local, long nA,
                               double *__restrict__ fhc, double *__restrict__ elevE, int16_t *__restrict__ underice,
                               uint32_t *__restrict__ flags, unsigned long long *__restrict__ nerr) {
    const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t f = 0;
    if (c < nA) {
        const double zland_min = P.p[A_zland_min][c], zland_max = P.p[A_zland_max][c];
        int zland_minhc = INT_MAX, zland_maxhc = INT_MIN;
        for (int ihc = 0; ihc < nhc_local; ++ihc) {
            const double e = hcdefs[ihc];
            elevE[ihc * nA + c] = e;
            if (e < zland_min) zland_minhc = ihc;
            if (e <= zland_max) zland_maxhc = ihc;
        }
        if (fabs(P.p[A_focean][c] - 1.0) > 1.e-14) {
            const int minghost = max(0, zland_minhc - 1);
            const int maxghost = min(zland_maxhc + 2, nhc_local - 1);
            for (int ihc = minghost; ihc <= maxghost; ++ihc) {
                if (fhc[ihc * nA + c] == 0) {
                    fhc[ihc * nA + c] = 1.e-30;
                    underice[ihc * nA + c] = UI_VGHOST;
                }
            }
        }
        for (int ihc = nhc_local; ihc < nhc; ++ihc) elevE[ihc * nA + c] = hcdefs[ihc];
        const double fgice = P.p[A_fgice][c];
        if (fgice > 0) {
            fhc[(long)nhc * nA + c] = (fgice == 0 ? 0 : 1e-30);
            underice[(long)nhc * nA + c] = UI_SEALAND;
        }
        elevE[(long)nhc * nA + c] = P.p[A_zatmo][c];
        const double all_frac = P.p[A_focean][c] + P.p[A_fgrnd][c] + P.p[A_flake][c] + fgice;
        if (fabs(all_frac - 1.0) > 1.e-13) f |= 1u;
        double all_fhc = 0;
        for (int ihc = 0; ihc <= nhc; ++ihc) all_fhc += fhc[ihc * nA + c];
        all_fhc += 1.0;
        if (all_fhc != 1.0 && fabs(all_fhc - 2.0) > 1.e-13) f |= 2u;
        flags[c] = f;
    }
    add_to_launch_total((unsigned long long)__popc(f), nerr);
}

struct TopoAArgs {
    int32_t imO, jmO, imA, jmA, nhc;
    double offiO, dlatO, offiA, dlatA;
    HcIndexing hc;          // indexingHCA
    const double *hcdefs;
    const int16_t *underice_hc;
    const ibh_weighted *AAmvEAm;
};

void check_topoA_args(const TopoAArgs &t) {
    IBH_CHECK(t.imO > 0 && t.jmO > 0 && t.imA > 0 && t.jmA > 0, "make_topoA: the grids are %d x %d and %d x %d", t.imO, t.jmO, t.imA, t.jmA);
    IBH_CHECK(t.nhc >= 0 && (t.nhc == 0 || (t.hcdefs && t.underice_hc)), "make_topoA: nhc=%d or null hcdefs / underice_hc", t.nhc);
    IBH_CHECK(t.hc.sA > 0 && t.hc.sHC > 0, "make_topoA: indexingHCA strides (%lld,%lld) must be positive", (long long)t.hc.sA, (long long)t.hc.sHC);
    IBH_CHECK(t.AAmvEAm != nullptr, "make_topoA: null AAmvEAm");
    check_current_device(t.AAmvEAm->device, "AAmvEAm");
    IBH_CHECK((int64_t)(t.nhc + 1) * t.imA * t.jmA < (1ll << 31), "make_topoA: %d classes of %d x %d cells overflow int32", t.nhc + 1, t.imA, t.jmA);
    const ibh_weighted &M = *t.AAmvEAm;
    IBH_CHECK(M.dims[0].get() && M.dims[1].get() && M.dims[0]->n() == M.nrow && M.dims[1]->n() == M.ncol,
              "make_topoA: AAmvEAm is %d x %d but its sets do not hold that many entries", M.nrow, M.ncol);
}

// the message of the smallest bad entry e of Segment 0, made on the host from the matrix's small tables
[[noreturn]] void fail_bad_entry(const TopoAArgs &t, uint32_t e, hipStream_t st) {
    const ibh_weighted &M = *t.AAmvEAm;
    std::vector<int32_t> rp((size_t)M.nrow + 1);
    int32_t col = 0;
    IBH_HIP(hipMemcpyAsync(rp.data(), M.rowptr.p, sizeof(int32_t) * rp.size(), hipMemcpyDeviceToHost, st));
    IBH_HIP(hipMemcpyAsync(&col, M.colind.p + e, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    IBH_HIP(hipStreamSynchronize(st));
    int r = 0;
    while (r + 1 < M.nrow && (uint32_t)rp[(size_t)r + 1] <= e) ++r;
    const int64_t iA = M.dims[0]->to_sparse_host()[r], iE = M.dims[1]->to_sparse_host()[col];
    int64_t iA2, ihc;
    t.hc.split(iE, iA2, ihc);
    const int64_t nA = (int64_t)t.imA * t.jmA;
    if (iA2 != iA) fail(IBH_EINVAL, "make_topoA: Matrix is non-local: iA=%ld, iE=%ld, iA2=%ld", (long)iA, (long)iE, (long)iA2);
    if (ihc < 0 || ihc >= t.nhc) fail(IBH_EINVAL, "make_topoA: ihc out of range [0,%d): %ld (iA=%ld, iE=%ld)", t.nhc, (long)ihc, (long)iA, (long)iE);
    fail(IBH_EINVAL, "make_topoA: iA out of range [0,%ld): %ld (iE=%ld)", (long)nA, (long)iA, (long)iE);
}

// O: the ten ocean planes (device), A / fhc / elevE / underice / flags: the outputs (device); returns the failing checks
int64_t make_topoA(const TopoAArgs &t, const double *const *O, const int16_t *mergemaskO, const PlanesA &P, double *fhc, double *elevE,
                   int16_t *underice, uint32_t *flags, hipStream_t st) {
    const long nO = (long)t.imO * t.jmO, nA = (long)t.imA * t.jmA;
    const ibh_weighted &M = *t.AAmvEAm;
    // Hntr hntr_AvO(17.17, hspecA, hspecO): B = the atmosphere grid, A = the ocean grid (:621)
    ibh_hntr *hraw = nullptr;
    rethrow(ibh_hntr_create(&hraw, t.imO, t.jmO, t.offiO, t.dlatO, t.imA, t.jmA, t.offiA, t.dlatA, 0.));
    std::unique_ptr<ibh_hntr, int (*)(ibh_hntr *)> hntr(hraw, ibh_hntr_destroy);
    std::vector<double> SINA((size_t)t.jmO + 1), SINB((size_t)t.jmA + 1), FMIN((size_t)t.imA), FMAX((size_t)t.imA), GMIN((size_t)t.jmA),
        GMAX((size_t)t.jmA);
    std::vector<int32_t> win((size_t)2 * t.imA + 2 * t.jmA);
    int32_t *IMIN = win.data(), *IMAX = IMIN + t.imA, *JMIN = IMAX + t.imA, *JMAX = JMIN + t.jmA;
    rethrow(ibh_hntr_partition(t.imO, t.jmO, t.offiO, t.dlatO, t.imA, t.jmA, t.offiA, t.dlatA, SINA.data(), SINB.data(), IMIN, IMAX, FMIN.data(),
                               FMAX.data(), JMIN, JMAX, GMIN.data(), GMAX.data()));
    for (int j = 0; j < t.jmA; ++j)
        IBH_CHECK(JMIN[j] >= 1 && JMAX[j] <= t.jmO, "internal: make_topoA: row window [%d, %d] outside the ocean grid", JMIN[j], JMAX[j]);
    const int32_t nhc = t.nhc;
    int32_t nhc_local = 0;                                  // the leading run of UI_LOCALICE (:686-690)
    while (nhc_local < nhc && t.underice_hc[nhc_local] == UI_LOCALICE) ++nhc_local;

    DevBuf<int32_t> dwin;
    DevBuf<double> dhc;
    DevBuf<int16_t> dui;
    DevBuf<unsigned long long> stat(2);                     // [0] failing checks, [1] (its low word) the smallest bad entry
    unsigned long long *nerr = stat.p;
    uint32_t *status = reinterpret_cast<uint32_t *>(stat.p + 1);
    dwin.upload(win.data(), win.size(), st);
    dhc.upload(t.hcdefs, (size_t)nhc, st);
    dui.upload(t.underice_hc, (size_t)nhc, st);
    IBH_HIP(hipMemsetAsync(nerr, 0, sizeof(unsigned long long), st));
    IBH_HIP(hipMemsetAsync(status, 0xFF, sizeof(unsigned long long), st));
    // (:623-630): six regrids under the constant weight 1 (const_array(shape, 1.0)), zicetop under fgiceOm
    for (int k = 0; k <= A_zicetop; ++k)
        rethrow(ibh_hntr_regrid_typed_device(hntr.get(), k == A_zicetop ? O[A_fgice] : nullptr, IBH_HNTR_F64, 0, 1., O[k], IBH_HNTR_F64, 1,
                                             nO, P.p[k], nA, 0, 1., 0., st));
    Windows w{dwin.p, dwin.p + t.imA, dwin.p + 2 * t.imA, dwin.p + 2 * t.imA + t.jmA, t.imO, t.jmO, t.imA, t.jmA};
    hipLaunchKernelGGL(k_topoa_window, dim3((unsigned)ceil_div(nA, T)), dim3(T), 0, st, w, O[A_zland_min], O[A_zland_max], mergemaskO,
                       P.p[A_zland_min], P.p[A_zland_max], P.mergemask);
    hipLaunchKernelGGL(k_topoa_poles, dim3(1), dim3(64), 0, st, P, (int)t.imA, (int)t.jmA);
    const long n3 = (long)(nhc + 1) * nA;
    hipLaunchKernelGGL(k_topoa_init3, dim3((unsigned)ceil_div(n3, T)), dim3(T), 0, st, fhc, elevE, underice, n3);
    IBH_HIP(hipGetLastError());
    if (M.nrow && M.nnz) {
        const int64_t *tsA = M.dims[0]->device_to_sparse(M.nrow, st), *tsE = M.dims[1]->device_to_sparse(M.ncol, st);
        hipLaunchKernelGGL(k_topoa_classes, dim3((unsigned)ceil_div(M.nrow, T)), dim3(T), 0, st, view(M), tsA, tsE, t.hc, nhc,
                           (int64_t)nA, dui.p, fhc, underice, status);
        IBH_HIP(hipGetLastError());
    }
    if (nhc) hipLaunchKernelGGL(k_topoa_fhc_pole, dim3((unsigned)ceil_div(nhc, 64)), dim3(64), 0, st, fhc, nhc, nA, (int)t.imA);
    hipLaunchKernelGGL(k_topoa_levels, dim3((unsigned)ceil_div(nA, T)), dim3(T), 0, st, P, dhc.p, nhc, nhc_local, nA, fhc, elevE, underice, flags,
                       nerr);
    IBH_HIP(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    readback_sync(h, stat.p, sizeof(h), st);                // the call's one host wait
    const uint32_t bad = (uint32_t)(h[1] & 0xFFFFFFFFull);
    if (bad != 0xFFFFFFFFu) fail_bad_entry(t, bad, st);
    return (int64_t)h[0];
}

void check_planes(const void *const *p, int n, const char *what) {
    IBH_CHECK(p != nullptr, "%s: null plane list", what);
    for (int k = 0; k < n; ++k) IBH_CHECK(p[k] != nullptr, "%s: plane %d is null", what, k);
}

}  // namespace
}  // namespace ibh

using namespace ibh;
extern "C" {

int ibh_weighted_row_stats_device(const ibh_weighted *w, const double *d_x, double *d_sum, double *d_min, double *d_max, void *stream) {
    return guarded([&] {
        IBH_CHECK(w != nullptr, "row_stats: null Weighted handle");
        check_current_device(w->device, "Weighted handle");
        IBH_CHECK(w->nrow >= 0 && w->nnz >= 0, "row_stats: the matrix is not built");
        IBH_CHECK(d_x != nullptr || w->nnz == 0, "row_stats: null x for a matrix of %lld entries", (long long)w->nnz);
        row_stats(*w, d_x, d_sum, d_min, d_max, static_cast<hipStream_t>(stream));
    });
}

int ibh_modele_merge_topoO_device(const ibh_regrid_matrices *const *emI_lands, int32_t nlands, const ibh_regrid_matrices *const *emI_ices,
                                  int32_t nices, int32_t imO, int32_t jmO, double eq_rad, double *const *d_planes, int16_t *d_mergemaskOm,
                                  uint32_t *d_flags, int64_t *nerrors, void *stream) {
    (void)eq_rad;
    return guarded([&] {
        const ibh_regridder *rg0 = nullptr;
        check_merge_args(emI_lands, nlands, emI_ices, nices, imO, jmO, &rg0);
        check_planes(reinterpret_cast<const void *const *>(d_planes), NP_MERGE, "merge_topoO");
        IBH_CHECK(d_mergemaskOm && d_flags && nerrors, "merge_topoO: null mergemaskOm, flags or nerrors");
        require_device();
        PlanesO P;
        for (int k = 0; k < NP_MERGE; ++k) P.p[k] = d_planes[k];
        P.mergemask = d_mergemaskOm;
        *nerrors = merge_topoO(emI_lands, emI_ices, nices, rg0, imO, jmO, P, d_flags, static_cast<hipStream_t>(stream));
    });
}

int ibh_modele_merge_topoO(const ibh_regrid_matrices *const *emI_lands, int32_t nlands, const ibh_regrid_matrices *const *emI_ices, int32_t nices,
                           int32_t imO, int32_t jmO, double eq_rad, double *const *planes, int16_t *mergemaskOm, uint32_t *flags,
                           int64_t *nerrors) {
    (void)eq_rad;
    return guarded([&] {
        const ibh_regridder *rg0 = nullptr;
        check_merge_args(emI_lands, nlands, emI_ices, nices, imO, jmO, &rg0);
        check_planes(reinterpret_cast<const void *const *>(planes), NP_MERGE, "merge_topoO");
        IBH_CHECK(mergemaskOm && flags && nerrors, "merge_topoO: null mergemaskOm, flags or nerrors");
        require_device();
        hipStream_t st = hipStreamPerThread;
        const size_t nO = (size_t)imO * jmO;
        DevBuf<double> d(nO * NP_MERGE);
        DevBuf<int16_t> dm(nO);
        DevBuf<uint32_t> df(nO);
        PlanesO P;
        for (int k = 0; k < NP_MERGE; ++k) P.p[k] = d.p + nO * k;
        P.mergemask = dm.p;
        for (int k = 0; k < NP_O; ++k) IBH_HIP(hipMemcpyAsync(P.p[k], planes[k], sizeof(double) * nO, hipMemcpyHostToDevice, st));
        const int64_t n = merge_topoO(emI_lands, emI_ices, nices, rg0, imO, jmO, P, df.p, st);
        for (int k = 0; k < NP_MERGE; ++k) IBH_HIP(hipMemcpyAsync(planes[k], P.p[k], sizeof(double) * nO, hipMemcpyDeviceToHost, st));
        IBH_HIP(hipMemcpyAsync(mergemaskOm, dm.p, sizeof(int16_t) * nO, hipMemcpyDeviceToHost, st));
        IBH_HIP(hipMemcpyAsync(flags, df.p, sizeof(uint32_t) * nO, hipMemcpyDeviceToHost, st));
        IBH_HIP(hipStreamSynchronize(st));
        *nerrors = n;
    });
}

int ibh_modele_make_topoA_device(const double *const *d_planesO, const int16_t *d_mergemaskOm, int32_t imO, int32_t jmO, double offiO, double dlatO,
                                 int32_t imA, int32_t jmA, double offiA, double dlatA, int64_t hc_stride_A, int64_t hc_stride_HC,
                                 const double *hcdefs, const int16_t *underice_hc, int32_t nhc, const ibh_weighted *AAmvEAm,
                                 double *const *d_planesA, int16_t *d_mergemaskA, double *d_fhc3, double *d_elevE3, int16_t *d_underice3,
                                 uint32_t *d_flags, int64_t *nerrors, void *stream) {
    return guarded([&] {
        const TopoAArgs t{imO, jmO, imA, jmA, nhc, offiO, dlatO, offiA, dlatA, HcIndexing{hc_stride_A, hc_stride_HC}, hcdefs, underice_hc, AAmvEAm};
        check_topoA_args(t);
        check_planes(reinterpret_cast<const void *const *>(d_planesO), NP_A, "make_topoA: O");
        check_planes(reinterpret_cast<const void *const *>(d_planesA), NP_A, "make_topoA: A");
        IBH_CHECK(d_mergemaskOm && d_mergemaskA && d_fhc3 && d_elevE3 && d_underice3 && d_flags && nerrors, "make_topoA: null argument");
        require_device();
        PlanesA P;
        for (int k = 0; k < NP_A; ++k) P.p[k] = d_planesA[k];
        P.mergemask = d_mergemaskA;
        *nerrors = make_topoA(t, d_planesO, d_mergemaskOm, P, d_fhc3, d_elevE3, d_underice3, d_flags, static_cast<hipStream_t>(stream));
    });
}

int ibh_modele_make_topoA(const double *const *planesO, const int16_t *mergemaskOm, int32_t imO, int32_t jmO, double offiO, double dlatO,
                          int32_t imA, int32_t jmA, double offiA, double dlatA, int64_t hc_stride_A, int64_t hc_stride_HC, const double *hcdefs,
                          const int16_t *underice_hc, int32_t nhc, const ibh_weighted *AAmvEAm, double *const *planesA, int16_t *mergemaskA,
                          double *fhc3, double *elevE3, int16_t *underice3, uint32_t *flags, int64_t *nerrors) {
    return guarded([&] {
        const TopoAArgs t{imO, jmO, imA, jmA, nhc, offiO, dlatO, offiA, dlatA, HcIndexing{hc_stride_A, hc_stride_HC}, hcdefs, underice_hc, AAmvEAm};
        check_topoA_args(t);
        check_planes(reinterpret_cast<const void *const *>(planesO), NP_A, "make_topoA: O");
        check_planes(reinterpret_cast<const void *const *>(planesA), NP_A, "make_topoA: A");
        IBH_CHECK(mergemaskOm && mergemaskA && fhc3 && elevE3 && underice3 && flags && nerrors, "make_topoA: null argument");
        require_device();
        hipStream_t st = hipStreamPerThread;
        const size_t nO = (size_t)imO * jmO, nA = (size_t)imA * jmA, n3 = nA * (size_t)(nhc + 1);
        DevBuf<double> dO(nO * NP_A), dA(nA * NP_A), d3(n3 * 2);
        DevBuf<int16_t> dmO(nO), dmA(nA), dui(n3);
        DevBuf<uint32_t> df(nA);
        const double *O[NP_A];
        PlanesA P;
        for (int k = 0; k < NP_A; ++k) {
            O[k] = dO.p + nO * k; P.p[k] = dA.p + nA * k;
            IBH_HIP(hipMemcpyAsync(dO.p + nO * k, planesO[k], sizeof(double) * nO, hipMemcpyHostToDevice, st));
        }
        IBH_HIP(hipMemcpyAsync(dmO.p, mergemaskOm, sizeof(int16_t) * nO, hipMemcpyHostToDevice, st));
        P.mergemask = dmA.p;
        const int64_t n = make_topoA(t, O, dmO.p, P, d3.p, d3.p + n3, dui.p, df.p, st);
        for (int k = 0; k < NP_A; ++k) IBH_HIP(hipMemcpyAsync(planesA[k], P.p[k], sizeof(double) * nA, hipMemcpyDeviceToHost, st));
        IBH_HIP(hipMemcpyAsync(mergemaskA, dmA.p, sizeof(int16_t) * nA, hipMemcpyDeviceToHost, st));
        IBH_HIP(hipMemcpyAsync(fhc3, d3.p, sizeof(double) * n3, hipMemcpyDeviceToHost, st));
        IBH_HIP(hipMemcpyAsync(elevE3, d3.p + n3, sizeof(double) * n3, hipMemcpyDeviceToHost, st));
        IBH_HIP(hipMemcpyAsync(underice3, dui.p, sizeof(int16_t) * n3, hipMemcpyDeviceToHost, st));
        IBH_HIP(hipMemcpyAsync(flags, df.p, sizeof(uint32_t) * nA, hipMemcpyDeviceToHost, st));
        IBH_HIP(hipStreamSynchronize(st));
        *nerrors = n;
    });
}

}  // extern "C"
