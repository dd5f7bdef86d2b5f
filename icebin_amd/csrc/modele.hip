// modele.hip -- GCMRegridder_ModelE::regrid_matrices (slib/icebin/modele/GCMRegridder_ModelE.cpp:487-571) composed from the
// O-grid matrix builds (assemble.hip), Hntr's clipped overlap (hntr.hip) and ONE sparse product.
//
// Where things live.  Every matrix and every weight vector stays in HBM; the products, the re-numbered copies (crop_mvp) and
// the weight vectors are kernels below.  The bookkeeping of the GCM-grid-sized SETS (dimAOp -> dimAOm, dimEOm, dimEAm: at
// most nO * nhc keys) runs on the host, where ibh_sparse_set keeps its keys: it reads the sets' keys, the INDICES of EOpvAOp
// (one entry per elevation class of an ice-bearing O cell) and, for raw_EOvEA's "weight != 0" test, the vector wEOm.  No
// entry of an ice-sized matrix travels to the host.
#include <algorithm>
#include <cmath>
#include <memory>

#include "assemble.h"
#include "common.h"
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
void require_device();      // capi.hip
namespace {

inline long ceil_div(long a, long b) { return (a + b - 1) / b; }
void rethrow(int rc) { if (rc != IBH_OK) throw Error(rc, ibh_last_error()); }

struct Csr { const int32_t *rowptr, *colind; const double *val; int nrow; };
Csr view(const ibh_weighted &w) { return Csr{w.rowptr.p, w.colind.p, w.val.p, w.nrow}; }

// ---- C = L * R -------------------------------------------------------------------------------------------------------------
// Eigen's conservative sparse product: C(r, c) = sum_k L(r, k) * R(k, c) over k ascending, the first term assigned.  Row r of
// L lists its k ascending, so walking it and, per k, row k of R emits the terms of every (r, c) in that order; a stable
// ordering by (r, c) and sequential sums of equal keys (csr_from_device_triplets: setFromTriplets) finish it.
__global__ void k_prod_count(Csr L, const int32_t *__restrict__ Rptr, uint32_t *__restrict__ cnt, unsigned long long *__restrict__ total) {
    __shared__ unsigned long long part[4];
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long c = 0;
    if (r < L.nrow) {
        for (int e = L.rowptr[r]; e < L.rowptr[r + 1]; ++e) {
            const int k = L.colind[e];
            c += (unsigned long long)(Rptr[k + 1] - Rptr[k]);
        }
        cnt[r] = (uint32_t)c;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x / 64] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < (int)(blockDim.x / 64); ++w) s += part[w];
        if (s) atomicAdd(total, s);
    }
}
// LANES lanes per row of L: 1 for short rows of R (ice rows: a term or two), 64 where a row of R is an O cell's ice cells
template <int LANES>
__global__ void k_prod_emit(Csr L, Csr R, const uint32_t *__restrict__ pos, int32_t *__restrict__ row, int32_t *__restrict__ col,
                            double *__restrict__ term) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long r = t / LANES;
    const int lane = (int)(t % LANES);
    if (r >= L.nrow) return;
    uint32_t p = pos[r];
    for (int e = L.rowptr[r]; e < L.rowptr[r + 1]; ++e) {
        const int k = L.colind[e];
        const double l = L.val[e];
        const int b = R.rowptr[k], n = R.rowptr[k + 1] - b;
        for (int q = lane; q < n; q += LANES) {
            row[p + q] = (int32_t)r; col[p + q] = R.colind[b + q]; term[p + q] = l * R.val[b + q];
        }
        p += (uint32_t)n;
    }
}
void csr_product(const ibh_weighted &L, const ibh_weighted &R, ibh_weighted *out, hipStream_t st) {
    IBH_CHECK(L.ncol == R.nrow, "product: L has %d columns, R %d rows", L.ncol, R.nrow);
    Arena &A = arena();
    A.reset();
    const int T = 256, n = L.nrow;
    uint32_t *pos = A.get<uint32_t>((size_t)n + 1);
    unsigned long long *tot = A.get<unsigned long long>(1);
    IBH_HIP(hipMemsetAsync(tot, 0, sizeof(unsigned long long), st));
    if (n) hipLaunchKernelGGL(k_prod_count, dim3(ceil_div(n, T)), dim3(T), 0, st, view(L), R.rowptr.p, pos, tot);
    IBH_HIP(hipGetLastError());
    unsigned long long total = 0;
    readback_sync(&total, tot, sizeof(total), st);          // the one host wait of the product
    IBH_CHECK(total <= INT32_MAX, "product: %llu terms exceed INT32_MAX", total);
    exclusive_scan_u32(pos, pos, (size_t)n, pos + n, st);
    int32_t *row = A.get<int32_t>((size_t)total), *col = A.get<int32_t>((size_t)total);
    double *term = A.get<double>((size_t)total);
    if (n && total) {
        if (total >= 8ull * (unsigned long long)n)
            hipLaunchKernelGGL(k_prod_emit<64>, dim3(ceil_div((long)n * 64, T)), dim3(T), 0, st, view(L), view(R), pos, row, col, term);
        else
            hipLaunchKernelGGL(k_prod_emit<1>, dim3(ceil_div(n, T)), dim3(T), 0, st, view(L), view(R), pos, row, col, term);
    }
    IBH_HIP(hipGetLastError());
    csr_from_device_triplets(out, L.nrow, R.ncol, (int64_t)total, row, col, term, st);
}

// ---- crop_mvp (GCMRegridder_ModelE.cpp:285-307) ----------------------------------------------------------------------------
// index 0: row m of the result is row src[m] of `in` (-1: none), its values rounded once as rs[src[m]] * v (rs may be null).
// One wave per row: a row is an O cell's (or elevation class's) ice cells.
__global__ void k_crop_rows_count(const int32_t *__restrict__ inptr, const int32_t *__restrict__ src, int nout, uint32_t *__restrict__ cnt) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m < nout) cnt[m] = src[m] >= 0 ? (uint32_t)(inptr[src[m] + 1] - inptr[src[m]]) : 0u;
}
__global__ void k_crop_rows_fill(Csr in, const int32_t *__restrict__ src, const double *__restrict__ rs, int nout,
                                 const int32_t *__restrict__ outptr, int32_t *__restrict__ col, double *__restrict__ val) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long m = t >> 6;
    const int lane = (int)(t & 63);
    if (m >= nout || src[m] < 0) return;
    const int p = src[m], b = in.rowptr[p], n = in.rowptr[p + 1] - b, o = outptr[m];
    const double s = rs ? rs[p] : 1.;
    for (int q = lane; q < n; q += 64) {
        col[o + q] = in.colind[b + q];
        val[o + q] = rs ? s * in.val[b + q] : in.val[b + q];
    }
}
// index 1: column k of `in` becomes map[k] (-1: the entry is dropped); value (rs[i] * v) * cs[map[k]], each factor optional and
// each product rounded.  One thread per row (an ice or exchange cell: a few entries), which then puts its columns in
// ascending order again by insertion (map is one-to-one: no ties).
__global__ void k_crop_cols_count(Csr in, const int32_t *__restrict__ map, uint32_t *__restrict__ cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= in.nrow) return;
    uint32_t c = 0;
    for (int e = in.rowptr[i]; e < in.rowptr[i + 1]; ++e) c += map[in.colind[e]] >= 0 ? 1u : 0u;
    cnt[i] = c;
}
__global__ void k_crop_cols_fill(Csr in, const int32_t *__restrict__ map, const double *__restrict__ rs, const double *__restrict__ cs,
                                 const int32_t *__restrict__ outptr, int32_t *__restrict__ col, double *__restrict__ val) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= in.nrow) return;
    const int o = outptr[i];
    int n = 0;
    for (int e = in.rowptr[i]; e < in.rowptr[i + 1]; ++e) {
        const int k = map[in.colind[e]];
        if (k < 0) continue;
        double v = in.val[e];
        if (rs) v = rs[i] * v;
        if (cs) v = v * cs[k];
        int q = n++;
        for (; q > 0 && col[o + q - 1] > k; --q) { col[o + q] = col[o + q - 1]; val[o + q] = val[o + q - 1]; }
        col[o + q] = k; val[o + q] = v;
    }
}
// rowptr = scan(cnt) with the total at the end; returns nnz (one host wait)
int64_t finish_rowptr(uint32_t *cnt, int nrow, ibh_weighted *out, hipStream_t st) {
    out->rowptr.alloc((size_t)nrow + 1);
    uint32_t *ptr = reinterpret_cast<uint32_t *>(out->rowptr.p);
    exclusive_scan_u32(cnt, ptr, (size_t)nrow, ptr + nrow, st);
    uint32_t nnz = 0;
    readback_sync(&nnz, ptr + nrow, sizeof(nnz), st);
    IBH_CHECK(nnz < (1u << 31), "nnz overflows int32");
    out->nnz = nnz;
    out->colind.alloc(nnz); out->val.alloc(nnz);
    return nnz;
}
// d_src: device int32 [nout]
void crop_rows(const ibh_weighted &in, const int32_t *d_src, int nout, const double *d_rs, ibh_weighted *out, hipStream_t st) {
    Arena &A = arena();
    const int T = 256;
    uint32_t *cnt = A.get<uint32_t>((size_t)nout);
    if (nout) hipLaunchKernelGGL(k_crop_rows_count, dim3(ceil_div(nout, T)), dim3(T), 0, st, in.rowptr.p, d_src, nout, cnt);
    out->nrow = nout; out->ncol = in.ncol;
    if (finish_rowptr(cnt, nout, out, st))
        hipLaunchKernelGGL(k_crop_rows_fill, dim3(ceil_div((long)nout * 64, T)), dim3(T), 0, st, view(in), d_src, d_rs, nout, out->rowptr.p,
                           out->colind.p, out->val.p);
    IBH_HIP(hipGetLastError());
}
void crop_cols(const ibh_weighted &in, const int32_t *d_map, int ncol_out, const double *d_rs, const double *d_cs, ibh_weighted *out,
               hipStream_t st) {
    Arena &A = arena();
    const int T = 256, n = in.nrow;
    uint32_t *cnt = A.get<uint32_t>((size_t)n);
    if (n) hipLaunchKernelGGL(k_crop_cols_count, dim3(ceil_div(n, T)), dim3(T), 0, st, view(in), d_map, cnt);
    out->nrow = n; out->ncol = ncol_out;
    if (finish_rowptr(cnt, n, out, st))
        hipLaunchKernelGGL(k_crop_cols_fill, dim3(ceil_div(n, T)), dim3(T), 0, st, view(in), d_map, d_rs, d_cs, out->rowptr.p, out->colind.p,
                           out->val.p);
    IBH_HIP(hipGetLastError());
}

// ---- the small vectors --------------------------------------------------------------------------------------------------------
// compute_wAOm (topo.cpp:84-109): wAOm[k] = 0 + (1 / fcont_p) * wAOp[src[k]]; src[k] < 0 where fcont_p == 0 (no entry: 0)
__global__ void k_wAOm(const double *__restrict__ inv_fcont, const int32_t *__restrict__ src, const double *__restrict__ wAOp, int n,
                       double *__restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = src[k] >= 0 ? 0. + inv_fcont[k] * wAOp[src[k]] : 0.;
}
// y = (M * diag(d)) * w: y[r] = sum over the row's columns k ascending, from 0, of (M(r, k) * d[k]) * w[k]
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
__global__ void k_recip(const double *__restrict__ in, int n, double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = 1. / in[i];
}
__global__ void k_mul(const double *__restrict__ a, const double *__restrict__ b, int n, double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = a[i] * b[i];
}
__global__ void k_gather(const double *__restrict__ in, const int32_t *__restrict__ idx, long n, double *__restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[idx[i]];
}
// diag(s) * M in place: s[r] * M(r, k)
__global__ void k_scale_rows(const int32_t *__restrict__ rowptr, int nrow, const double *__restrict__ s, double *__restrict__ val) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrow) return;
    for (int e = rowptr[r]; e < rowptr[r + 1]; ++e) val[e] = s[r] * val[e];
}
__global__ void k_expand_rows(const int32_t *__restrict__ rowptr, int nrow, int32_t *__restrict__ row) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrow) return;
    for (int e = rowptr[r]; e < rowptr[r + 1]; ++e) row[e] = r;
}
void recip(const double *in, int n, DevBuf<double> &out, hipStream_t st) {
    out.alloc((size_t)n);
    if (n) hipLaunchKernelGGL(k_recip, dim3(ceil_div(n, 256)), dim3(256), 0, st, in, n, out.p);
}
// the transpose's CSR (rows few and short: a matrix over the GCM grids)
void transpose_csr(const ibh_weighted &in, ibh_weighted *out, hipStream_t st) {
    Arena &A = arena();
    A.reset();
    int32_t *row = A.get<int32_t>((size_t)in.nnz);
    if (in.nrow) hipLaunchKernelGGL(k_expand_rows, dim3(ceil_div(in.nrow, 256)), dim3(256), 0, st, in.rowptr.p, in.nrow, row);
    IBH_HIP(hipGetLastError());
    csr_from_device_triplets(out, in.ncol, in.nrow, in.nnz, in.colind.p, row, in.val.p, st);
}
template <class T>
void upload(DevBuf<T> &b, const std::vector<T> &h, hipStream_t st) { b.alloc(h.size()); b.upload(h.data(), h.size(), st); }

std::unique_ptr<ibh_weighted> o_matrix(const ibh_modele_matrices *mm, const char *name, ibh_sparse_set *d0, ibh_sparse_set *d1, int correctA) {
    const double zero[3] = {0, 0, 0};
    ibh_weighted *w = nullptr;
    assemble_matrix(mm->rmO, name, d0, d1, 0, correctA, zero, &w);
    return std::unique_ptr<ibh_weighted>(w);
}

// ---- ComputeXAmvGp_Helper (:168-280) and the two generators (:318-368, :379-433) ------------------------------------------------
// dimXAm, dimGp: the caller's sets (copies: the caller's own change only when the matrix is built).  XvG: true = XAmvGp.
void modele_matrix(const ibh_modele_matrices *mm, char gridX, char gridG, bool XvG, int scale, ibh_sparse_set &dimXAm,
                   ibh_sparse_set &dimGp, ibh_weighted *ret) {
    hipStream_t st = hipStreamPerThread;
    const int T = 256;
    const char nameAvG[4] = {'A', 'v', gridG, 0}, nameXvG[4] = {gridX, 'v', gridG, 0}, nameGvX[4] = {gridG, 'v', gridX, 0};
    const int64_t nO = mm->nO;

    // AOpvIp with correctA, for wAOp
    ibh_sparse_set dimAOp, dimAOm, dimEOp, dimEOm;
    DevBuf<double> wAOm;
    std::vector<int32_t> aop2aom;               // dense AOp -> dense AOm, -1: ocean for ModelE
    {
        auto AOpvIp_c = o_matrix(mm, nameAvG, &dimAOp, &dimGp, 1);
        const int nAOp = dimAOp.n();
        const int64_t *ts = dimAOp.to_sparse_host();
        std::vector<int64_t> keys;
        std::vector<double> inv_fcont;
        std::vector<int32_t> src;
        aop2aom.assign((size_t)nAOp, -1);
        for (int d = 0; d < nAOp; ++d)          // dimAOm: the cells of dimAOp, in dense order, that ModelE calls land
            if (mm->foceanAOm[(size_t)ts[d]] == 0) { aop2aom[(size_t)d] = (int32_t)keys.size(); keys.push_back(ts[d]); }
        inv_fcont.assign(keys.size(), 0.); src.assign(keys.size(), -1);
        for (int d = 0; d < nAOp; ++d) {        // scaled_AOmvAOp (topo.cpp:50-81)
            const double fcont_p = 1.0 - mm->foceanAOp[(size_t)ts[d]], fcont_m = 1.0 - mm->foceanAOm[(size_t)ts[d]];
            if (fcont_m == 0.0) continue;
            if (fcont_m != 1.0) fail(IBH_EINVAL, "fcont_m[%ld] = %g, must be 0 or 1", (long)ts[d], fcont_m);
            if (fcont_p == 0.0) continue;
            const int k = aop2aom[(size_t)d];
            if (k < 0) continue;                // (fcont_m == 1 means foceanAOm == 0: always in dimAOm)
            inv_fcont[(size_t)k] = 1. / fcont_p; src[(size_t)k] = d;
        }
        dimAOm.assign_host(nO, keys.data(), (int32_t)keys.size());
        Arena &A = arena();
        A.reset();
        const int nAOm = dimAOm.n();
        double *d_inv = A.get<double>((size_t)nAOm);
        int32_t *d_src = A.get<int32_t>((size_t)nAOm);
        wAOm.alloc((size_t)nAOm);
        if (nAOm) {
            IBH_HIP(hipMemcpyAsync(d_inv, inv_fcont.data(), sizeof(double) * (size_t)nAOm, hipMemcpyHostToDevice, st));
            IBH_HIP(hipMemcpyAsync(d_src, src.data(), sizeof(int32_t) * (size_t)nAOm, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_wAOm, dim3(ceil_div(nAOm, T)), dim3(T), 0, st, d_inv, d_src, AOpvIp_c->wM.p, nAOm, wAOm.p);
        }
        IBH_HIP(hipGetLastError());
        IBH_HIP(hipStreamSynchronize(st));      // the host vectors and AOpvIp_c go away here
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
        // compute_EOmvAOm_unscaled (topo.cpp:211-240): EOpvAOp visited by columns, rows ascending inside; kept where the column
        // is a cell of dimAOm; dimEOm numbered first-seen
        ibh_sparse_set dimEOp2, dimAOp2;
        auto EOpvAOp = o_matrix(mm, "EvA", &dimEOp2, &dimAOp2, 0);
        const int nE2 = EOpvAOp->nrow, nA2 = EOpvAOp->ncol;
        const long nnz2 = (long)EOpvAOp->nnz;
        std::vector<int32_t> rp((size_t)nE2 + 1), ci((size_t)nnz2);
        EOpvAOp->rowptr.download(rp.data(), (size_t)nE2 + 1, st);
        EOpvAOp->colind.download(ci.data(), (size_t)nnz2, st);
        std::vector<int32_t> colptr((size_t)nA2 + 1, 0), by_col((size_t)nnz2), row_of((size_t)nnz2);
        for (long e = 0; e < nnz2; ++e) ++colptr[(size_t)ci[(size_t)e] + 1];
        for (int c = 0; c < nA2; ++c) colptr[(size_t)c + 1] += colptr[(size_t)c];
        {
            std::vector<int32_t> fill(colptr.begin(), colptr.end() - 1);
            for (int r = 0; r < nE2; ++r)
                for (int e = rp[(size_t)r]; e < rp[(size_t)r + 1]; ++e) { by_col[(size_t)fill[(size_t)ci[(size_t)e]]++] = e; row_of[(size_t)e] = r; }
        }
        dimEOm.set_sparse_extent(nO * mm->nhc);
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
        ibh_weighted EOmvAOm;
        DevBuf<double> EOmvAOms;
        {
            Arena &A = arena();
            A.reset();
            int32_t *d_row = A.get<int32_t>((size_t)nt), *d_col = A.get<int32_t>((size_t)nt), *d_src = A.get<int32_t>((size_t)nt);
            double *d_val = A.get<double>((size_t)nt);
            if (nt) {
                IBH_HIP(hipMemcpyAsync(d_row, trow.data(), sizeof(int32_t) * (size_t)nt, hipMemcpyHostToDevice, st));
                IBH_HIP(hipMemcpyAsync(d_col, tcol.data(), sizeof(int32_t) * (size_t)nt, hipMemcpyHostToDevice, st));
                IBH_HIP(hipMemcpyAsync(d_src, tsrc.data(), sizeof(int32_t) * (size_t)nt, hipMemcpyHostToDevice, st));
                hipLaunchKernelGGL(k_gather, dim3(ceil_div(nt, T)), dim3(T), 0, st, EOpvAOp->val.p, d_src, nt, d_val);
            }
            weighted_from_device_triplets(&EOmvAOm, nEOm, nAOm, nt, d_row, d_col, d_val, st);
            // wEOm = EOmvAOm * diag(sum(EOmvAOm, 1, '-')) * wAOm (:226-228)
            recip(EOmvAOm.Mw.p, nAOm, EOmvAOms, st);
            wEOm.alloc((size_t)nEOm);
            if (nEOm) hipLaunchKernelGGL(k_scaled_matvec, dim3(ceil_div(nEOm, T)), dim3(T), 0, st, view(EOmvAOm), EOmvAOms.p, wAOm.p, wEOm.p);
            IBH_HIP(hipGetLastError());
        }
        wXOm = wEOm.p;
        // raw_EOvEA (topo.cpp:112-204): Hntr's O -> A overlap clipped by dimAOm, every entry expanded over the elevation classes
        std::vector<double> wEOm_h((size_t)nEOm);
        wEOm.download(wEOm_h.data(), (size_t)nEOm, st);     // (synchronises: the host vectors above are free)
        int64_t ns = 0;
        rethrow(ibh_hntr_triplets(mm->hntr, IBH_HNTR_OVERLAP, mm->eq_rad, includeO.data(), &ns, nullptr, nullptr, nullptr));
        std::vector<int32_t> sO((size_t)ns), sA((size_t)ns);
        std::vector<double> sv((size_t)ns);
        if (ns) rethrow(ibh_hntr_triplets(mm->hntr, IBH_HNTR_OVERLAP, mm->eq_rad, includeO.data(), &ns, sO.data(), sA.data(), sv.data()));
        trow.clear(); tcol.clear();
        for (int64_t p = 0; p < ns; ++p) {
            if (std::abs(sv[(size_t)p]) < 1e-8) fail(IBH_EINVAL, "Found a stray overlap; what should we do about it?");
            for (int ihc = 0; ihc < mm->nhc; ++ihc) {
                const int dEO = dimEOm.to_dense(sO[(size_t)p] * mm->sA_O + ihc * mm->sHC_O);
                if (dEO < 0 || wEOm_h[(size_t)dEO] == 0) continue;
                trow.push_back(dEO);
                tcol.push_back(dimXAm.add_dense_host(sA[(size_t)p] * mm->sA_A + ihc * mm->sHC_A));
            }
        }
        const long ne = (long)trow.size();
        XOmvXAm.reset(new ibh_weighted);
        Arena &A = arena();
        A.reset();
        int32_t *d_row = A.get<int32_t>((size_t)ne), *d_col = A.get<int32_t>((size_t)ne);
        double *d_val = A.get<double>((size_t)ne);
        if (ne) {
            IBH_HIP(hipMemcpyAsync(d_row, trow.data(), sizeof(int32_t) * (size_t)ne, hipMemcpyHostToDevice, st));
            IBH_HIP(hipMemcpyAsync(d_col, tcol.data(), sizeof(int32_t) * (size_t)ne, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_gather, dim3(ceil_div(ne, T)), dim3(T), 0, st, wEOm.p, d_row, ne, d_val);
        }
        weighted_from_device_triplets(XOmvXAm.get(), nEOm, dimXAm.n(), ne, d_row, d_col, d_val, st);
        IBH_HIP(hipStreamSynchronize(st));
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
    if (nXAm) hipLaunchKernelGGL(k_scaled_matvec, dim3(ceil_div(nXAm, T)), dim3(T), 0, st, view(XAmvXOm), XAmvXOms.p, wXOm, wXAm.p);
    IBH_HIP(hipGetLastError());

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
    ibh_weighted cropped;
    const int nG = dimGp.n();
    if (XvG) {
        // M = diag(scale ? sXAm : wXAm * sXAm) * XAmvXOm * crop_mvp(dimXOm, dimXOp, 0, diag(1 / XOpvIp.wM) * XOpvIp.M)   (:346-365)
        DevBuf<double> sXOpvIp;
        recip(XOpvIp->wM.p, nXOp, sXOpvIp, st);
        upload(d_map, om2op, st);
        arena().reset();
        crop_rows(*XOpvIp, d_map.p, nXOm, sXOpvIp.p, &cropped, st);
        const double *ls = sXAm.p;
        if (!scale) {
            lscale.alloc((size_t)nXAm);
            if (nXAm) hipLaunchKernelGGL(k_mul, dim3(ceil_div(nXAm, T)), dim3(T), 0, st, wXAm.p, sXAm.p, nXAm, lscale.p);
            ls = lscale.p;
        }
        if (nXAm) hipLaunchKernelGGL(k_scale_rows, dim3(ceil_div(nXAm, T)), dim3(T), 0, st, XAmvXOm.rowptr.p, nXAm, ls, XAmvXOm.val.p);
        IBH_HIP(hipGetLastError());
        csr_product(XAmvXOm, cropped, ret, st);
        ret->wM = std::move(wXAm);
        ret->Mw.alloc((size_t)nG);
        if (nG) IBH_HIP(hipMemcpyAsync(ret->Mw.p, XOpvIp->Mw.p, sizeof(double) * (size_t)nG, hipMemcpyDeviceToDevice, st));
    } else {
        // M = crop_mvp(dimXOm, dimXOp, 1, [diag(1 / IpvXOp.wM) *] IpvXOp.M) * diag(XAmvXOms) * XOmvXAm   (:402-430)
        auto IpvXOp = o_matrix(mm, nameGvX, &dimGp, dimXOp, 0);
        IBH_CHECK(IpvXOp->ncol == nXOp && IpvXOp->nrow == nG, "internal: %s added cells to a set the O-grid builds had numbered", nameGvX);
        DevBuf<double> sIpvXOp;
        if (scale) recip(IpvXOp->wM.p, nG, sIpvXOp, st);
        upload(d_map, op2om, st);
        arena().reset();
        crop_cols(*IpvXOp, d_map.p, nXOm, scale ? sIpvXOp.p : nullptr, XAmvXOms.p, &cropped, st);
        csr_product(cropped, *XOmvXAm, ret, st);
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
    IBH_CHECK(s->sparse_extent() == -1 || s->sparse_extent() == extent, "ModelE matrix_d: %s has sparse extent %lld, the grid %lld cells",
              which, (long long)s->sparse_extent(), (long long)extent);
    s->check_entries_within(extent, which);
}

void check_device(const ibh_regridder *rg) {
    int dev = -1;
    IBH_HIP(hipGetDevice(&dev));
    IBH_CHECK(dev == rg->device, "regridder belongs to device %d, current device is %d", rg->device, dev);
}

void modele_matrix_d(const ibh_modele_matrices *mm, const char *spec, ibh_sparse_set *dim0, ibh_sparse_set *dim1, int scale,
                     ibh_weighted **out) {
    const Parsed p = parse_spec(spec);
    const ibh_regridder *rg = mm->rmO->rg;
    check_device(rg);
    IBH_CHECK(dim0 == nullptr || dim0 != dim1, "dims[0] and dims[1] must be distinct sets");
    std::unique_ptr<ibh_weighted> w;
    std::unique_ptr<ibh_sparse_set> work[2];
    ibh_sparse_set *dims[2] = {dim0, dim1};
    if (p.kind >= 2) {
        // compute_AOmvAAm (:92-121): dims {dimAOm, dimAAm} whichever way the matrix is stored; the clip is dimAOm as it comes
        check_extent(dim0, mm->nO, "dimAOm");
        check_extent(dim1, mm->nA, "dimAAm");
        for (int k = 0; k < 2; ++k) work[k].reset(dims[k] ? new ibh_sparse_set(*dims[k]) : new ibh_sparse_set);
        std::vector<uint8_t> includeO((size_t)mm->nO, 0);
        for (int k = 0; k < work[0]->n(); ++k) includeO[(size_t)work[0]->to_sparse_host()[k]] = 1;
        ibh_weighted *h = nullptr;
        rethrow(ibh_hntr_matrix_d(mm->hntr, IBH_HNTR_OVERLAP, mm->eq_rad, includeO.data(), work[0].get(), IBH_TO_DENSE_IGNORE_MISSING,
                                  work[1].get(), IBH_ADD_DENSE, p.kind == 3, &h));
        w.reset(h);
    } else {
        const int iX = p.kind == 0 ? 0 : 1, iG = 1 - iX;       // where the atmosphere set and the ice set stand
        check_extent(dims[iX], p.gridX == 'E' ? mm->nA * mm->nhc : mm->nA, p.gridX == 'E' ? "dimEAm" : "dimAAm");
        check_extent(dims[iG], p.gridG == 'I' ? rg->nI : rg->nX, p.gridG == 'I' ? "dimIp" : "dimXp");
        for (int k = 0; k < 2; ++k) work[k].reset(dims[k] ? new ibh_sparse_set(*dims[k]) : new ibh_sparse_set);
        w.reset(new ibh_weighted);
        IBH_HIP(hipGetDevice(&w->device));
        modele_matrix(mm, p.gridX, p.gridG, p.kind == 0, scale, *work[iX], *work[iG], w.get());
    }
    // built: the caller's sets take the numbering, the result names them (or owns the fresh ones)
    const bool swapped = p.kind == 3;       // hntr's transpose stores {dimAAm, dimAOm}
    for (int k = 0; k < 2; ++k) {
        const int kk = swapped ? 1 - k : k;
        if (dims[k]) { *dims[k] = std::move(*work[k]); w->dims[kk] = dims[k]; w->owns[kk] = false; }
        else { w->dims[kk] = work[k].release(); w->owns[kk] = true; }
    }
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
    check_device(rg);
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
    int64_t ns = 0;
    rethrow(ibh_hntr_triplets(h, IBH_HNTR_OVERLAP, 1.0, includeO.data(), &ns, nullptr, nullptr, nullptr));
    std::vector<int32_t> sO((size_t)ns), sA((size_t)ns);
    std::vector<double> sv((size_t)ns);
    if (ns) rethrow(ibh_hntr_triplets(h, IBH_HNTR_OVERLAP, 1.0, includeO.data(), &ns, sO.data(), sA.data(), sv.data()));
    ibh_sparse_set dimA((int64_t)(imO / 2) * (jmO / 2));
    for (int64_t p = 0; p < ns; ++p) dimA.add_dense_host(sA[(size_t)p]);
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
int ibh_modele_matrices_matrix_d(const ibh_modele_matrices *mm, const char *spec, ibh_sparse_set *dim0, ibh_sparse_set *dim1, int scale,
                                 ibh_weighted **out) {
    if (out) *out = nullptr;
    return guarded([&] {
        IBH_CHECK(mm && spec && out, "null argument");
        modele_matrix_d(mm, spec, dim0, dim1, scale, out);
    });
}
int ibh_modele_matrices_destroy(ibh_modele_matrices *mm) { delete mm; return IBH_OK; }
int ibh_modele_agridA(const ibh_regridder *rgO, int32_t imO, int32_t jmO, double offiO, double dlatO, int32_t *nA_dense,
                      int64_t *to_sparse) {
    return guarded([&] { modele_agridA(rgO, imO, jmO, offiO, dlatO, nA_dense, to_sparse); });
}
int ibh_selftest_csr_product(const ibh_weighted *L, const ibh_weighted *R, ibh_weighted **out) {
    if (out) *out = nullptr;
    return guarded([&] {
        IBH_CHECK(L && R && out, "null argument");
        require_device();
        hipStream_t st = hipStreamPerThread;
        std::unique_ptr<ibh_weighted> w(new ibh_weighted);
        IBH_HIP(hipGetDevice(&w->device));
        csr_product(*L, *R, w.get(), st);
        w->wM.alloc((size_t)w->nrow); w->wM.zero(st);
        w->Mw.alloc((size_t)w->ncol); w->Mw.zero(st);
        IBH_HIP(hipStreamSynchronize(st));
        w->conservative = L->conservative; w->scaled = L->scaled;
        for (int k = 0; k < 2; ++k) { w->dims[k] = new ibh_sparse_set; w->owns[k] = true; }
        w->dims[0]->make_identity(w->nrow);
        w->dims[1]->make_identity(w->ncol);
        *out = w.release();
    });
}

}  // extern "C"
