// csrops.hip -- the generic CSR pieces and the two builds composed of them, E1vE0 and I2vX (csrops.h).  Arithmetic notes: every product
// is rounded where it is written (the library is compiled with -ffp-contract=off), and sums run in the order the comments give.
#include "csrbuild.h"
#include "csrops.h"
#include "prims.h"

namespace ibh {
namespace {

// ---- C = L * R -------------------------------------------------------------------------------------------------------------
// Eigen's conservative sparse product: C(r, c) = sum_k L(r, k) * R(k, c) over k ascending, the first term assigned.  Row r of
// L lists its k ascending, so walking it and, per k, row k of R emits the terms of every (r, c) in that order; a stable
// ordering by (r, c) and sequential sums of equal keys (csr_from_device_triplets: setFromTriplets) finish it.
__global__ void k_prod_count(Csr L, const int32_t *__restrict__ Rptr, uint32_t *__restrict__ cnt, unsigned long long *__restrict__ total) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long c = 0;
    if (r < L.nrow) {
        for (int e = L.rowptr[r]; e < L.rowptr[r + 1]; ++e) {
            const int k = L.colind[e];
            c += (unsigned long long)(Rptr[k + 1] - Rptr[k]);
        }
        cnt[r] = (uint32_t)c;
    }
    add_to_launch_total(c, total);
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
}  // namespace
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

namespace {
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
}  // namespace
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

// ---- the small vectors and row scalings ---------------------------------------------------------------------------------------
namespace {
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
__global__ void k_scale_rows(const int32_t *__restrict__ rowptr, int nrow, const double *__restrict__ s, double *__restrict__ val) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrow) return;
    for (int e = rowptr[r]; e < rowptr[r + 1]; ++e) val[e] = s[r] * val[e];
}
__global__ void k_scale_cols(const int32_t *__restrict__ colind, long nnz, const double *__restrict__ d, double *__restrict__ val) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nnz) val[e] = val[e] * d[colind[e]];
}
__global__ void k_scale_rows_recip(const int32_t *__restrict__ rowptr, int nrow, double *__restrict__ val, const double *__restrict__ sum) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrow) return;
    const int b = rowptr[r], e = rowptr[r + 1];
    if (b == e) return;
    const double s = 1. / sum[r];
    for (int k = b; k < e; ++k) val[k] = val[k] * s;
}
__global__ void k_expand_rows(const int32_t *__restrict__ rowptr, int nrow, int32_t *__restrict__ row) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrow) return;
    for (int e = rowptr[r]; e < rowptr[r + 1]; ++e) row[e] = r;
}
}  // namespace
void recip(const double *in, int n, DevBuf<double> &out, hipStream_t st) {
    out.alloc((size_t)n);
    if (n) hipLaunchKernelGGL(k_recip, dim3(ceil_div(n, 256)), dim3(256), 0, st, in, n, out.p);
}
void mul(const double *a, const double *b, int n, double *out, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_mul, dim3(ceil_div(n, 256)), dim3(256), 0, st, a, b, n, out);
}
void gather(const double *in, const int32_t *idx, long n, double *out, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_gather, dim3(ceil_div(n, 256)), dim3(256), 0, st, in, idx, n, out);
}
void scale_rows(const int32_t *rowptr, int nrow, const double *s, double *val, hipStream_t st) {
    if (nrow) hipLaunchKernelGGL(k_scale_rows, dim3(ceil_div(nrow, 256)), dim3(256), 0, st, rowptr, nrow, s, val);
}
void scale_cols(const int32_t *colind, int64_t nnz, const double *d, double *val, hipStream_t st) {
    if (nnz) hipLaunchKernelGGL(k_scale_cols, dim3(ceil_div(nnz, 256)), dim3(256), 0, st, colind, (long)nnz, d, val);
}
void scale_rows_recip(const int32_t *rowptr, int nrow, const double *sum, double *val, hipStream_t st) {
    if (nrow) hipLaunchKernelGGL(k_scale_rows_recip, dim3(ceil_div(nrow, 256)), dim3(256), 0, st, rowptr, nrow, val, sum);
}
void expand_rows(const int32_t *rowptr, int nrow, int32_t *row, hipStream_t st) {
    if (nrow) hipLaunchKernelGGL(k_expand_rows, dim3(ceil_div(nrow, 256)), dim3(256), 0, st, rowptr, nrow, row);
}
void transpose_csr(const ibh_weighted &in, ibh_weighted *out, hipStream_t st) {
    Arena &A = arena();
    A.reset();
    int32_t *row = A.get<int32_t>((size_t)in.nnz);
    expand_rows(in.rowptr.p, in.nrow, row, st);
    IBH_HIP(hipGetLastError());
    csr_from_device_triplets(out, in.ncol, in.nrow, in.nnz, in.colind.p, row, in.val.p, st);
}

// ---- E1vE0 (slib/icebin/e1ve0.cpp:55-106 compute_E1vE0c) ------------------------------------------------
//   E1vE0c = diag(1 / sum_sheets Mw(XuE1)) * sum_sheets[ E1uX * (XvE0 - XvE1) ], consolidated,
// XvE = diag(1/wM) * XuE.  Every exchange cell x has <= a handful of entries in XuE1 and XuE0, so the
// product through X is again a keyed sum: per x, every (e1 of XuE1 row x) x (e of the merged row of
// XvE0 - XvE1) contributes u1 * d to key (e1, e), summed over x ascending with the first term assigned
// (Eigen's conservative sparse product) -- the triplets -> CSR layer (contributions -> order -> sequential
// sums, csrbuild.h) does the rest.  Keys are SPARSE E indices (the reference works on sparsified matrices).
namespace {
struct XuEView {
    const int32_t *rowptr, *colind;
    const double *val, *wM;
    const int64_t *col_s;        // dense E -> sparse E
    const int32_t *rowmap;       // sparse x -> dense row, nullptr: identity
    int nrow;
};
__device__ __forceinline__ int xue_row(const XuEView &m, long x) {
    if (!m.rowmap) return x < m.nrow ? (int)x : -1;
    return m.rowmap[x];
}
constexpr int E1_MAXROW = 16;    // entries of one XuE row handled in registers (Z_INTERP gives <= 2)
template <int PASS>
__global__ void k_e1ve0(XuEView m1, XuEView m0, long nX, uint32_t *__restrict__ cnt, const uint32_t *__restrict__ pos,
                        uint64_t *__restrict__ keys, uint32_t *__restrict__ idx, double *__restrict__ term,
                        uint32_t *__restrict__ too_long)
{
    const long x = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nX) return;
    const int r1 = xue_row(m1, x), r0 = xue_row(m0, x);
    const int b1 = r1 >= 0 ? m1.rowptr[r1] : 0, n1 = r1 >= 0 ? m1.rowptr[r1 + 1] - b1 : 0;
    const int b0 = r0 >= 0 ? m0.rowptr[r0] : 0, n0 = r0 >= 0 ? m0.rowptr[r0 + 1] - b0 : 0;
    if (n1 > E1_MAXROW || n0 > E1_MAXROW) { *too_long = 1u; if (!PASS) cnt[x] = 0; return; }
    // merged row of D = XvE0 - XvE1 by sparse column: entries of E0 first, then the E1 entries E0 lacks
    int nd = n0;
    for (int j = 0; j < n1; ++j) {
        const int64_t e = m1.col_s[m1.colind[b1 + j]];
        bool in0 = false;
        for (int i = 0; i < n0; ++i) in0 = in0 || m0.col_s[m0.colind[b0 + i]] == e;
        nd += in0 ? 0 : 1;
    }
    if (!PASS) { cnt[x] = (uint32_t)(n1 * nd); return; }
    if (n1 == 0 || nd == 0) return;
    const double s0 = r0 >= 0 ? 1. / m0.wM[r0] : 0.0, s1 = 1. / m1.wM[r1];
    uint32_t p = pos[x];
    for (int a = 0; a < n1; ++a) {
        const int64_t e1 = m1.col_s[m1.colind[b1 + a]];
        const double u1 = m1.val[b1 + a];
        for (int i = 0; i < n0; ++i) {                        // columns stored in E0 (a - b, or a)
            const int64_t e = m0.col_s[m0.colind[b0 + i]];
            double d = s0 * m0.val[b0 + i];
            for (int j = 0; j < n1; ++j)
                if (m1.col_s[m1.colind[b1 + j]] == e) d = d - s1 * m1.val[b1 + j];
            keys[p] = ((uint64_t)e1 << 32) | (uint64_t)e; idx[p] = p; term[p] = u1 * d; ++p;
        }
        for (int j = 0; j < n1; ++j) {                        // columns only E1 stores (0 - b)
            const int64_t e = m1.col_s[m1.colind[b1 + j]];
            bool in0 = false;
            for (int i = 0; i < n0; ++i) in0 = in0 || m0.col_s[m0.colind[b0 + i]] == e;
            if (in0) continue;
            keys[p] = ((uint64_t)e1 << 32) | (uint64_t)e; idx[p] = p; term[p] = u1 * (0.0 - s1 * m1.val[b1 + j]); ++p;
        }
    }
}
__global__ void k_scatter_rowmap(const int64_t *__restrict__ to_sparse, int n, int32_t *__restrict__ rowmap) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) rowmap[to_sparse[i]] = i;
}
__global__ void k_add_by_sparse(const double *__restrict__ v, const int64_t *__restrict__ to_sparse, int n, double *__restrict__ acc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const int64_t s = to_sparse[i]; acc[s] = acc[s] + v[i]; }       // sparse ids of one matrix are distinct
}
__global__ void k_csr_to_contrib(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colind, const double *__restrict__ val,
                                 int nrow, uint32_t base, uint64_t *__restrict__ keys, uint32_t *__restrict__ idx, double *__restrict__ term) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrow) return;
    for (int k = rowptr[r]; k < rowptr[r + 1]; ++k) {
        const uint32_t p = base + (uint32_t)k;
        keys[p] = ((uint64_t)(uint32_t)r << 32) | (uint32_t)colind[k]; idx[p] = p; term[p] = val[k];
    }
}
__global__ void k_fill_f64(double *p, size_t n, double v) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
}  // namespace

void e1ve0_compute(int nsheets, const ibh_weighted *const *XuE1s, const ibh_weighted *const *XuE0s, int64_t nE, ibh_weighted *out) {
    IBH_CHECK(nsheets >= 1 && XuE1s && XuE0s && out, "bad arguments");
    IBH_CHECK(nE > 0 && nE < (1ll << 31), "nE=%ld out of range", (long)nE);
    hipStream_t st = nullptr;
    Arena &A = arena();
    A.reset();
    const int T = 256;
    double *sE1 = A.get<double>((size_t)nE);
    IBH_HIP(hipMemsetAsync(sE1, 0, sizeof(double) * (size_t)nE, st));
    std::vector<std::unique_ptr<ibh_weighted>> locals;
    for (int s = 0; s < nsheets; ++s) {
        const ibh_weighted *w1 = XuE1s[s], *w0 = XuE0s[s];
        IBH_CHECK(w1 && w0, "null matrix for sheet %d", s);
        IBH_CHECK(w1->dims[1]->sparse_extent() <= nE && w0->dims[1]->sparse_extent() <= nE, "sheet %d: E extent exceeds nE", s);
        const int64_t nX = w1->dims[0]->sparse_extent();
        IBH_CHECK(nX == w0->dims[0]->sparse_extent() && nX >= 0 && nX < (1ll << 31), "sheet %d: XuE1 and XuE0 disagree on nX", s);
        XuEView v[2];
        const ibh_weighted *ws[2] = {w1, w0};
        for (int k = 0; k < 2; ++k) {
            const ibh_weighted *w = ws[k];
            v[k] = XuEView{w->rowptr.p, w->colind.p, w->val.p, w->wM.p, w->dims[1]->device_to_sparse(w->ncol, st), nullptr, w->nrow};
            const bool ident = w->dims[0]->identity() && w->dims[0]->n() >= w->nrow;
            if (!ident) {
                int32_t *rm = A.get<int32_t>((size_t)nX);
                IBH_HIP(hipMemsetAsync(rm, 0xFF, sizeof(int32_t) * (size_t)nX, st));
                const int64_t *rs = w->dims[0]->device_to_sparse(w->nrow, st);
                if (w->nrow) hipLaunchKernelGGL(k_scatter_rowmap, dim3(ceil_div(w->nrow, T)), dim3(T), 0, st, rs, w->nrow, rm);
                v[k].rowmap = rm;
            }
        }
        if (w1->ncol) hipLaunchKernelGGL(k_add_by_sparse, dim3(ceil_div(w1->ncol, T)), dim3(T), 0, st, w1->Mw.p, v[0].col_s, w1->ncol, sE1);
        uint32_t *cnt = A.get<uint32_t>((size_t)nX + 2), *pos = A.get<uint32_t>((size_t)nX + 1);
        uint32_t *d_total = cnt + nX, *too_long = cnt + nX + 1;
        IBH_HIP(hipMemsetAsync(cnt + nX, 0, 2 * sizeof(uint32_t), st));
        const dim3 grid(nX ? ceil_div(nX, T) : 1);
        hipLaunchKernelGGL(k_e1ve0<0>, grid, dim3(T), 0, st, v[0], v[1], (long)nX, cnt, (const uint32_t *)nullptr, (uint64_t *)nullptr,
                           (uint32_t *)nullptr, (double *)nullptr, too_long);
        exclusive_scan_u32(cnt, pos, (size_t)nX, d_total, st);
        uint32_t h[2];
        readback_sync(h, d_total, sizeof(h), st);
        IBH_CHECK(!h[1], "E1vE0: an XuE row has more than %d entries", E1_MAXROW);
        Triplets t = triplets_in_arena(h[0]);
        if (t.n) hipLaunchKernelGGL(k_e1ve0<1>, grid, dim3(T), 0, st, v[0], v[1], (long)nX, cnt, pos, t.keys, t.idx, t.term, too_long);
        IBH_HIP(hipGetLastError());
        std::unique_ptr<ibh_weighted> loc(new ibh_weighted);
        int32_t *row = nullptr;
        build_csr_from_contributions(loc.get(), t, (int)nE, (int)nE, &row, st);
        locals.push_back(std::move(loc));
    }
    // scale by 1 / (sum over sheets of Mw(XuE1)), then consolidate across sheets
    for (auto &loc : locals) scale_rows_recip(loc->rowptr.p, (int)nE, sE1, loc->val.p, st);     // ii->value() *= sE1(iE1)
    IBH_HIP(hipGetLastError());
    if (locals.size() == 1) {
        out->rowptr = std::move(locals[0]->rowptr); out->colind = std::move(locals[0]->colind); out->val = std::move(locals[0]->val);
        out->nnz = locals[0]->nnz;
    } else {
        size_t nt = 0;
        for (auto &loc : locals) nt += (size_t)loc->nnz;
        IBH_CHECK(nt < (1ul << 31), "E1vE0 too large");
        Triplets t = triplets_in_arena(nt);
        uint32_t base = 0;
        for (auto &loc : locals) {          // sheet-major emission order: equal (iE1, iE0) are summed in sheet order
            hipLaunchKernelGGL(k_csr_to_contrib, dim3(ceil_div(nE, T)), dim3(T), 0, st, loc->rowptr.p, loc->colind.p, loc->val.p, (int)nE,
                               base, t.keys, t.idx, t.term);
            base += (uint32_t)loc->nnz;
        }
        int32_t *row = nullptr;
        build_csr_from_contributions(out, t, (int)nE, (int)nE, &row, st);
    }
    out->nrow = out->ncol = (int)nE;
    out->wM.alloc((size_t)nE); out->Mw.alloc((size_t)nE);
    hipLaunchKernelGGL(k_fill_f64, dim3(ceil_div(nE, T)), dim3(T), 0, st, out->wM.p, (size_t)nE, 1.0);
    hipLaunchKernelGGL(k_fill_f64, dim3(ceil_div(nE, T)), dim3(T), 0, st, out->Mw.p, (size_t)nE, 1.0);
    IBH_HIP(hipGetLastError());
    IBH_HIP(hipStreamSynchronize(st));
}

// ---- make_I2vX (modele/global_ec.cpp:345-376) -----------------------------------------------------------------------
//   M  = (I2vI * diag(1/IvX.wM)) * IvX.M,   wM = (I2vI * diag(sum(I2vI, 1, '-'))) * IvX.wM
// IvI2 is I2vI stored by its columns: row i (dense I) lists its I2 rows ascending, Eigen's storage order of column i.  Both
// products sum over the dense I index ascending, so they are keyed sums with terms emitted in row order of IvI2: per I cell,
// every (i2 of IvI2 row i) x (x of IvX row i) contributes (v * (1/wM_i)) * m to key (i2, x), and every i2 contributes
// (v * (1/colsum_i)) * wM_i to key i2 -- the triplets -> CSR layer (contributions -> order -> sequential sums, first term
// assigned) does the rest.  The column sum of I2vI runs over its rows ascending from 0, as spsparse's sum(M, 1, '-').
namespace {
__global__ void k_i2vx_count(const int32_t *__restrict__ r2, const int32_t *__restrict__ rx, int nI, uint32_t *__restrict__ cnt,
                             unsigned long long *__restrict__ total) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long c = 0;
    if (i < nI) {
        c = (unsigned long long)(r2[i + 1] - r2[i]) * (unsigned long long)(rx[i + 1] - rx[i]);
        cnt[i] = (uint32_t)c;
    }
    add_to_launch_total(c, total);
}
__global__ void k_i2vx_terms(const int32_t *__restrict__ r2, const int32_t *__restrict__ c2, const double *__restrict__ v2,
                             const int32_t *__restrict__ rx, const int32_t *__restrict__ cx, const double *__restrict__ vx,
                             const double *__restrict__ wMx, int nI, const uint32_t *__restrict__ pos, Triplets m, Triplets w) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nI) return;
    const int b2 = r2[i], e2 = r2[i + 1], bx = rx[i], ex = rx[i + 1];
    if (b2 == e2) return;
    double cs = 0;
    for (int k = b2; k < e2; ++k) cs = cs + v2[k];
    const double sI = 1. / cs;                 // sum(I2vI, 1, '-')
    const double sX = 1. / wMx[i];             // 1. / IvX.wM
    uint32_t p = pos[i];
    for (int k = b2; k < e2; ++k) {
        const uint64_t i2 = (uint64_t)(uint32_t)c2[k];
        w.keys[k] = i2 << 32; w.idx[k] = (uint32_t)k; w.term[k] = (v2[k] * sI) * wMx[i];
        const double L = v2[k] * sX;
        for (int q = bx; q < ex; ++q, ++p) { m.keys[p] = (i2 << 32) | (uint32_t)cx[q]; m.idx[p] = p; m.term[p] = L * vx[q]; }
    }
}
__global__ void k_i2vx_wM(const int32_t *__restrict__ rowptr, const double *__restrict__ val, int n, double *__restrict__ wM) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) wM[r] = rowptr[r + 1] > rowptr[r] ? val[rowptr[r]] : 0.;
}
}  // namespace

void i2vx_compute(const ibh_weighted *IvI2, const ibh_weighted *IvX, ibh_weighted *out) {
    IBH_CHECK(IvI2->nrow == IvX->nrow, "make_I2vX: I2vI has %d ice columns, IvX %d ice rows", IvI2->nrow, IvX->nrow);
    hipStream_t st = nullptr;
    Arena &A = arena();
    A.reset();
    const int T = 256, nI = IvX->nrow, nI2 = IvI2->ncol, nX = IvX->ncol;
    uint32_t *pos = A.get<uint32_t>((size_t)nI + 1);
    unsigned long long *tot = A.get<unsigned long long>(1);
    IBH_HIP(hipMemsetAsync(tot, 0, sizeof(unsigned long long), st));
    if (nI) hipLaunchKernelGGL(k_i2vx_count, dim3(ceil_div(nI, T)), dim3(T), 0, st, IvI2->rowptr.p, IvX->rowptr.p, nI, pos, tot);
    IBH_HIP(hipGetLastError());
    unsigned long long total = 0;
    readback_sync(&total, tot, sizeof(total), st);
    IBH_CHECK(total <= INT32_MAX, "make_I2vX: %llu product terms exceed INT32_MAX", total);
    exclusive_scan_u32(pos, pos, (size_t)nI, pos + nI, st);
    Triplets m = triplets_in_arena((size_t)total), w = triplets_in_arena((size_t)IvI2->nnz);
    if (nI) hipLaunchKernelGGL(k_i2vx_terms, dim3(ceil_div(nI, T)), dim3(T), 0, st, IvI2->rowptr.p, IvI2->colind.p, IvI2->val.p,
                               IvX->rowptr.p, IvX->colind.p, IvX->val.p, IvX->wM.p, nI, pos, m, w);
    IBH_HIP(hipGetLastError());
    int32_t *row = nullptr;
    build_csr_from_contributions(out, m, nI2, nX, &row, st);
    ibh_weighted wsum;
    build_csr_from_contributions(&wsum, w, nI2, 1, &row, st);
    out->wM.alloc((size_t)nI2);
    if (nI2) hipLaunchKernelGGL(k_i2vx_wM, dim3(ceil_div(nI2, T)), dim3(T), 0, st, wsum.rowptr.p, wsum.val.p, nI2, out->wM.p);
    out->Mw.alloc((size_t)nX);
    if (nX) IBH_HIP(hipMemcpyAsync(out->Mw.p, IvX->Mw.p, sizeof(double) * (size_t)nX, hipMemcpyDeviceToDevice, st));
    IBH_HIP(hipGetLastError());
    IBH_HIP(hipStreamSynchronize(st));
    out->conservative = IvX->conservative;
    out->scaled = 0;
}

}  // namespace ibh

using namespace ibh;
extern "C" {

int ibh_selftest_csr_product(const ibh_weighted *L, const ibh_weighted *R, ibh_weighted **out) {
    if (out) *out = nullptr;
    return guarded([&] {
        IBH_CHECK(L && R && out, "null argument");
        require_device();
        hipStream_t st = hipStreamPerThread;
        auto w = new_weighted();
        csr_product(*L, *R, w.get(), st);
        w->wM.alloc((size_t)w->nrow); w->wM.zero(st);
        w->Mw.alloc((size_t)w->ncol); w->Mw.zero(st);
        IBH_HIP(hipStreamSynchronize(st));
        w->conservative = L->conservative; w->scaled = L->scaled;
        w->dims[0] = DimRef::owned_identity(w->nrow); w->dims[1] = DimRef::owned_identity(w->ncol);
        *out = w.release();
    });
}

int ibh_selftest_csr_op(int op, const ibh_weighted *in, const int32_t *idx, int64_t nidx, const double *a, int64_t na, const double *b,
                        int64_t nb, int64_t nout, ibh_weighted **mat_out, void *vec_out) {
    if (mat_out) *mat_out = nullptr;
    return guarded([&] {
        const bool matrix_op = op >= IBH_CSROP_TRANSPOSE && op <= IBH_CSROP_SCALE_ROWS_RECIP;
        IBH_CHECK(op >= IBH_CSROP_TRANSPOSE && op <= IBH_CSROP_EXPAND_ROWS, "unknown op %d", op);
        IBH_CHECK(nidx >= 0 && na >= 0 && nb >= 0 && nout >= 0 && std::max({nidx, na, nb, nout}) < (1ll << 31), "bad lengths");
        IBH_CHECK((nidx == 0 || idx) && (na == 0 || a) && (nb == 0 || b), "a length without its array");
        IBH_CHECK(!(nidx == 0 && idx) && !(na == 0 && a) && !(nb == 0 && b), "an array without its length");
        IBH_CHECK(matrix_op ? mat_out != nullptr : (vec_out != nullptr || nout == 0 || op == IBH_CSROP_EXPAND_ROWS), "no output");
        IBH_CHECK((matrix_op || op == IBH_CSROP_EXPAND_ROWS) == (in != nullptr), "op %d %s a matrix", op, in ? "takes no" : "needs");
        if (op == IBH_CSROP_EXPAND_ROWS) IBH_CHECK(vec_out || in->nnz == 0, "no output");
        const auto all_within = [&](int64_t lo, int64_t hi) {
            for (int64_t k = 0; k < nidx; ++k)
                if (idx[k] < lo || idx[k] >= hi) return false;
            return true;
        };
        switch (op) {
        case IBH_CSROP_TRANSPOSE: case IBH_CSROP_EXPAND_ROWS:
            IBH_CHECK(!nidx && !na && !nb, "op %d takes the matrix alone", op);
            break;
        case IBH_CSROP_CROP_ROWS:
            IBH_CHECK(nidx == nout && (na == 0 || na == in->nrow) && !nb, "crop_rows: src[nout], rs[nrow] or none");
            IBH_CHECK(all_within(-1, in->nrow), "crop_rows: a source row outside [-1, %d)", in->nrow);
            break;
        case IBH_CSROP_CROP_COLS: {
            IBH_CHECK(nidx == in->ncol && (na == 0 || na == in->nrow) && (nb == 0 || nb == nout), "crop_cols: map[ncol], rs[nrow], cs[nout]");
            IBH_CHECK(all_within(-1, nout), "crop_cols: a target column outside [-1, %lld)", (long long)nout);
            std::vector<char> hit((size_t)nout, 0);
            for (int64_t k = 0; k < nidx; ++k)
                if (idx[k] >= 0) { IBH_CHECK(!hit[(size_t)idx[k]], "crop_cols: the map is not one-to-one"); hit[(size_t)idx[k]] = 1; }
            break;
        }
        case IBH_CSROP_SCALE_ROWS: case IBH_CSROP_SCALE_ROWS_RECIP:
            IBH_CHECK(!nidx && na == in->nrow && !nb, "a row scaling takes a[nrow]");
            break;
        case IBH_CSROP_SCALE_COLS:
            IBH_CHECK(!nidx && na == in->ncol && !nb, "scale_cols takes a[ncol]");
            break;
        case IBH_CSROP_RECIP:
            IBH_CHECK(!nidx && na == nout && !nb, "recip takes a[nout]");
            break;
        case IBH_CSROP_MUL:
            IBH_CHECK(!nidx && na == nout && nb == nout, "mul takes a[nout], b[nout]");
            break;
        case IBH_CSROP_GATHER:
            IBH_CHECK(nidx == nout && !nb && all_within(0, na), "gather takes idx[nout] into a[na]");
            break;
        }
        require_device();
        if (in) check_current_device(in->device, "the matrix");
        hipStream_t st = hipStreamPerThread;
        Arena &A = arena();
        A.reset();
        // (the operands live outside the arena: csr_product and transpose_csr reset it)
        DevBuf<int32_t> d_idx; DevBuf<double> d_a, d_b, d_out;
        if (nidx) d_idx.upload(idx, (size_t)nidx, st);
        if (na) d_a.upload(a, (size_t)na, st);
        if (nb) d_b.upload(b, (size_t)nb, st);
        if (matrix_op) {
            auto w = new_weighted();
            if (op == IBH_CSROP_TRANSPOSE) {
                transpose_csr(*in, w.get(), st);
            } else if (op == IBH_CSROP_CROP_ROWS) {
                crop_rows(*in, d_idx.p, (int)nout, na ? d_a.p : nullptr, w.get(), st);
            } else if (op == IBH_CSROP_CROP_COLS) {
                crop_cols(*in, d_idx.p, (int)nout, na ? d_a.p : nullptr, nb ? d_b.p : nullptr, w.get(), st);
            } else {                                        // the scalings work in place: on a copy of the CSR
                w->nrow = in->nrow; w->ncol = in->ncol; w->nnz = in->nnz;
                w->rowptr.alloc((size_t)in->nrow + 1); w->colind.alloc((size_t)in->nnz); w->val.alloc((size_t)in->nnz);
                IBH_HIP(hipMemcpyAsync(w->rowptr.p, in->rowptr.p, sizeof(int32_t) * ((size_t)in->nrow + 1), hipMemcpyDeviceToDevice, st));
                if (in->nnz) {
                    IBH_HIP(hipMemcpyAsync(w->colind.p, in->colind.p, sizeof(int32_t) * (size_t)in->nnz, hipMemcpyDeviceToDevice, st));
                    IBH_HIP(hipMemcpyAsync(w->val.p, in->val.p, sizeof(double) * (size_t)in->nnz, hipMemcpyDeviceToDevice, st));
                }
                if (op == IBH_CSROP_SCALE_ROWS) scale_rows(w->rowptr.p, w->nrow, d_a.p, w->val.p, st);
                else if (op == IBH_CSROP_SCALE_COLS) scale_cols(w->colind.p, w->nnz, d_a.p, w->val.p, st);
                else scale_rows_recip(w->rowptr.p, w->nrow, d_a.p, w->val.p, st);
            }
            IBH_HIP(hipGetLastError());
            w->wM.alloc((size_t)w->nrow); w->wM.zero(st);
            w->Mw.alloc((size_t)w->ncol); w->Mw.zero(st);
            IBH_HIP(hipStreamSynchronize(st));
            w->conservative = in->conservative; w->scaled = in->scaled;
            w->dims[0] = DimRef::owned_identity(w->nrow); w->dims[1] = DimRef::owned_identity(w->ncol);
            *mat_out = w.release();
            return;
        }
        if (op == IBH_CSROP_EXPAND_ROWS) {
            DevBuf<int32_t> d_row((size_t)in->nnz);
            expand_rows(in->rowptr.p, in->nrow, d_row.p, st);
            IBH_HIP(hipGetLastError());
            d_row.download(static_cast<int32_t *>(vec_out), (size_t)in->nnz, st);
            return;
        }
        if (op == IBH_CSROP_RECIP) {
            recip(d_a.p, (int)nout, d_out, st);
        } else {
            d_out.alloc((size_t)nout);
            if (op == IBH_CSROP_MUL) mul(d_a.p, d_b.p, (int)nout, d_out.p, st);
            else gather(d_a.p, d_idx.p, (long)nout, d_out.p, st);
        }
        IBH_HIP(hipGetLastError());
        d_out.download(static_cast<double *>(vec_out), (size_t)nout, st);
    });
}

}  // extern "C"
