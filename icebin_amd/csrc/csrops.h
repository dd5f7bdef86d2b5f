// csrops.h -- small algebra on CSR matrices that are already in HBM (csrops.hip): the sparse product, re-numbered copies, the
// transpose, and row / vector scalings.  Each piece exists once; the matrix builds outside the exchange-grid assembly (modele.hip,
// l1.hip, hntr.hip, globalave.hip, topo.hip) compose them, and so do the two builds at the end of this header, E1vE0 and I2vX,
// which are keyed sums over matrices already in HBM.  Everything is enqueued on the caller's stream and uses the calling
// thread's arena; what waits for the device says so.
#pragma once
#include "common.h"

namespace ibh {

struct Csr { const int32_t *rowptr, *colind; const double *val; int nrow; };
inline Csr view(const ibh_weighted &w) { return Csr{w.rowptr.p, w.colind.p, w.val.p, w.nrow}; }

// out's CSR = L * R as Eigen's conservative sparse product sums it (csrops.hip); resets the arena, one host wait
void csr_product(const ibh_weighted &L, const ibh_weighted &R, ibh_weighted *out, hipStream_t st);
// crop_mvp (GCMRegridder_ModelE.cpp:285-307) along the rows / the columns; one host wait each
//   rows: row m of out is row d_src[m] of `in` (-1: none), its values d_rs[d_src[m]] * v (d_rs may be null)
//   cols: column k of `in` becomes d_map[k] (-1: dropped), values (d_rs[row] * v) * d_cs[d_map[k]], either factor may be null
void crop_rows(const ibh_weighted &in, const int32_t *d_src, int nout, const double *d_rs, ibh_weighted *out, hipStream_t st);
void crop_cols(const ibh_weighted &in, const int32_t *d_map, int ncol_out, const double *d_rs, const double *d_cs, ibh_weighted *out,
               hipStream_t st);
// ---- crop_cols(L) * R where every row of R holds at most one entry (csrcompose.hip) ------------------------------
// The I-row matrices of to_modele: R = XOmvXAm sends an O cell (or one of its elevation classes) to ONE atmosphere column, so the
// product relabels the columns of each row of L and merges equal ones -- a row-local operation, no triplet stream, no global sort.
// Per entry (i, p, v) of L: k = d_map[p] (dropped when k < 0 or row k of R is empty), c = R.colind[R.rowptr[k]],
// t = ((d_rs ? d_rs[i] * v : v) * d_cs[k]) * R.val[R.rowptr[k]] (d_cs may be null as well), every product rounded.  Row i of the
// result: columns c ascending, C(i, c) = its terms summed in ascending k, the first assigned -- the bits of crop_cols + csr_product.
enum ComposeForm { COMPOSED_NONE = 0, COMPOSED_PRODUCT = 1, COMPOSED_ROWLOCAL = 2 };     // as ibh_weighted_composed_by reports them
// Lanes that serve one row: a smoothed ice row holds 19-24 entries on average (8 unsmoothed), so half a wave takes a typical row
// in one pass where a whole wave would idle two lanes in three.
constexpr int COMPOSE_LANES = 32;
// Entries of one row kept in LDS: the longest smoothed row measured is 44, so 128 leaves a factor of three, and the eight rows of
// a workgroup then take 28 KiB -- five workgroups share a CU's 160 KiB.
constexpr int COMPOSE_ROWCAP = 128;
// "modele_rowlocal": 1 whenever the row-local form can serve, 0 never, -1 (default) for smoothed builds only -- unsmoothed rows hold
// a few entries and stay where they were measured
inline bool compose_rowlocal_wanted(bool smoothed) {
    const int v = get_tuning("modele_rowlocal", -1);
    return v > 0 || (v < 0 && smoothed);
}
// out's CSR by the row-local form when `rowlocal` and it can serve -- no row keeps more than COMPOSE_ROWCAP entries and no row of R
// holds two, both found in its counting pass -- else by crop_cols + csr_product; returns the form that built it.  d_map: L.ncol
// entries in [-1, R.nrow), one-to-one.  Resets the arena; two host waits (row-local) or those of the two pieces.
ComposeForm compose_cols(const ibh_weighted &L, const int32_t *d_map, const double *d_rs, const double *d_cs, const ibh_weighted &R,
                         bool rowlocal, ibh_weighted *out, hipStream_t st);
// out's CSR = the transpose of in's (rows few and short: a matrix over the GCM grids); resets the arena
void transpose_csr(const ibh_weighted &in, ibh_weighted *out, hipStream_t st);
// row[e] = the row of entry e, one thread per row (short rows)
void expand_rows(const int32_t *rowptr, int nrow, int32_t *row, hipStream_t st);
// out = 1 / in (out is allocated);  out = a * b;  out[i] = in[idx[i]]
void recip(const double *in, int n, DevBuf<double> &out, hipStream_t st);
void mul(const double *a, const double *b, int n, double *out, hipStream_t st);
void gather(const double *in, const int32_t *idx, long n, double *out, hipStream_t st);
// diag(s) * M in place: val = s[row] * val
void scale_rows(const int32_t *rowptr, int nrow, const double *s, double *val, hipStream_t st);
// M * diag(d) in place: val = val * d[col], each product rounded on its own
void scale_cols(const int32_t *colind, int64_t nnz, const double *d, double *val, hipStream_t st);
// diag(1 / sum) * M in place: one reciprocal per row, val = val * (1 / sum[row]); rows without entries are skipped (their
// sum may be 0)
void scale_rows_recip(const int32_t *rowptr, int nrow, const double *sum, double *val, hipStream_t st);
// compute_E1vE0c (e1ve0.cpp:55-106) on device; `out` comes with identity dims over nE.
void e1ve0_compute(int nsheets, const ibh_weighted *const *XuE1s, const ibh_weighted *const *XuE0s, int64_t nE, ibh_weighted *out);
// make_I2vX's products (global_ec.cpp:345-376): IvI2 = I2vI by columns (rows dense I); fills out's CSR, wM, Mw and flags
void i2vx_compute(const ibh_weighted *IvI2, const ibh_weighted *IvX, ibh_weighted *out);

#ifdef __HIPCC__
// Adds this thread's count into a per-launch total: wave shuffle, one partial per wave in LDS, one atomic per block.  Every
// thread of the block calls it (it synchronises the block); blocks of at most 256 threads.
__device__ inline void add_to_launch_total(unsigned long long c, unsigned long long *__restrict__ total) {
    __shared__ unsigned long long part[4];
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x / 64] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < (int)(blockDim.x / 64); ++w) s += part[w];
        if (s) atomicAdd(total, s);
    }
}
#endif

}  // namespace ibh
