// csrbuild.h -- the triplets -> CSR layer (csrbuild.hip): contributions (key = (row, col), emission index, term) -> unique CSR
// entries summed in emission order with the first term assigned, the row pointer, the row and column sums in spsparse's order, and
// the COO entry points on top of them.  Every matrix builder of the library ends here: the exchange-grid assembly (assemble.hip), the smoother
// (smooth.hip), the CSR algebra (csrops.hip) and, through the COO entry points, hntr / l1 / modele / globalave.  Everything is
// enqueued on the caller's stream and uses the calling thread's arena; what waits for the device says so.
#pragma once
#include "common.h"

namespace ibh {
// The forms one triplets -> CSR build took (build_csr_from_contributions), as ibh_selftest_triplets reports them; introspection only
enum { ORDER_IN_ORDER = 0, ORDER_PIECES = 1, ORDER_RADIX = 2 };     // the contributions were in order / pieces sorted in LDS / radix
enum { SRB_NOT_TRIED = 0, SRB_TAKEN = 1, SRB_DECLINED = 2 };        // per-row slots (a row over SRB_MAX declines, then the sort)
enum { OPT_NOT_TRIED = 0, OPT_HELD = 1, OPT_FAILED = 2 };           // the optimistic row-only sort and its check
enum { SEG_NONE = 0, SEG_THREAD = 1, SEG_WAVE = 2 };                // seg_sums: no launch / a thread / a wave per segment
enum { PTR_NONE = 0, PTR_SEARCH = 1, PTR_HEADS_FILL = 2 };          // rowptr_from_rows: every row searches / heads + fill
struct CsrBuildTrace { int order = ORDER_IN_ORDER, short_rows = SRB_NOT_TRIED, optimistic = OPT_NOT_TRIED, seg_form = SEG_NONE,
                       rowptr_form = PTR_NONE; };

// n contributions in emission order: keys = (row << 32) | col over dense ids, idx = the emission index, term = the value; the
// *_alt buffers are the other half of the sort's ping-pong
struct Triplets { uint64_t *keys, *keys_alt; uint32_t *idx, *idx_alt; double *term; size_t n; };
Triplets triplets_in_arena(size_t n);
// w's CSR (rowptr, colind, val, nrow, ncol, nnz) from the contributions; *row_out: the row of every entry (arena; null when
// there is none).  expect_local: the keys are nearly in order (GCM-cell rows), else ice / exchange rows with a handful of
// contributions each.  Waits for the device (nnz is read back).  trace (may be null): the forms this build took
void build_csr_from_contributions(ibh_weighted *w, Triplets t, int nrow, int ncol, int32_t **row_out, hipStream_t st,
                                  bool expect_local = true, CsrBuildTrace *trace = nullptr);
// rowptr from the (sorted) row index of every entry; returns the form taken (CsrBuildTrace: PTR_*)
int rowptr_from_rows(const int32_t *row, long nnz, int nrow, int32_t *rowptr, hipStream_t st);
// out[r] = the sequential sum of val over segment r (through idx when it is not null): from 0, or <false> the first term
// assigned; returns the form taken (CsrBuildTrace: SEG_*).  The two instantiations are csrbuild.hip's.
template <bool FROM_ZERO>
int seg_sums(const int32_t *ptr, const uint32_t *idx, const double *val, int nseg, long nnz, double *out, hipStream_t st);
// out[u] = (int32_t)keys[u]
void keys_to_i32(const uint64_t *keys, long n, int32_t *out, hipStream_t st);
// cs[c] = spsparse sum(M, 1, '+') of column c of w's CSR: the entries ordered by column (a stable radix sort keeps the rows of a
// column ascending), then summed per column.  Enqueued on st.
// forms (may be null): {the seg_sums form, the rowptr_from_rows form} it took
void col_sums_by_sort(const ibh_weighted *w, int ncol, double *cs, hipStream_t st, int *forms = nullptr);
// the matrices whose column sums go through the slots (col_sums_by_slots) instead of the sort (col_sums_by_sort)
inline bool short_columns(long nnz, int ncol) { return nnz && nnz <= 4l * ncol; }
// Per-column slots of a CSR's entries (`row`: the row of every entry): column c owns [colptr[c], colptr[c + 1]), slot p holds the
// row lrow[p] of entry lidx[p], in no particular order inside a column.  nlong: a zeroed device counter behind the slots' counters
// (col_sums_by_slots counts there the columns that went to k_col_sums_long).  Arena; enqueued on st.
struct ColSlots { uint32_t *colptr = nullptr, *lidx = nullptr; int32_t *lrow = nullptr; uint32_t *nlong = nullptr; };
ColSlots col_slots(const int32_t *colind, const int32_t *row, long nnz, int ncol, hipStream_t st);
// cs = the column sums of w's CSR through per-column slots, for short_columns().  The slots are handed back for build_bands (applystruct.h).
// Enqueued on st.
ColSlots col_sums_by_slots(const ibh_weighted *w, const int32_t *row, int ncol, double *cs, hipStream_t st);

// Eigen setFromTriplets (to_eigen_M, eigen_types.cpp:9-34) on device: fills w's CSR from host COO.
void weighted_from_coo_device(ibh_weighted *w, int nrow, int ncol, int64_t n, const int32_t *row, const int32_t *col,
                              const double *val);
// setFromTriplets from DEVICE triplets (dense ids, input order) plus wM / Mw = sum(M, dim, '+'), enqueued on st
void weighted_from_device_triplets(ibh_weighted *w, int nrow, int ncol, int64_t n, const int32_t *drow, const int32_t *dcol,
                                   const double *dval, hipStream_t st);
// the same without the weights: only w's CSR (csrops.hip: the products and re-numbered copies)
void csr_from_device_triplets(ibh_weighted *w, int nrow, int ncol, int64_t n, const int32_t *drow, const int32_t *dcol,
                              const double *dval, hipStream_t st);
}  // namespace ibh
