// csrbuild.hip -- the triplets -> CSR layer (csrbuild.h): contributions in emission order -> stable order by (row_d, col_d) ->
// sequential sum per segment, the first term assigned (the order and rounding of Eigen's conservative sparse product and of
// setFromTriplets).  Row sums run sequentially along CSR rows (ascending column) and column sums along a stable by-column
// reordering (ascending row): the orders of spsparse sum().  All of it is index/byte work bound by HBM traffic; no float atomics,
// no FMA contraction (the library is compiled with -ffp-contract=off).
#include "csrbuild.h"
#include "prims.h"
#include <algorithm>

namespace ibh {

// ---- sorted contributions -> unique CSR entries ------------------------------------------------
__global__ void k_head_flags(const uint64_t *__restrict__ keys, size_t n, uint32_t *__restrict__ head,
                             uint32_t *__restrict__ unsorted) {
    size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint64_t key = keys[k], prev = k ? keys[k - 1] : 0;
    head[k] = (k == 0 || key != prev) ? 1u : 0u;
    if (unsorted && k && key < prev) *unsorted = 1u;        // verification of an optimistic (high-field-only) sort
}
// Duplicate (row,col) contributions are summed in sorted (== emission) order, the first term
// ASSIGNED (Eigen's product and setFromTriplets both start from the first value, which keeps a
// signed zero): k_segment_heads lists the segment boundaries, seg_sums<false> does the chains.
__global__ void k_segment_heads(const uint64_t *__restrict__ keys, size_t n, const uint32_t *__restrict__ upos,
                                uint32_t nseg, int32_t *__restrict__ segptr, int32_t *__restrict__ row,
                                int32_t *__restrict__ col) {
    size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint64_t key = keys[k];
    if (k == 0) segptr[nseg] = (int32_t)n;
    if (k != 0 && keys[k - 1] == key) return;
    const uint32_t u = upos[k];
    segptr[u] = (int32_t)k;
    row[u] = (int32_t)(key >> 32);
    col[u] = (int32_t)(key & 0xffffffffu);
}
// rowptr from the (sorted) row index of every entry.  Rows that own entries get their start from the
// entry that opens them; rows WITHOUT entries (a caller-supplied identity set spans every ice cell,
// most of them masked: millions of consecutive empty rows) find theirs by binary search, each on
// its own thread -- a per-entry loop over the gap in front of it would serialise on exactly those runs.
__global__ void k_rowptr_heads(const int32_t *__restrict__ row, long nnz, int32_t *__restrict__ rowptr) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nnz) return;
    const int r = row[u];
    if (u == 0 || row[u - 1] != r) rowptr[r] = (int32_t)u;
}
// first entry whose row is >= q
__device__ __forceinline__ long first_entry_from_row(const int32_t *__restrict__ row, long nnz, int q) {
    long lo = 0, hi = nnz;
    while (lo < hi) {
        const long mid = lo + ((hi - lo) >> 1);
        if (row[mid] < q) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__global__ void k_rowptr_fill(const int32_t *__restrict__ row, long nnz, int nrow, int32_t *__restrict__ rowptr) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q > nrow) return;
    if (q == nrow) { rowptr[q] = (int32_t)nnz; return; }
    if (rowptr[q] >= 0) return;
    rowptr[q] = (int32_t)first_entry_from_row(row, nnz, q);
}
__global__ void k_rowptr_search(const int32_t *__restrict__ row, long nnz, int nrow, int32_t *__restrict__ rowptr) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q > nrow) return;
    rowptr[q] = (int32_t)first_entry_from_row(row, nnz, q);
}
// returns the form taken (CsrBuildTrace: PTR_*)
int rowptr_from_rows(const int32_t *row, long nnz, int nrow, int32_t *rowptr, hipStream_t st) {
    if (nrow < (1 << 16)) {                      // few rows: one launch, every row searches (the small builds are launch-bound)
        hipLaunchKernelGGL(k_rowptr_search, dim3(ceil_div(nrow + 1, 256)), dim3(256), 0, st, row, nnz, nrow, rowptr);
        return PTR_SEARCH;
    }
    IBH_HIP(hipMemsetAsync(rowptr, 0xFF, sizeof(int32_t) * ((size_t)nrow + 1), st));
    if (nnz) hipLaunchKernelGGL(k_rowptr_heads, dim3(ceil_div(nnz, 256)), dim3(256), 0, st, row, nnz, rowptr);
    hipLaunchKernelGGL(k_rowptr_fill, dim3(ceil_div(nrow + 1, 256)), dim3(256), 0, st, row, nnz, nrow, rowptr);
    return PTR_HEADS_FILL;
}
// spsparse sum(M,dim,'+'): one sequential chain per segment (a CSR row in ascending column order,
// or a column in ascending row order through the stable by-column permutation `idx`), exactly
// ret = ret + v starting from 0.  Thread-per-segment suits 1-3 entry segments; the wave form
// loads 64 values coalesced and replays the same sequential chain from registers (every lane
// computes the identical sum), which is what long rows (10^2..10^4 entries) need.
template <bool FROM_ZERO>
__global__ void k_seg_sums_thread(const int32_t *__restrict__ ptr, const uint32_t *__restrict__ idx,
                                  const double *__restrict__ val, int nseg, double *__restrict__ out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nseg) return;
    int k = ptr[r];
    const int end = ptr[r + 1];
    double s = 0.0;
    if (!FROM_ZERO && k < end) { s = val[idx ? idx[k] : (uint32_t)k]; ++k; }
    for (; k < end; ++k) s = s + val[idx ? idx[k] : (uint32_t)k];
    out[r] = s;
}
template <bool FROM_ZERO>
__global__ void k_seg_sums_wave(const int32_t *__restrict__ ptr, const uint32_t *__restrict__ idx,
                                const double *__restrict__ val, int nseg, double *__restrict__ out) {
    const int r = (int)(((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= nseg) return;
    const int beg = ptr[r], end = ptr[r + 1];
    double s = 0.0;
    for (int base = beg; base < end; base += 64) {
        const int k = base + lane;
        const double v = k < end ? val[idx ? idx[k] : (uint32_t)k] : 0.0;
        const int cnt = min(64, end - base);
        const int lo = __double2loint(v), hi = __double2hiint(v);
        int j = 0;
        if (!FROM_ZERO && base == beg) {      // first term assigned
            s = __hiloint2double(__builtin_amdgcn_readlane(hi, 0), __builtin_amdgcn_readlane(lo, 0));
            j = 1;
        }
        if (cnt == 64 && j == 0) {
#pragma unroll
            for (int q = 0; q < 64; ++q)
                s = s + __hiloint2double(__builtin_amdgcn_readlane(hi, q), __builtin_amdgcn_readlane(lo, q));
        } else {
            for (; j < cnt; ++j)
                s = s + __hiloint2double(__builtin_amdgcn_readlane(hi, j), __builtin_amdgcn_readlane(lo, j));
        }
    }
    if (lane == 0) out[r] = s;
}
// returns the form taken (CsrBuildTrace: SEG_*)
template <bool FROM_ZERO>
int seg_sums(const int32_t *ptr, const uint32_t *idx, const double *val, int nseg, long nnz, double *out,
             hipStream_t st) {
    if (nseg == 0) return SEG_NONE;
    if (nnz >= 8l * nseg) {
        hipLaunchKernelGGL(k_seg_sums_wave<FROM_ZERO>, dim3(ceil_div((long)nseg * 64, 256)), dim3(256), 0, st, ptr, idx, val, nseg, out);
        return SEG_WAVE;
    }
    hipLaunchKernelGGL(k_seg_sums_thread<FROM_ZERO>, dim3(ceil_div(nseg, 256)), dim3(256), 0, st, ptr, idx, val, nseg, out);
    return SEG_THREAD;
}
template int seg_sums<true>(const int32_t *, const uint32_t *, const double *, int, long, double *, hipStream_t);
template int seg_sums<false>(const int32_t *, const uint32_t *, const double *, int, long, double *, hipStream_t);
__global__ void k_col_keys(const int32_t *__restrict__ col, long nnz, uint64_t *__restrict__ keys, uint32_t *__restrict__ idx) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u < nnz) { keys[u] = (uint64_t)(uint32_t)col[u]; idx[u] = (uint32_t)u; }
}
__global__ void k_keys_to_i32(const uint64_t *__restrict__ keys, long n, int32_t *__restrict__ out) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u < n) out[u] = (int32_t)keys[u];
}
void keys_to_i32(const uint64_t *keys, long n, int32_t *out, hipStream_t st) {
    hipLaunchKernelGGL(k_keys_to_i32, dim3(ceil_div(n, 256)), dim3(256), 0, st, keys, n, out);
}
// cs[c] = spsparse sum(M, 1, '+') of column c of w's CSR: the entries ordered by column (a stable radix sort keeps the rows of a
// column ascending), then summed per column.  Enqueued on st.
// forms (may be null): {the seg_sums form, the rowptr_from_rows form} it took
void col_sums_by_sort(const ibh_weighted *w, int ncol, double *cs, hipStream_t st, int *forms) {
    const long nnz = w->nnz;
    if (forms) forms[0] = SEG_NONE, forms[1] = PTR_NONE;
    if (!nnz) {
        if (ncol) IBH_HIP(hipMemsetAsync(cs, 0, sizeof(double) * (size_t)ncol, st));
        return;
    }
    Arena &A = arena();
    const int T = 256;
    uint64_t *ck = A.get<uint64_t>((size_t)nnz), *ck2 = A.get<uint64_t>((size_t)nnz);
    uint32_t *ci = A.get<uint32_t>((size_t)nnz), *ci2 = A.get<uint32_t>((size_t)nnz);
    hipLaunchKernelGGL(k_col_keys, dim3(ceil_div(nnz, T)), dim3(T), 0, st, w->colind.p, nnz, ck, ci);
    KeyField f{0, bits_for((uint64_t)ncol)};
    if (f.nbits > 0 && radix_sort_pairs(ck, ck2, ci, ci2, (size_t)nnz, &f, 1, st)) { std::swap(ck, ck2); std::swap(ci, ci2); }
    int32_t *scol = A.get<int32_t>((size_t)nnz), *colptr = A.get<int32_t>((size_t)ncol + 1);
    keys_to_i32(ck, nnz, scol, st);
    const int pf = rowptr_from_rows(scol, nnz, ncol, colptr, st);
    const int sf = seg_sums<true>(colptr, ci, w->val.p, ncol, nnz, cs, st);
    if (forms) forms[0] = sf, forms[1] = pf;
}

// ---- column sums for matrices with short columns (AvI, EvI, AvX, EvX, AvE: <= a few rows per column) ----
// spsparse sum(M, 1, '+') visits a column in ascending row order.  Instead of reordering all nnz
// entries by column (three radix passes), the entries are dropped into per-column slots
// (integer atomics: which slot an entry gets is not deterministic, the SET in a column is) and each
// column is summed by one thread: 1 or 2 entries need no order at all ((0+a)+b == (0+b)+a bit for
// bit); longer columns pick their entries in ascending row order by repeated selection (rows are
// unique inside a column).  Columns of more than 64 entries go to a wave each.  Only used when
// nnz <= 4*ncol, so long columns are the exception (an ice cell under a GCM-cell corner: 4).
__global__ void k_col_count(const int32_t *__restrict__ col, long nnz, uint32_t *__restrict__ cnt) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u < nnz) atomicAdd(&cnt[col[u]], 1u);
}
__global__ void k_col_scatter(const int32_t *__restrict__ row, const int32_t *__restrict__ col, long nnz,
                              const uint32_t *__restrict__ colptr, uint32_t *__restrict__ fillc,
                              int32_t *__restrict__ lrow, uint32_t *__restrict__ lidx) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nnz) return;
    const int c = col[u];
    const uint32_t p = colptr[c] + atomicAdd(&fillc[c], 1u);
    lrow[p] = row[u];
    lidx[p] = (uint32_t)u;
}
__global__ void k_col_sums(const uint32_t *__restrict__ colptr, int ncol, const int32_t *__restrict__ lrow,
                           const uint32_t *__restrict__ lidx, const double *__restrict__ val, double *__restrict__ cs,
                           uint32_t *__restrict__ nlong, int32_t *__restrict__ longcols) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncol) return;
    const uint32_t b = colptr[c], e = colptr[c + 1];
    const uint32_t n = e - b;
    double s = 0.0;
    if (n <= 2) {
        if (n > 0) s = s + val[lidx[b]];
        if (n > 1) s = s + val[lidx[b + 1]];
    } else if (n <= 64) {
        int prev = -1;
        for (uint32_t k = 0; k < n; ++k) {
            int best = 0x7fffffff; uint32_t at = b;
            for (uint32_t j = b; j < e; ++j) {
                const int r = lrow[j];
                if (r > prev && r < best) { best = r; at = j; }
            }
            s = s + val[lidx[at]];
            prev = best;
        }
    } else {
        longcols[atomicAdd(nlong, 1u)] = c;
        return;
    }
    cs[c] = s;
}
__global__ void k_col_sums_long(const uint32_t *__restrict__ colptr, const int32_t *__restrict__ lrow,
                                const uint32_t *__restrict__ lidx, const double *__restrict__ val, double *__restrict__ cs,
                                const uint32_t *__restrict__ nlong, const int32_t *__restrict__ longcols) {
    const int lane = threadIdx.x & 63;
    const uint32_t nl = *nlong;
    for (uint32_t q = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; q < nl; q += (gridDim.x * blockDim.x) >> 6) {
        const int c = longcols[q];
        const uint32_t b = colptr[c], e = colptr[c + 1];
        double s = 0.0;
        int prev = -1;
        for (uint32_t k = b; k < e; ++k) {            // one selection round per entry, 64 candidates per step
            int best = 0x7fffffff; uint32_t at = b;
            for (uint32_t j = b + lane; j < e; j += 64) {
                const int r = lrow[j];
                if (r > prev && r < best) { best = r; at = j; }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const int ob = __shfl_xor(best, off, 64); const uint32_t oa = __shfl_xor(at, off, 64);
                if (ob < best) { best = ob; at = oa; }
            }
            s = s + val[lidx[at]];
            prev = best;
        }
        if (lane == 0) cs[c] = s;
    }
}
ColSlots col_slots(const int32_t *colind, const int32_t *row, long nnz, int ncol, hipStream_t st) {
    Arena &A = arena();
    const int T = 256;
    ColSlots s;
    s.colptr = A.get<uint32_t>((size_t)ncol + 1);
    uint32_t *cntc = A.get<uint32_t>(2 * (size_t)ncol + 1), *fillc = cntc + ncol;    // zeroed together
    s.nlong = fillc + ncol;
    s.lrow = A.get<int32_t>((size_t)nnz);
    s.lidx = A.get<uint32_t>((size_t)nnz);
    IBH_HIP(hipMemsetAsync(cntc, 0, sizeof(uint32_t) * (2 * (size_t)ncol + 1), st));
    hipLaunchKernelGGL(k_col_count, dim3(ceil_div(nnz, T)), dim3(T), 0, st, colind, nnz, cntc);
    exclusive_scan_u32(cntc, s.colptr, (size_t)ncol, s.colptr + ncol, st);
    hipLaunchKernelGGL(k_col_scatter, dim3(ceil_div(nnz, T)), dim3(T), 0, st, row, colind, nnz, s.colptr, fillc, s.lrow, s.lidx);
    return s;
}
ColSlots col_sums_by_slots(const ibh_weighted *w, const int32_t *row, int ncol, double *cs, hipStream_t st) {
    const int T = 256;
    const ColSlots s = col_slots(w->colind.p, row, w->nnz, ncol, st);
    int32_t *longcols = arena().get<int32_t>((size_t)ncol);
    hipLaunchKernelGGL(k_col_sums, dim3(ceil_div(ncol, T)), dim3(T), 0, st, s.colptr, ncol, s.lrow, s.lidx, w->val.p, cs, s.nlong, longcols);
    hipLaunchKernelGGL(k_col_sums_long, dim3(256), dim3(T), 0, st, s.colptr, s.lrow, s.lidx, w->val.p, cs, s.nlong, longcols);
    return s;
}

// ---- shared: sorted (row,col,idx) contributions -> Weighted CSR ---------------------------------
Triplets triplets_in_arena(size_t n) {
    Arena &A = arena();
    Triplets t;
    t.n = n;
    t.keys = A.get<uint64_t>(n); t.keys_alt = A.get<uint64_t>(n);
    t.idx = A.get<uint32_t>(n); t.idx_alt = A.get<uint32_t>(n);
    t.term = A.get<double>(n);
    return t;
}

// ---- contributions -> CSR for matrices with short rows (IvA, IvE, XvA, XvE: 1-8 contributions per row) ----
// No ordering of the whole list: contributions are dropped into per-row slots (integer atomics: the
// slot inside a row is arbitrary, the SET is not) and one thread per row lists its entries in
// ascending (column, emission index) order by repeated selection, summing equal columns in emission
// order with the first term assigned -- exactly what the sort-based path produces.  Rows of more than
// SR_MAX contributions set a flag and the caller falls back to that path.
constexpr int SRB_MAX = 32;
__global__ void k_srb_count(const uint64_t *__restrict__ keys, size_t n, uint32_t *__restrict__ cnt) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) atomicAdd(&cnt[keys[k] >> 32], 1u);
}
__global__ void k_srb_scatter(const uint64_t *__restrict__ keys, size_t n, const uint32_t *__restrict__ slotptr,
                              uint32_t *__restrict__ fillr, uint32_t *__restrict__ scol, uint32_t *__restrict__ sidx) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint64_t key = keys[k];
    const uint32_t r = (uint32_t)(key >> 32);
    const uint32_t p = slotptr[r] + atomicAdd(&fillr[r], 1u);
    scol[p] = (uint32_t)key;
    sidx[p] = (uint32_t)k;                   // emission index (contributions are still in emission order)
}
// next (col, idx) pair after (pc, pi) in the row's slots; returns false when there is none
__device__ __forceinline__ bool srb_next(const uint32_t *__restrict__ scol, const uint32_t *__restrict__ sidx, uint32_t b,
                                         uint32_t e, bool first, uint32_t pc, uint32_t pi, uint32_t &bc, uint32_t &bi) {
    bool any = false;
    for (uint32_t j = b; j < e; ++j) {
        const uint32_t c = scol[j], i = sidx[j];
        const bool after = first || c > pc || (c == pc && i > pi);
        if (after && (!any || c < bc || (c == bc && i < bi))) { bc = c; bi = i; any = true; }
    }
    return any;
}
__global__ void k_srb_unique(const uint32_t *__restrict__ slotptr, int nrow, const uint32_t *__restrict__ scol,
                             uint32_t *__restrict__ ucnt, uint32_t *__restrict__ too_long) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrow) return;
    const uint32_t b = slotptr[r], e = slotptr[r + 1];
    if (e - b > (uint32_t)SRB_MAX) { *too_long = 1u; ucnt[r] = 0; return; }
    uint32_t u = 0;
    for (uint32_t j = b; j < e; ++j) {        // distinct columns: count the first occurrence of each
        bool seen = false;
        for (uint32_t q = b; q < j; ++q) seen = seen || scol[q] == scol[j];
        u += seen ? 0u : 1u;
    }
    ucnt[r] = u;
}
__global__ void k_srb_emit(const uint32_t *__restrict__ slotptr, int nrow, const uint32_t *__restrict__ scol,
                           const uint32_t *__restrict__ sidx, const double *__restrict__ term,
                           const int32_t *__restrict__ rowptr, int32_t *__restrict__ row, int32_t *__restrict__ col,
                           double *__restrict__ val) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrow) return;
    const uint32_t b = slotptr[r], e = slotptr[r + 1];
    int out = rowptr[r] - 1;
    uint32_t pc = 0, pi = 0, bc = 0, bi = 0;
    bool first = true;
    double s = 0.0;
    while (srb_next(scol, sidx, b, e, first, pc, pi, bc, bi)) {
        if (first || bc != pc) {               // a new (row, col): the first term is assigned
            if (!first) val[out] = s;
            ++out;
            row[out] = r; col[out] = (int32_t)bc;
            s = term[bi];
        } else {
            s = s + term[bi];                  // duplicates in emission order
        }
        pc = bc; pi = bi; first = false;
    }
    if (!first) val[out] = s;
}
// returns false (nothing built) when a row is too long for the per-thread selection
static bool build_csr_short_rows(ibh_weighted *w, const Triplets &t, int nrow, int ncol, int32_t **row_out, hipStream_t st) {
    Arena &A = arena();
    const int T = 256;
    uint32_t *cnt = A.get<uint32_t>(2 * (size_t)nrow + 2), *fillr = cnt + nrow, *too_long = fillr + nrow, *d_nnz = too_long + 1;
    uint32_t *slotptr = A.get<uint32_t>((size_t)nrow + 1), *ucnt = A.get<uint32_t>((size_t)nrow);
    uint32_t *scol = A.get<uint32_t>(t.n), *sidx = A.get<uint32_t>(t.n);
    IBH_HIP(hipMemsetAsync(cnt, 0, sizeof(uint32_t) * (2 * (size_t)nrow + 2), st));
    hipLaunchKernelGGL(k_srb_count, dim3(ceil_div(t.n, T)), dim3(T), 0, st, t.keys, t.n, cnt);
    exclusive_scan_u32(cnt, slotptr, (size_t)nrow, slotptr + nrow, st);
    hipLaunchKernelGGL(k_srb_scatter, dim3(ceil_div(t.n, T)), dim3(T), 0, st, t.keys, t.n, slotptr, fillr, scol, sidx);
    hipLaunchKernelGGL(k_srb_unique, dim3(ceil_div(nrow, T)), dim3(T), 0, st, slotptr, nrow, scol, ucnt, too_long);
    w->rowptr.alloc((size_t)nrow + 1);
    exclusive_scan_u32(ucnt, reinterpret_cast<uint32_t *>(w->rowptr.p), (size_t)nrow, d_nnz, st);
    uint32_t h[2];
    readback_sync(h, too_long, sizeof(h), st);
    if (h[0]) return false;
    const uint32_t nnz = h[1];
    IBH_CHECK(nnz < (1u << 31), "nnz overflows int32");
    w->nrow = nrow; w->ncol = ncol; w->nnz = nnz;
    IBH_HIP(hipMemcpyAsync(w->rowptr.p + nrow, d_nnz, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    w->colind.alloc(nnz); w->val.alloc(nnz);
    int32_t *row = A.get<int32_t>(nnz);
    hipLaunchKernelGGL(k_srb_emit, dim3(ceil_div(nrow, T)), dim3(T), 0, st, slotptr, nrow, scol, sidx, t.term, w->rowptr.p, row,
                       w->colind.p, w->val.p);
    IBH_HIP(hipGetLastError());
    *row_out = row;
    return true;
}

// trace (may be null): the forms this build took
void build_csr_from_contributions(ibh_weighted *w, Triplets t, int nrow, int ncol, int32_t **row_out,
                                  hipStream_t st, bool expect_local, CsrBuildTrace *trace) {
    Arena &A = arena();
    const int T = 256;
    CsrBuildTrace unread;
    CsrBuildTrace &tr = trace ? *trace : unread;
    tr = CsrBuildTrace{};
    w->nrow = nrow; w->ncol = ncol;
    w->rowptr.alloc((size_t)nrow + 1);
    if (t.n == 0) {
        w->nnz = 0;
        w->rowptr.zero(st);
        w->colind.alloc(0); w->val.alloc(0);
        *row_out = nullptr;
        return;
    }
    // ice / exchange rows with a handful of contributions each: per-row slots, no ordering of the list
    // (measured: always for ~1 contribution per row; with 2+ per row -- IvE -- only while the build is
    // launch-bound, at 35 M contributions the radix passes are cheaper than the per-row selection)
    if (!expect_local && nrow > 0 && t.n <= 8 * (size_t)nrow && (2 * t.n <= 3 * (size_t)nrow || t.n < (4u << 20))) {
        const bool taken = build_csr_short_rows(w, t, nrow, ncol, row_out, st);
        tr.short_rows = taken ? SRB_TAKEN : SRB_DECLINED;
        if (taken) return;
    }
    // Order analysis + piece sort, then (speculatively, on the data as it stands) the duplicate
    // flags and their scan: ONE host synchronisation returns both the analysis and nnz.  Only when a
    // piece was too long for LDS (nothing was touched) does the radix sort run and the tail repeat.
    const int lo_bits = bits_for((uint64_t)ncol), hi_bits = bits_for((uint64_t)nrow);
    struct Readback { OrderInfo info; uint32_t total, unsorted; } rb;
    Readback *d_rb = A.get<Readback>(1);
    uint32_t *head = A.get<uint32_t>(t.n);
    uint32_t *d_total = &d_rb->total;
    auto flags_and_count = [&](bool verify) {
        hipLaunchKernelGGL(k_head_flags, dim3(ceil_div(t.n, T)), dim3(T), 0, st, t.keys, t.n, head, verify ? &d_rb->unsorted : nullptr);
        exclusive_scan_u32(head, head, t.n, d_total, st);
    };
    order_and_chunk_sort(t.keys, t.idx, t.n, &d_rb->info, st, expect_local);
    IBH_HIP(hipMemsetAsync(&d_rb->unsorted, 0, sizeof(uint32_t), st));
    if (expect_local) flags_and_count(false);
    readback_sync(&rb, d_rb, sizeof(rb), st);
    order_debug(rb.info, t.n, lo_bits, hi_bits);
    const bool resort = t.n >= 2 && !order_is_final(rb.info);
    if (resort) {
        // Ice-cell rows: the column field is not monotone along the whole sequence (elevation classes),
        // but inside each ROW it is when the exchange grid is sorted (later cells = later GCM cells =
        // later class ids).  Then a stable sort by the row field alone is the full order: do that
        // first and verify; only a failed check pays for the column passes.
        const bool optimistic = !expect_local && (rb.info.flags & ORD_LO_DEC) && hi_bits > 0;
        OrderInfo plan = rb.info;
        if (optimistic) plan.flags &= ~(uint32_t)ORD_LO_DEC;
        tr.order = ORDER_RADIX;
        if (optimistic) tr.optimistic = OPT_HELD;
        if (radix_after_analysis(plan, t.keys, t.keys_alt, t.idx, t.idx_alt, t.n, lo_bits, hi_bits, st)) {
            std::swap(t.keys, t.keys_alt); std::swap(t.idx, t.idx_alt);
        }
        flags_and_count(optimistic);
        readback_sync(&rb.total, d_total, 2 * sizeof(uint32_t), st);
        if (optimistic && rb.unsorted) {
            tr.optimistic = OPT_FAILED;
            if (radix_after_analysis(rb.info, t.keys, t.keys_alt, t.idx, t.idx_alt, t.n, lo_bits, hi_bits, st)) {
                std::swap(t.keys, t.keys_alt); std::swap(t.idx, t.idx_alt);
            }
            flags_and_count(false);
            readback_sync(&rb.total, d_total, sizeof(uint32_t), st);
        }
    } else {
        tr.order = t.n >= 2 && (rb.info.flags & ORD_FULL_DEC) ? ORDER_PIECES : ORDER_IN_ORDER;
        if (!expect_local) {
            flags_and_count(false);
            readback_sync(&rb.total, d_total, sizeof(uint32_t), st);
        }
    }
    const uint32_t nnz = rb.total;
    IBH_CHECK(nnz < (1u << 31), "nnz overflows int32");
    w->nnz = nnz;
    w->colind.alloc(nnz); w->val.alloc(nnz);
    int32_t *row = A.get<int32_t>(nnz);
    int32_t *segptr = A.get<int32_t>((size_t)nnz + 1);
    hipLaunchKernelGGL(k_segment_heads, dim3(ceil_div(t.n, T)), dim3(T), 0, st, t.keys, t.n, head, nnz, segptr, row, w->colind.p);
    tr.seg_form = seg_sums<false>(segptr, t.idx, t.term, (int)nnz, (long)t.n, w->val.p, st);
    tr.rowptr_form = rowptr_from_rows(row, (long)nnz, nrow, w->rowptr.p, st);
    IBH_HIP(hipGetLastError());
    *row_out = row;
}

// ---- ibh_weighted_from_coo: Eigen setFromTriplets on device -----------------------------------
__global__ void k_coo_keys(const int32_t *__restrict__ row, const int32_t *__restrict__ col, size_t n,
                           uint64_t *__restrict__ keys, uint32_t *__restrict__ idx) {
    size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) { keys[k] = ((uint64_t)(uint32_t)row[k] << 32) | (uint32_t)col[k]; idx[k] = (uint32_t)k; }
}
// n COO triplets (dense ids, input order) as contributions in the arena.  kind == hipMemcpyHostToDevice: host arrays, the indices
// are uploaded into the arena first; hipMemcpyDeviceToDevice: device arrays, the indices are read where they are
static Triplets triplets_from_coo(int64_t n, const int32_t *row, const int32_t *col, const double *val, hipMemcpyKind kind,
                                  hipStream_t st) {
    Triplets t = triplets_in_arena((size_t)n);
    if (!n) return t;
    if (kind == hipMemcpyHostToDevice) {
        Arena &A = arena();
        int32_t *drow = A.get<int32_t>((size_t)n), *dcol = A.get<int32_t>((size_t)n);
        IBH_HIP(hipMemcpyAsync(drow, row, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
        IBH_HIP(hipMemcpyAsync(dcol, col, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
        row = drow; col = dcol;
    }
    IBH_HIP(hipMemcpyAsync(t.term, val, sizeof(double) * t.n, kind, st));
    hipLaunchKernelGGL(k_coo_keys, dim3(ceil_div(n, 256)), dim3(256), 0, st, row, col, t.n, t.keys, t.idx);
    return t;
}
// Eigen setFromTriplets of n triplets (dense ids, input order), host or device arrays by `kind`
static void csr_from_triplets(ibh_weighted *w, int nrow, int ncol, int64_t n, const int32_t *row, const int32_t *col, const double *val,
                              hipMemcpyKind kind, hipStream_t st) {
    const Triplets t = triplets_from_coo(n, row, col, val, kind, st);
    int32_t *erow = nullptr;
    build_csr_from_contributions(w, t, nrow, ncol, &erow, st);
}
void weighted_from_coo_device(ibh_weighted *w, int nrow, int ncol, int64_t n, const int32_t *row, const int32_t *col,
                              const double *val) {
    hipStream_t st = nullptr;
    arena().reset();
    csr_from_triplets(w, nrow, ncol, n, row, col, val, hipMemcpyHostToDevice, st);
    IBH_HIP(hipStreamSynchronize(st));
}

void csr_from_device_triplets(ibh_weighted *w, int nrow, int ncol, int64_t n, const int32_t *drow, const int32_t *dcol,
                              const double *dval, hipStream_t st) {
    csr_from_triplets(w, nrow, ncol, n, drow, dcol, dval, hipMemcpyDeviceToDevice, st);
    IBH_HIP(hipGetLastError());
}

// setFromTriplets from triplets already on the device (dense ids, input order) and the plain weights wM / Mw = spsparse
// sum(M, dim, '+') (columns visited ascending, rows ascending inside): the general-dims path of the Hntr matrices (hntr.hip).
// Enqueued on `st`; reads nothing back but nnz.  The arena is not reset: the caller's triplets may live there.  n == 0: the
// empty CSR over the given shape with zeroed wM / Mw.
void weighted_from_device_triplets(ibh_weighted *w, int nrow, int ncol, int64_t n, const int32_t *drow, const int32_t *dcol,
                                   const double *dval, hipStream_t st) {
    csr_from_triplets(w, nrow, ncol, n, drow, dcol, dval, hipMemcpyDeviceToDevice, st);
    w->wM.alloc((size_t)nrow); w->Mw.alloc((size_t)ncol);
    seg_sums<true>(w->rowptr.p, nullptr, w->val.p, nrow, w->nnz, w->wM.p, st);
    if (!w->nnz && nrow) IBH_HIP(hipMemsetAsync(w->wM.p, 0, sizeof(double) * (size_t)nrow, st));
    col_sums_by_sort(w, ncol, w->Mw.p, st);
    IBH_HIP(hipGetLastError());
}

// ibh_selftest_triplets: the shared triplets -> CSR build on host triplets, with the weights as a matrix build takes them
static void selftest_triplets(int nrow, int ncol, int64_t n, const int32_t *row, const int32_t *col, const double *val, bool expect_local,
                              ibh_weighted *w, int32_t *info) {
    hipStream_t st = hipStreamPerThread;
    arena().reset();
    const Triplets t = triplets_from_coo(n, row, col, val, hipMemcpyHostToDevice, st);
    CsrBuildTrace tr;
    int32_t *erow = nullptr;
    build_csr_from_contributions(w, t, nrow, ncol, &erow, st, expect_local, &tr);
    const long nnz = w->nnz;
    w->wM.alloc((size_t)nrow); w->Mw.alloc((size_t)ncol);
    const int wM_form = seg_sums<true>(w->rowptr.p, nullptr, w->val.p, nrow, nnz, w->wM.p, st);
    int Mw_forms[2] = {SEG_NONE, PTR_NONE};
    uint32_t nlong = 0;
    const bool slots = short_columns(nnz, ncol);
    if (slots) {
        const ColSlots s = col_sums_by_slots(w, erow, ncol, w->Mw.p, st);
        readback_sync(&nlong, s.nlong, sizeof(nlong), st);
    } else {
        col_sums_by_sort(w, ncol, w->Mw.p, st, Mw_forms);
    }
    IBH_HIP(hipGetLastError());
    IBH_HIP(hipStreamSynchronize(st));
    const int32_t out[IBH_TRIPLETS_INFO] = {tr.order, tr.short_rows, tr.optimistic, tr.seg_form, tr.rowptr_form, wM_form,
                                            slots ? 1 : nnz ? 2 : 0, (int32_t)nlong, Mw_forms[0], Mw_forms[1]};
    std::copy(out, out + IBH_TRIPLETS_INFO, info);
}

}  // namespace ibh

using namespace ibh;
extern "C" {

int ibh_selftest_triplets(int32_t nrow, int32_t ncol, int64_t n, const int32_t *row, const int32_t *col, const double *val, int mode,
                          ibh_weighted **out, int32_t *info_out) {
    if (out) *out = nullptr;
    return guarded([&] {
        IBH_CHECK(out && info_out, "null argument");
        IBH_CHECK(nrow >= 0 && ncol >= 0 && n >= 0 && n < (1ll << 31), "bad sizes %d x %d, %lld triplets", nrow, ncol, (long long)n);
        IBH_CHECK(n == 0 || (row && col && val), "null triplets");
        IBH_CHECK(mode == 0 || mode == 1, "mode %d is neither 0 (expect_local) nor 1", mode);
        for (int64_t k = 0; k < n; ++k)
            IBH_CHECK(row[k] >= 0 && row[k] < nrow && col[k] >= 0 && col[k] < ncol, "triplet %lld (%d, %d) outside %d x %d", (long long)k,
                      row[k], col[k], nrow, ncol);
        require_device();
        auto w = new_weighted();
        selftest_triplets(nrow, ncol, n, row, col, val, mode == 0, w.get(), info_out);
        w->conservative = 1; w->scaled = 0;
        w->dims[0] = DimRef::owned_identity(nrow); w->dims[1] = DimRef::owned_identity(ncol);
        *out = w.release();
    });
}

}  // extern "C"
