// applystruct.hip -- the builders of a matrix's apply structures on gfx950: bands (rowdual), the column sweep (colsweep), row
// groups and their tiles (rowgroup, grouptile).  Each takes a finished CSR and returns a value of its type (common.h) that the
// apply kernels read (spmm.hip, sweep_kernel.inl; which structure an apply wants: apply_plan.h).  spmm.hip calls the *_from_csr
// forms lazily; the assembly (assemble.hip) calls build_bands while it still has the per-column slots.  Index and byte work only:
// scans, stable radix sorts (prims.h) and exact copies of M's values.
#include "applystruct.h"
#include "csrbuild.h"
#include "prims.h"
#include "sweep_kernel.inl"      // SWEEP_HAS*: the item meta word (no kernel of it is instantiated here)
#include <cstdlib>
#include <vector>

namespace ibh {

// ---- bands for the rowdual apply kernel (spmm.hip) -----------------------------------------------
// An ice cell between two elevation classes is a column of TWO rows of an E-row matrix: (cell a,
// class k) with weight 1-r and (a, k+1) with weight r.  Row by row its field value is fetched twice.
// The band structure lists every (GCM cell, ice cell) pair ONCE, in the lower row, with both weights:
// band r = the entries of row r that are not the upper partner of an entry of the row below, in CSR
// order (columns ascending); an upper partner is attached to its lower entry.  Pairing is decided per
// column from its few entries (per-column slots of the short-column path): within one GCM cell,
// classes pair up from the lowest (k, k+1), so the partner row of a band is always the same row.
// A filtered copy of the CSR: no sorting, exact copies of M's values.
// (hc.split<true>: a regridder's strides are checked when it is made)
__global__ void k_band_roles(HcIndexing hc, const int64_t *__restrict__ row_s, const uint32_t *__restrict__ colptr, int ncol,
                             const int32_t *__restrict__ lrow, const uint32_t *__restrict__ lidx,
                             uint32_t *__restrict__ lower, int32_t *__restrict__ partner) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncol) return;
    const uint32_t b = colptr[c], e = colptr[c + 1];
    for (uint32_t i = b; i < e; ++i) {
        long ai, hi;
        hc.split<true>(row_s[lrow[i]], ai, hi);
        // number of consecutive classes directly below this entry in the same GCM cell: odd -> upper partner
        int below = 0;
        int32_t up = -1;                       // the entry one class above (its partner if this one is a lower entry)
        for (long t = hi - 1;; --t) {
            bool found = false;
            for (uint32_t j = b; j < e && !found; ++j) {
                long aj, hj;
                hc.split<true>(row_s[lrow[j]], aj, hj);
                found = aj == ai && hj == t;
            }
            if (!found) break;
            ++below;
        }
        for (uint32_t j = b; j < e; ++j) {
            long aj, hj;
            hc.split<true>(row_s[lrow[j]], aj, hj);
            if (aj == ai && hj == hi + 1) up = (int32_t)lidx[j];
        }
        const bool is_lower = (below & 1) == 0;
        lower[lidx[i]] = is_lower ? 1u : 0u;
        partner[lidx[i]] = is_lower ? up : -1;
    }
}
__global__ void k_band_emit(const int32_t *__restrict__ row, const int32_t *__restrict__ col, const double *__restrict__ val,
                            long nnz, const uint32_t *__restrict__ lower, const uint32_t *__restrict__ dpos,
                            const int32_t *__restrict__ partner, int32_t *__restrict__ bcol, double *__restrict__ bv0,
                            double *__restrict__ bv1, int32_t *__restrict__ rb1) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nnz || !lower[u]) return;
    const uint32_t d = dpos[u];
    const int32_t p = partner[u];
    bcol[d] = (int32_t)((uint32_t)col[u] | 0x40000000u | (p >= 0 ? 0x80000000u : 0u));
    bv0[d] = val[u];
    bv1[d] = p >= 0 ? val[p] : 0.0;
    if (p >= 0) rb1[row[p]] = row[u];          // every lower entry of this row names the same partner row
}
__global__ void k_band_ptr(const int32_t *__restrict__ rowptr, int nrow, long nnz, const uint32_t *__restrict__ dpos,
                           const uint32_t *__restrict__ d_total, int32_t *__restrict__ bptr) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > nrow) return;
    const int k = rowptr[r];
    bptr[r] = k < nnz ? (int32_t)dpos[k] : (int32_t)*d_total;
}
// (the arguments: applystruct.h)
Bands build_bands(const ibh_weighted *w, HcIndexing hc, const int64_t *row_s, const int32_t *row, const uint32_t *colptr,
                  const int32_t *lrow, const uint32_t *lidx, uint32_t *d_total, hipStream_t st) {
    Arena &A = arena();
    const int T = 256;
    const int nrow = w->nrow, ncol = w->ncol;
    const long nnz = w->nnz;
    uint32_t *lower = A.get<uint32_t>((size_t)nnz), *dpos = A.get<uint32_t>((size_t)nnz);
    int32_t *partner = A.get<int32_t>((size_t)nnz);
    hipLaunchKernelGGL(k_band_roles, dim3(ceil_div(ncol, T)), dim3(T), 0, st, hc, row_s, colptr, ncol, lrow, lidx, lower, partner);
    exclusive_scan_u32(lower, dpos, (size_t)nnz, d_total, st);
    Bands b;
    b.nrow = nrow;
    b.ptr.alloc((size_t)nrow + 1); b.rb1.alloc((size_t)nrow);
    b.col.alloc((size_t)nnz); b.v0.alloc((size_t)nnz); b.v1.alloc((size_t)nnz);       // upper bound; >= nnz/2 are used
    IBH_HIP(hipMemsetAsync(b.rb1.p, 0xFF, sizeof(int32_t) * (size_t)nrow, st));
    hipLaunchKernelGGL(k_band_emit, dim3(ceil_div(nnz, T)), dim3(T), 0, st, row, w->colind.p, w->val.p, nnz, lower, dpos, partner,
                       b.col.p, b.v0.p, b.v1.p, b.rb1.p);
    hipLaunchKernelGGL(k_band_ptr, dim3(ceil_div(nrow + 1, T)), dim3(T), 0, st, w->rowptr.p, nrow, nnz, dpos, d_total, b.ptr.p);
    IBH_HIP(hipGetLastError());
    return b;
}

// The same structure for a matrix that already exists (either assembly path; spmm.hip calls this when an E-row matrix is
// applied again and again): per-column slots from the CSR, then build_bands.  One synchronisation (the band count).
// (csrops.h's expand_rows gives a thread a row: for the short rows of the GCM-grid matrices)
__global__ void k_expand_long_rows(const int32_t *__restrict__ rowptr, int nrow, int32_t *__restrict__ row) {
    const int r = blockIdx.x;                         // one workgroup per row: rows of E matrices hold 10^1..10^4 entries
    for (int k = rowptr[r] + threadIdx.x; k < rowptr[r + 1]; k += blockDim.x) row[k] = r;
}
Bands build_bands_from_csr(const ibh_weighted *w, hipStream_t st) {
    if (!w->band_eligible || w->nnz == 0 || w->nrow == 0 || w->ncol >= (1 << 28)) return {};
    const ibh_sparse_set *rset = w->dims[0];
    if (!rset || !rset->on_device(w->nrow)) return {};                    // the row keys must be on the device
    Arena &A = arena();
    A.reset();
    const int T = 256, nrow = w->nrow, ncol = w->ncol;
    const long nnz = w->nnz;
    int32_t *row = A.get<int32_t>((size_t)nnz);
    hipLaunchKernelGGL(k_expand_long_rows, dim3(nrow), dim3(T), 0, st, w->rowptr.p, nrow, row);
    const ColSlots s = col_slots(w->colind.p, row, nnz, ncol, st);
    uint32_t *d_nb = A.get<uint32_t>(1);
    Bands b = build_bands(w, HcIndexing{w->band_sA, w->band_sHC}, rset->device_to_sparse(nrow, st), row, s.colptr, s.lrow, s.lidx, d_nb, st);
    uint32_t nb = 0;
    readback_sync(&nb, d_nb, sizeof(uint32_t), st);
    b.n = nb;
    return b;
}

// ---- the keyed entry streams of the sweep and the row groups ---------------------------------------------------------------
// Both order the entries of the CSR by a key that ends in the column, and cut the sorted keys into runs.
// the stream, one workgroup per row: keys[k] = column of entry k, below (grp_of_row[r] << 32) where a group table is given (null: no
// high word); idx[k] = k; erow[k] = the entry's row
__global__ void k_expand_keyed_rows(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colind, int nrow, const int32_t *__restrict__ grp_of_row,
                                    uint64_t *__restrict__ keys, uint32_t *__restrict__ idx, int32_t *__restrict__ erow) {
    const int r = blockIdx.x;
    const uint64_t g = grp_of_row ? (uint64_t)(uint32_t)grp_of_row[r] << 32 : 0;
    for (int k = rowptr[r] + threadIdx.x; k < rowptr[r + 1]; k += blockDim.x) { keys[k] = g | (uint32_t)colind[k]; idx[k] = (uint32_t)k; erow[k] = r; }
}
// h[i] = sorted key i opens a run of equal keys.  d_bad (may be null): set when a run holds three keys or more
__global__ void k_key_heads(const uint64_t *__restrict__ keys, long n, uint32_t *__restrict__ h, uint32_t *__restrict__ d_bad) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    h[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
    if (d_bad && i >= 2 && keys[i] == keys[i - 1] && keys[i] == keys[i - 2]) *d_bad = 1u;
}

// ---- column-sweep structure (sweep_kernel.inl) of a matrix with short columns, from its CSR --------------------------
// ALL columns are swept once, in ascending order.  The entries are ordered by column (stable radix sort: a column's
// entries stay in row order) and paired up: one ITEM = a column + <= 2 of its entries (an ice cell of an E-row matrix has
// the two classes of its GCM cell: one item; a cell that straddles two GCM cells has four entries: two items).  64 items
// make a block, `tb` blocks a task.  A task keeps partial sums for the rows its columns touch: its local row table =
// the distinct rows of its entries in ascending order ("slots", <= SWEEP_MAX_SLOTS, else tb is halved), found by sorting
// the (task, row) pairs; the rows of the partial-sum array are exactly those distinct pairs.  The combine lists (which
// partial rows make up row r, in task order) come from one more sort by row.  Exact copies of M's values throughout.
// Host synchronisations for sizes; runs once per matrix, lazily (spmm.hip).
constexpr int SWEEP_MAX_SLOTS = 32;
// per sorted entry: is it the first of its column (-> colstart), then: does it open an item (even position in its column)
__global__ void k_sw_colstart(const uint64_t *__restrict__ keys, long n, int32_t *__restrict__ colstart) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (i == 0 || keys[i] != keys[i - 1]) colstart[(uint32_t)keys[i]] = (int32_t)i;
}
__global__ void k_sw_itemheads(const uint64_t *__restrict__ keys, long n, const int32_t *__restrict__ colstart, uint32_t *__restrict__ ih) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ih[i] = ((i - colstart[(uint32_t)keys[i]]) & 1) == 0 ? 1u : 0u;
}
// (task, row) of every sorted entry; payload = the entry's sorted position
__global__ void k_sw_taskrow(const uint32_t *__restrict__ ih, const uint32_t *__restrict__ iscan, const uint32_t *__restrict__ idx, long n,
                             const int32_t *__restrict__ erow, int items_per_task, uint64_t *__restrict__ tk, uint32_t *__restrict__ tv) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t item = iscan[i] + ih[i] - 1;
    tk[i] = ((uint64_t)(item / (uint32_t)items_per_task) << 32) | (uint32_t)erow[idx[i]];
    tv[i] = (uint32_t)i;
}
// task_p0[t] = index of the task's first distinct (task, row) pair; uniq_row / uniq list for the combine
__global__ void k_sw_taskfirst(const uint64_t *__restrict__ tk, const uint32_t *__restrict__ u, const uint32_t *__restrict__ uscan, long n,
                               int32_t *__restrict__ task_p0, int32_t *__restrict__ urow) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n || !u[k]) return;
    const uint32_t t = (uint32_t)(tk[k] >> 32);
    urow[uscan[k]] = (int32_t)(uint32_t)tk[k];
    if (k == 0 || (uint32_t)(tk[k - 1] >> 32) != t) task_p0[t] = (int32_t)uscan[k];
}
__global__ void k_sw_slots(const uint64_t *__restrict__ tk, const uint32_t *__restrict__ tv, const uint32_t *__restrict__ u,
                           const uint32_t *__restrict__ uscan, long n, const int32_t *__restrict__ task_p0, uint8_t *__restrict__ eslot) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t t = (uint32_t)(tk[k] >> 32);
    eslot[tv[k]] = (uint8_t)(uscan[k] + u[k] - 1 - (uint32_t)task_p0[t]);
}
__global__ void k_sw_task_ns(const int32_t *__restrict__ task_p0, int ntask, int nuniq, int32_t *__restrict__ task_ns,
                             uint32_t *__restrict__ d_maxns) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntask) return;
    const int ns = (t + 1 < ntask ? task_p0[t + 1] : nuniq) - task_p0[t];
    task_ns[t] = ns;
    atomicMax(d_maxns, (uint32_t)ns);
}
__global__ void k_sw_items(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ ih,
                           const uint32_t *__restrict__ iscan, long n, const uint8_t *__restrict__ eslot, const double *__restrict__ val,
                           int32_t *__restrict__ it_col, uint32_t *__restrict__ meta, double *__restrict__ v0, double *__restrict__ v1,
                           uint32_t *__restrict__ d_notident) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !ih[i]) return;
    const long it = (long)iscan[i];
    if ((long)(uint32_t)keys[i] != it) *d_notident = 1u;     // some column has no item, or more than one
    const uint32_t s0 = eslot[i];
    uint32_t m = s0 | (s0 << 8) | SWEEP_HAS0;
    double w1 = 0.0;
    if (i + 1 < n && keys[i + 1] == keys[i]) {      // the odd entry of the pair
        m = s0 | ((uint32_t)eslot[i + 1] << 8) | SWEEP_HAS0 | SWEEP_HAS1;
        w1 = val[idx[i + 1]];
    }
    it_col[it] = (int32_t)(uint32_t)keys[i]; meta[it] = m; v0[it] = val[idx[i]]; v1[it] = w1;
}
__global__ void k_sw_combkeys(const int32_t *__restrict__ urow, int nuniq, uint64_t *__restrict__ ck, uint32_t *__restrict__ cv) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nuniq) { ck[k] = (uint64_t)(uint32_t)urow[k]; cv[k] = (uint32_t)k; }
}
Sweep build_sweep_from_csr(const ibh_weighted *w, hipStream_t st) {
    if (w->nnz == 0 || w->nrow == 0 || w->nnz >= (1ll << 31) - 64) return {};
    Sweep s;
    Arena &A = arena();
    A.reset();
    const int T = 256, nrow = w->nrow, ncol = w->ncol;
    const long nnz = w->nnz;
    uint32_t *d_cnt = A.get<uint32_t>(8);
    IBH_HIP(hipMemsetAsync(d_cnt, 0, sizeof(uint32_t) * 8, st));
    // entries by column
    uint64_t *keys = A.get<uint64_t>((size_t)nnz), *keys2 = A.get<uint64_t>((size_t)nnz);
    uint32_t *idx = A.get<uint32_t>((size_t)nnz), *idx2 = A.get<uint32_t>((size_t)nnz);
    int32_t *erow = A.get<int32_t>((size_t)nnz);
    hipLaunchKernelGGL(k_expand_keyed_rows, dim3(nrow), dim3(T), 0, st, w->rowptr.p, w->colind.p, nrow, (const int32_t *)nullptr, keys, idx, erow);
    KeyField kf{0, bits_for((uint64_t)ncol)};
    if (kf.nbits > 0) radix_sort_pairs_front(keys, keys2, idx, idx2, (size_t)nnz, &kf, 1, st);
    // items: the entries of a column in pairs
    int32_t *colstart = A.get<int32_t>((size_t)ncol);
    uint32_t *ih = A.get<uint32_t>((size_t)nnz), *iscan = A.get<uint32_t>((size_t)nnz);
    hipLaunchKernelGGL(k_sw_colstart, dim3(ceil_div(nnz, T)), dim3(T), 0, st, keys, nnz, colstart);
    hipLaunchKernelGGL(k_sw_itemheads, dim3(ceil_div(nnz, T)), dim3(T), 0, st, keys, nnz, colstart, ih);
    exclusive_scan_u32(ih, iscan, (size_t)nnz, d_cnt + 0, st);
    uint32_t h[8];
    readback_sync(h, d_cnt, sizeof(h), st);
    const long nitems = (long)h[0];
    const int nblk = (int)((nitems + 63) / 64);
    if (nitems <= 0 || (long)nblk * 64 >= (1ll << 31)) return {};
    // tasks and their local row tables; tb halves until every task touches <= SWEEP_MAX_SLOTS rows
    int tb = get_tuning("sweep_tb", 0);
    if (tb <= 0) {                                  // the largest power of two <= 16 that leaves >= 1024 tasks (two per CU and round: measured at
        tb = 16;                                    // 1 km, 64 fields: tb 2 / 4 / 6 / 8 -> 276 / 234 / 230 / 214 us; beyond 8 the row tables outgrow the LDS)
        while (tb > 1 && nblk / tb < 1024) tb /= 2;
    }
    uint64_t *tk = A.get<uint64_t>((size_t)nnz), *tk2 = A.get<uint64_t>((size_t)nnz);
    uint32_t *tv = A.get<uint32_t>((size_t)nnz), *tv2 = A.get<uint32_t>((size_t)nnz);
    uint32_t *u = A.get<uint32_t>((size_t)nnz), *uscan = A.get<uint32_t>((size_t)nnz);
    int32_t *urow = A.get<int32_t>((size_t)nnz);
    uint8_t *eslot = A.get<uint8_t>((size_t)nnz);
    int ntask = 0, nuniq = 0, maxns = 0;
    for (;; tb /= 2) {
        if (tb < 1) return {};                   // 64 items touch more rows than the kernel's table holds
        ntask = ceil_div(nblk, tb);
        uint64_t *a = tk, *b2 = tk2;
        uint32_t *av = tv, *bv = tv2;
        hipLaunchKernelGGL(k_sw_taskrow, dim3(ceil_div(nnz, T)), dim3(T), 0, st, ih, iscan, idx, nnz, erow, 64 * tb, a, av);
        KeyField tf[2] = {{0, bits_for((uint64_t)nrow)}, {32, bits_for((uint64_t)ntask)}};
        radix_sort_pairs_front(a, b2, av, bv, (size_t)nnz, tf, 2, st);
        hipLaunchKernelGGL(k_key_heads, dim3(ceil_div(nnz, T)), dim3(T), 0, st, a, nnz, u, (uint32_t *)nullptr);
        exclusive_scan_u32(u, uscan, (size_t)nnz, d_cnt + 1, st);
        s.task_p0.alloc((size_t)ntask + 1); s.task_ns.alloc((size_t)ntask + 1);
        hipLaunchKernelGGL(k_sw_taskfirst, dim3(ceil_div(nnz, T)), dim3(T), 0, st, a, u, uscan, nnz, s.task_p0.p, urow);
        readback_sync(h, d_cnt, sizeof(h), st);
        nuniq = (int)h[1];
        IBH_HIP(hipMemsetAsync(d_cnt + 2, 0, sizeof(uint32_t), st));
        hipLaunchKernelGGL(k_sw_task_ns, dim3(ceil_div(ntask, T)), dim3(T), 0, st, s.task_p0.p, ntask, nuniq, s.task_ns.p, d_cnt + 2);
        readback_sync(h, d_cnt, sizeof(h), st);
        maxns = (int)h[2];
        // LDS per workgroup = tile (33 KB) + 4 waves x maxns x 512 B: <= 22 slots keep two workgroups on a CU, <= 9 three
        const int soft = get_tuning("sweep_soft_slots", 22);
        if (getenv("IBH_SWEEP_DEBUG")) fprintf(stderr, "sweep: nitems %ld nblk %d tb %d ntask %d nuniq %d maxns %d\n", nitems, nblk, tb, ntask, nuniq, maxns);
        if (maxns <= SWEEP_MAX_SLOTS && (maxns <= soft || tb == 1)) {
            hipLaunchKernelGGL(k_sw_slots, dim3(ceil_div(nnz, T)), dim3(T), 0, st, a, av, u, uscan, nnz, s.task_p0.p, eslot);
            break;
        }
    }
    // items
    s.col.alloc((size_t)nblk * 64);
    s.meta.alloc((size_t)nblk * 64); s.v0.alloc((size_t)nblk * 64); s.v1.alloc((size_t)nblk * 64);
    IBH_HIP(hipMemsetAsync(s.col.p, 0, sizeof(int32_t) * (size_t)nblk * 64, st));
    IBH_HIP(hipMemsetAsync(s.meta.p, 0, sizeof(uint32_t) * (size_t)nblk * 64, st));
    IBH_HIP(hipMemsetAsync(s.v0.p, 0, sizeof(double) * (size_t)nblk * 64, st));
    IBH_HIP(hipMemsetAsync(s.v1.p, 0, sizeof(double) * (size_t)nblk * 64, st));
    hipLaunchKernelGGL(k_sw_items, dim3(ceil_div(nnz, T)), dim3(T), 0, st, keys, idx, ih, iscan, nnz, eslot, w->val.p, s.col.p,
                       s.meta.p, s.v0.p, s.v1.p, d_cnt + 5);
    // combine lists: the distinct (task, row) pairs by row, tasks ascending inside a row
    uint64_t *ck = A.get<uint64_t>((size_t)nuniq), *ck2 = A.get<uint64_t>((size_t)nuniq);
    uint32_t *cv = A.get<uint32_t>((size_t)nuniq), *cv2 = A.get<uint32_t>((size_t)nuniq);
    hipLaunchKernelGGL(k_sw_combkeys, dim3(ceil_div(nuniq, T)), dim3(T), 0, st, urow, nuniq, ck, cv);
    KeyField cf{0, bits_for((uint64_t)nrow)};
    if (cf.nbits > 0) radix_sort_pairs_front(ck, ck2, cv, cv2, (size_t)nuniq, &cf, 1, st);
    int32_t *srow = A.get<int32_t>((size_t)nuniq);
    keys_to_i32(ck, (long)nuniq, srow, st);
    s.comb_ptr.alloc((size_t)nrow + 1); s.comb_p.alloc((size_t)nuniq);
    rowptr_from_rows(srow, (long)nuniq, nrow, s.comb_ptr.p, st);
    IBH_HIP(hipMemcpyAsync(s.comb_p.p, cv, sizeof(uint32_t) * (size_t)nuniq, hipMemcpyDeviceToDevice, st));
    IBH_HIP(hipGetLastError());
    readback_sync(h, d_cnt, sizeof(h), st);         // (the arena is reused by the next build)
    s.ident = (h[5] == 0 && nitems == (long)ncol) ? 1 : 0;
    if (s.ident) s.col.release();     // column = item index: the list is never read
    s.tb = tb; s.nitems = (int32_t)nitems;
    s.nprow = nuniq;
    s.nblk = nblk;
    s.nslot = maxns < 1 ? 1 : maxns;
    s.ntask = ntask;
    return s;
}

// ---- row-group structure (spmm.hip rowgroup) of an E-row matrix, from its CSR -------------------------------------------
// A group = the rows whose keys decode to the same GCM cell (its elevation classes), in ascending row order: slot s of
// group g.  The group's entries are ordered by column and paired per column into items (an ice cell lies between two classes
// of a GCM cell: one item with both weights).  Exact copies of M's values.  Declined (an unbuilt value) when a group has
// more than IBH_GSLOTS rows or a column more than two entries in one group.  Host synchronisations for sizes; runs once per
// matrix (ibh_weighted_prepare, or lazily from a later apply).
constexpr uint32_t GRP_HAS0 = 1u << 16, GRP_HAS1 = 1u << 17;
__global__ void k_rg_rowkeys(HcIndexing hc, const int64_t *__restrict__ row_s, int nrow, uint64_t *__restrict__ keys, uint32_t *__restrict__ idx) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrow) return;
    long a, c;
    hc.split<true>(row_s[r], a, c);
    keys[r] = (uint64_t)a; idx[r] = (uint32_t)r;
}
// sorted rows -> (group, slot): gstart[g] = position of the group's first row
__global__ void k_rg_gstart(const uint32_t *__restrict__ h, const uint32_t *__restrict__ hscan, int nrow, int32_t *__restrict__ gstart) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nrow && h[i]) gstart[hscan[i]] = i;
}
__global__ void k_rg_slots(const uint32_t *__restrict__ h, const uint32_t *__restrict__ hscan, const uint32_t *__restrict__ srow, int nrow,
                           int ngrp, const int32_t *__restrict__ gstart, int32_t *__restrict__ grp_of_row, int32_t *__restrict__ slot_of_row,
                           int32_t *__restrict__ slotrow, int32_t *__restrict__ grp_ns, uint32_t *__restrict__ d_maxns) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrow) return;
    const int g = (int)(hscan[i] + h[i]) - 1, s = i - gstart[g];
    const int r = (int)srow[i];
    grp_of_row[r] = g; slot_of_row[r] = s;
    if (s < IBH_GSLOTS) slotrow[g * IBH_GSLOTS + s] = r;
    if (i + 1 == nrow || h[i + 1]) { grp_ns[g] = s + 1; atomicMax(d_maxns, (uint32_t)(s + 1)); }
}
__global__ void k_rg_items(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ h,
                           const uint32_t *__restrict__ hscan, long n, const int32_t *__restrict__ erow, const int32_t *__restrict__ slot_of_row,
                           const double *__restrict__ val, int32_t *__restrict__ it_col, uint32_t *__restrict__ meta, double *__restrict__ v0,
                           double *__restrict__ v1, int32_t *__restrict__ it_grp) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !h[i]) return;
    const long it = (long)hscan[i];
    const uint32_t s0 = (uint32_t)slot_of_row[erow[idx[i]]];
    uint32_t m = s0 | GRP_HAS0;
    double w1 = 0.0;
    if (i + 1 < n && keys[i + 1] == keys[i]) {
        m |= ((uint32_t)slot_of_row[erow[idx[i + 1]]] << 8) | GRP_HAS1;
        w1 = val[idx[i + 1]];
    }
    it_col[it] = (int32_t)(uint32_t)keys[i]; meta[it] = m; v0[it] = val[idx[i]]; v1[it] = w1;
    it_grp[it] = (int32_t)(keys[i] >> 32);
}
// ---- tiles of the row groups (spmm.hip grouptile) ------------------------------------------------------------
// One workgroup per tile of SEG items: the columns (padded by repeating the last), and the entries of the tile sorted by
// (slot, item) -- ascending item = ascending column = the order of the CSR row -- with their offsets per slot.  Every slot's
// list is padded to a multiple of four entries with {item SEG, weight 0}: the kernel keeps a zero in that place of its
// X tile, so a padded entry adds 0 * 0 and the inner loop needs no predicate (a padded weight never meets a field value: 0 * NaN).
template <int SEG>
__global__ __launch_bounds__(SEG) void k_gt_build(const int32_t *__restrict__ tile_grp, const int32_t *__restrict__ tile_i0,
                                                          const int32_t *__restrict__ grp_ptr, const int32_t *__restrict__ it_col,
                                                          const uint32_t *__restrict__ it_meta, const double *__restrict__ it_v0,
                                                          const double *__restrict__ it_v1, int32_t *__restrict__ gt_col,
                                                          uint16_t *__restrict__ gt_ek, double *__restrict__ gt_ev, uint16_t *__restrict__ gt_eptr) {
    constexpr int NWV = SEG / 64;
    __shared__ uint16_t wc[NWV][IBH_GSLOTS];
    __shared__ uint16_t base[NWV][IBH_GSLOTS];
    __shared__ uint16_t s_end[IBH_GSLOTS], s_pend[IBH_GSLOTS];
    const long t = blockIdx.x;
    const int g = tile_grp[t], i0 = tile_i0[t];
    const int n = min(SEG, grp_ptr[g + 1] - i0);
    const int k = threadIdx.x, lane = k & 63, wv = k >> 6;
    const bool has = k < n;
    const long it = (long)i0 + (has ? k : n - 1);
    gt_col[t * SEG + k] = it_col[it];
    const uint32_t m = has ? it_meta[it] : 0u;
    const bool h0 = (m & GRP_HAS0) != 0, h1 = (m & GRP_HAS1) != 0;
    const int s0 = (int)(m & 0xffu), s1 = (int)((m >> 8) & 0xffu);
    int r0 = 0, r1 = 0;
    const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (int s = 0; s < IBH_GSLOTS; ++s) {
        const bool a = h0 && s0 == s, b = h1 && s1 == s;
        const unsigned long long mk = __ballot(a || b);       // (the two entries of an item sit in different rows)
        if (lane == 0) wc[wv][s] = (uint16_t)__popcll(mk);
        const int r = __popcll(mk & lt);
        if (a) r0 = r;
        if (b) r1 = r;
    }
    __syncthreads();
    const long e0 = t * ibh_gt_ecap(SEG);
    if (k == 0) {
        int off = 0;
        for (int s = 0; s < IBH_GSLOTS; ++s) {
            gt_eptr[t * IBH_GT_EP + s] = (uint16_t)off;
            for (int q = 0; q < NWV; ++q) { base[q][s] = (uint16_t)off; off += wc[q][s]; }
            s_end[s] = (uint16_t)off;
            off = (off + 3) & ~3;
            s_pend[s] = (uint16_t)off;
        }
        gt_eptr[t * IBH_GT_EP + IBH_GSLOTS] = (uint16_t)off;
        gt_eptr[t * IBH_GT_EP + IBH_GSLOTS + 1] = 0;
    }
    __syncthreads();
    if (h0) { const long e = e0 + base[wv][s0] + r0; gt_ek[e] = (uint16_t)(k * 8); gt_ev[e] = it_v0[it]; }
    if (h1) { const long e = e0 + base[wv][s1] + r1; gt_ek[e] = (uint16_t)(k * 8); gt_ev[e] = it_v1[it]; }
    if (k < IBH_GSLOTS)
        for (int e = s_end[k]; e < s_pend[k]; ++e) { gt_ek[e0 + e] = (uint16_t)(SEG * 8); gt_ev[e0 + e] = 0.0; }
}
static RowGroups::Tiles build_group_tiles(const int32_t *d_grp_ptr, int ngrp, const int32_t *it_col, const uint32_t *it_meta,
                                          const double *it_v0, const double *it_v1, long nitems, hipStream_t st) {
    // Tiles of 256 items walked by eight waves, or of 128 by four: many small groups (the Antarctic sheet under a half-degree grid:
    // ~600 items per GCM cell, tens of thousands of cells) leave less of a small tile empty and keep more workgroups on a CU --
    // measured, 128 fields: 3.62 against 3.76 ms; few or large groups (1 km Greenland: 3 400 items per cell) take the large one
    // (218 against 235 us at 64 fields).
    int seg = get_tuning("grouptile_seg", (ngrp >= 2048 && nitems < 1024l * ngrp) ? 128 : 256);
    if (seg != 128) seg = 256;
    const int ecap = ibh_gt_ecap(seg);
    std::vector<int32_t> gp((size_t)ngrp + 1), tp((size_t)ngrp + 1);
    IBH_HIP(hipMemcpyAsync(gp.data(), d_grp_ptr, sizeof(int32_t) * gp.size(), hipMemcpyDeviceToHost, st));
    IBH_HIP(hipStreamSynchronize(st));
    long nt = 0;
    for (int g = 0; g < ngrp; ++g) { tp[(size_t)g] = (int32_t)nt; nt += ((long)gp[(size_t)g + 1] - gp[(size_t)g] + seg - 1) / seg; }
    tp[(size_t)ngrp] = (int32_t)nt;
    if (nt <= 0 || nt * ecap >= (1l << 31)) return {};
    std::vector<int32_t> tg((size_t)nt), ti((size_t)nt);
    for (int g = 0; g < ngrp; ++g)
        for (int t = tp[(size_t)g], i = gp[(size_t)g]; t < tp[(size_t)g + 1]; ++t, i += seg) { tg[(size_t)t] = g; ti[(size_t)t] = i; }
    RowGroups::Tiles t;
    DevBuf<int32_t> d_tg((size_t)nt), d_ti((size_t)nt);
    t.ptr.alloc((size_t)ngrp + 1); t.col.alloc((size_t)nt * seg);
    t.ek.alloc((size_t)nt * ecap); t.eptr.alloc((size_t)nt * IBH_GT_EP); t.ev.alloc((size_t)nt * ecap);
    d_tg.upload(tg.data(), tg.size(), st); d_ti.upload(ti.data(), ti.size(), st); t.ptr.upload(tp.data(), tp.size(), st);
    t.ek.zero(st); t.ev.zero(st);
    if (seg == 128)
        hipLaunchKernelGGL(k_gt_build<128>, dim3((unsigned)nt), dim3(128), 0, st, d_tg.p, d_ti.p, d_grp_ptr, it_col, it_meta, it_v0, it_v1, t.col.p,
                           t.ek.p, t.ev.p, t.eptr.p);
    else
        hipLaunchKernelGGL(k_gt_build<256>, dim3((unsigned)nt), dim3(256), 0, st, d_tg.p, d_ti.p, d_grp_ptr, it_col, it_meta, it_v0, it_v1, t.col.p,
                           t.ek.p, t.ev.p, t.eptr.p);
    IBH_HIP(hipGetLastError());
    IBH_HIP(hipStreamSynchronize(st));              // (the host vectors and the tile maps die here)
    t.seg = seg;
    t.ntile = (int32_t)nt;
    return t;
}
RowGroups build_groups_from_csr(const ibh_weighted *w, hipStream_t st) {
    if (!w->band_eligible || w->nnz == 0 || w->nrow == 0 || w->nnz >= (1ll << 31) - 64) return {};
    if (!w->dims[0]) return {};
    Arena &A = arena();
    A.reset();
    const int T = 256, nrow = w->nrow;
    const long nnz = w->nnz;
    const int64_t *row_s = w->dims[0]->device_to_sparse(nrow, st);     // the row keys (a caller-supplied set may live on the host only)
    uint32_t *d_cnt = A.get<uint32_t>(8);
    IBH_HIP(hipMemsetAsync(d_cnt, 0, sizeof(uint32_t) * 8, st));
    // rows by GCM cell (stable: ascending row inside a group)
    uint64_t *rk = A.get<uint64_t>((size_t)nrow), *rk2 = A.get<uint64_t>((size_t)nrow);
    uint32_t *ri = A.get<uint32_t>((size_t)nrow), *ri2 = A.get<uint32_t>((size_t)nrow);
    hipLaunchKernelGGL(k_rg_rowkeys, dim3(ceil_div(nrow, T)), dim3(T), 0, st, HcIndexing{w->band_sA, w->band_sHC}, row_s, nrow, rk, ri);
    KeyField rf{0, 32};
    radix_sort_pairs_front(rk, rk2, ri, ri2, (size_t)nrow, &rf, 1, st);
    uint32_t *rh = A.get<uint32_t>((size_t)nrow), *rhs = A.get<uint32_t>((size_t)nrow);
    hipLaunchKernelGGL(k_key_heads, dim3(ceil_div(nrow, T)), dim3(T), 0, st, rk, (long)nrow, rh, (uint32_t *)nullptr);
    exclusive_scan_u32(rh, rhs, (size_t)nrow, d_cnt + 0, st);
    uint32_t h[8];
    readback_sync(h, d_cnt, sizeof(h), st);
    const int ngrp = (int)h[0];
    if (ngrp <= 0) return {};
    int32_t *gstart = A.get<int32_t>((size_t)ngrp);
    int32_t *grp_of_row = A.get<int32_t>((size_t)nrow), *slot_of_row = A.get<int32_t>((size_t)nrow);
    RowGroups g;
    g.slotrow.alloc((size_t)ngrp * IBH_GSLOTS); g.ns.alloc((size_t)ngrp); g.ptr.alloc((size_t)ngrp + 1);
    IBH_HIP(hipMemsetAsync(g.slotrow.p, 0, sizeof(int32_t) * (size_t)ngrp * IBH_GSLOTS, st));
    hipLaunchKernelGGL(k_rg_gstart, dim3(ceil_div(nrow, T)), dim3(T), 0, st, rh, rhs, nrow, gstart);
    hipLaunchKernelGGL(k_rg_slots, dim3(ceil_div(nrow, T)), dim3(T), 0, st, rh, rhs, ri, nrow, ngrp, gstart, grp_of_row, slot_of_row, g.slotrow.p,
                       g.ns.p, d_cnt + 1);
    // entries by (group, column): stable, so the two entries of a column keep their row (= slot) order; a run of equal keys is one
    // item (two entries at most: else d_cnt[3])
    uint64_t *keys = A.get<uint64_t>((size_t)nnz), *keys2 = A.get<uint64_t>((size_t)nnz);
    uint32_t *idx = A.get<uint32_t>((size_t)nnz), *idx2 = A.get<uint32_t>((size_t)nnz);
    int32_t *erow = A.get<int32_t>((size_t)nnz);
    hipLaunchKernelGGL(k_expand_keyed_rows, dim3(nrow), dim3(T), 0, st, w->rowptr.p, w->colind.p, nrow, grp_of_row, keys, idx, erow);
    KeyField ef[2] = {{0, bits_for((uint64_t)w->ncol)}, {32, bits_for((uint64_t)ngrp)}};
    radix_sort_pairs_front(keys, keys2, idx, idx2, (size_t)nnz, ef, 2, st);
    uint32_t *ih = A.get<uint32_t>((size_t)nnz), *ihs = A.get<uint32_t>((size_t)nnz);
    hipLaunchKernelGGL(k_key_heads, dim3(ceil_div(nnz, T)), dim3(T), 0, st, keys, nnz, ih, d_cnt + 3);
    exclusive_scan_u32(ih, ihs, (size_t)nnz, d_cnt + 2, st);
    readback_sync(h, d_cnt, sizeof(h), st);
    const int maxns = (int)h[1];
    const long nitems = (long)h[2];
    if (getenv("IBH_SWEEP_DEBUG")) fprintf(stderr, "groups: nrow %d ngrp %d maxns %d nitems %ld bad %u\n", nrow, ngrp, maxns, nitems, h[3]);
    if (maxns > IBH_GSLOTS || h[3] != 0 || nitems <= 0) return {};
    g.col.alloc((size_t)nitems); g.meta.alloc((size_t)nitems); g.v0.alloc((size_t)nitems); g.v1.alloc((size_t)nitems);
    int32_t *it_grp = A.get<int32_t>((size_t)nitems);
    hipLaunchKernelGGL(k_rg_items, dim3(ceil_div(nnz, T)), dim3(T), 0, st, keys, idx, ih, ihs, nnz, erow, slot_of_row, w->val.p, g.col.p, g.meta.p,
                       g.v0.p, g.v1.p, it_grp);
    rowptr_from_rows(it_grp, nitems, ngrp, g.ptr.p, st);
    IBH_HIP(hipGetLastError());
    IBH_HIP(hipStreamSynchronize(st));              // (the arena is reused by the next build)
    g.nslot = maxns; g.nitems = (int32_t)nitems;
    g.n = ngrp;
    g.tiles = build_group_tiles(g.ptr.p, ngrp, g.col.p, g.meta.p, g.v0.p, g.v1.p, nitems, st);
    return g;
}

}  // namespace ibh
