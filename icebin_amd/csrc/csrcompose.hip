// csrcompose.hip -- crop_cols(L) * R as one row-local operation (csrops.h: compose_cols), for an R whose rows hold at most one entry
// each: the I-row matrices of to_modele over smoothed rows of tens of entries.  Arithmetic as in csrops.hip: every product is
// rounded where it is written (-ffp-contract=off), the sums run in ascending k.
#include <vector>

#include "csrops.h"
#include "prims.h"

namespace ibh {
namespace {
constexpr int CC_THREADS = 256, CC_ROWS = CC_THREADS / COMPOSE_LANES;

// COMPOSE_LANES lanes per row of L, CC_ROWS rows per workgroup.  A row's kept entries go to LDS as (key = c << 32 | k, t) in any
// order; the keys are distinct (the map is one-to-one), so counting the smaller keys gives each entry its place in (c, k) order;
// the lane that finds the head of a run of equal c walks the run, which keeps the sum sequential.  FILL = false counts the heads
// (cnt[i]) and looks for what the form cannot serve: declined[0] a row of R with two entries, declined[1] a row with more than
// COMPOSE_ROWCAP kept entries.  Every thread reaches every barrier: a row past the end, or too long, has m = 0 entries.
template <bool FILL>
__global__ void __launch_bounds__(CC_THREADS)
k_compose_rowlocal(Csr L, const int32_t *__restrict__ map, const double *__restrict__ rs, const double *__restrict__ cs, Csr R,
                   uint32_t *__restrict__ cnt, uint32_t *__restrict__ declined, const int32_t *__restrict__ outptr,
                   int32_t *__restrict__ col, double *__restrict__ val) {
    __shared__ unsigned long long s_key[CC_ROWS][COMPOSE_ROWCAP];
    __shared__ double s_t[CC_ROWS][COMPOSE_ROWCAP], s_sum[CC_ROWS][COMPOSE_ROWCAP];
    __shared__ int32_t s_col[CC_ROWS][COMPOSE_ROWCAP];
    __shared__ int s_n[CC_ROWS];
    const int g = threadIdx.x / COMPOSE_LANES, lane = threadIdx.x % COMPOSE_LANES;
    const long i = (long)blockIdx.x * CC_ROWS + g;
    const bool live = i < L.nrow;
    if (!FILL) {
        bool two = false;
        for (long k = (long)blockIdx.x * CC_THREADS + threadIdx.x; k < R.nrow; k += (long)gridDim.x * CC_THREADS)
            two = two || R.rowptr[k + 1] - R.rowptr[k] > 1;
        if (two) declined[0] = 1u;
    }
    if (lane == 0) s_n[g] = 0;
    __syncthreads();
    const int b = live ? L.rowptr[i] : 0, end = live ? L.rowptr[i + 1] : 0;
    for (int e = b + lane; e < end; e += COMPOSE_LANES) {
        const int k = map[L.colind[e]];
        if (k < 0) continue;
        const int rb = R.rowptr[k];
        if (R.rowptr[k + 1] == rb) continue;
        const int slot = atomicAdd(&s_n[g], 1);
        if (slot >= COMPOSE_ROWCAP) continue;
        double v = L.val[e];
        if (rs) v = rs[i] * v;
        if (cs) v = v * cs[k];
        s_key[g][slot] = ((unsigned long long)(uint32_t)R.colind[rb] << 32) | (uint32_t)k;
        s_t[g][slot] = v * R.val[rb];
    }
    __syncthreads();
    const int n = s_n[g], m = n > COMPOSE_ROWCAP ? 0 : n;
    if (!FILL && n > COMPOSE_ROWCAP && lane == 0) declined[1] = 1u;
    for (int a = lane; a < m; a += COMPOSE_LANES) {
        const unsigned long long key = s_key[g][a];
        int rank = 0;
        for (int q = 0; q < m; ++q) rank += s_key[g][q] < key ? 1 : 0;
        s_col[g][rank] = (int32_t)(key >> 32);
        s_sum[g][rank] = s_t[g][a];
    }
    __syncthreads();
    uint32_t heads = 0;
    for (int j = lane; j < m; j += COMPOSE_LANES) {
        const int32_t c = s_col[g][j];
        if (j > 0 && s_col[g][j - 1] == c) continue;
        if (!FILL) { ++heads; continue; }
        int o = 0;                                  // the heads in front of this one
        for (int q = 1; q <= j; ++q) o += s_col[g][q] != s_col[g][q - 1] ? 1 : 0;
        double s = s_sum[g][j];
        for (int q = j + 1; q < m && s_col[g][q] == c; ++q) s = s + s_sum[g][q];
        col[outptr[i] + o] = c;
        val[outptr[i] + o] = s;
    }
    if (!FILL) {
        for (int off = COMPOSE_LANES / 2; off > 0; off >>= 1) heads += __shfl_xor(heads, off, COMPOSE_LANES);
        if (live && lane == 0) cnt[i] = heads;
    }
}

bool compose_rowlocal(const ibh_weighted &L, const int32_t *d_map, const double *d_rs, const double *d_cs, const ibh_weighted &R,
                      ibh_weighted *out, hipStream_t st) {
    Arena &A = arena();
    A.reset();
    const int n = L.nrow;
    uint32_t *cnt = A.get<uint32_t>((size_t)n), *declined = A.get<uint32_t>(2);
    IBH_HIP(hipMemsetAsync(declined, 0, 2 * sizeof(uint32_t), st));
    const dim3 grid(n ? ceil_div(n, CC_ROWS) : 1);
    hipLaunchKernelGGL(k_compose_rowlocal<false>, grid, dim3(CC_THREADS), 0, st, view(L), d_map, d_rs, d_cs, view(R), cnt, declined,
                       (const int32_t *)nullptr, (int32_t *)nullptr, (double *)nullptr);
    IBH_HIP(hipGetLastError());
    uint32_t h[2];
    readback_sync(h, declined, sizeof(h), st);
    if (h[0] || h[1]) return false;
    out->nrow = n; out->ncol = R.ncol;
    out->rowptr.alloc((size_t)n + 1);
    uint32_t *ptr = reinterpret_cast<uint32_t *>(out->rowptr.p);
    exclusive_scan_u32(cnt, ptr, (size_t)n, ptr + n, st);
    uint32_t nnz = 0;
    readback_sync(&nnz, ptr + n, sizeof(nnz), st);
    IBH_CHECK(nnz < (1u << 31), "nnz overflows int32");
    out->nnz = nnz;
    out->colind.alloc(nnz); out->val.alloc(nnz);
    if (nnz)
        hipLaunchKernelGGL(k_compose_rowlocal<true>, grid, dim3(CC_THREADS), 0, st, view(L), d_map, d_rs, d_cs, view(R), (uint32_t *)nullptr,
                           (uint32_t *)nullptr, out->rowptr.p, out->colind.p, out->val.p);
    IBH_HIP(hipGetLastError());
    return true;
}
}  // namespace

ComposeForm compose_cols(const ibh_weighted &L, const int32_t *d_map, const double *d_rs, const double *d_cs, const ibh_weighted &R,
                         bool rowlocal, ibh_weighted *out, hipStream_t st) {
    if (rowlocal && compose_rowlocal(L, d_map, d_rs, d_cs, R, out, st)) return COMPOSED_ROWLOCAL;
    ibh_weighted cropped;
    arena().reset();
    crop_cols(L, d_map, R.nrow, d_rs, d_cs, &cropped, st);
    csr_product(cropped, R, out, st);
    return COMPOSED_PRODUCT;
}

}  // namespace ibh

using namespace ibh;
extern "C" {

int ibh_selftest_compose_cols(const ibh_weighted *L, const int32_t *map, int64_t nmap, const double *rs, const double *cs,
                              const ibh_weighted *R, int form, ibh_weighted **out) {
    if (out) *out = nullptr;
    return guarded([&] {
        IBH_CHECK(L && R && out && (map || nmap == 0), "null argument");
        IBH_CHECK(form == COMPOSED_PRODUCT || form == COMPOSED_ROWLOCAL, "form %d is neither 1 (the product) nor 2 (row-local)", form);
        IBH_CHECK(nmap == L->ncol, "compose_cols: map has %lld entries, L %d columns", (long long)nmap, L->ncol);
        std::vector<char> hit((size_t)R->nrow, 0);
        for (int64_t p = 0; p < nmap; ++p) {
            IBH_CHECK(map[p] >= -1 && map[p] < R->nrow, "compose_cols: a target outside [-1, %d)", R->nrow);
            if (map[p] < 0) continue;
            IBH_CHECK(!hit[(size_t)map[p]], "compose_cols: the map is not one-to-one");
            hit[(size_t)map[p]] = 1;
        }
        require_device();
        check_current_device(L->device, "L");
        check_current_device(R->device, "R");
        hipStream_t st = hipStreamPerThread;
        // (the operands live outside the arena: compose_cols resets it)
        DevBuf<int32_t> d_map;
        DevBuf<double> d_rs, d_cs;
        d_map.alloc((size_t)nmap);
        if (nmap) d_map.upload(map, (size_t)nmap, st);
        if (rs) { d_rs.alloc((size_t)L->nrow); if (L->nrow) d_rs.upload(rs, (size_t)L->nrow, st); }
        if (cs) { d_cs.alloc((size_t)R->nrow); if (R->nrow) d_cs.upload(cs, (size_t)R->nrow, st); }
        auto w = new_weighted();
        w->composed_by = compose_cols(*L, d_map.p, rs ? d_rs.p : nullptr, cs ? d_cs.p : nullptr, *R, form == COMPOSED_ROWLOCAL, w.get(), st);
        w->wM.alloc((size_t)w->nrow); w->wM.zero(st);
        w->Mw.alloc((size_t)w->ncol); w->Mw.zero(st);
        IBH_HIP(hipStreamSynchronize(st));
        w->conservative = L->conservative; w->scaled = L->scaled;
        w->dims[0] = DimRef::owned_identity(w->nrow); w->dims[1] = DimRef::owned_identity(w->ncol);
        *out = w.release();
    });
}

}  // extern "C"
