// multivec.hip -- the coupler's exchange vectors on gfx950: icebin::VectorMultivec (slib/icebin/multivec.{hpp,cpp}) resident in
// HBM, with the loops that fill it from a regridded field (IceCoupler.cpp:447-458), merge the entries of all ice sheets into
// the GCM's arrays (multivec.cpp:35-81, modele/GCMCoupler_ModelE.cpp:864-892) and densify the GCM's vector onto dimE0
// (IceCoupler.cpp:294-314).
//
// Every sum over entries naming the same cell runs in ENTRY order, one product then one add (-ffp-contract=off), so each
// result is the reference loop's bit for bit: the entries are sorted stably by index (radix_sort_pairs, payload = entry
// position), the heads of the runs are ranked by a scan, and one lane walks each run front to back.  No floating-point
// atomics.  The grouping (permutation + run starts) is kept in the handle until the vector changes: to_dense_scale and the
// to_dense / update_dense after it share one sort.
#include "prims.h"
#include <memory>

struct ibh_multivec {
    int device = 0;
    int32_t nvar = 0;
    int64_t n = 0, cap = 0;                 // entries, entries the three buffers hold without growing
    ibh::DevBuf<int64_t> index;             // [cap]
    ibh::DevBuf<double> weights, vals;      // [cap], [cap * nvar] entry-major: vals[ix * nvar + ivar]
    // the entries grouped by index, made by the first merge call after a change (ensure_grouping)
    struct Grouping {
        bool valid = false;
        int64_t max_index = -1;             // the largest index (all are >= 0 once the grouping exists)
        ibh::DevBuf<uint32_t> perm;         // [n] entry positions sorted by (index, position)
        ibh::DevBuf<uint32_t> runstart;     // [n + 1] first sorted position of every run, then n; [nrun + 1] are used
        ibh::DevBuf<uint32_t> nrun;         // [1]
    };
    mutable Grouping grp;
};

namespace ibh {

// ---- append: field-major [nvar x nrow] -> entry-major [nrow x nvar] ----------------------------------------------------------
// A block takes AP_ROWS dense rows and walks the variables in chunks of AP_VC.  Reads: a wave reads 64 consecutive rows of one
// variable (512 contiguous bytes).  Writes: consecutive lanes take consecutive (row, variable) pairs, variable fastest, which
// are consecutive addresses of vals for nvar <= AP_VC and runs of 256 bytes beyond.  The tile between them is [AP_VC][AP_LD]
// with AP_LD odd: the column read of the write phase then falls on distinct banks wherever a 32-lane group spans 32 variables,
// and is at worst 2-way where it spans two rows of 16.
constexpr int AP_ROWS = 64, AP_VC = 32, AP_LD = AP_ROWS + 1, AP_THREADS = 256;
__global__ __launch_bounds__(AP_THREADS) void k_mv_append(const double *__restrict__ B, long ldb, int nrow, int nvar,
                                                         const int64_t *__restrict__ to_sparse, const double *__restrict__ wM,
                                                         int64_t *__restrict__ index, double *__restrict__ weights,
                                                         double *__restrict__ vals) {
    __shared__ double tile[AP_VC * AP_LD];
    const int t = threadIdx.x;
    const int row0 = blockIdx.x * AP_ROWS;
    const int nr = min(AP_ROWS, nrow - row0);
    if (t < nr) {
        index[row0 + t] = to_sparse ? to_sparse[row0 + t] : (int64_t)(row0 + t);
        weights[row0 + t] = wM[row0 + t];
    }
    const int lr = t & (AP_ROWS - 1), lv = t / AP_ROWS;
    for (int v0 = 0; v0 < nvar; v0 += AP_VC) {
        const int nc = min(AP_VC, nvar - v0);
        if (lr < nr)
            for (int v = lv; v < nc; v += AP_THREADS / AP_ROWS) tile[v * AP_LD + lr] = B[(long)(v0 + v) * ldb + row0 + lr];
        __syncthreads();
        for (int o = t; o < nr * nc; o += AP_THREADS) {
            const int r = o / nc, v = o - r * nc;
            vals[(long)(row0 + r) * nvar + v0 + v] = tile[v * AP_LD + r];
        }
        __syncthreads();
    }
}

// ---- append_planes: the masked, ordered pack of field planes (modele/GCMCoupler_ModelE.cpp:1099-1164) -------------------------
// A cell c is KEPT when mask[c] != 0 || mask0[c] != 0.  The kept cells are listed in ascending order ONCE per call -- list[rank]
// = cell -- and every pack of the call, and every class of a pack, reads that list: entry n0 + ihc * nkept + rank.
//
// The list is made by tiles of PK_TILE cells, PK_I passes of one cell per thread: a pass's kept flags are one ballot per wave,
// a cell's rank inside its tile is the kept cells of the (pass, wave) pairs before its own plus the set bits below its lane,
// and the kept cells of the tiles before come from k_mv_pack_count's per-tile counts -- summed by the tile's own block up to
// PK_SELF_TILES tiles (two launches; 2 M cells, every atmosphere grid there is), scanned by prims.h's scan beyond (three).  No
// atomics, and no block waits for another.
constexpr int PK_T = 256, PK_I = 8, PK_TILE = PK_T * PK_I, PK_SELF_TILES = 1024;
__device__ __forceinline__ bool pk_kept(const int16_t *__restrict__ mask, const int16_t *__restrict__ mask0, long c, long ncell) {
    return c < ncell && (mask[c] != 0 || (mask0 && mask0[c] != 0));
}
__global__ __launch_bounds__(PK_T) void k_mv_pack_count(const int16_t *__restrict__ mask, const int16_t *__restrict__ mask0, long ncell,
                                                       uint32_t *__restrict__ cnt) {
    __shared__ uint32_t s_wave[PK_T / 64];
    const long base = (long)blockIdx.x * PK_TILE;
    uint32_t n = 0;
#pragma unroll
    for (int i = 0; i < PK_I; ++i) n += (uint32_t)__popcll(__ballot(pk_kept(mask, mask0, base + i * PK_T + threadIdx.x, ncell)));
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
#pragma unroll
        for (int w = 0; w < PK_T / 64; ++w) tot += s_wave[w];
        cnt[blockIdx.x] = tot;
    }
}
// PRESCANNED: cnt[b] is already the kept cells before tile b; else the count of tile b alone.  *total: the kept cells in all.
template <bool PRESCANNED>
__global__ __launch_bounds__(PK_T) void k_mv_pack_rank(const int16_t *__restrict__ mask, const int16_t *__restrict__ mask0, long ncell,
                                                      const uint32_t *__restrict__ cnt, uint32_t *__restrict__ list,
                                                      uint32_t *__restrict__ total) {
    __shared__ uint32_t s_cnt[PK_I][PK_T / 64];
    __shared__ uint32_t s_before[PK_T / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long base = (long)blockIdx.x * PK_TILE;
    unsigned long long kept[PK_I];              // (wave-uniform; the loops over it are unrolled)
#pragma unroll
    for (int i = 0; i < PK_I; ++i) {
        kept[i] = __ballot(pk_kept(mask, mask0, base + i * PK_T + threadIdx.x, ncell));
        if (lane == 0) s_cnt[i][wave] = (uint32_t)__popcll(kept[i]);
    }
    if (!PRESCANNED) {
        uint32_t s = 0;
        for (uint32_t b = threadIdx.x; b < blockIdx.x; b += PK_T) s += cnt[b];
        for (int d = 32; d; d >>= 1) s += __shfl_xor(s, d, 64);
        if (lane == 0) s_before[wave] = s;
    }
    __syncthreads();
    uint32_t run = 0;
    if (PRESCANNED) run = cnt[blockIdx.x];
    else {
#pragma unroll
        for (int w = 0; w < PK_T / 64; ++w) run += s_before[w];
    }
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int i = 0; i < PK_I; ++i) {
        uint32_t mine = 0;
#pragma unroll
        for (int w = 0; w < PK_T / 64; ++w) {
            if (w == wave) mine = run;
            run += s_cnt[i][w];
        }
        if (kept[i] >> lane & 1ull) list[mine + (uint32_t)__popcll(kept[i] & below)] = (uint32_t)(base + i * PK_T + threadIdx.x);
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *total = run;
}
// One unit = AP_ROWS kept cells of one class, staged like k_mv_append's tile: a wave gathers 64 kept cells of one variable
// (adjacent in the plane wherever the mask is dense), then consecutive lanes write consecutive (entry, variable) pairs.  A double
// plane is copied as 64-bit words, an int16 plane converted: no other floating-point operation.  Blocks stride over the units.
__global__ __launch_bounds__(AP_THREADS) void k_mv_pack(const void *const *__restrict__ planes, const int32_t *__restrict__ types, int nvar,
                                                       long class_stride, const uint32_t *__restrict__ list, uint32_t nkept, long nunit,
                                                       long stride_cell, long stride_class, int64_t *__restrict__ index,
                                                       double *__restrict__ weights, unsigned long long *__restrict__ vals) {
    __shared__ unsigned long long tile[AP_VC * AP_LD];
    const int t = threadIdx.x;
    const int lr = t & (AP_ROWS - 1), lv = t / AP_ROWS;
    const long ntile = (nkept + AP_ROWS - 1) / AP_ROWS;
    for (long u = blockIdx.x; u < nunit; u += gridDim.x) {
        const long ihc = u / ntile;
        const long row0 = (u - ihc * ntile) * AP_ROWS;
        const int nr = (int)min((long)AP_ROWS, (long)nkept - row0);
        const long pos0 = ihc * (long)nkept + row0;
        const long cell = lr < nr ? (long)list[row0 + lr] : 0;
        if (t < nr) {
            index[pos0 + t] = cell * stride_cell + ihc * stride_class;
            weights[pos0 + t] = 1.0;
        }
        const long src = ihc * class_stride + cell;
        for (int v0 = 0; v0 < nvar; v0 += AP_VC) {
            const int nc = min(AP_VC, nvar - v0);
            if (lr < nr)
                for (int v = lv; v < nc; v += AP_THREADS / AP_ROWS) {
                    const void *p = planes[v0 + v];
                    tile[v * AP_LD + lr] = types[v0 + v]
                                               ? (unsigned long long)__double_as_longlong((double)static_cast<const int16_t *>(p)[src])
                                               : static_cast<const unsigned long long *>(p)[src];
                }
            __syncthreads();
            for (int o = t; o < nr * nc; o += AP_THREADS) {
                const int r = o / nc, v = o - r * nc;
                vals[(pos0 + r) * nvar + v0 + v] = tile[v * AP_LD + r];
            }
            __syncthreads();
        }
    }
}

// ---- affine: couple()'s unit conversion (GCMCoupler_ModelE.cpp:1216-1228) ------------------------------------------------------
// vals[ix * nvar + k] = vals[ix * nvar + k] * mm[k] + bb[k] for AFF_VC variables from v0 on; the coefficients ride in the kernel
// arguments, so the call is a pure enqueue.  One product, then one add (-ffp-contract=off).
constexpr int AFF_VC = 16;
struct AffineArgs { double mm[AFF_VC], bb[AFF_VC]; };
__global__ __launch_bounds__(256) void k_mv_affine(double *__restrict__ vals, long n, int nvar, int v0, int nc, AffineArgs P) {
    const long total = n * nc;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long ix = i / nc;
        const int k = (int)(i - ix * nc);
        double *p = vals + ix * nvar + v0 + k;
        *p = *p * P.mm[k] + P.bb[k];
    }
}

// ---- grouping ---------------------------------------------------------------------------------------------------------------
// What the host reads back: badinv = 0xFFFFFFFF - (the first offending entry), 0: none (entries are < 2^31); maxkey = largest key
struct MvStatus { uint32_t badinv, pad; unsigned long long maxkey; };

// keys[off + i] = src[i], payload = off + i; an entry outside [0, limit) is reported (check != 0: the multivec's own entries)
__global__ __launch_bounds__(256) void k_mv_keys(const int64_t *__restrict__ src, uint32_t n, uint32_t off, int64_t limit, int check,
                                                 uint64_t *__restrict__ keys, uint32_t *__restrict__ pos, MvStatus *__restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long mx = 0;
    uint32_t bad = 0;
    if (i < n) {
        const int64_t k = src[i];
        keys[off + i] = (uint64_t)k;
        pos[off + i] = off + i;
        if (k < 0 || k >= limit) { if (check) bad = 0xFFFFFFFFu - i; }
        else mx = (unsigned long long)k;
    }
    for (int d = 32; d; d >>= 1) {          // every lane takes part
        const unsigned long long omx = __shfl_xor(mx, d, 64);
        const uint32_t obad = __shfl_xor(bad, d, 64);
        mx = omx > mx ? omx : mx;
        bad = obad > bad ? obad : bad;
    }
    if ((threadIdx.x & 63) == 0) {
        if (mx) atomicMax(&status->maxkey, mx);
        if (bad) atomicMax(&status->badinv, bad);
    }
}
// the first entry of index[] outside [0, limit), for the message of a refused call
__global__ __launch_bounds__(256) void k_mv_first_outside(const int64_t *__restrict__ index, uint32_t n, int64_t limit,
                                                          MvStatus *__restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && (index[i] < 0 || index[i] >= limit)) atomicMax(&status->badinv, 0xFFFFFFFFu - i);
}
// head[i] = sorted position i starts a run.  n0 > 0: positions below n0 are a set's entries, and a run that does not start with
// one names a key the set lacks: report != 0 records the first such ENTRY, isnew marks it (by entry) as a key to add.
__global__ __launch_bounds__(256) void k_mv_heads(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ perm, uint32_t n,
                                                  uint32_t n0, uint8_t *__restrict__ head, int report, uint8_t *__restrict__ isnew,
                                                  MvStatus *__restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool h = i == 0 || keys[i] != keys[i - 1];
    head[i] = h ? 1 : 0;
    if (h && perm[i] >= n0) {
        if (report) atomicMax(&status->badinv, 0xFFFFFFFFu - (perm[i] - n0));
        if (isnew) isnew[perm[i] - n0] = 1;
    }
}
__global__ __launch_bounds__(256) void k_mv_runstart(const uint8_t *__restrict__ head, const uint32_t *__restrict__ rank, uint32_t n,
                                                     const uint32_t *__restrict__ nrun, uint32_t *__restrict__ runstart) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && head[i]) runstart[rank[i]] = i;
    if (i == 0) runstart[*nrun] = n;
}
// the new keys of a set in first-seen order, behind its n0 old ones
__global__ __launch_bounds__(256) void k_mv_emit_new(const int64_t *__restrict__ index, const uint8_t *__restrict__ isnew,
                                                     const uint32_t *__restrict__ rank, uint32_t n, int64_t *__restrict__ table_new) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && isnew[i]) table_new[rank[i]] = index[i];
}

// ---- the walks --------------------------------------------------------------------------------------------------------------
// One lane per run, so the stores of consecutive runs (ascending cell) fall together; blockIdx.y picks WALK_VC variables, held
// in registers (the loops over them are unrolled: no private array is indexed dynamically).
enum { WALK_SCALE = 0, WALK_TO_DENSE = 1, WALK_UPDATE = 2, WALK_DENSIFY = 3 };
constexpr int WALK_VC = 4;
template <int MODE>
__global__ __launch_bounds__(256) void k_mv_walk(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ runstart,
                                                 const uint32_t *__restrict__ nrun, uint32_t n0, const int64_t *__restrict__ index,
                                                 const double *__restrict__ weights, const double *__restrict__ vals, int nvar,
                                                 const double *__restrict__ scale, double fill, double *__restrict__ out, long ld) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= *nrun) return;
    uint32_t b = runstart[r];
    const uint32_t e = runstart[r + 1];
    long cell;
    if (MODE == WALK_DENSIFY) {             // the run starts with the set's entry: its position is the dense index
        cell = perm[b];
        if (cell >= (long)n0) return;       // a key the set lacks: reported by k_mv_heads, nothing is written
        ++b;
    } else {
        cell = index[perm[b]];
    }
    if (MODE == WALK_SCALE) {
        double acc = 0.0;
        for (uint32_t k = b; k < e; ++k) acc += weights[perm[k]];
        out[cell] = acc;
        return;
    }
    const int v0 = blockIdx.y * WALK_VC;
    const double sc = MODE == WALK_DENSIFY ? 1.0 : scale[cell];
    double acc[WALK_VC];
#pragma unroll
    for (int j = 0; j < WALK_VC; ++j) acc[j] = MODE == WALK_TO_DENSE ? __builtin_nan("") : 0.0;
    for (uint32_t k = b; k < e; ++k) {
        const uint32_t p = perm[k];
        if (p < n0) continue;               // (a set never holds a key twice)
        const double *vp = vals + (long)(p - n0) * nvar + v0;
#pragma unroll
        for (int j = 0; j < WALK_VC; ++j) {
            if (v0 + j < nvar) {
                const double term = MODE == WALK_DENSIFY ? vp[j] : vp[j] * sc;
                if (MODE == WALK_TO_DENSE) acc[j] = acc[j] != acc[j] ? term : acc[j] + term;       // multivec.cpp:69-73
                else acc[j] += term;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < WALK_VC; ++j)
        if (v0 + j < nvar) out[(long)(v0 + j) * ld + cell] = (MODE == WALK_TO_DENSE && acc[j] != acc[j]) ? fill : acc[j];
}
__global__ __launch_bounds__(256) void k_mv_recip(double *__restrict__ s, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) s[i] = 1.0 / s[i];
}
__global__ __launch_bounds__(256) void k_mv_fill(double *__restrict__ out, long ld, long n, double v) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[(long)blockIdx.y * ld + i] = v;
}

// ---- host side --------------------------------------------------------------------------------------------------------------
static void check_mv(const ibh_multivec *mv) {
    IBH_CHECK(mv != nullptr, "null VectorMultivec handle");
    int dev = -1;
    IBH_HIP(hipGetDevice(&dev));
    IBH_CHECK(dev == mv->device, "VectorMultivec handle belongs to device %d, current device is %d", mv->device, dev);
}

// room for `need` entries; growing is geometric and copies the entries on `st`
static void mv_reserve(ibh_multivec *mv, int64_t need, hipStream_t st) {
    IBH_CHECK(need >= 0 && need < (1ll << 31), "VectorMultivec: %lld entries (fewer than 2^31 supported)", (long long)need);
    if (need <= mv->cap) return;
    int64_t cap = std::max<int64_t>(need, std::max<int64_t>(2 * mv->cap, 64));
    if (cap >= (1ll << 31)) cap = (1ll << 31) - 1;
    DevBuf<int64_t> index((size_t)cap);
    DevBuf<double> weights((size_t)cap), vals((size_t)cap * (size_t)mv->nvar);
    if (mv->n) {
        IBH_HIP(hipMemcpyAsync(index.p, mv->index.p, sizeof(int64_t) * (size_t)mv->n, hipMemcpyDeviceToDevice, st));
        IBH_HIP(hipMemcpyAsync(weights.p, mv->weights.p, sizeof(double) * (size_t)mv->n, hipMemcpyDeviceToDevice, st));
        IBH_HIP(hipMemcpyAsync(vals.p, mv->vals.p, sizeof(double) * (size_t)mv->n * (size_t)mv->nvar, hipMemcpyDeviceToDevice, st));
    }
    mv->index = std::move(index);
    mv->weights = std::move(weights);
    mv->vals = std::move(vals);
    mv->cap = cap;
}
static void mv_grew(ibh_multivec *mv, int64_t added) {
    mv->n += added;
    if (added) mv->grp.valid = false;
}
static void mv_append_device(ibh_multivec *mv, int64_t k, const int64_t *index, const double *weights, const double *vals,
                             hipMemcpyKind kind, hipStream_t st) {
    if (k == 0) return;
    mv_reserve(mv, mv->n + k, st);
    IBH_HIP(hipMemcpyAsync(mv->index.p + mv->n, index, sizeof(int64_t) * (size_t)k, kind, st));
    IBH_HIP(hipMemcpyAsync(mv->weights.p + mv->n, weights, sizeof(double) * (size_t)k, kind, st));
    IBH_HIP(hipMemcpyAsync(mv->vals.p + (size_t)mv->n * (size_t)mv->nvar, vals, sizeof(double) * (size_t)k * (size_t)mv->nvar, kind, st));
    mv_grew(mv, k);
}

[[noreturn]] static void fail_index(const ibh_multivec *mv, uint32_t entry, int64_t limit, const char *what) {
    int64_t ix = 0;
    IBH_HIP(hipMemcpy(&ix, mv->index.p + entry, sizeof(ix), hipMemcpyDeviceToHost));
    fail(IBH_EINVAL, "%s: entry %u: Index out of range: %ld vs. %ld", what, entry, (long)ix, (long)limit);
}

// The (prefix, multivec) keys sorted stably, with the run heads ranked; everything lives in the arena (which the caller has reset).
struct Grouped {
    uint32_t n = 0;                 // n0 + the multivec's entries
    uint64_t *keys = nullptr;       // [n] sorted
    uint32_t *perm = nullptr;       // [n] positions, sorted by (key, position)
    uint32_t *runstart = nullptr;   // [n + 1]
    uint32_t *nrun = nullptr;       // [1] device
    MvStatus *status = nullptr;     // device; zeroed again after the range check
    int64_t max_index = -1;
};
// prefix: n0 keys on the device (a set's dense -> sparse table) sorted in front of the multivec's; limit: the multivec's indices
// must lie in [0, limit).  Synchronises `st` once (the range check and the key width of the sort come from one read-back).
// report_missing / isnew: see k_mv_heads.
// (Sort-based, not sparseset.h's table numbering, on purpose: a multivec's set may have an unbounded sparse extent.)
static Grouped group_entries(const ibh_multivec *mv, const int64_t *prefix, uint32_t n0, int64_t limit, const char *what,
                             int report_missing, uint8_t *isnew, hipStream_t st) {
    Arena &A = arena();
    const int T = 256;
    const uint32_t nm = (uint32_t)mv->n;
    Grouped g;
    g.n = n0 + nm;
    IBH_CHECK((int64_t)n0 + mv->n < (1ll << 31), "%s: %lld keys (fewer than 2^31 supported)", what, (long long)n0 + (long long)mv->n);
    uint64_t *keys = A.get<uint64_t>(g.n), *keys_alt = A.get<uint64_t>(g.n);
    uint32_t *pos = A.get<uint32_t>(g.n), *pos_alt = A.get<uint32_t>(g.n);
    g.status = A.get<MvStatus>(1);
    g.runstart = A.get<uint32_t>((size_t)g.n + 1);
    g.nrun = A.get<uint32_t>(1);
    IBH_HIP(hipMemsetAsync(g.status, 0, sizeof(MvStatus), st));
    IBH_HIP(hipMemsetAsync(g.nrun, 0, sizeof(uint32_t), st));
    if (n0) hipLaunchKernelGGL(k_mv_keys, dim3(ceil_div(n0, T)), dim3(T), 0, st, prefix, n0, 0u, (int64_t)INT64_MAX, 0, keys, pos, g.status);
    if (nm) hipLaunchKernelGGL(k_mv_keys, dim3(ceil_div(nm, T)), dim3(T), 0, st, mv->index.p, nm, n0, limit, 1, keys, pos, g.status);
    IBH_HIP(hipGetLastError());
    MvStatus h{};
    readback_sync(&h, g.status, sizeof(h), st);
    if (h.badinv) fail_index(mv, 0xFFFFFFFFu - h.badinv, limit, what);
    g.max_index = (int64_t)h.maxkey;
    if (g.n == 0) { g.keys = keys; g.perm = pos; return g; }
    const int bits = std::max(1, bits_for(h.maxkey + 1));
    const KeyField f[2] = {{0, std::min(bits, 32)}, {32, bits - 32}};
    if (radix_sort_pairs(keys, keys_alt, pos, pos_alt, g.n, f, bits > 32 ? 2 : 1, st)) { keys = keys_alt; pos = pos_alt; }
    g.keys = keys; g.perm = pos;
    uint8_t *head = A.get<uint8_t>(g.n);
    uint32_t *rank = A.get<uint32_t>(g.n);
    hipLaunchKernelGGL(k_mv_heads, dim3(ceil_div(g.n, T)), dim3(T), 0, st, keys, pos, g.n, n0, head, report_missing, isnew, g.status);
    exclusive_scan_u8(head, rank, g.n, g.nrun, st);
    hipLaunchKernelGGL(k_mv_runstart, dim3(ceil_div(g.n, T)), dim3(T), 0, st, head, rank, g.n, g.nrun, g.runstart);
    IBH_HIP(hipGetLastError());
    return g;
}

// the multivec's own grouping, cached; every index is then known to be >= 0, and those below nE are checked against max_index
static const ibh_multivec::Grouping &ensure_grouping(const ibh_multivec *mv, int64_t nE, const char *what, hipStream_t st) {
    ibh_multivec::Grouping &G = mv->grp;
    if (!G.valid) {
        Arena &A = arena();
        A.reset();
        ibh_multivec::Grouping fresh;
        if (mv->n) {
            const Grouped g = group_entries(mv, nullptr, 0, nE, what, 0, nullptr, st);
            fresh.perm.alloc(g.n); fresh.runstart.alloc((size_t)g.n + 1); fresh.nrun.alloc(1);
            IBH_HIP(hipMemcpyAsync(fresh.perm.p, g.perm, sizeof(uint32_t) * g.n, hipMemcpyDeviceToDevice, st));
            IBH_HIP(hipMemcpyAsync(fresh.runstart.p, g.runstart, sizeof(uint32_t) * ((size_t)g.n + 1), hipMemcpyDeviceToDevice, st));
            IBH_HIP(hipMemcpyAsync(fresh.nrun.p, g.nrun, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
            fresh.max_index = g.max_index;
        }
        fresh.valid = true;
        G = std::move(fresh);
    } else if (G.max_index >= nE) {         // name the entry: one pass and one read-back, on the refusal only
        Arena &A = arena();
        A.reset();
        MvStatus *status = A.get<MvStatus>(1);
        IBH_HIP(hipMemsetAsync(status, 0, sizeof(MvStatus), st));
        hipLaunchKernelGGL(k_mv_first_outside, dim3(ceil_div(mv->n, 256)), dim3(256), 0, st, mv->index.p, (uint32_t)mv->n, nE, status);
        MvStatus h{};
        readback_sync(&h, status, sizeof(h), st);
        fail_index(mv, 0xFFFFFFFFu - h.badinv, nE, what);
    }
    return G;
}

template <int MODE>
static void launch_walk(const uint32_t *perm, const uint32_t *runstart, const uint32_t *nrun, uint32_t nruns_max, uint32_t n0,
                        const ibh_multivec *mv, const double *scale, double fill, double *out, long ld, hipStream_t st) {
    if (!nruns_max) return;
    const dim3 grid(ceil_div(nruns_max, 256), MODE == WALK_SCALE ? 1 : ceil_div(mv->nvar, WALK_VC));
    hipLaunchKernelGGL(k_mv_walk<MODE>, grid, dim3(256), 0, st, perm, runstart, nrun, n0, mv->index.p, mv->weights.p, mv->vals.p,
                       mv->nvar, scale, fill, out, ld);
    IBH_HIP(hipGetLastError());
}

static void mv_check_dense_args(const ibh_multivec *mv, const void *a, const void *b, int64_t ld, int64_t nE, const char *what) {
    check_mv(mv);
    IBH_CHECK(nE >= 0 && nE < (1ll << 31), "%s: nE=%lld out of range", what, (long long)nE);
    IBH_CHECK(nE == 0 || (a && b), "%s: null array", what);
    IBH_CHECK(ld >= nE, "%s: ld=%lld is shorter than nE=%lld", what, (long long)ld, (long long)nE);
}

// ---- append_planes, host side ------------------------------------------------------------------------------------------------
// Everything that can be refused without the count, before anything is launched or touched.  `what` names the entry.
static void check_packs(const ibh_plane_pack *packs, int32_t npack, int64_t ncell, const int16_t *mask, const char *what) {
    IBH_CHECK(npack >= 1 && packs != nullptr, "%s: at least one pack is needed", what);
    IBH_CHECK(ncell >= 0 && ncell < (1ll << 31), "%s: ncell=%lld (0 .. 2^31 - 1 supported)", what, (long long)ncell);
    IBH_CHECK(ncell == 0 || mask != nullptr, "%s: null mask", what);
    for (int p = 0; p < npack; ++p) {
        const ibh_plane_pack &k = packs[p];
        IBH_CHECK(k.mv != nullptr, "%s: pack %d: null VectorMultivec handle", what, p);
        check_mv(k.mv);
        for (int q = 0; q < p; ++q) IBH_CHECK(packs[q].mv != k.mv, "%s: packs %d and %d name the same VectorMultivec", what, q, p);
        IBH_CHECK(k.nvar == k.mv->nvar, "%s: pack %d: Inconsistant nvar: %d vs %d", what, p, k.mv->nvar, k.nvar);
        IBH_CHECK(k.nclass >= 0, "%s: pack %d: nclass=%d is negative", what, p, k.nclass);
        IBH_CHECK(k.plane_class_stride >= 0, "%s: pack %d: plane_class_stride=%lld is negative", what, p, (long long)k.plane_class_stride);
        IBH_CHECK(k.nclass <= 1 || k.plane_class_stride <= (INT64_MAX / 16 - ncell) / (k.nclass - 1),
                  "%s: pack %d: %d classes of stride %lld overflow", what, p, k.nclass, (long long)k.plane_class_stride);
        for (int v = 0; v < k.nvar; ++v)
            IBH_CHECK(!k.plane_type || k.plane_type[v] == 0 || k.plane_type[v] == 1, "%s: pack %d: plane %d has type %d (0: double, 1: int16)",
                      what, p, v, k.plane_type[v]);
        if (ncell == 0 || k.nclass == 0) continue;              // nothing is read
        IBH_CHECK(k.planes != nullptr, "%s: pack %d: null plane array", what, p);
        for (int v = 0; v < k.nvar; ++v) IBH_CHECK(k.planes[v] != nullptr, "%s: pack %d: plane %d is null", what, p, v);
    }
}

// The kept cells of (mask, mask0), ascending, in the arena; their number comes back in the call's one host wait.
static const uint32_t *list_kept(const int16_t *d_mask, const int16_t *d_mask0, int64_t ncell, uint32_t *nkept, hipStream_t st) {
    Arena &A = arena();
    const uint32_t nb = (uint32_t)ceil_div(ncell, (int64_t)PK_TILE);
    uint32_t *list = A.get<uint32_t>((size_t)ncell), *cnt = A.get<uint32_t>(nb), *total = A.get<uint32_t>(1);
    hipLaunchKernelGGL(k_mv_pack_count, dim3(nb), dim3(PK_T), 0, st, d_mask, d_mask0, (long)ncell, cnt);
    if (nb <= (uint32_t)PK_SELF_TILES) {
        hipLaunchKernelGGL(k_mv_pack_rank<false>, dim3(nb), dim3(PK_T), 0, st, d_mask, d_mask0, (long)ncell, cnt, list, total);
    } else {
        exclusive_scan_u32(cnt, cnt, nb, nullptr, st);
        hipLaunchKernelGGL(k_mv_pack_rank<true>, dim3(nb), dim3(PK_T), 0, st, d_mask, d_mask0, (long)ncell, cnt, list, total);
    }
    IBH_HIP(hipGetLastError());
    readback_sync(nkept, total, sizeof(uint32_t), st);
    return list;
}

static void append_planes_many(const ibh_plane_pack *packs, int32_t npack, int64_t ncell, const int16_t *d_mask, const int16_t *d_mask0,
                               int64_t *nkept_out, hipStream_t st) {
    const char *what = "append_planes";
    check_packs(packs, npack, ncell, d_mask, what);
    if (nkept_out) *nkept_out = 0;
    if (ncell == 0) return;
    Arena &A = arena();
    A.reset();
    // the plane tables go up in front of the mask pass: its host wait covers them
    std::vector<const void **> d_planes((size_t)npack, nullptr);
    std::vector<int32_t *> d_types((size_t)npack, nullptr);
    for (int p = 0; p < npack; ++p) {
        const ibh_plane_pack &k = packs[p];
        if (k.nclass == 0) continue;
        d_planes[(size_t)p] = A.get<const void *>((size_t)k.nvar);
        d_types[(size_t)p] = A.get<int32_t>((size_t)k.nvar);
        IBH_HIP(hipMemcpyAsync(d_planes[(size_t)p], k.planes, sizeof(void *) * (size_t)k.nvar, hipMemcpyHostToDevice, st));
        if (k.plane_type) IBH_HIP(hipMemcpyAsync(d_types[(size_t)p], k.plane_type, sizeof(int32_t) * (size_t)k.nvar, hipMemcpyHostToDevice, st));
        else IBH_HIP(hipMemsetAsync(d_types[(size_t)p], 0, sizeof(int32_t) * (size_t)k.nvar, st));
    }
    uint32_t nkept = 0;
    const uint32_t *list = list_kept(d_mask, d_mask0, ncell, &nkept, st);
    for (int p = 0; p < npack; ++p) {
        const long long total = (long long)packs[p].mv->n + (long long)packs[p].nclass * (long long)nkept;
        IBH_CHECK(total < (1ll << 31), "%s: pack %d: %lld entries (fewer than 2^31 supported)", what, p, total);
    }
    if (nkept_out) *nkept_out = nkept;
    for (int p = 0; p < npack && nkept; ++p) {
        const ibh_plane_pack &k = packs[p];
        if (k.nclass == 0) continue;
        ibh_multivec *mv = k.mv;
        const int64_t added = (int64_t)k.nclass * nkept;
        mv_reserve(mv, mv->n + added, st);
        const long nunit = (long)ceil_div((int64_t)nkept, (int64_t)AP_ROWS) * k.nclass;
        hipLaunchKernelGGL(k_mv_pack, dim3((unsigned)std::min<long>(nunit, 1l << 20)), dim3(AP_THREADS), 0, st, d_planes[(size_t)p],
                           d_types[(size_t)p], (int)k.nvar, (long)k.plane_class_stride, list, nkept, nunit, (long)k.index_stride_cell,
                           (long)k.index_stride_class, mv->index.p + mv->n, mv->weights.p + mv->n,
                           reinterpret_cast<unsigned long long *>(mv->vals.p + (size_t)mv->n * (size_t)k.nvar));
        IBH_HIP(hipGetLastError());
        mv_grew(mv, added);
    }
}

}  // namespace ibh

using namespace ibh;

extern "C" {

int ibh_multivec_create(int32_t nvar, ibh_multivec **out) {
    return guarded([&] {
        IBH_CHECK(out != nullptr, "null argument");
        *out = nullptr;
        IBH_CHECK(nvar >= 1, "VectorMultivec: nvar=%d, at least 1 is needed", nvar);
        require_device();
        std::unique_ptr<ibh_multivec> mv(new ibh_multivec);
        IBH_HIP(hipGetDevice(&mv->device));
        mv->nvar = nvar;
        *out = mv.release();
    });
}
int ibh_multivec_destroy(ibh_multivec *mv) { delete mv; return IBH_OK; }
int ibh_multivec_size(const ibh_multivec *mv, int64_t *n, int32_t *nvar) {
    return guarded([&] {
        IBH_CHECK(mv != nullptr, "null VectorMultivec handle");
        if (n) *n = mv->n;
        if (nvar) *nvar = mv->nvar;
    });
}
int ibh_multivec_clear(ibh_multivec *mv) {
    return guarded([&] {
        IBH_CHECK(mv != nullptr, "null VectorMultivec handle");
        mv->n = 0;
        mv->grp.valid = false;
    });
}
int ibh_multivec_reserve(ibh_multivec *mv, int64_t n) {
    return guarded([&] {
        check_mv(mv);
        mv_reserve(mv, n, nullptr);
    });
}
int ibh_multivec_add_host(ibh_multivec *mv, int64_t n, const int64_t *index, const double *weights, const double *vals) {
    return guarded([&] {
        check_mv(mv);
        IBH_CHECK(n >= 0 && (n == 0 || (index && weights && vals)), "VectorMultivec add: null array");
        mv_append_device(mv, n, index, weights, vals, hipMemcpyHostToDevice, nullptr);
        IBH_HIP(hipStreamSynchronize(nullptr));       // the host arrays are borrowed for the call only
    });
}
int ibh_multivec_get(const ibh_multivec *mv, int64_t *index, double *weights, double *vals) {
    return guarded([&] {
        check_mv(mv);
        if (mv->n == 0) return;
        if (index) mv->index.download(index, (size_t)mv->n);
        if (weights) mv->weights.download(weights, (size_t)mv->n);
        if (vals) mv->vals.download(vals, (size_t)mv->n * (size_t)mv->nvar);
    });
}
int ibh_multivec_device_view_get(const ibh_multivec *mv, ibh_multivec_device_view *out) {
    return guarded([&] {
        IBH_CHECK(mv && out, "null argument");
        *out = ibh_multivec_device_view{mv->n, mv->nvar, mv->index.p, mv->weights.p, mv->vals.p};
    });
}

int ibh_multivec_append_weighted_device(ibh_multivec *mv, const ibh_weighted *w, const double *dB_b, int32_t nvar, int64_t ldb,
                                        void *stream) {
    return guarded([&] {
        check_mv(mv);
        IBH_CHECK(w != nullptr, "null Weighted handle");
        IBH_CHECK(w->device == mv->device, "append_weighted: the matrix lives on device %d, the VectorMultivec on %d", w->device, mv->device);
        IBH_CHECK(nvar == mv->nvar, "append_weighted: Inconsistant nvar: %d vs %d", mv->nvar, nvar);
        const int nrow = w->nrow;
        if (nrow == 0) return;
        IBH_CHECK(dB_b != nullptr, "append_weighted: null field array");
        IBH_CHECK(ldb >= nrow, "append_weighted: ldb=%lld is shorter than the %d dense rows", (long long)ldb, nrow);
        hipStream_t st = (hipStream_t)stream;
        mv_reserve(mv, mv->n + nrow, st);
        const ibh_sparse_set *d0 = w->dims[0];
        const int64_t *to_sparse = nullptr;             // nullptr: the identity
        if (d0 && !d0->identity()) {
            IBH_CHECK(d0->dense_extent() >= nrow, "append_weighted: dims[0] holds %d entries, the matrix has %d rows", d0->dense_extent(), nrow);
            if (!d0->on_device(nrow)) arena().reset();
            to_sparse = d0->device_to_sparse(nrow, st);
        }
        hipLaunchKernelGGL(k_mv_append, dim3(ceil_div(nrow, AP_ROWS)), dim3(AP_THREADS), 0, st, dB_b, (long)ldb, nrow, (int)nvar, to_sparse,
                           w->wM.p, mv->index.p + mv->n, mv->weights.p + mv->n, mv->vals.p + (size_t)mv->n * (size_t)nvar);
        IBH_HIP(hipGetLastError());
        mv_grew(mv, nrow);
    });
}

int ibh_multivec_append_planes_many_device(const ibh_plane_pack *packs, int32_t npack, int64_t ncell, const int16_t *d_mask,
                                           const int16_t *d_mask0, int64_t *nkept, void *stream) {
    return guarded([&] { append_planes_many(packs, npack, ncell, d_mask, d_mask0, nkept, (hipStream_t)stream); });
}
int ibh_multivec_append_planes_device(ibh_multivec *mv, const void *const *d_planes, const int32_t *plane_type, int32_t nvar, int64_t ncell,
                                      int32_t nclass, int64_t plane_class_stride, const int16_t *d_mask, const int16_t *d_mask0,
                                      int64_t index_stride_cell, int64_t index_stride_class, int64_t *nkept, void *stream) {
    const ibh_plane_pack pack = {mv, d_planes, plane_type, nvar, nclass, plane_class_stride, index_stride_cell, index_stride_class};
    return ibh_multivec_append_planes_many_device(&pack, 1, ncell, d_mask, d_mask0, nkept, stream);
}
int ibh_multivec_append_planes_many_host(const ibh_plane_pack *packs, int32_t npack, int64_t ncell, const int16_t *mask, const int16_t *mask0,
                                         int64_t *nkept) {
    return guarded([&] {
        check_packs(packs, npack, ncell, mask, "append_planes");
        require_device();
        DevBuf<int16_t> dm((size_t)ncell), dm0(mask0 ? (size_t)ncell : 0);
        dm.upload(mask, (size_t)ncell);
        if (mask0) dm0.upload(mask0, (size_t)ncell);
        std::vector<DevBuf<char>> bufs;
        std::vector<std::vector<const void *>> tables((size_t)npack);
        std::vector<ibh_plane_pack> dpacks(packs, packs + npack);
        for (int p = 0; p < npack; ++p) {
            const ibh_plane_pack &k = packs[p];
            if (ncell == 0 || k.nclass == 0) continue;
            const size_t count = (size_t)(k.nclass - 1) * (size_t)k.plane_class_stride + (size_t)ncell;
            for (int v = 0; v < k.nvar; ++v) {
                const size_t bytes = count * (k.plane_type && k.plane_type[v] ? sizeof(int16_t) : sizeof(double));
                bufs.emplace_back(bytes);
                bufs.back().upload(static_cast<const char *>(k.planes[v]), bytes);
                tables[(size_t)p].push_back(bufs.back().p);
            }
            dpacks[(size_t)p].planes = tables[(size_t)p].data();
        }
        rethrow(ibh_multivec_append_planes_many_device(dpacks.data(), npack, ncell, dm.p, mask0 ? dm0.p : nullptr, nkept, nullptr));
        IBH_HIP(hipStreamSynchronize(nullptr));       // the host arrays are borrowed for the call only, the copies go away
    });
}
int ibh_multivec_append_planes_host(ibh_multivec *mv, const void *const *planes, const int32_t *plane_type, int32_t nvar, int64_t ncell,
                                    int32_t nclass, int64_t plane_class_stride, const int16_t *mask, const int16_t *mask0,
                                    int64_t index_stride_cell, int64_t index_stride_class, int64_t *nkept) {
    const ibh_plane_pack pack = {mv, planes, plane_type, nvar, nclass, plane_class_stride, index_stride_cell, index_stride_class};
    return ibh_multivec_append_planes_many_host(&pack, 1, ncell, mask, mask0, nkept);
}
int ibh_multivec_affine_device(ibh_multivec *mv, const double *mm, const double *bb, void *stream) {
    return guarded([&] {
        check_mv(mv);
        IBH_CHECK(mm && bb, "affine: null coefficient array");
        if (mv->n == 0) return;
        for (int v0 = 0; v0 < mv->nvar; v0 += AFF_VC) {
            const int nc = std::min(AFF_VC, mv->nvar - v0);
            AffineArgs P{};
            for (int k = 0; k < nc; ++k) { P.mm[k] = mm[v0 + k]; P.bb[k] = bb[v0 + k]; }
            const long blocks = std::min<long>(((long)mv->n * nc + 255) / 256, 1l << 20);
            hipLaunchKernelGGL(k_mv_affine, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, mv->vals.p, (long)mv->n, (int)mv->nvar, v0,
                               nc, P);
        }
        IBH_HIP(hipGetLastError());
    });
}

int ibh_multivec_append(ibh_multivec *mv, const ibh_multivec *other) {
    return guarded([&] {
        check_mv(mv);
        check_mv(other);
        IBH_CHECK(mv->nvar == other->nvar, "Inconsistant nvar: %d vs %d", mv->nvar, other->nvar);
        const int64_t k = other->n;
        mv_reserve(mv, mv->n + k, nullptr);             // (other may be mv itself: its buffers are read after they have moved)
        mv_append_device(mv, k, other->index.p, other->weights.p, other->vals.p, hipMemcpyDeviceToDevice, nullptr);
    });
}
int ibh_multivec_concatenate(int32_t k, const ibh_multivec *const *mvs, ibh_multivec **out) {
    return guarded([&] {
        IBH_CHECK(out != nullptr, "null argument");
        *out = nullptr;
        IBH_CHECK(k >= 1 && mvs, "Must concatenate at least one vector");
        int64_t total = 0;
        for (int i = 0; i < k; ++i) {
            check_mv(mvs[i]);
            IBH_CHECK(mvs[i]->nvar == mvs[0]->nvar, "Inconsistant nvar: %d vs %d (vector %d)", mvs[0]->nvar, mvs[i]->nvar, i);
            total += mvs[i]->n;
        }
        std::unique_ptr<ibh_multivec> mv(new ibh_multivec);
        mv->device = mvs[0]->device;
        mv->nvar = mvs[0]->nvar;
        mv_reserve(mv.get(), total, nullptr);
        for (int i = 0; i < k; ++i)
            mv_append_device(mv.get(), mvs[i]->n, mvs[i]->index.p, mvs[i]->weights.p, mvs[i]->vals.p, hipMemcpyDeviceToDevice, nullptr);
        *out = mv.release();
    });
}

int ibh_multivec_to_dense_scale(const ibh_multivec *mv, int64_t nE, double *d_scale, void *stream) {
    return guarded([&] {
        mv_check_dense_args(mv, d_scale, d_scale, nE, nE, "to_dense_scale");
        hipStream_t st = (hipStream_t)stream;
        const ibh_multivec::Grouping &G = ensure_grouping(mv, nE, "to_dense_scale", st);
        if (nE == 0) return;
        IBH_HIP(hipMemsetAsync(d_scale, 0, sizeof(double) * (size_t)nE, st));
        launch_walk<WALK_SCALE>(G.perm.p, G.runstart.p, G.nrun.p, (uint32_t)mv->n, 0, mv, nullptr, 0.0, d_scale, nE, st);
        hipLaunchKernelGGL(k_mv_recip, dim3(ceil_div(nE, 256)), dim3(256), 0, st, d_scale, (long)nE);
        IBH_HIP(hipGetLastError());
    });
}
int ibh_multivec_to_dense(const ibh_multivec *mv, const double *d_scale, double fill, double *d_out, int64_t ld, int64_t nE,
                          void *stream) {
    return guarded([&] {
        mv_check_dense_args(mv, d_scale, d_out, ld, nE, "to_dense");
        hipStream_t st = (hipStream_t)stream;
        const ibh_multivec::Grouping &G = ensure_grouping(mv, nE, "to_dense", st);
        if (nE == 0) return;
        hipLaunchKernelGGL(k_mv_fill, dim3(ceil_div(nE, 256), mv->nvar), dim3(256), 0, st, d_out, (long)ld, (long)nE, fill);
        IBH_HIP(hipGetLastError());
        launch_walk<WALK_TO_DENSE>(G.perm.p, G.runstart.p, G.nrun.p, (uint32_t)mv->n, 0, mv, d_scale, fill, d_out, ld, st);
    });
}
int ibh_multivec_update_dense(const ibh_multivec *mv, const double *d_scale, double *d_out, int64_t ld, int64_t nE, void *stream) {
    return guarded([&] {
        mv_check_dense_args(mv, d_scale, d_out, ld, nE, "update_dense");
        hipStream_t st = (hipStream_t)stream;
        const ibh_multivec::Grouping &G = ensure_grouping(mv, nE, "update_dense", st);
        launch_walk<WALK_UPDATE>(G.perm.p, G.runstart.p, G.nrun.p, (uint32_t)mv->n, 0, mv, d_scale, 0.0, d_out, ld, st);
    });
}

int ibh_sparse_set_add_dense_multivec(ibh_sparse_set *set, const ibh_multivec *mv, void *stream) {
    return guarded([&] {
        IBH_CHECK(set != nullptr, "null SparseSet handle");
        check_mv(mv);
        if (mv->n == 0) return;
        hipStream_t st = (hipStream_t)stream;
        Arena &A = arena();
        A.reset();
        const uint32_t n0 = (uint32_t)set->dense_extent(), nm = (uint32_t)mv->n;
        const int64_t limit = set->sparse_extent() >= 0 ? set->sparse_extent() : (int64_t)INT64_MAX;
        int64_t *table = A.get<int64_t>((size_t)n0 + nm);      // the old entries, then the new ones in first-seen order
        set->copy_to_sparse(table, (int)n0, st);
        uint8_t *isnew = A.get<uint8_t>(nm);
        uint32_t *rank = A.get<uint32_t>(nm), *d_new = A.get<uint32_t>(1);
        IBH_HIP(hipMemsetAsync(isnew, 0, nm, st));
        (void)group_entries(mv, table, n0, limit, "add_dense", 0, isnew, st);
        exclusive_scan_u8(isnew, rank, nm, d_new, st);
        hipLaunchKernelGGL(k_mv_emit_new, dim3(ceil_div(nm, 256)), dim3(256), 0, st, mv->index.p, isnew, rank, nm, table + n0);
        IBH_HIP(hipGetLastError());
        uint32_t n_new = 0;
        readback_sync(&n_new, d_new, sizeof(n_new), st);
        if (n_new == 0) return;
        IBH_CHECK((int64_t)n0 + n_new < 0x7fffffffll, "dense extent overflows int32");
        DevBuf<int64_t> grown((size_t)n0 + n_new);
        IBH_HIP(hipMemcpyAsync(grown.p, table, sizeof(int64_t) * ((size_t)n0 + n_new), hipMemcpyDeviceToDevice, st));
        IBH_HIP(hipStreamSynchronize(st));
        set->adopt_device(std::move(grown), (int32_t)(n0 + n_new), set->sparse_extent());
    });
}

int ibh_multivec_densify_device(const ibh_multivec *mv, const ibh_sparse_set *set, double *d_out, int64_t ld, void *stream) {
    return guarded([&] {
        IBH_CHECK(set != nullptr, "null SparseSet handle");
        const int64_t nd = set->dense_extent();
        mv_check_dense_args(mv, d_out, d_out, ld, nd, "densify");
        hipStream_t st = (hipStream_t)stream;
        Arena &A = arena();
        A.reset();
        const uint32_t n0 = (uint32_t)nd;
        int64_t *table = A.get<int64_t>(n0);
        set->copy_to_sparse(table, (int)n0, st);
        const Grouped g = group_entries(mv, table, n0, (int64_t)INT64_MAX, "densify", 1, nullptr, st);
        if (mv->n) {
            MvStatus h{};
            readback_sync(&h, g.status, sizeof(h), st);
            if (h.badinv) {
                const uint32_t entry = 0xFFFFFFFFu - h.badinv;
                int64_t ix = 0;
                IBH_HIP(hipMemcpy(&ix, mv->index.p + entry, sizeof(ix), hipMemcpyDeviceToHost));
                fail(IBH_EINVAL, "densify: entry %u: index %ld is not in the SparseSet", entry, (long)ix);
            }
        }
        if (nd) hipLaunchKernelGGL(k_mv_fill, dim3(ceil_div(nd, 256), mv->nvar), dim3(256), 0, st, d_out, (long)ld, (long)nd, 0.0);
        if (mv->n) launch_walk<WALK_DENSIFY>(g.perm, g.runstart, g.nrun, g.n, n0, mv, nullptr, 0.0, d_out, ld, st);
    });
}

// ---- host-array forms (a caller without device arrays of its own: the C++ mirror's to_dense_scale / to_dense / add) ----------
int ibh_multivec_append_weighted_host(ibh_multivec *mv, const ibh_weighted *w, const double *B_b, int32_t nvar, int64_t ldb) {
    return guarded([&] {
        IBH_CHECK(w != nullptr, "null Weighted handle");
        IBH_CHECK(nvar >= 1 && ldb >= w->nrow && (w->nrow == 0 || B_b), "append_weighted: bad field array");
        require_device();
        DevBuf<double> dB((size_t)nvar * (size_t)ldb);
        dB.upload(B_b, (size_t)nvar * (size_t)ldb);
        rethrow(ibh_multivec_append_weighted_device(mv, w, dB.p, nvar, ldb, nullptr));
        IBH_HIP(hipStreamSynchronize(nullptr));
    });
}
int ibh_multivec_to_dense_scale_host(const ibh_multivec *mv, int64_t nE, double *scale) {
    return guarded([&] {
        IBH_CHECK(nE >= 0 && (nE == 0 || scale), "to_dense_scale: null array");
        require_device();
        DevBuf<double> d((size_t)nE);
        rethrow(ibh_multivec_to_dense_scale(mv, nE, d.p, nullptr));
        d.download(scale, (size_t)nE);
    });
}
int ibh_multivec_to_dense_host(const ibh_multivec *mv, const double *scale, double fill, double *out, int64_t ld, int64_t nE) {
    return guarded([&] {
        check_mv(mv);
        IBH_CHECK(nE >= 0 && ld >= nE && (nE == 0 || (scale && out)), "to_dense: bad arrays");
        DevBuf<double> ds((size_t)nE), dout((size_t)mv->nvar * (size_t)nE);
        ds.upload(scale, (size_t)nE);
        rethrow(ibh_multivec_to_dense(mv, ds.p, fill, dout.p, nE, nE, nullptr));
        IBH_HIP(hipMemcpy2D(out, sizeof(double) * (size_t)ld, dout.p, sizeof(double) * (size_t)nE, sizeof(double) * (size_t)nE,
                            (size_t)mv->nvar, hipMemcpyDeviceToHost));
    });
}

}  // extern "C"
