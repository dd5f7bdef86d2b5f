// assemble.hip -- K2-K4: regrid-matrix assembly on gfx950 (COO -> CSR, weights, scaling).
//
// Replaces, for IceRegridder_L0 exchange grids, the whole of compute_AEvI /
// compute_IvAE / compute_EvA (RegridMatrices_Dynamic.cpp:50-332): the Ur-matrix
// generators GvAp / GvI / GvEp (IceRegridder_L0.cpp:100-214), spsparse's
// first-seen dense numbering (MakeDenseEigenT ... ADD_DENSE), Eigen's
// setFromTriplets, the sparse*diag*sparse products, sum(), and the diagonal
// scalings.  For an L0 exchange grid every exchange cell x has exactly one
// atmosphere cell and one ice cell, so each product collapses to a keyed sum
//     T[r,c] = sum over x ASCENDING of  fl( fl(lhs_x * sinv_x) * rhs_x )
// (the order and rounding of Eigen's conservative sparse product, see
// oracle/icebin_oracle.c), which is computed as: emit contributions in x
// order (here) -> stable order by (row_d, col_d) -> sequential sum per segment
// (the triplets -> CSR layer, csrbuild.h, which also sums the rows and the
// columns in the orders of spsparse sum()).  All of it is index/byte work bound
// by HBM traffic; no float atomics, no FMA contraction (this file is compiled
// with -ffp-contract=off), so the CSR structure, dims, wM, Mw and M are
// bit-identical to the oracle.  The smoother and the apply structures of a
// matrix (bands, sweep, row groups, tiles) are built here as well.
#include "assemble.h"
#include "asm_plan.h"
#include "smooth_plan.h"
#include "csrbuild.h"
#include "prims.h"
#include "sparseset.h"
#include "sweep_kernel.inl"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>

namespace ibh {

// (LIST_*, KEY_*, FAM_*: asm_plan.h)
// contribution formulas: t = fl(fl(lhs * sinv) * rhs)
enum { TERM_PLAIN_A = 0,   // a                       (AvX, XvA)
       TERM_PLAIN_E,       // vE                      (EvX, XvE)
       TERM_A_A,           // lhs=a,  sinv=1/a,  rhs=a    (AvI, IvA), needs x in GvAp and GvI
       TERM_E_A,           // lhs=vE, sinv=1/a,  rhs=a    (EvI needs GvI; EvA needs GvAp)
       TERM_A_E };         // lhs=a,  sinv=1/rs, rhs=vE   (IvE needs GvI; AvE needs GvAp)

struct MatSpec {
    const char *name;
    int family;
    int row_list, row_key, col_list, col_key;
    int term;
    int need_list;     // extra list the contributing x must belong to (LIST_AP / LIST_I), -1 none
    int epx;           // contributions per x: 1 or 2 (2 when GvEp entries are enumerated)
};
static const MatSpec SPECS[] = {
    // name  family    rows               cols               term          need     epx
    {"AvI", FAM_AEVI, LIST_AP, KEY_A, LIST_I,  KEY_I, TERM_A_A,     LIST_I,  1},
    {"EvI", FAM_AEVI, LIST_EP, KEY_E, LIST_I,  KEY_I, TERM_E_A,     LIST_I,  2},
    {"AvX", FAM_AEVI, LIST_AP, KEY_A, LIST_AP, KEY_X, TERM_PLAIN_A, -1,      1},
    {"EvX", FAM_AEVI, LIST_EP, KEY_E, LIST_EP, KEY_X, TERM_PLAIN_E, -1,      2},
    {"IvA", FAM_IVAE, LIST_I,  KEY_I, LIST_AP, KEY_A, TERM_A_A,     LIST_I,  1},
    {"IvE", FAM_IVAE, LIST_I,  KEY_I, LIST_EP, KEY_E, TERM_A_E,     LIST_I,  2},
    {"XvA", FAM_IVAE, LIST_AP, KEY_X, LIST_AP, KEY_A, TERM_PLAIN_A, -1,      1},
    {"XvE", FAM_IVAE, LIST_EP, KEY_X, LIST_EP, KEY_E, TERM_PLAIN_E, -1,      2},
    {"EvA", FAM_EVA,  LIST_EP, KEY_E, LIST_AP, KEY_A, TERM_E_A,     LIST_AP, 2},
    {"AvE", FAM_EVA,  LIST_AP, KEY_A, LIST_EP, KEY_E, TERM_A_E,     LIST_AP, 2},
};
// the sparse extent of a key's index space
static int64_t key_extent(const ibh_regridder *g, int key) {
    return key == KEY_A ? g->nA : key == KEY_E ? g->nA * (int64_t)g->nhc : key == KEY_I ? g->nI : g->nX;
}
// the elevation of exchange cell x's ice cell lies outside hcdefs: the message of linterp_1d_b, IceRegridder_L0.cpp:84-85
[[noreturn]] static void fail_elevation_range(const ibh_regrid_matrices *rm, uint32_t x) {
    const ibh_regridder *g = rm->rg;
    int32_t ij[2];
    IBH_HIP(hipMemcpy(ij, g->ex_indices.p + 2 * (size_t)x, sizeof(ij), hipMemcpyDeviceToHost));
    double e = 0;
    IBH_HIP(hipMemcpy(&e, rm->elevmaskI.p + ij[1], sizeof(double), hipMemcpyDeviceToHost));
    fail(IBH_ERANGE, "Elevation %g out of bounds (%g, %g)", e < 0 ? 0.0 : e, g->hcdefs_h.front(), g->hcdefs_h.back());
}

struct RgView {
    const int32_t *exi;
    const double *area, *em, *hc;
    const double *ratioA;   // by sparse A index; 0 = A cell not realised
    long nX, nA;
    int nhc, interp;
    long sA, sHC;
};

// ---- per-exchange-cell generators (device restatement of IceRegridder_L0.cpp:100-214) ----------
struct XCell {
    long iA, iI;
    double a;
    bool unmasked, inAp, inI;
    int nep;            // GvEp entries actually emitted (0..2)
    long iE0, iE1;      // scalars, not arrays: dynamically indexed private arrays live in scratch memory
    double vE0, vE1;
    double rsE;         // sum(GvEp row x): one entry -> v, two -> fl(v0 + v1)
    bool range_error;
};

__device__ __forceinline__ int dev_lower_bound(const double *__restrict__ xp, int n, double xx) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (xp[mid] < xx) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// hcdefs staged in LDS for the elevation-class generators (binary search per cell); falls back to
// global memory for very long tables
constexpr int HC_LDS = 512;
template <bool WITH_EP>
__device__ __forceinline__ void stage_hc(RgView &rg, double *s_hc) {
    if (WITH_EP && rg.nhc <= HC_LDS) {
        for (int i = threadIdx.x; i < rg.nhc; i += blockDim.x) s_hc[i] = rg.hc[i];
        __syncthreads();
        rg.hc = s_hc;
    }
}
// the arithmetic of a cell from its four inputs (callers that stage the loads of several cells themselves use this form)
// (hint: the result of the class search when the caller already has it -- the upper class index of Z_INTERP, the class of
// ELEV_CLASS_INTERP; < 0: search)
template <bool WITH_EP>
__device__ __forceinline__ XCell make_cell(const RgView &rg, long iA, long iI, double a, double e, int hint = -1) {
    XCell c;
    c.iA = iA;
    c.iI = iI;
    c.a = a;
    c.unmasked = !(e != e);                       // !std::isnan, IceRegridder_L0.cpp:121,186,208
    c.inAp = c.unmasked && c.a > 0;               // :208-209
    c.inI = c.unmasked && c.a != 0;               // :186-187 (+ include_zero=false)
    c.nep = 0;
    c.iE0 = c.iE1 = -1;
    c.vE0 = c.vE1 = 0.0;
    c.rsE = 0.0;
    c.range_error = false;
    if (WITH_EP && c.unmasked) {
        const double elevation = e < 0.0 ? 0.0 : e;          // std::max(elev, 0.0), :123
        if (rg.interp == 0) {                                // Z_INTERP, :127-145
            int i1 = hint >= 0 ? hint : dev_lower_bound(rg.hc, rg.nhc, elevation);
            if (i1 <= 0) i1 = 1;
            if (i1 >= rg.nhc) { c.range_error = true; return c; }      // :84-85
            const int i0 = i1 - 1;
            const double ratio = (elevation - rg.hc[i0]) / (rg.hc[i1] - rg.hc[i0]);
            const double w0 = 1.0 - ratio, w1 = ratio;
            bool h0 = false, h1 = false;
            double v0 = 0.0, v1 = 0.0;
            if (w0 != 0) { v0 = c.a * w0; h0 = v0 != 0; }
            if (w1 != 0) { v1 = c.a * w1; h1 = v1 != 0; }
            const long k0 = c.iA * rg.sA + (long)i0 * rg.sHC, k1 = c.iA * rg.sA + (long)i1 * rg.sHC;
            if (h0) {
                c.iE0 = k0; c.vE0 = v0; c.nep = 1;
                if (h1) { c.iE1 = k1; c.vE1 = v1; c.nep = 2; }
            } else if (h1) {
                c.iE0 = k1; c.vE0 = v1; c.nep = 1;
            }
        } else {                                             // ELEV_CLASS_INTERP, :146-150 + nearest_1d :43-67
            const int n = rg.nhc;
            int i1 = hint >= 0 ? 0 : dev_lower_bound(rg.hc, n, elevation);
            int ih;
            if (hint >= 0) ih = hint;
            else if (i1 <= 0) ih = 0;
            else if (i1 >= n) ih = n - 1;
            else {
                const int i0 = i1 - 1;
                const double d0 = fabs(elevation - rg.hc[i0]), d1 = fabs(rg.hc[i1] - elevation);
                ih = d0 <= d1 ? i0 : i1;
            }
            if (c.a != 0) { c.iE0 = c.iA * rg.sA + (long)ih * rg.sHC; c.vE0 = c.a; c.nep = 1; }
        }
        if (c.nep == 1) c.rsE = c.vE0;
        else if (c.nep == 2) c.rsE = c.vE0 + c.vE1;
    }
    return c;
}
// the class search of make_cell for one elevation, to be handed back to it as `hint` by a caller that evaluates several exchange
// cells of the same ice cell
__device__ __forceinline__ int cell_hint(const RgView &rg, double e) {
    if (e != e || rg.nhc < 1) return -1;
    const double elevation = e < 0.0 ? 0.0 : e;
    const int i1 = dev_lower_bound(rg.hc, rg.nhc, elevation);
    if (rg.interp == 0) return i1;
    const int n = rg.nhc;
    if (i1 <= 0) return 0;
    if (i1 >= n) return n - 1;
    const int i0 = i1 - 1;
    const double d0 = fabs(elevation - rg.hc[i0]), d1 = fabs(rg.hc[i1] - elevation);
    return d0 <= d1 ? i0 : i1;
}
template <bool WITH_EP>
__device__ __forceinline__ XCell load_cell(const RgView &rg, long x) {
    const long iA = rg.exi[2 * x], iI = rg.exi[2 * x + 1];
    return make_cell<WITH_EP>(rg, iA, iI, rg.area[x], rg.em[iI]);
}

// entries of `list` at cell c: count and sparse keys of kind `key`
__device__ __forceinline__ int list_entries(const XCell &c, long x, int list, int key, long &k0, long &k1) {
    int n;
    if (list == LIST_AP) n = c.inAp ? 1 : 0;
    else if (list == LIST_I) n = c.inI ? 1 : 0;
    else n = c.nep;
    const long base = key == KEY_A ? c.iA : key == KEY_I ? c.iI : x;
    k0 = key == KEY_E ? c.iE0 : base;
    k1 = key == KEY_E ? c.iE1 : base;
    // an X key is emitted once per list entry; duplicates are harmless to first-seen numbering
    return n;
}

// ---- dense numbering (spsparse::SparseSet::add_dense in emission order) ------------------------
// The assembly's own, on purpose: TWO sets per exchange-cell visit, not the one key stream of sparseset.h (the set's members: there).
// The generator passes handle BOTH sets of a matrix (rows and columns) per exchange-cell visit:
//   pass 1 (k_first2)  first[key] = smallest emission position 2x+j naming the key (atomicMin)
//   pass 2 (k_flag2)   pk[x] = which of the cell's entries are first occurrences + its number of
//                      contributions; ONE packed scan then ranks rows, columns and contributions
//   pass 3 (k_contrib_emit) dense id of any key = old id, or base + rank of its first occurrence
//                      (looked up through first[]); first occurrences also record to_sparse.
struct SetArgs {
    int enabled, list, key, base;
    long ident_n;               // >= 0: the set's old part is the identity on [0, ident_n)
    const int32_t *tab;         // old sparse -> dense table (-1 missing); nullptr when there is no old part / identity
    uint32_t *first;            // [sparse_extent] smallest emission position 2x+j that names the key
    int64_t *to_sparse;         // [capacity] dense -> sparse
    const uint32_t *off;        // [nX] new keys of this set emitted before cell x (after the scan)
    int pkshift;                // this set's flag pair inside pk[x]
};
__device__ __forceinline__ int old_dense(const SetArgs &a, long key) {
    if (a.ident_n >= 0) return key < a.ident_n ? (int)key : -1;
    return a.tab ? a.tab[key] : -1;
}

// Keys shared by many cells (atmosphere cells, elevation classes: ~10^2..10^3 cells name each one)
// are de-duplicated inside the wave first: lanes holding the same key elect the lowest lane, whose
// position is the smallest (positions grow with the lane), and only that lane issues the global
// atomicMin.  Device-scope atomics are resolved beyond the per-XCD L2; a 38.8 M-cell grid would
// otherwise issue 7.7e7 of them on ~10^5 addresses.  Keys that are (almost) unique per cell (ice
// cells, exchange cells) go to memory directly.
__device__ __forceinline__ bool shared_keys(const SetArgs &a) { return a.key == KEY_A || a.key == KEY_E; }
__device__ __forceinline__ void first_entry(const SetArgs &a, long key, bool has, uint32_t pos, bool dedupe, int lane) {
    if (!dedupe) {
        if (has) atomicMin(&a.first[key], pos);
        return;
    }
    unsigned long long todo = __ballot(has);          // every lane takes part in the ballots
    bool is_leader = false;
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const long k = __shfl(key, leader, 64);
        const unsigned long long same = __ballot(has && key == k);
        if (lane == leader) is_leader = true;
        todo &= ~same;
    }
    // ONE atomic instruction for all elected lanes
    if (is_leader) atomicMin(&a.first[key], pos);
}
__device__ __forceinline__ void first_one(const SetArgs &a, const XCell &c, long x, bool valid) {
    long k0 = -1, k1 = -1;
    const int n = valid ? list_entries(c, x, a.list, a.key, k0, k1) : 0;
    const bool dedupe = shared_keys(a);
    const int lane = threadIdx.x & 63;
    first_entry(a, k0, n > 0 && old_dense(a, k0) < 0, (uint32_t)(2 * x), dedupe, lane);
    if (a.list == LIST_EP)          // uniform: only elevation-class lists have second entries
        first_entry(a, k1, n > 1 && old_dense(a, k1) < 0, (uint32_t)(2 * x + 1), dedupe, lane);
}
template <bool WITH_EP>
__global__ __launch_bounds__(256) void k_first2(RgView rg, SetArgs a, SetArgs b, uint32_t *__restrict__ err_x) {
    __shared__ double s_hc[WITH_EP ? HC_LDS : 1];
    stage_hc<WITH_EP>(rg, s_hc);
    const long x = (long)blockIdx.x * blockDim.x + threadIdx.x;
    XCell c;
    bool valid = false;                         // no early return: every lane takes part in the ballots
    if (x < rg.nX) {
        c = load_cell<WITH_EP>(rg, x);
        if (WITH_EP && c.range_error) atomicMin(err_x, (uint32_t)x);
        else valid = true;
    }
    if (a.enabled) first_one(a, c, x, valid);
    if (b.enabled) first_one(b, c, x, valid);
}

__device__ __forceinline__ uint32_t flag_one(const SetArgs &a, const XCell &c, long x) {
    long k0, k1;
    const int n = list_entries(c, x, a.list, a.key, k0, k1);
    uint32_t f = 0;
    if (n > 0 && old_dense(a, k0) < 0 && a.first[k0] == (uint32_t)(2 * x)) f |= 1u;
    if (n > 1 && old_dense(a, k1) < 0 && a.first[k1] == (uint32_t)(2 * x + 1)) f |= 2u;
    return f;
}
// dense id of `key` (any cell may ask): old id, else base + rank of the key's first occurrence
__device__ __forceinline__ int dense_of(const SetArgs &a, long key, const uint32_t *__restrict__ pk) {
    if (!a.enabled) return (int)key;                       // identity over the whole sparse extent
    const int t = old_dense(a, key);
    if (t >= 0) return t;
    const uint32_t p = a.first[key];
    const uint32_t xf = p >> 1;
    uint32_t r = a.off[xf];
    if (p & 1u) r += (pk[xf] >> a.pkshift) & 1u;           // second entry of its cell: after the first if that one was new too
    return a.base + (int)r;
}
// the cell's own first occurrences record dense -> sparse
__device__ __forceinline__ void record_new(const SetArgs &a, const XCell &c, long x, uint32_t pkx) {
    const uint32_t f = (pkx >> a.pkshift) & 3u;
    if (!f) return;
    long k0, k1;
    (void)list_entries(c, x, a.list, a.key, k0, k1);
    const uint32_t r = a.off[x];
    if (f & 1u) a.to_sparse[a.base + r] = k0;
    if (f & 2u) a.to_sparse[a.base + r + (f & 1u)] = k1;
}

struct DeviceSet {
    int64_t *to_sparse = nullptr; // [capacity] dense -> sparse
    int n_old = 0, n = 0;
};

// Host side of the dense numbering of one set (spsparse::SparseSet::add_dense in emission order,
// appending to whatever the caller's set already holds): prepare() builds the device tables,
// the fused kernels above do the work, finish() adopts the new keys once the host knows how many.
struct Numbering {
    DeviceSet ds;
    ibh_sparse_set *set = nullptr;
    SetArgs args{};
    int64_t max_new = 0;
};

static Numbering number_set_prepare(const RgView &rg, ibh_sparse_set *set, int64_t sparse_extent, int list, int key,
                                    int64_t max_new, int pkshift, uint32_t *first_storage, hipStream_t st) {
    Arena &A = arena();
    set->set_sparse_extent(sparse_extent);                   // set_sparse_extent, RegridMatrices_Dynamic.cpp:69-72
    set->check_entries_within(sparse_extent, "dims");
    Numbering nb;
    nb.set = set;
    DeviceSet &ds = nb.ds;
    ds.n_old = set->dense_extent();
    IBH_CHECK(sparse_extent < 0xffffffffll, "sparse extent %ld does not fit 32 bits", (long)sparse_extent);
    if (max_new > sparse_extent - ds.n_old) max_new = sparse_extent - ds.n_old;
    nb.max_new = max_new;
    const int64_t cap = (int64_t)ds.n_old + max_new;
    ds.to_sparse = A.get<int64_t>((size_t)cap);
    SetArgs &a = nb.args;
    a.list = list; a.key = key; a.base = ds.n_old; a.to_sparse = ds.to_sparse; a.pkshift = pkshift;
    a.ident_n = -1; a.tab = nullptr;
    set->copy_to_sparse(ds.to_sparse, ds.n_old, st);
    if (ds.n_old && set->identity()) {
        a.ident_n = ds.n_old;
    } else if (ds.n_old) {
        int32_t *tab = A.get<int32_t>((size_t)sparse_extent);
        fill_to_dense_table(tab, sparse_extent, ds.to_sparse, ds.n_old, st);
        a.tab = tab;
    }
    ds.n = ds.n_old;
    a.enabled = !(set->identity() && ds.n_old == sparse_extent);    // an identity set that covers everything gains nothing
    a.first = first_storage;            // [sparse_extent], preset to 0xFFFFFFFF by the caller (one fill for both sets)
    return nb;
}

static void number_set_finish(Numbering &nb, uint32_t n_new, hipStream_t st) {
    DeviceSet &ds = nb.ds;
    if (!nb.args.enabled || n_new == 0) return;
    ds.n = ds.n_old + (int)n_new;
    // the set keeps its table on the device; the host copy is completed only when somebody asks
    DevBuf<int64_t> grown((size_t)ds.n);
    IBH_HIP(hipMemcpyAsync(grown.p, ds.to_sparse, sizeof(int64_t) * (size_t)ds.n, hipMemcpyDeviceToDevice, st));
    nb.set->adopt_device(std::move(grown), ds.n, nb.set->sparse_extent());
}

// ---- contributions ---------------------------------------------------------------------------
struct Contrib { long r0, r1, c0, c1; double t0, t1; };
__device__ __forceinline__ int contributions(const XCell &c, long x, const MatSpec &s, Contrib &o) {
    if (s.need_list == LIST_I && !c.inI) return 0;
    if (s.need_list == LIST_AP && !c.inAp) return 0;
    switch (s.term) {
        case TERM_PLAIN_A:
            if (!c.inAp) return 0;
            o.r0 = s.row_key == KEY_X ? x : c.iA; o.c0 = s.col_key == KEY_X ? x : c.iA; o.t0 = c.a;
            return 1;
        case TERM_PLAIN_E:
            o.r0 = s.row_key == KEY_X ? x : c.iE0; o.c0 = s.col_key == KEY_X ? x : c.iE0; o.t0 = c.vE0;
            o.r1 = s.row_key == KEY_X ? x : c.iE1; o.c1 = s.col_key == KEY_X ? x : c.iE1; o.t1 = c.vE1;
            return c.nep;
        case TERM_A_A: {
            if (!c.inAp) return 0;
            const double sinv = 1.0 / c.a;
            const double l = c.a * sinv;
            o.r0 = s.row_key == KEY_A ? c.iA : c.iI; o.c0 = s.col_key == KEY_A ? c.iA : c.iI; o.t0 = l * c.a;
            return 1;
        }
        case TERM_E_A: {      // rows E; cols I (EvI) or A (EvA)
            const double sinv = 1.0 / c.a;
            const long ck = s.col_key == KEY_A ? c.iA : c.iI;
            const double l0 = c.vE0 * sinv, l1 = c.vE1 * sinv;
            o.r0 = c.iE0; o.c0 = ck; o.t0 = l0 * c.a;
            o.r1 = c.iE1; o.c1 = ck; o.t1 = l1 * c.a;
            return c.nep;
        }
        default: {            // TERM_A_E: cols E; rows I (IvE) or A (AvE)
            if (c.nep == 0) return 0;
            const double sinv = 1.0 / c.rsE;
            const double l = c.a * sinv;
            const long rk = s.row_key == KEY_A ? c.iA : c.iI;
            o.r0 = rk; o.c0 = c.iE0; o.t0 = l * c.vE0;
            o.r1 = rk; o.c1 = c.iE1; o.t1 = l * c.vE1;
            return c.nep;
        }
    }
}

template <bool WITH_EP>
__global__ void k_flag2(RgView rg, SetArgs a, SetArgs b, MatSpec s, uint32_t *__restrict__ pk) {
    __shared__ double s_hc[WITH_EP ? HC_LDS : 1];
    stage_hc<WITH_EP>(rg, s_hc);
    const long x = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= rg.nX) return;
    const XCell c = load_cell<WITH_EP>(rg, x);
    uint32_t v = 0;
    if (!(WITH_EP && c.range_error)) {
        if (a.enabled) v |= flag_one(a, c, x) << a.pkshift;
        if (b.enabled) v |= flag_one(b, c, x) << b.pkshift;
        Contrib o;
        v |= (uint32_t)contributions(c, x, s, o) << 4;
    }
    pk[x] = v;
}
template <bool WITH_EP>
__global__ void k_contrib_emit(RgView rg, MatSpec s, SetArgs a, SetArgs b, const uint32_t *__restrict__ pk,
                               const uint32_t *__restrict__ pos, uint64_t *__restrict__ keys, uint32_t *__restrict__ idx,
                               double *__restrict__ term) {
    __shared__ double s_hc[WITH_EP ? HC_LDS : 1];
    stage_hc<WITH_EP>(rg, s_hc);
    const long x = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= rg.nX) return;
    const uint32_t pkx = pk[x];
    if (!pkx) return;                          // nothing new, nothing contributed (masked cells, range errors)
    const XCell c = load_cell<WITH_EP>(rg, x);
    if (a.enabled) record_new(a, c, x, pkx);
    if (b.enabled) record_new(b, c, x, pkx);
    Contrib o;
    const int n = contributions(c, x, s, o);
    const uint32_t p = pos[x];
    if (n == 0) return;
    uint64_t q0 = ((uint64_t)(uint32_t)dense_of(a, o.r0, pk) << 32) | (uint32_t)dense_of(b, o.c0, pk);
    if (n > 1) {
        // The two entries of a cell name different elevation classes, so they are never summed
        // together and may be emitted in either order: ascending key keeps the sequence closer to
        // sorted (the first-seen class numbering is not monotone in the class index).
        uint64_t q1 = ((uint64_t)(uint32_t)dense_of(a, o.r1, pk) << 32) | (uint32_t)dense_of(b, o.c1, pk);
        if (q1 < q0) { const uint64_t tq = q0; q0 = q1; q1 = tq; const double tt = o.t0; o.t0 = o.t1; o.t1 = tt; }
        keys[p + 1] = q1; idx[p + 1] = p + 1; term[p + 1] = o.t1;
    }
    keys[p] = q0; idx[p] = p; term[p] = o.t0;
}

// ---- weights and scaling (RegridMatrices_Dynamic.cpp:100-146, 201-233, 290-329) ----------------
__device__ __forceinline__ double ratio_of(const RgView &rg, int keykind, int64_t sparse) {
    int64_t iA = sparse, ihc;
    if (keykind == KEY_E) HcIndexing{rg.sA, rg.sHC}.split(sparse, iA, ihc);
    return rg.ratioA[iA];
}
struct FinalizeArgs {
    int family, scale, correctA, row_key, col_key;
    int nrow, ncol;
    const int64_t *row_s, *col_s;     // dense -> sparse
    const double *rs, *cs;
    double *wM, *Mw, *rowmul, *colmul; // rowmul/colmul: per-row / per-column factors applied to T
};
__global__ void k_weights(RgView rg, FinalizeArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.nrow) {
        const double rs = a.rs[i];
        double wM, mul = 1.0;
        if (a.family == FAM_AEVI) {
            if (a.correctA) {
                const double r = ratio_of(rg, a.row_key, a.row_s[i]);
                wM = r * rs;                                   // :112-115
                if (a.scale) mul = (1.0 / r) * (1.0 / rs);     // :118-122
            } else {
                wM = rs;                                       // :135-136
                if (a.scale) mul = 1.0 / rs;                   // :140
            }
        } else if (a.family == FAM_IVAE) {
            wM = rs;                                           // :201
            if (a.scale) mul = 1.0 / rs;                       // :218,228
        } else {
            if (a.correctA) {
                const double r = ratio_of(rg, a.row_key, a.row_s[i]);
                wM = r * rs;                                   // :303-304
                if (a.scale) mul = 1.0 / wM;                   // :313
            } else {
                wM = rs;                                       // :321
                if (a.scale) mul = 1.0 / rs;                   // :324
            }
        }
        a.wM[i] = wM;
        a.rowmul[i] = mul;
    }
    if (i < a.ncol) {
        const double cs = a.cs[i];
        double Mw = cs, cm = 1.0;                              // :100, :226, :322
        if (a.correctA && a.family != FAM_AEVI) {
            const double r = ratio_of(rg, a.col_key, a.col_s[i]);
            Mw = r * cs;                                       // :214-215, :309-310
            cm = r;                                            // * sApvA, :220,223,315,317
        }
        a.Mw[i] = Mw;
        a.colmul[i] = cm;
    }
}
// M = [diag(rowmul)] * T [* diag(colmul)], each product separately rounded, in the reference's order
__global__ void k_scale(const int32_t *__restrict__ row, const int32_t *__restrict__ col, double *__restrict__ val,
                        long nnz, const double *__restrict__ rowmul, const double *__restrict__ colmul,
                        int apply_row, int apply_col) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nnz) return;
    double v = val[u];
    if (apply_row) v = rowmul[row[u]] * v;
    if (apply_col) v = v * colmul[col[u]];
    val[u] = v;
}

// ---- bands for the rowdual apply kernel (spmm.hip) -----------------------------------------------
// An ice cell between two elevation classes is a column of TWO rows of an E-row matrix: (cell a,
// class k) with weight 1-r and (a, k+1) with weight r.  Row by row its field value is fetched twice.
// The band structure lists every (GCM cell, ice cell) pair ONCE, in the lower row, with both weights:
// band r = the entries of row r that are not the upper partner of an entry of the row below, in CSR
// order (columns ascending); an upper partner is attached to its lower entry.  Pairing is decided per
// column from its few entries (per-column slots of the short-column path): within one GCM cell,
// classes pair up from the lowest (k, k+1), so the partner row of a band is always the same row.
// A filtered copy of the CSR: no sorting, exact copies of M's values.
__device__ __forceinline__ void e_decode(const RgView &rg, int64_t e, long &a, long &hc) {
    HcIndexing{rg.sA, rg.sHC}.split<true>(e, a, hc);      // (a regridder's strides are checked when it is made)
}
__global__ void k_band_roles(RgView rg, const int64_t *__restrict__ row_s, const uint32_t *__restrict__ colptr, int ncol,
                             const int32_t *__restrict__ lrow, const uint32_t *__restrict__ lidx,
                             uint32_t *__restrict__ lower, int32_t *__restrict__ partner) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncol) return;
    const uint32_t b = colptr[c], e = colptr[c + 1];
    for (uint32_t i = b; i < e; ++i) {
        long ai, hi;
        e_decode(rg, row_s[lrow[i]], ai, hi);
        // number of consecutive classes directly below this entry in the same GCM cell: odd -> upper partner
        int below = 0;
        int32_t up = -1;                       // the entry one class above (its partner if this one is a lower entry)
        for (long t = hi - 1;; --t) {
            bool found = false;
            for (uint32_t j = b; j < e && !found; ++j) {
                long aj, hj;
                e_decode(rg, row_s[lrow[j]], aj, hj);
                found = aj == ai && hj == t;
            }
            if (!found) break;
            ++below;
        }
        for (uint32_t j = b; j < e; ++j) {
            long aj, hj;
            e_decode(rg, row_s[lrow[j]], aj, hj);
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
// colptr/lrow/lidx: the per-column slots built for the column sums.  *d_total receives the number of band entries: the caller
// reads it back into Bands::n.
static Bands build_bands(const ibh_weighted *w, const RgView &rg, const int64_t *row_s, const int32_t *row, const uint32_t *colptr,
                        const int32_t *lrow, const uint32_t *lidx, uint32_t *d_total, hipStream_t st) {
    Arena &A = arena();
    const int T = 256;
    const int nrow = w->nrow, ncol = w->ncol;
    const long nnz = w->nnz;
    uint32_t *lower = A.get<uint32_t>((size_t)nnz), *dpos = A.get<uint32_t>((size_t)nnz);
    int32_t *partner = A.get<int32_t>((size_t)nnz);
    hipLaunchKernelGGL(k_band_roles, dim3(ceil_div(ncol, T)), dim3(T), 0, st, rg, row_s, colptr, ncol, lrow, lidx, lower, partner);
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

// ---- smoothing (sigma != 0): M <- smoothI * M  (smoother.cpp:8-99, RegridMatrices_Dynamic.cpp:237-248) ------
// smoothI[i,j] = exp(-.5 d2(i,j)) * area_j / sum_j(...) over the unmasked ice cells j of dimI with
// d2 = sum_k ((c_j[k]-c_i[k])/sigma[k])^2 < 4, c = (x, y, elevation), area = wM.  The reference finds
// neighbours with an RTree; here: uniform bins a margin wider than 2*sigma_x x 2*sigma_y (smooth_plan.h), 3x3 bins searched per cell.
// Everything downstream reuses the assembly machinery: neighbour triplets -> sort by (i,j) -> row
// denominators (sequential) -> products with the rows of M as contributions -> sort by (i,a) ->
// sequential sums.  exp() is the device library's: entries agree with the oracle to rounding, not bitwise.
struct SmoothView {
    const int64_t *row_s;       // dense ice id -> sparse
    const double *em, *cen, *area;
    int n;                      // dense ice cells
    double sx, sy, sz, x0, y0, bw, bh;
    int nbx, nby;
};
__device__ __forceinline__ bool smooth_tuple(const SmoothView &v, int d, double c[3]) {
    const int64_t s = v.row_s[d];
    const double e = v.em[s];
    if (e != e) return false;               // masked cells are not tuples (smoother.cpp:83-84)
    c[0] = v.cen[2 * s]; c[1] = v.cen[2 * s + 1]; c[2] = e;
    return true;
}
__device__ __forceinline__ int smooth_bin(const SmoothView &v, const double c[3]) {
    int bx = (int)((c[0] - v.x0) / v.bw), by = (int)((c[1] - v.y0) / v.bh);
    bx = bx < 0 ? 0 : bx >= v.nbx ? v.nbx - 1 : bx;
    by = by < 0 ? 0 : by >= v.nby ? v.nby - 1 : by;
    return by * v.nbx + bx;
}
// bad: SMOOTH_NO_BAD unless an unmasked row has no area; bad_cell: the smallest SPARSE index of such a row -- the reference walks the
// cells in ascending index and names the first (smoother.cpp:83-90); dense rows are numbered first-seen, in another order
__global__ void k_smooth_bin_count(SmoothView v, uint32_t *__restrict__ bincnt, int *__restrict__ bad, unsigned long long *__restrict__ bad_cell) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= v.n) return;
    double c[3];
    if (!smooth_tuple(v, d, c)) return;
    if (v.area[d] == 0.0) {                           // "Area of cell %ld must be non-zero", smoother.cpp:89-90
        atomicMin(bad, d);
        atomicMin(bad_cell, (unsigned long long)v.row_s[d]);
    }
    atomicAdd(&bincnt[smooth_bin(v, c)], 1u);
}
// the members of every bin in ascending dense row: key = bin (nbins: masked, sorted past the last bin), value = row, ordered by
// the stable radix sort.  The direct and tile forms sum in member order, so the order must not depend on atomics: with it, every
// build -- on one rank or shared by several -- gives the same bits.
__global__ void k_smooth_bin_keys(SmoothView v, uint32_t nbins, uint64_t *__restrict__ keys, uint32_t *__restrict__ rows) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= v.n) return;
    double c[3];
    keys[d] = smooth_tuple(v, d, c) ? (uint64_t)smooth_bin(v, c) : (uint64_t)nbins;
    rows[d] = (uint32_t)d;
}
// pass 0: count neighbours of cell d; pass 1: emit (d<<32|j, w) at off[d]
template <int PASS>
__global__ void k_smooth_neighbours(SmoothView v, const uint32_t *__restrict__ binstart, const int32_t *__restrict__ members,
                                    uint32_t *__restrict__ cnt, const uint32_t *__restrict__ off,
                                    uint64_t *__restrict__ keys, uint32_t *__restrict__ idx, double *__restrict__ wraw) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= v.n) return;
    double c[3];
    uint32_t n = 0;
    if (smooth_tuple(v, d, c)) {
        const int b = smooth_bin(v, c), bx = b % v.nbx, by = b / v.nbx;
        const uint32_t o = PASS ? off[d] : 0;
        for (int yy = max(by - 1, 0); yy <= min(by + 1, v.nby - 1); ++yy)
            for (int xx = max(bx - 1, 0); xx <= min(bx + 1, v.nbx - 1); ++xx) {
                const int bb = yy * v.nbx + xx;
                for (uint32_t q = binstart[bb]; q < binstart[bb + 1]; ++q) {
                    const int j = members[q];
                    double cj[3];
                    (void)smooth_tuple(v, j, cj);
                    const double d0 = (cj[0] - c[0]) / v.sx, d1 = (cj[1] - c[1]) / v.sy, d2 = (cj[2] - c[2]) / v.sz;
                    double nds = 0;
                    nds = nds + d0 * d0; nds = nds + d1 * d1; nds = nds + d2 * d2;      // smoother.cpp:29-33
                    if (nds < 4.0) {                                                      // nsigma^2
                        if (PASS) {
                            keys[o + n] = ((uint64_t)(uint32_t)d << 32) | (uint32_t)j;
                            idx[o + n] = o + n;
                            wraw[o + n] = exp(-.5 * nds) * v.area[j];                     // :35-36
                        }
                        ++n;
                    }
                }
            }
    }
    if (!PASS) cnt[d] = n;
}
__global__ void k_smooth_rowptr(const uint32_t *__restrict__ off, int n, uint32_t total, int32_t *__restrict__ rowptr) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d < n) rowptr[d] = (int32_t)off[d];
    if (d == 0) rowptr[n] = (int32_t)total;
}
// number of M entries each smoothing entry (i,j) multiplies = length of row j of M
__global__ void k_smooth_prod_count(const uint64_t *__restrict__ skeys, size_t ns, const int32_t *__restrict__ rowptr,
                                    uint32_t *__restrict__ cnt) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= ns) return;
    const int j = (int)(skeys[q] & 0xffffffffu);
    cnt[q] = (uint32_t)(rowptr[j + 1] - rowptr[j]);
}
__global__ void k_smooth_prod_emit(const uint64_t *__restrict__ skeys, const uint32_t *__restrict__ sidx,
                                   const double *__restrict__ wraw, const double *__restrict__ denom, size_t ns,
                                   const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colind,
                                   const double *__restrict__ val, const uint32_t *__restrict__ pos,
                                   uint64_t *__restrict__ keys, uint32_t *__restrict__ idx, double *__restrict__ term) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= ns) return;
    const uint64_t k = skeys[q];
    const int i = (int)(k >> 32), j = (int)(k & 0xffffffffu);
    const double factor = 1.0 / denom[i];
    const double s = factor * wraw[sidx[q]];                     // factor * ii->second, smoother.cpp:62-64
    uint32_t p = pos[q];
    for (int e = rowptr[j]; e < rowptr[j + 1]; ++e, ++p) {
        keys[p] = ((uint64_t)(uint32_t)i << 32) | (uint32_t)colind[e];
        idx[p] = p;
        term[p] = s * val[e];
    }
}

// ---- smoothI * M without the triplets (round 2) ---------------------------------------------------------------------
// The pipeline below materialises smoothI (~10^8 neighbour triplets at 5 km) and the ~2 x 10^8 products, and sorts both.
// Row i of smoothI * M touches only the few columns its neighbours' rows of M hold (GCM cells / elevation classes within
// two sigmas), so ONE WAVE computes it directly: pass 1 walks the candidates of the 3 x 3 bins (three contiguous member
// ranges), sums the denominator and collects the distinct columns in a small LDS hash set; the set is ranked (ascending
// columns = the CSR order); pass 2 walks the candidates again, parks the hits (j, w_ij / denom) in LDS and lets lane c
// accumulate column c over the hit list, every lane reading the same rows of M (broadcast loads).  Sums run in candidate
// order instead of ascending j: entries agree with the triplet pipeline to rounding (the smoothing test's tolerance: the
// reference's RTree order is not reproducible either); the structure is identical.  Rows with more than SMD_MAXCOL columns
// send the build to the triplet pipeline.
// (SMD_HASH, SMD_MAXCOL, SMD_HITS, SMD_WAVES: smooth_plan.h)
__device__ __forceinline__ double smd_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
template <bool EMIT>
__global__ __launch_bounds__(SMD_WAVES * 64) void k_smooth_direct(SmoothView v, const uint32_t *__restrict__ binstart, const int32_t *__restrict__ members,
                                                                  const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colind,
                                                                  const double *__restrict__ val, uint32_t *__restrict__ rowlen,
                                                                  const int32_t *__restrict__ orowptr, int32_t *__restrict__ ocol,
                                                                  double *__restrict__ oval, uint32_t *__restrict__ overflow) {
    __shared__ int s_hash[SMD_WAVES][SMD_HASH];
    __shared__ int s_cols[SMD_WAVES][SMD_MAXCOL];
    __shared__ int s_hj[EMIT ? SMD_WAVES : 1][EMIT ? SMD_HITS : 1];
    __shared__ double s_hw[EMIT ? SMD_WAVES : 1][EMIT ? SMD_HITS : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * SMD_WAVES + wave;
    if (i >= v.n) return;
    double ci[3];
    if (!smooth_tuple(v, i, ci)) {                   // a masked cell is no tuple: an empty row
        if (!EMIT && lane == 0) rowlen[i] = 0;
        return;
    }
    int *hk = s_hash[wave];
    for (int q = lane; q < SMD_HASH; q += 64) hk[q] = -1;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int b = smooth_bin(v, ci), bx = b % v.nbx, by = b / v.nbx;
    const int x0 = max(bx - 1, 0), x1 = min(bx + 1, v.nbx - 1), y0 = max(by - 1, 0), y1 = min(by + 1, v.nby - 1);
    // weight of candidate j, < 0: not a neighbour (smoother.cpp:29-36)
    auto weight = [&](int j) {
        double cj[3];
        (void)smooth_tuple(v, j, cj);
        const double d0 = (cj[0] - ci[0]) / v.sx, d1 = (cj[1] - ci[1]) / v.sy, d2 = (cj[2] - ci[2]) / v.sz;
        double nds = 0;
        nds = nds + d0 * d0; nds = nds + d1 * d1; nds = nds + d2 * d2;
        return nds < 4.0 ? exp(-.5 * nds) * v.area[j] : -1.0;
    };
    // ---- pass 1: denominator and the set of columns
    double dpart = 0.0;
    for (int yy = y0; yy <= y1; ++yy) {
        const uint32_t qb = binstart[yy * v.nbx + x0], qe = binstart[yy * v.nbx + x1 + 1];
        for (uint32_t q = qb + lane; q < qe; q += 64) {
            const int j = members[q];
            const double wgt = weight(j);
            if (wgt >= 0.0) {
                dpart += wgt;
                for (int e = rowptr[j]; e < rowptr[j + 1]; ++e) {
                    const int c = colind[e];
                    unsigned h = ((unsigned)c * 2654435761u) >> 24;
                    for (int probe = 0; probe < SMD_HASH; ++probe) {
                        const int old = atomicCAS(&hk[h], -1, c);
                        if (old == -1 || old == c) break;
                        h = (h + 1) & (SMD_HASH - 1);
                    }
                }
            }
        }
    }
    const double denom = smd_wave_sum(dpart);
    // the set, compacted (slot order) and ranked (ascending)
    int *cols = s_cols[wave];
    int mykeys[SMD_HASH / 64], nk = 0;
    int K = 0;
#pragma unroll
    for (int r = 0; r < SMD_HASH / 64; ++r) {
        const int k = hk[r * 64 + lane];
        const unsigned long long m = __ballot(k >= 0);
        mykeys[r] = k;
        K += __popcll(m);
        (void)nk;
    }
    if (K > SMD_MAXCOL) {                            // (also a full hash table: K == SMD_HASH)
        if (lane == 0) { atomicOr(overflow, 1u); if (!EMIT) rowlen[i] = 0; }
        return;
    }
    if (!EMIT) { if (lane == 0) rowlen[i] = (uint32_t)K; return; }
    // rank of a key = number of smaller keys in the table (keys are distinct)
#pragma unroll
    for (int r = 0; r < SMD_HASH / 64; ++r) {
        const int k = mykeys[r];
        if (k >= 0) {
            int rank = 0;
            for (int q = 0; q < SMD_HASH; ++q) { const int o = hk[q]; rank += (o >= 0 && o < k) ? 1 : 0; }
            cols[rank] = k;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int c0 = lane < K ? cols[lane] : -2, c1 = 64 + lane < K ? cols[64 + lane] : -2;
    double a0 = 0.0, a1 = 0.0;
    const double factor = 1.0 / denom;                // smoother.cpp:62
    int *hj = s_hj[wave];
    double *hw = s_hw[wave];
    int nh = 0;
    auto drain = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int h = 0; h < nh; ++h) {
            const int j = hj[h];
            const double sc = hw[h];
            for (int e = rowptr[j]; e < rowptr[j + 1]; ++e) {
                const int c = colind[e];
                const double t = sc * val[e];
                if (c == c0) a0 = a0 + t;
                else if (c == c1) a1 = a1 + t;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        nh = 0;
    };
    // ---- pass 2: the hits, parked SMD_HITS at a time, accumulated column by lane
    for (int yy = y0; yy <= y1; ++yy) {
        const uint32_t qb = binstart[yy * v.nbx + x0], qe = binstart[yy * v.nbx + x1 + 1];
        for (uint32_t qq = qb; qq < qe; qq += 64) {
            const uint32_t q = qq + lane;
            double wgt = -1.0;
            int j = 0;
            if (q < qe) { j = members[q]; wgt = weight(j); }
            const unsigned long long m = __ballot(wgt >= 0.0);
            if (nh + 64 > SMD_HITS) drain();
            if (wgt >= 0.0) {
                const int pos = nh + __popcll(m & ((1ull << lane) - 1ull));
                hj[pos] = j; hw[pos] = factor * wgt;
            }
            nh += __popcll(m);
        }
    }
    drain();
    const int ob = orowptr[i];
    if (lane < K) { ocol[ob + lane] = c0; oval[ob + lane] = a0; }
    if (64 + lane < K) { ocol[ob + 64 + lane] = c1; oval[ob + 64 + lane] = a1; }
}

// ---- smoothI * M by spatial tiles (round 3): grids too large for one wave per row ---------------------------------------
// The direct kernel above lets every row walk its ~3 600 candidates alone (three passes, five gathers per candidate: 13 ms at
// 5 km); the triplet pipeline materialises ~10^8 neighbour pairs and sorts them twice (12 ms).  But the rows of one spatial bin
// share their candidates -- the members of the 3 x 3 bins around it.  So: ONE WAVE per 64 rows of a bin; the candidates are
// staged 64 at a time in LDS (compact records in bin order: position, elevation, area, and the candidate's row of M already
// translated to slots of the bin's column table) and every lane runs its own row against the staged candidate, which is
// wave-uniform: broadcast LDS reads, no gathers in the inner loop.  One pass sums the denominator and adds w_ij * M[j, c] into an
// LDS table acc[slot][lane] with ds_add_f64 (no return: nothing waits), noting the slot in a 128-bit presence mask per lane --
// row i holds column c iff a neighbour within two sigmas does, exactly the reference's structure; the sums are divided by the
// denominator at the end.  The bin's column table (the distinct columns of all members of its 3 x 3 neighbourhood, ascending) comes from a
// small pre-kernel; a compaction kernel turns (presence, table) into CSR rows.  Sums run in candidate order (bin by bin,
// member by member, the members of a bin in ascending row: k_smooth_bin_keys), fixed: reproducible; entries agree with the
// oracle's ascending-j order to rounding (the test's 1e-12).
// More than SMT_KMAX columns around a bin, or a member row of M with more than SMT_ROWMAX entries: the triplet pipeline serves
// the build.
// (SMT_KMAX, SMT_ROWMAX, SMT_HASH, SmtCand: smooth_plan.h)
// compact records in member (bin) order: position / elevation / area, and the member's row of M entry-major
// (mcol[e * nmem + q], mval[...]): the tile kernel stages them with coalesced, independent loads
// (the member positions [q0, q1): a rank of a shared build packs the candidates of its own bins only)
__global__ void k_smt_pack(SmoothView v, const int32_t *__restrict__ members, int q0, int q1, int nmem, const int32_t *__restrict__ rowptr,
                           const int32_t *__restrict__ colind, const double *__restrict__ val, SmtCand *__restrict__ cand,
                           unsigned char *__restrict__ mne, int32_t *__restrict__ mcol, double *__restrict__ mval) {
    const int q = q0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (q >= q1) return;
    const int d = members[q];
    double c[3];
    (void)smooth_tuple(v, d, c);
    cand[q] = SmtCand{c[0], c[1], c[2], v.area[d]};
    const int e0 = rowptr[d], ne = min(rowptr[d + 1] - e0, SMT_ROWMAX);
    mne[q] = (unsigned char)ne;
    for (int e = 0; e < SMT_ROWMAX; ++e) {
        mcol[(size_t)e * nmem + q] = e < ne ? colind[e0 + e] : 0;
        mval[(size_t)e * nmem + q] = e < ne ? val[e0 + e] : 0.0;
    }
}
// per bin: the distinct columns of the members of its 3 x 3 neighbourhood, ascending -> bincols[b * SMT_KMAX ..], binK[b];
// waves the bin needs (64 rows each) -> binwaves[b]
__global__ __launch_bounds__(256) void k_smt_bincols(SmoothView v, const uint32_t *__restrict__ binstart, const int32_t *__restrict__ members,
                                                     const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colind,
                                                     int32_t *__restrict__ bincols, int32_t *__restrict__ binK, uint32_t *__restrict__ binwaves,
                                                     uint32_t *__restrict__ flags) {
    __shared__ int s_hash[SMT_HASH];
    __shared__ int s_n;
    const int b = blockIdx.x, bx = b % v.nbx, by = b / v.nbx;
    const uint32_t mine = binstart[b + 1] - binstart[b];
    if (threadIdx.x == 0) { binwaves[b] = (mine + 63) / 64; s_n = 0; }
    if (mine == 0) { if (threadIdx.x == 0) binK[b] = 0; return; }
    for (int q = threadIdx.x; q < SMT_HASH; q += blockDim.x) s_hash[q] = -1;
    __syncthreads();
    const int x0 = max(bx - 1, 0), x1 = min(bx + 1, v.nbx - 1), y0 = max(by - 1, 0), y1 = min(by + 1, v.nby - 1);
    for (int yy = y0; yy <= y1; ++yy) {
        const uint32_t qb = binstart[yy * v.nbx + x0], qe = binstart[yy * v.nbx + x1 + 1];
        for (uint32_t q = qb + threadIdx.x; q < qe; q += blockDim.x) {
            const int j = members[q];
            if (rowptr[j + 1] - rowptr[j] > SMT_ROWMAX) atomicOr(flags, 2u);
            for (int e = rowptr[j]; e < rowptr[j + 1]; ++e) {
                const int c = colind[e];
                unsigned h = ((unsigned)c * 2654435761u) >> 22;
                for (int probe = 0; probe < SMT_HASH; ++probe) {
                    const int old = atomicCAS(&s_hash[h], -1, c);
                    if (old == -1) { atomicAdd(&s_n, 1); break; }
                    if (old == c) break;
                    h = (h + 1) & (SMT_HASH - 1);
                }
            }
        }
    }
    __syncthreads();
    const int K = s_n;
    if (threadIdx.x == 0) binK[b] = K;
    if (K > SMT_KMAX) { if (threadIdx.x == 0) atomicOr(flags, 1u); return; }
    for (int q = threadIdx.x; q < SMT_HASH; q += blockDim.x) {
        const int k = s_hash[q];
        if (k < 0) continue;
        int rank = 0;
        for (int t = 0; t < SMT_HASH; ++t) { const int o = s_hash[t]; rank += (o >= 0 && o < k) ? 1 : 0; }
        bincols[(size_t)b * SMT_KMAX + rank] = k;
    }
}
// wavebin[w] = the bin of wave w (wstart: exclusive scan of binwaves)
__global__ void k_smt_wavebin(const uint32_t *__restrict__ wstart, const uint32_t *__restrict__ binwaves, int nbins, int32_t *__restrict__ wavebin) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nbins) return;
    for (uint32_t k = 0; k < binwaves[b]; ++k) wavebin[wstart[b] + k] = b;
}
__global__ __launch_bounds__(64) void k_smt_tile(SmoothView v, const uint32_t *__restrict__ binstart, const int32_t *__restrict__ members,
                                                 const SmtCand *__restrict__ cand, const unsigned char *__restrict__ mne,
                                                 const int32_t *__restrict__ mcol, const double *__restrict__ mval, int nmem,
                                                 const int32_t *__restrict__ bincols, const int32_t *__restrict__ binK,
                                                 const uint32_t *__restrict__ wstart, const int32_t *__restrict__ wavebin, int w0, int kstride,
                                                 double *__restrict__ scratch, unsigned long long *__restrict__ pres, uint32_t *__restrict__ rowlen) {
    extern __shared__ double smt_mem[];
    const SmtLds at = smt_lds(kstride);                          // (the layout and its size: smooth_plan.h)
    unsigned char *const lds = reinterpret_cast<unsigned char *>(smt_mem);
    double *acc = reinterpret_cast<double *>(lds + at.acc);      // [K][64]
    SmtCand *s_c = reinterpret_cast<SmtCand *>(lds + at.s_c);    // [64]
    double *s_val = reinterpret_cast<double *>(lds + at.s_val);  // [64][SMT_ROWMAX]
    int *s_cols = reinterpret_cast<int *>(lds + at.s_cols);      // [SMT_KMAX]
    unsigned char *s_slot = lds + at.s_slot;                     // [64][SMT_ROWMAX]
    unsigned char *s_ne = lds + at.s_ne;                         // [64]
    const int w = w0 + (int)blockIdx.x, lane = threadIdx.x;       // (w0: the first wave of a rank's bins in a shared build)
    const int b = wavebin[w], bx = b % v.nbx, by = b / v.nbx;
    const int K = binK[b];
    const uint32_t q0 = binstart[b] + (uint32_t)(w - (int)wstart[b]) * 64u, qend = binstart[b + 1];
    const bool live = q0 + lane < qend;
    const SmtCand me = cand[live ? q0 + lane : qend - 1];
    for (int k = lane; k < K; k += 64) s_cols[k] = bincols[(size_t)b * SMT_KMAX + k];
    for (int k = 0; k < K; ++k) acc[k * 64 + lane] = 0.0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    const int x0 = max(bx - 1, 0), x1 = min(bx + 1, v.nbx - 1), y0 = max(by - 1, 0), y1 = min(by + 1, v.nby - 1);
    // weight of the staged candidate for this lane's row, < 0: not a neighbour (smoother.cpp:29-36).  The reference divides by
    // the sigmas; three f64 divisions per pair are most of the arithmetic here, so the distance is formed with reciprocals and
    // only a pair within 1e-9 of the cut (nds == 4: cells exactly two sigmas apart on a regular grid) repeats the reference's
    // divisions to decide on which side it falls -- the structure stays exactly the reference's, the weights differ from the
    // divided form in the last bit at most.
    const double rx = 1.0 / v.sx, ry = 1.0 / v.sy, rz = 1.0 / v.sz;
    auto weight = [&](const SmtCand &c) {
        const double d0 = (c.x - me.x) * rx, d1 = (c.y - me.y) * ry, d2 = (c.z - me.z) * rz;
        double nds = 0;
        nds = nds + d0 * d0; nds = nds + d1 * d1; nds = nds + d2 * d2;
        bool in = nds < 4.0;
        if (fabs(nds - 4.0) < 1e-9) {
            const double e0 = (c.x - me.x) / v.sx, e1 = (c.y - me.y) / v.sy, e2 = (c.z - me.z) / v.sz;
            double ex = 0;
            ex = ex + e0 * e0; ex = ex + e1 * e1; ex = ex + e2 * e2;
            in = ex < 4.0;
        }
        return in ? exp(-.5 * nds) * c.area : -1.0;
    };
    // ONE pass: the denominator and the unnormalised sums together (the reference multiplies every term by factor = 1 / denom
    // first, smoother.cpp:62-64; factoring it out of the sum changes the rounding, not the value: the test's 1e-12)
    double denom = 0.0;
    unsigned long long p0 = 0ull, p1 = 0ull;
    for (int yy = y0; yy <= y1; ++yy) {
        const uint32_t qb = binstart[yy * v.nbx + x0], qe = binstart[yy * v.nbx + x1 + 1];
        // the records of chunk c+1 are loaded (coalesced, independent: one round trip) while chunk c is consumed
        auto fetch = [&](uint32_t qq, SmtCand &fc, int &fne, int &c0, int &c1, double &a0, double &a1) {
            const uint32_t q = min(qq + (uint32_t)lane, qe - 1);
            fc = cand[q]; fne = mne[q]; c0 = mcol[q]; c1 = mcol[(size_t)nmem + q]; a0 = mval[q]; a1 = mval[(size_t)nmem + q];
        };
        SmtCand fc; int fne, fc0, fc1; double fa0, fa1;
        if (qb < qe) fetch(qb, fc, fne, fc0, fc1, fa0, fa1);
        for (uint32_t qq = qb; qq < qe; qq += 64) {
            const int nst = (int)min(64u, qe - qq);
            __builtin_amdgcn_wave_barrier();                     // the previous chunk has been consumed
            auto slot_of = [&](int c) {                          // the column is in the bin's table by construction
                int lo = 0, hi = K - 1;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_cols[mid] < c) lo = mid + 1; else hi = mid; }
                return lo;
            };
            if (lane < nst) {
                s_c[lane] = fc;
                s_ne[lane] = (unsigned char)fne;
                if (fne > 0) { s_slot[lane * SMT_ROWMAX] = (unsigned char)slot_of(fc0); s_val[lane * SMT_ROWMAX] = fa0; }
                if (fne > 1) { s_slot[lane * SMT_ROWMAX + 1] = (unsigned char)slot_of(fc1); s_val[lane * SMT_ROWMAX + 1] = fa1; }
                for (int e = 2; e < fne; ++e) {                  // (an ice cell under several GCM cells: rare)
                    s_slot[lane * SMT_ROWMAX + e] = (unsigned char)slot_of(mcol[(size_t)e * nmem + qq + lane]);
                    s_val[lane * SMT_ROWMAX + e] = mval[(size_t)e * nmem + qq + lane];
                }
            }
            if (qq + 64 < qe) fetch(qq + 64, fc, fne, fc0, fc1, fa0, fa1);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            for (int t = 0; t < nst; ++t) {
                const double wgt = weight(s_c[t]);
                const bool hit = live && wgt >= 0.0;
                if (hit) denom += wgt;
                const int ne = s_ne[t];
                for (int e = 0; e < ne; ++e) {                   // (wave-uniform: every lane looks at the same candidate)
                    const int k = s_slot[t * SMT_ROWMAX + e];
                    if (hit) {
                        __hip_atomic_fetch_add(acc + k * 64 + lane, wgt * s_val[t * SMT_ROWMAX + e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (k < 64) p0 |= 1ull << k; else p1 |= 1ull << (k - 64);
                    }
                }
            }
        }
    }
    const double factor = live ? 1.0 / denom : 0.0;              // smoother.cpp:62
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    for (int k = 0; k < K; ++k) scratch[((size_t)w * kstride + k) * 64 + lane] = factor * acc[k * 64 + lane];
    if (live) {
        pres[2 * (size_t)(q0 + lane)] = p0; pres[2 * (size_t)(q0 + lane) + 1] = p1;
        rowlen[members[q0 + lane]] = (uint32_t)(__popcll(p0) + __popcll(p1));
    }
}
// rows of the member positions [q0, q1) -> at orowptr[row] (mpos == nullptr), or packed in member order at mpos[q] (a shared build)
__global__ void k_smt_emit(const uint32_t *__restrict__ binstart, const int32_t *__restrict__ members, int q0, int q1, const uint32_t *__restrict__ wstart,
                           const int32_t *__restrict__ memberbin, const int32_t *__restrict__ bincols, int kstride, const double *__restrict__ scratch,
                           const unsigned long long *__restrict__ pres, const int32_t *__restrict__ orowptr, const uint32_t *__restrict__ mpos,
                           int32_t *__restrict__ ocol, double *__restrict__ oval) {
    const int q = q0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (q >= q1) return;
    const int b = memberbin[q];
    const uint32_t rel = (uint32_t)q - binstart[b];
    const size_t w = wstart[b] + rel / 64;
    const int lane = (int)(rel & 63u);
    int o = mpos ? (int)mpos[q] : orowptr[members[q]];
    for (int half = 0; half < 2; ++half) {
        unsigned long long m = pres[2 * (size_t)q + half];
        while (m) {
            const int k = __builtin_ctzll(m) + 64 * half;
            m &= m - 1;
            ocol[o] = bincols[(size_t)b * SMT_KMAX + k];
            oval[o] = scratch[(w * kstride + k) * 64 + lane];
            ++o;
        }
    }
}
// bin of every member position (for the compaction kernel)
__global__ void k_smt_memberbin(const uint32_t *__restrict__ binstart, int nbins, int32_t *__restrict__ memberbin) {
    const int b = blockIdx.x;
    for (uint32_t q = binstart[b] + threadIdx.x; q < binstart[b + 1]; q += blockDim.x) memberbin[q] = b;
}
// ---- the tile form shared by the ranks of a communicator: rank k smooths the rows of a contiguous range of bins, the rows
// travel in member order (positions [binstart[b0], binstart[b1]) of the bins' members), every rank places them into the CSR
// row lengths of this rank's member positions [q0, q1), in member order
__global__ void k_smt_mlen(const int32_t *__restrict__ members, int q0, int q1, const uint32_t *__restrict__ rowlen, uint32_t *__restrict__ mlen) {
    const int q = q0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (q < q1) mlen[q] = rowlen[members[q]];
}
// ... and back by row, for all members (rows of masked cells stay empty)
__global__ void k_smt_rowlen(const int32_t *__restrict__ members, int nmem, const uint32_t *__restrict__ mlen, uint32_t *__restrict__ rowlen) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nmem) rowlen[members[q]] = mlen[q];
}
// the row of member q, packed at mptr[q], to its place in the CSR
__global__ void k_smt_place(const int32_t *__restrict__ members, int nmem, const uint32_t *__restrict__ mlen, const uint32_t *__restrict__ mptr,
                            const int32_t *__restrict__ orowptr, const int32_t *__restrict__ pcol, const double *__restrict__ pval,
                            int32_t *__restrict__ ocol, double *__restrict__ oval) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nmem) return;
    const uint32_t s = mptr[q], len = mlen[q];
    const int o = orowptr[members[q]];
    for (uint32_t e = 0; e < len; ++e) { ocol[o + e] = pcol[s + e]; oval[o + e] = pval[s + e]; }
}

static void smooth_check(const ibh_regrid_matrices *rm, const double sigma[3]) {
    IBH_CHECK(rm->rg->has_centroid, "smoothing (sigma != 0) needs the ice grid's centroid_xy (ibh_regridder_desc.I_centroid_xy)");
    IBH_CHECK(sigma[0] > 0 && sigma[1] > 0 && sigma[2] > 0, "smoothing needs three positive sigmas, got (%g, %g, %g)", sigma[0], sigma[1], sigma[2]);
}
// ---- the smoothed build on the host: smooth_matrix (below) takes the plan (smooth_plan.h), bins the rows and tries the plan's forms in
// order; a form builds a new CSR beside the one it reads and returns false, with nothing touched, when its tables overflow
constexpr int SMOOTH_NO_BAD = 0x7fffffff;
struct SmoothBins {
    SmoothView v;
    size_t nbins;
    const uint32_t *binstart;   // [nbins + 1]: the bins' first member positions
    const int32_t *members;     // [binstart[nbins]] unmasked rows, bin by bin, ascending in a bin
    uint32_t *d_cnt;            // four words a form reads back at once: three of its own, and the smallest dense row whose area is zero
                                // (SMOOTH_NO_BAD: none); behind them, read only on that failure:
    const unsigned long long *bad_cell;     // the smallest sparse index of a row whose area is zero
};
struct SmoothedCsr {
    DevBuf<int32_t> rowptr, colind;
    DevBuf<double> val;
    int64_t nnz = 0;
    bool shared = false;        // the ranks of a communicator built it together
};
// "Area of cell %ld must be non-zero", smoother.cpp:89-90: d = the fourth counter word, as a form's first read-back brought it; the
// cell named is the reference's, the one with the smallest index
static void fail_zero_area(const SmoothBins &B, int d) {
    if (d == SMOOTH_NO_BAD) return;
    unsigned long long sc = 0;
    IBH_HIP(hipMemcpy(&sc, B.bad_cell, sizeof(sc), hipMemcpyDeviceToHost));
    fail(IBH_EINVAL, "Area of cell %ld must be non-zero", (long)sc);
}
// bin count -> scan -> keys -> sort
static SmoothBins smooth_bins(const ibh_weighted *w, const ibh_regrid_matrices *rm, const int64_t *row_s, const SmoothGrid &sg,
                              const double sigma[3], hipStream_t st) {
    const ibh_regridder *g = rm->rg;
    Arena &A = arena();
    const int T = 256, n = w->nrow;
    SmoothBins B{};
    B.v = SmoothView{row_s, rm->elevmaskI.p, g->I_centroid.p, w->wM.p, n, sigma[0], sigma[1], sigma[2], sg.x0, sg.y0, sg.bw, sg.bh, sg.nbx, sg.nby};
    B.nbins = sg.nbins();
    const size_t nbins = B.nbins;
    uint32_t *binstart = A.get<uint32_t>(nbins + 1);
    uint64_t *bkeys = A.get<uint64_t>((size_t)n), *bkeys2 = A.get<uint64_t>((size_t)n);
    uint32_t *brows = A.get<uint32_t>((size_t)n), *brows2 = A.get<uint32_t>((size_t)n);
    B.d_cnt = A.get<uint32_t>(6);                   // (the arena aligns to 256 bytes: words 4, 5 hold a 64-bit value)
    int *d_bad = reinterpret_cast<int *>(B.d_cnt + 3);
    unsigned long long *d_bad_cell = reinterpret_cast<unsigned long long *>(B.d_cnt + 4);
    B.bad_cell = d_bad_cell;
    const int big = SMOOTH_NO_BAD;
    IBH_HIP(hipMemsetAsync(binstart, 0, sizeof(uint32_t) * (nbins + 1), st));
    IBH_HIP(hipMemcpyAsync(d_bad, &big, sizeof(int), hipMemcpyHostToDevice, st));
    IBH_HIP(hipMemsetAsync(d_bad_cell, 0xff, sizeof(unsigned long long), st));
    const dim3 grid(ceil_div(n, T));
    hipLaunchKernelGGL(k_smooth_bin_count, grid, dim3(T), 0, st, B.v, binstart, d_bad, d_bad_cell);
    exclusive_scan_u32(binstart, binstart, nbins + 1, nullptr, st);
    hipLaunchKernelGGL(k_smooth_bin_keys, grid, dim3(T), 0, st, B.v, (uint32_t)nbins, bkeys, brows);
    const KeyField bf{0, bits_for((uint64_t)nbins + 1)};
    if (bf.nbits > 0 && radix_sort_pairs(bkeys, bkeys2, brows, brows2, (size_t)n, &bf, 1, st)) std::swap(brows, brows2);
    B.binstart = binstart;
    B.members = reinterpret_cast<const int32_t *>(brows);
    return B;
}

// ---- the tile form (k_smt_*): column tables per bin -> one wave per 64 rows of a bin -> compaction ------------------------------------
struct SmtBuild {               // what the steps of the tile form share
    int32_t *bincols, *binK;
    uint32_t *binwaves, *wstart;
    int nwaves, nmem, kmax;     // waves and members of all bins (the members = the unmasked rows), the widest column table
    uint32_t *rowlen;
    SmtCand *cand;
    int32_t *wavebin, *memberbin;
    double *scratch;
    unsigned long long *pres;
    unsigned char *mne;
    int32_t *mcol;
    double *mval;
};
// the column tables, the waves per bin and the overflow flags; the first read-back.  world > 1: the flag is taken by all ranks
// together (it is a whole-grid quantity: equal anyway).  false: more than SMT_KMAX columns around a bin, or a member row longer than
// SMT_ROWMAX
static bool smt_tables(const SmoothBins &B, const ibh_weighted *w, ibh_comm *comm, hipStream_t st, SmtBuild *t) {
    Arena &A = arena();
    const size_t nbins = B.nbins;
    uint32_t h4[4];
    IBH_HIP(hipMemsetAsync(B.d_cnt, 0, 3 * sizeof(uint32_t), st));
    t->bincols = A.get<int32_t>(nbins * SMT_KMAX); t->binK = A.get<int32_t>(nbins);
    t->binwaves = A.get<uint32_t>(nbins + 1); t->wstart = A.get<uint32_t>(nbins + 1);
    hipLaunchKernelGGL(k_smt_bincols, dim3((int)nbins), dim3(256), 0, st, B.v, B.binstart, B.members, w->rowptr.p, w->colind.p, t->bincols, t->binK,
                       t->binwaves, B.d_cnt + 1);
    exclusive_scan_u32(t->binwaves, t->wstart, nbins, B.d_cnt, st);
    IBH_HIP(hipMemcpyAsync(B.d_cnt + 2, B.binstart + nbins, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    readback_sync(h4, B.d_cnt, sizeof(h4), st);
    fail_zero_area(B, (int)h4[3]);
    if (comm && comm_world(comm) > 1) {
        const int world = comm_world(comm);
        double *d_fl = A.get<double>((size_t)world);
        const double mine = (double)h4[1];
        IBH_HIP(hipMemcpyAsync(d_fl + comm_rank(comm), &mine, sizeof(double), hipMemcpyHostToDevice, st));
        comm_exchange_blocks(comm, d_fl, 1, 1, st);
        std::vector<double> fl((size_t)world);
        readback_sync(fl.data(), d_fl, sizeof(double) * (size_t)world, st);
        for (double f : fl) h4[1] |= (uint32_t)f;
    }
    if (h4[1] != 0) return false;
    t->nwaves = (int)h4[0]; t->nmem = (int)h4[2];
    std::vector<int32_t> hK(nbins);
    IBH_HIP(hipMemcpy(hK.data(), t->binK, sizeof(int32_t) * nbins, hipMemcpyDeviceToHost));
    t->kmax = 1;
    for (size_t q = 0; q < nbins; ++q) t->kmax = std::max(t->kmax, hK[q]);
    return true;
}
// the kernel's dynamic-LDS limit is raised once per device, when a build first needs more than the default
static void smt_raise_lds_limit(int device, size_t lds) {
    static std::mutex mu;
    static bool raised[64] = {};
    if (lds <= 64 * 1024) return;
    std::lock_guard<std::mutex> lk(mu);
    if (raised[device & 63]) return;
    IBH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_smt_tile), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SMT_LDS_RAISED));
    raised[device & 63] = true;
}
// pack the candidates of a share and run its waves
static void smt_run_share(const SmoothBins &B, const ibh_weighted *w, const SmtBuild &t, const SmtShare &s, hipStream_t st) {
    if (!t.nmem) return;
    const int T = 256, nb = (int)B.nbins;
    if (s.c1 > s.c0)
        hipLaunchKernelGGL(k_smt_pack, dim3(ceil_div(s.c1 - s.c0, T)), dim3(T), 0, st, B.v, B.members, s.c0, s.c1, t.nmem, w->rowptr.p, w->colind.p, w->val.p,
                           t.cand, t.mne, t.mcol, t.mval);
    hipLaunchKernelGGL(k_smt_wavebin, dim3(ceil_div(nb, T)), dim3(T), 0, st, t.wstart, t.binwaves, nb, t.wavebin);
    hipLaunchKernelGGL(k_smt_memberbin, dim3(nb), dim3(64), 0, st, B.binstart, nb, t.memberbin);
    const size_t lds = smt_lds(t.kmax).total;
    smt_raise_lds_limit(w->device, lds);
    if (s.w1 > s.w0)
        hipLaunchKernelGGL(k_smt_tile, dim3(s.w1 - s.w0), dim3(64), lds, st, B.v, B.binstart, B.members, t.cand, t.mne, t.mcol, t.mval, t.nmem, t.bincols,
                           t.binK, t.wstart, t.wavebin, s.w0, t.kmax, t.scratch, t.pres, t.rowlen);
}
// one rank: row lengths -> row pointer (the second read-back: nnz) -> the rows
static void smt_collect(const SmoothBins &B, const SmtBuild &t, hipStream_t st, SmoothedCsr *out) {
    const int T = 256, n = B.v.n;
    uint32_t h4[4];
    exclusive_scan_u32(t.rowlen, reinterpret_cast<uint32_t *>(out->rowptr.p), (size_t)n, B.d_cnt, st);
    readback_sync(h4, B.d_cnt, sizeof(h4), st);
    const uint32_t nnz2 = h4[0];
    IBH_CHECK(nnz2 < (1u << 31), "smoothed matrix too large (%u entries)", nnz2);
    IBH_HIP(hipMemcpyAsync(out->rowptr.p + n, B.d_cnt, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    out->colind.alloc((size_t)nnz2); out->val.alloc((size_t)nnz2);
    if (t.nmem) hipLaunchKernelGGL(k_smt_emit, dim3(ceil_div(t.nmem, T)), dim3(T), 0, st, B.binstart, B.members, 0, t.nmem, t.wstart, t.memberbin, t.bincols, t.kmax,
                                   t.scratch, t.pres, out->rowptr.p, (const uint32_t *)nullptr, out->colind.p, out->val.p);
    out->nnz = nnz2;
}
// several ranks: every rank's rows reach every rank -- the row lengths in member order (gatherv) -> the row pointer and the
// member-order offsets (scans) -> the rows packed in member order (gatherv) -> placed into the CSR.  ms: smt_member_starts
static void smt_collect_ranks(const SmoothBins &B, const SmtBuild &t, const SmtShare &s, const std::vector<uint32_t> &ms, ibh_comm *comm, hipStream_t st,
                              SmoothedCsr *out) {
    Arena &A = arena();
    const int T = 256, n = B.v.n, nmem = t.nmem;
    const size_t nr = ms.size();        // world + 1
    uint32_t *mlen = A.get<uint32_t>((size_t)nmem + 1), *mptr = A.get<uint32_t>((size_t)nmem + 1);
    if (s.m1 > s.m0) hipLaunchKernelGGL(k_smt_mlen, dim3(ceil_div(s.m1 - s.m0, T)), dim3(T), 0, st, B.members, s.m0, s.m1, t.rowlen, mlen);
    {
        const std::vector<int64_t> ol = smt_gather_offsets(ms, 4);
        void *bases[1] = {mlen};
        const int64_t *offs[1] = {ol.data()};
        comm_gatherv(comm, 1, bases, offs, st);
    }
    if (nmem) hipLaunchKernelGGL(k_smt_rowlen, dim3(ceil_div(nmem, T)), dim3(T), 0, st, B.members, nmem, mlen, t.rowlen);
    exclusive_scan_u32(t.rowlen, reinterpret_cast<uint32_t *>(out->rowptr.p), (size_t)n, B.d_cnt, st);
    exclusive_scan_u32(mlen, mptr, (size_t)nmem, mptr + nmem, st);
    IBH_HIP(hipMemcpyAsync(out->rowptr.p + n, B.d_cnt, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    std::vector<uint32_t> hp(nr);       // the packed rows of rank r start at hp[r]; hp[world] = nnz
    for (size_t r = 0; r < nr; ++r) IBH_HIP(hipMemcpyAsync(&hp[r], mptr + ms[r], sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    IBH_HIP(hipStreamSynchronize(st));
    const uint32_t nnz2 = hp[nr - 1];
    IBH_CHECK(nnz2 < (1u << 31), "smoothed matrix too large (%u entries)", nnz2);
    DevBuf<int32_t> pcol((size_t)nnz2);
    DevBuf<double> pval((size_t)nnz2);
    if (s.m1 > s.m0) hipLaunchKernelGGL(k_smt_emit, dim3(ceil_div(s.m1 - s.m0, T)), dim3(T), 0, st, B.binstart, B.members, s.m0, s.m1, t.wstart, t.memberbin, t.bincols,
                                        t.kmax, t.scratch, t.pres, (const int32_t *)nullptr, mptr, pcol.p, pval.p);
    {
        const std::vector<int64_t> oc = smt_gather_offsets(hp, 4), ov = smt_gather_offsets(hp, 8);
        void *bases[2] = {pcol.p, pval.p};
        const int64_t *offs[2] = {oc.data(), ov.data()};
        comm_gatherv(comm, 2, bases, offs, st);
    }
    out->colind.alloc((size_t)nnz2); out->val.alloc((size_t)nnz2);
    if (nmem) hipLaunchKernelGGL(k_smt_place, dim3(ceil_div(nmem, T)), dim3(T), 0, st, B.members, nmem, mlen, mptr, out->rowptr.p, pcol.p, pval.p,
                                 out->colind.p, out->val.p);
    IBH_HIP(hipGetLastError());
    IBH_HIP(hipStreamSynchronize(st));          // (pcol / pval are freed on leaving this scope)
    out->nnz = nnz2;
    out->shared = true;
}
static bool smooth_by_tiles(const SmoothBins &B, const ibh_weighted *w, ibh_comm *comm, hipStream_t st, SmoothedCsr *out) {
    Arena &A = arena();
    const int n = w->nrow, nb = (int)B.nbins;
    const int world = comm ? comm_world(comm) : 1;
    SmtBuild t{};
    if (!smt_tables(B, w, comm, st, &t)) return false;
    const size_t nmem1 = (size_t)std::max(t.nmem, 1), nwaves1 = (size_t)std::max(t.nwaves, 1);
    t.rowlen = A.get<uint32_t>((size_t)n + 1);
    IBH_HIP(hipMemsetAsync(t.rowlen, 0, sizeof(uint32_t) * ((size_t)n + 1), st));
    t.cand = A.get<SmtCand>(nmem1);
    t.wavebin = A.get<int32_t>(nwaves1); t.memberbin = A.get<int32_t>(nmem1);
    t.scratch = A.get<double>(nwaves1 * t.kmax * 64);
    t.pres = A.get<unsigned long long>(2 * nmem1);
    t.mne = A.get<unsigned char>(nmem1);
    t.mcol = A.get<int32_t>(nmem1 * SMT_ROWMAX);
    t.mval = A.get<double>(nmem1 * SMT_ROWMAX);
    SmoothedCsr r;
    r.rowptr.alloc((size_t)n + 1);
    if (world == 1) {
        smt_run_share(B, w, t, smt_whole(nb, t.nmem, t.nwaves), st);
        smt_collect(B, t, st, &r);
    } else {
        std::vector<uint32_t> hb(B.nbins + 1);
        IBH_HIP(hipMemcpy(hb.data(), B.binstart, sizeof(uint32_t) * (B.nbins + 1), hipMemcpyDeviceToHost));
        const std::vector<int> bs = smt_split(hb, B.v.nbx, B.v.nby, world);
        const SmtShare s = smt_share(hb, bs, comm_rank(comm), B.v.nbx);
        smt_run_share(B, w, t, s, st);
        smt_collect_ranks(B, t, s, smt_member_starts(hb, bs), comm, st, &r);
    }
    *out = std::move(r);
    return true;
}
// ---- the direct form (k_smooth_direct): count -> scan -> emit; one read-back (error word, overflow flag, nnz).  false: a row with more
// than SMD_MAXCOL columns
static bool smooth_by_rows(const SmoothBins &B, const ibh_weighted *w, hipStream_t st, SmoothedCsr *out) {
    Arena &A = arena();
    const int n = w->nrow;
    uint32_t *rowlen = A.get<uint32_t>((size_t)n + 1);
    IBH_HIP(hipMemsetAsync(B.d_cnt, 0, 3 * sizeof(uint32_t), st));
    const dim3 gd(ceil_div(n, SMD_WAVES));
    hipLaunchKernelGGL(k_smooth_direct<false>, gd, dim3(SMD_WAVES * 64), 0, st, B.v, B.binstart, B.members, w->rowptr.p, w->colind.p, w->val.p, rowlen,
                       (const int32_t *)nullptr, (int32_t *)nullptr, (double *)nullptr, B.d_cnt + 1);
    SmoothedCsr r;
    r.rowptr.alloc((size_t)n + 1);
    exclusive_scan_u32(rowlen, reinterpret_cast<uint32_t *>(r.rowptr.p), (size_t)n, B.d_cnt, st);
    uint32_t hd[4];
    readback_sync(hd, B.d_cnt, sizeof(hd), st);
    fail_zero_area(B, (int)hd[3]);
    if (hd[1] != 0) return false;
    const uint32_t nnz2 = hd[0];
    IBH_CHECK(nnz2 < (1u << 31), "smoothed matrix too large (%u entries)", nnz2);
    IBH_HIP(hipMemcpyAsync(r.rowptr.p + n, B.d_cnt, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    r.colind.alloc((size_t)nnz2); r.val.alloc((size_t)nnz2);
    hipLaunchKernelGGL(k_smooth_direct<true>, gd, dim3(SMD_WAVES * 64), 0, st, B.v, B.binstart, B.members, w->rowptr.p, w->colind.p, w->val.p,
                       (uint32_t *)nullptr, r.rowptr.p, r.colind.p, r.val.p, B.d_cnt + 1);
    r.nnz = nnz2;
    *out = std::move(r);
    return true;
}
// ---- the triplet pipeline: neighbour triplets -> sort by (i, j) -> row denominators -> products with the rows of M as contributions ->
// build_csr_from_contributions.  No limit of its own: never false
static bool smooth_by_triplets(const SmoothBins &B, const ibh_weighted *w, hipStream_t st, SmoothedCsr *out) {
    Arena &A = arena();
    const int T = 256, n = w->nrow;
    const dim3 grid(ceil_div(n, T));
    uint32_t *ncnt = A.get<uint32_t>((size_t)n);
    hipLaunchKernelGGL(k_smooth_neighbours<0>, grid, dim3(T), 0, st, B.v, B.binstart, B.members, ncnt, (const uint32_t *)nullptr,
                       (uint64_t *)nullptr, (uint32_t *)nullptr, (double *)nullptr);
    exclusive_scan_u32(ncnt, ncnt, (size_t)n, B.d_cnt, st);
    uint32_t h[4];
    IBH_HIP(hipMemcpyAsync(h, B.d_cnt, sizeof(h), hipMemcpyDeviceToHost, st));
    IBH_HIP(hipStreamSynchronize(st));
    fail_zero_area(B, (int)h[3]);
    const size_t ns = h[0];
    IBH_CHECK(ns < (1ul << 31), "smoothing matrix too large (%zu entries)", ns);
    uint64_t *sk = A.get<uint64_t>(ns), *sk2 = A.get<uint64_t>(ns);
    uint32_t *si = A.get<uint32_t>(ns), *si2 = A.get<uint32_t>(ns);
    double *wraw = A.get<double>(ns);
    hipLaunchKernelGGL(k_smooth_neighbours<1>, grid, dim3(T), 0, st, B.v, B.binstart, B.members, (uint32_t *)nullptr, ncnt, sk, si, wraw);
    // order the triplets by (i, j): rows become contiguous with ascending columns
    KeyField sf[2] = {{0, bits_for((uint64_t)n)}, {32, bits_for((uint64_t)n)}};
    if (ns && sf[0].nbits > 0 && radix_sort_pairs(sk, sk2, si, si2, ns, sf, 2, st)) { std::swap(sk, sk2); std::swap(si, si2); }
    int32_t *srowptr = A.get<int32_t>((size_t)n + 1);
    hipLaunchKernelGGL(k_smooth_rowptr, grid, dim3(T), 0, st, ncnt, n, (uint32_t)ns, srowptr);
    double *denom = A.get<double>((size_t)n);
    seg_sums<true>(srowptr, si, wraw, n, (long)ns, denom, st);          // denom_sum, smoother.cpp:37,51
    // smoothI * M as contributions in (i, j ascending) order
    uint32_t *pcnt = A.get<uint32_t>(ns ? ns : 1);
    if (ns) hipLaunchKernelGGL(k_smooth_prod_count, dim3(ceil_div(ns, T)), dim3(T), 0, st, sk, ns, w->rowptr.p, pcnt);
    exclusive_scan_u32(pcnt, pcnt, ns, B.d_cnt + 1, st);
    IBH_HIP(hipMemcpyAsync(h, B.d_cnt, sizeof(h), hipMemcpyDeviceToHost, st));
    IBH_HIP(hipStreamSynchronize(st));
    IBH_CHECK(h[1] < (1ul << 31), "smoothed matrix too large (%zu products)", (size_t)h[1]);
    Triplets t = triplets_in_arena(h[1]);
    if (ns) hipLaunchKernelGGL(k_smooth_prod_emit, dim3(ceil_div(ns, T)), dim3(T), 0, st, sk, si, wraw, denom, ns, w->rowptr.p,
                               w->colind.p, w->val.p, pcnt, t.keys, t.idx, t.term);
    IBH_HIP(hipGetLastError());
    ibh_weighted tmp;
    int32_t *row = nullptr;
    build_csr_from_contributions(&tmp, t, w->nrow, w->ncol, &row, st);
    out->rowptr = std::move(tmp.rowptr); out->colind = std::move(tmp.colind); out->val = std::move(tmp.val);
    out->nnz = tmp.nnz;
    return true;
}
// Every form reads w's CSR while it builds the new one into fresh buffers: wait for it, then swap.
static void commit_smoothed(ibh_weighted *w, SmoothedCsr *out, SmoothForm form, hipStream_t st) {
    IBH_HIP(hipGetLastError());
    IBH_HIP(hipStreamSynchronize(st));          // the old CSR was read until here
    w->rowptr = std::move(out->rowptr); w->colind = std::move(out->colind); w->val = std::move(out->val);
    w->nnz = out->nnz;
    w->conservative = 0;            // conservative = !smooth, RegridMatrices_Dynamic.cpp:167
    w->smoothed_by = (int)form;
    if (out->shared) w->built_fast = 3;
}
// comm (world > 1): every rank of the communicator calls this with the same matrix; the tile form is shared (w->built_fast = 3),
// the direct form and the triplet pipeline run on every rank.  The result is the same bits on every rank and for every world.
static void smooth_matrix(ibh_weighted *w, const ibh_regrid_matrices *rm, const int64_t *row_s, const double sigma[3],
                          hipStream_t st, ibh_comm *comm = nullptr) {
    smooth_check(rm, sigma);
    if (w->nrow == 0) {             // nothing to smooth, no form runs; still conservative = !smooth (RegridMatrices_Dynamic.cpp:167)
        w->conservative = 0;
        return;
    }
    const SmoothPlan plan = plan_smooth(w->nrow, rm->rg->cmin, rm->rg->cmax, sigma);
    const SmoothBins B = smooth_bins(w, rm, row_s, plan.grid, sigma, st);
    SmoothedCsr out;
    for (int k = 0; k < plan.nform; ++k) {
        const SmoothForm form = plan.form[k];
        const bool built = form == SMOOTH_TILE ? smooth_by_tiles(B, w, comm, st, &out)
                         : form == SMOOTH_DIRECT ? smooth_by_rows(B, w, st, &out) : smooth_by_triplets(B, w, st, &out);
        if (built) return commit_smoothed(w, &out, form, st);
    }
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
    RgView rg{};
    rg.sA = w->band_sA; rg.sHC = w->band_sHC;
    int32_t *row = A.get<int32_t>((size_t)nnz);
    hipLaunchKernelGGL(k_expand_long_rows, dim3(nrow), dim3(T), 0, st, w->rowptr.p, nrow, row);
    const ColSlots s = col_slots(w->colind.p, row, nnz, ncol, st);
    uint32_t *d_nb = A.get<uint32_t>(1);
    Bands b = build_bands(w, rg, rset->device_to_sparse(nrow, st), row, s.colptr, s.lrow, s.lidx, d_nb, st);
    uint32_t nb = 0;
    readback_sync(&nb, d_nb, sizeof(uint32_t), st);
    b.n = nb;
    return b;
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
__global__ void k_sw_expand(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colind, int nrow, uint64_t *__restrict__ keys,
                            uint32_t *__restrict__ idx, int32_t *__restrict__ erow) {
    const int r = blockIdx.x;                       // one workgroup per row
    for (int k = rowptr[r] + threadIdx.x; k < rowptr[r + 1]; k += blockDim.x) { keys[k] = (uint64_t)(uint32_t)colind[k]; idx[k] = (uint32_t)k; erow[k] = r; }
}
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
__global__ void k_sw_uniq(const uint64_t *__restrict__ tk, long n, uint32_t *__restrict__ u) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    u[k] = (k == 0 || tk[k] != tk[k - 1]) ? 1u : 0u;
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
    hipLaunchKernelGGL(k_sw_expand, dim3(nrow), dim3(T), 0, st, w->rowptr.p, w->colind.p, nrow, keys, idx, erow);
    KeyField kf{0, bits_for((uint64_t)ncol)};
    if (kf.nbits > 0 && radix_sort_pairs(keys, keys2, idx, idx2, (size_t)nnz, &kf, 1, st)) { std::swap(keys, keys2); std::swap(idx, idx2); }
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
        if (radix_sort_pairs(a, b2, av, bv, (size_t)nnz, tf, 2, st)) { std::swap(a, b2); std::swap(av, bv); }
        hipLaunchKernelGGL(k_sw_uniq, dim3(ceil_div(nnz, T)), dim3(T), 0, st, a, nnz, u);
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
    if (cf.nbits > 0 && radix_sort_pairs(ck, ck2, cv, cv2, (size_t)nuniq, &cf, 1, st)) { std::swap(ck, ck2); std::swap(cv, cv2); }
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
__global__ void k_rg_rowkeys(RgView rg, const int64_t *__restrict__ row_s, int nrow, uint64_t *__restrict__ keys, uint32_t *__restrict__ idx) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrow) return;
    long a, hc;
    e_decode(rg, row_s[r], a, hc);
    keys[r] = (uint64_t)a; idx[r] = (uint32_t)r;
}
__global__ void k_rg_heads(const uint64_t *__restrict__ keys, long n, uint32_t *__restrict__ h) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) h[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
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
__global__ void k_rg_entrykeys(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colind, int nrow, const int32_t *__restrict__ grp_of_row,
                               uint64_t *__restrict__ keys, uint32_t *__restrict__ idx, int32_t *__restrict__ erow) {
    const int r = blockIdx.x;                       // one workgroup per row
    const uint64_t g = (uint64_t)(uint32_t)grp_of_row[r] << 32;
    for (int k = rowptr[r] + threadIdx.x; k < rowptr[r + 1]; k += blockDim.x) { keys[k] = g | (uint32_t)colind[k]; idx[k] = (uint32_t)k; erow[k] = r; }
}
// item heads of the (group, column)-sorted entries: a run of equal keys is one item (two entries at most: else *d_bad)
__global__ void k_rg_itemheads(const uint64_t *__restrict__ keys, long n, uint32_t *__restrict__ h, uint32_t *__restrict__ d_bad) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool head = i == 0 || keys[i] != keys[i - 1];
    h[i] = head ? 1u : 0u;
    if (i >= 2 && keys[i] == keys[i - 1] && keys[i] == keys[i - 2]) *d_bad = 1u;
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
    RgView rg{};
    rg.sA = w->band_sA; rg.sHC = w->band_sHC;
    uint32_t *d_cnt = A.get<uint32_t>(8);
    IBH_HIP(hipMemsetAsync(d_cnt, 0, sizeof(uint32_t) * 8, st));
    // rows by GCM cell (stable: ascending row inside a group)
    uint64_t *rk = A.get<uint64_t>((size_t)nrow), *rk2 = A.get<uint64_t>((size_t)nrow);
    uint32_t *ri = A.get<uint32_t>((size_t)nrow), *ri2 = A.get<uint32_t>((size_t)nrow);
    hipLaunchKernelGGL(k_rg_rowkeys, dim3(ceil_div(nrow, T)), dim3(T), 0, st, rg, row_s, nrow, rk, ri);
    KeyField rf{0, 32};
    if (radix_sort_pairs(rk, rk2, ri, ri2, (size_t)nrow, &rf, 1, st)) { std::swap(rk, rk2); std::swap(ri, ri2); }
    uint32_t *rh = A.get<uint32_t>((size_t)nrow), *rhs = A.get<uint32_t>((size_t)nrow);
    hipLaunchKernelGGL(k_rg_heads, dim3(ceil_div(nrow, T)), dim3(T), 0, st, rk, (long)nrow, rh);
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
    // entries by (group, column): stable, so the two entries of a column keep their row (= slot) order
    uint64_t *keys = A.get<uint64_t>((size_t)nnz), *keys2 = A.get<uint64_t>((size_t)nnz);
    uint32_t *idx = A.get<uint32_t>((size_t)nnz), *idx2 = A.get<uint32_t>((size_t)nnz);
    int32_t *erow = A.get<int32_t>((size_t)nnz);
    hipLaunchKernelGGL(k_rg_entrykeys, dim3(nrow), dim3(T), 0, st, w->rowptr.p, w->colind.p, nrow, grp_of_row, keys, idx, erow);
    KeyField ef[2] = {{0, bits_for((uint64_t)w->ncol)}, {32, bits_for((uint64_t)ngrp)}};
    if (radix_sort_pairs(keys, keys2, idx, idx2, (size_t)nnz, ef, 2, st)) { std::swap(keys, keys2); std::swap(idx, idx2); }
    uint32_t *ih = A.get<uint32_t>((size_t)nnz), *ihs = A.get<uint32_t>((size_t)nnz);
    hipLaunchKernelGGL(k_rg_itemheads, dim3(ceil_div(nnz, T)), dim3(T), 0, st, keys, nnz, ih, d_cnt + 3);
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

#include "fastasm.inl"
#include "streamasm.inl"

// ---- the sorted-grid builds: facts -> plan_build (asm_plan.h) -> the plan's candidate paths in order ----------------------------
// The only place that reads the handles for a decision.  (The sheet's static plan is made here, by the first build that wants it.)
static BuildFacts facts_of_build(const ibh_regrid_matrices *rm, const MatSpec *sp, ibh_sparse_set *const dims[2], bool smooth, bool bands_wanted,
                                 ibh_comm *comm, hipStream_t st) {
    const ibh_regridder *gr = rm->rg;
    BuildFacts f;
    f.family = sp->family; f.row_key = sp->row_key; f.col_key = sp->col_key; f.row_list = sp->row_list; f.col_list = sp->col_list;
    f.nX = gr->nX; f.nI = gr->nI; f.nhc = gr->nhc;
    for (int k = 0; k < 2; ++k) {
        const ibh_sparse_set *s = dims[k];
        f.set[k].extent = key_extent(gr, k == 0 ? sp->row_key : sp->col_key);
        if (s) { f.set[k].n = s->n(); f.set[k].identity = s->identity(); }
    }
    f.same_set = dims[0] == dims[1];
    f.smooth = smooth; f.bands_wanted = bands_wanted;
    f.shared = comm != nullptr; f.world = comm ? comm_world(comm) : 1;
    f.plan_ok = fast_path_wanted(f) && ensure_plan(gr, st);
    if (f.plan_ok) {
        const ibh_plan &P = gr->plan;
        f.nAr = P.nAr; f.nmulti = P.nmulti; f.nmulti3 = P.nmulti3; f.npair = P.npair; f.maxrange = P.maxrange;
        f.tiny = P.tiny; f.icnt_pos = P.icnt_pos.p != nullptr; f.icnt_nz = P.icnt_nz.p != nullptr;
    }
    return f;
}
// Batch builds (assemble_batch): everything a concurrent fast build would otherwise create lazily in shared objects --
// the sheet's plan, the inverse table of a pre-populated column set -- is created up front on the calling thread.
static void fast_prewarm(const ibh_regrid_matrices *rm, const MatSpec *sp, ibh_sparse_set *dims[2], hipStream_t st) {
    const BuildPlan bp = plan_build(facts_of_build(rm, sp, dims, false, false, nullptr, st));
    if (!bp.prepop_table) return;
    (void)dims[1]->device_to_dense(bp.roles.gext, st);
    IBH_HIP(hipStreamSynchronize(st));
}
// returns the path that built the matrix; PATH_GENERAL: none did (nothing has been touched: the caller runs the general pipeline)
static BuildPath fast_build(const ibh_regrid_matrices *rm, const MatSpec *sp, const BuildPlan &bp, ibh_sparse_set *dims[2], int scale, int correctA,
                            const RgView &rg, ibh_weighted *w, hipStream_t st, ibh_comm *comm) {
    const Roles &role = bp.roles;
    const FaSets sets{dims[role.g_is_row ? 0 : 1], dims[role.g_is_row ? 1 : 0]};
    for (int k = 0; k < bp.npath; ++k) {
        const BuildPath path = bp.path[k];
        bool built = false;
        if (path == PATH_EVA) built = fast_build_eva(rm, sp, bp.range, dims, scale, correctA, rg, w, st);
        else if (path == PATH_STREAM_SHARED || path == PATH_STREAM) {
            const StreamPlan &s = path == PATH_STREAM ? bp.stream : bp.stream_shared;
            ibh_comm *c = path == PATH_STREAM ? nullptr : comm;
            built = role.EP ? stream_build<true>(rm, sp, role, sets, s, scale, correctA, rg, w, st, c)
                            : stream_build<false>(rm, sp, role, sets, s, scale, correctA, rg, w, st, c);
        } else if (path == PATH_RANGE)
            built = role.EP ? fast_build_gp<true>(rm, sp, role, sets, bp.range, scale, correctA, rg, w, st)
                            : fast_build_gp<false>(rm, sp, role, sets, bp.range, scale, correctA, rg, w, st);
        if (built) return path;
    }
    return PATH_GENERAL;
}

bool elevmask_classes(const ibh_regrid_matrices *rm, hipStream_t stream, const double *d_src) {
    const ibh_regridder *gr = rm->rg;
    if (gr->nhc > 64 || !stream_default(gr->nX)) return false;      // (not a grid of the streamed build: the first build that wants the bytes makes them)
    elevmask_classes_impl(rm, stream, d_src);
    return true;
}

// ---- RegridMatrices_Dynamic::matrix_d ----------------------------------------------------------
static const MatSpec *find_spec(const char *spec_name) {
    const MatSpec *sp = nullptr;
    for (const auto &s : SPECS) if (!strcmp(s.name, spec_name)) sp = &s;
    if (!sp) fail(IBH_ENOKEY, "unknown regrid matrix '%s' (expected one of AvI IvA AvX XvA EvI IvE EvX XvE EvA AvE)", spec_name);
    return sp;
}
// fast_only: build through the plan-based fast path or not at all (returns false, nothing touched) -- the mode of the
// concurrent builds of a batch, which must not append to a set another build of the same wave is reading
bool assemble_matrix(const ibh_regrid_matrices *rm, const char *spec_name, ibh_sparse_set *dim0, ibh_sparse_set *dim1,
                     int scale, int correctA, const double sigma[3], ibh_weighted **out, bool fast_only, ibh_comm *comm) {
    IBH_CHECK(rm && spec_name && out, "null argument");
    const MatSpec *sp = find_spec(spec_name);
    // RegridParams::smooth() (RegridMatrices.hpp:31): only compute_IvAE smooths (RegridMatrices_Dynamic.cpp:237-248)
    const bool smooth = sigma && sigma[0] != 0 && sp->family == FAM_IVAE;
    if (smooth && sp->row_key != KEY_I)
        fail(IBH_ENOTIMPL, "smoothing of '%s' (rows on the exchange grid) is not supported: the smoother needs ice-grid centroids", spec_name);
    const ibh_regridder *g = rm->rg;
    const bool uses_ep = sp->row_list == LIST_EP || sp->col_list == LIST_EP;
    if (uses_ep && g->nhc == 0) fail(IBH_EINVAL, "IceRegridder_L0::GvEp(): hcdefs is zero-length!");   // IceRegridder_L0.cpp:108-109
    // the calling thread's own stream: builds issued by different host threads (assemble_batch) overlap on the GPU
    hipStream_t st = hipStreamPerThread;
    Arena &A = arena();
    A.reset();

    RgView rg{g->ex_indices.p, g->ex_area.p, rm->elevmaskI.p, g->hcdefs.p, g->A_ratio_s.p, g->nX, g->nA,
              g->nhc, g->interp_style, g->hc_stride_A, g->hc_stride_HC};

    auto w = new_weighted();
    ibh_sparse_set *dims[2] = {dim0, dim1};
    for (int k = 0; k < 2; ++k) {
        w->dims[k] = dims[k] ? DimRef::borrowed(dims[k]) : DimRef::owned(std::make_unique<ibh_sparse_set>());
        dims[k] = w->dims[k].get();
    }
    w->conservative = 1;              // :63, :167 (no smoothing), :258
    w->scaled = scale;                // :421
    if (band_eligible(sp->row_key, sp->col_key)) {       // EvI, EvX: bands may be built later (ensure_bands)
        w->band_eligible = 1; w->band_sA = g->hc_stride_A; w->band_sHC = g->hc_stride_HC;
    }

    // sorted exchange grid + dims shapes it covers: the plan-based fast path (fastasm.inl); smoothing and the
    // band structure work on intermediates of the general pipeline
    const bool bands_wanted = bands_at_build(sp->row_key, sp->col_key);
    // A SHARED smoothed build (comm): the unsmoothed matrix from the shared build -- the same bits as the general pipeline's --
    // then the smoothing, shared as well, over the row cells of its own row set
    if (smooth && comm) smooth_check(rm, sigma);
    const BuildPath built = fast_build(rm, sp, plan_build(facts_of_build(rm, sp, dims, smooth, bands_wanted, comm, st)), dims, scale, correctA, rg,
                                       w.get(), st, comm);
    if (built != PATH_GENERAL) {
        w->built_fast = built == PATH_EVA ? (int)PATH_RANGE : (int)built;
        if (smooth) {
            w->built_fast = 1;                          // (3 again when the smoothing is shared as well)
            smooth_matrix(w.get(), rm, dims[0]->device_to_sparse(w->nrow, st), sigma, st, comm);
        }
        *out = w.release();
        return true;
    }
    if (fast_only) return false;
    A.reset();
    // counters read back with ONE sync: [0] first out-of-range exchange cell, [1] new row keys,
    // [2] new column keys, [3] number of contributions
    // [first(rows) | first(cols) | counters] are one allocation, preset to 0xFF.. with one fill
    const size_t er = (size_t)key_extent(g, sp->row_key), ec = (size_t)key_extent(g, sp->col_key);
    uint32_t *first_r = A.get<uint32_t>(er + ec + 4), *first_c = first_r + er;
    uint32_t *d_cnt = first_c + ec;
    uint32_t *d_err = d_cnt;
    const uint32_t big = 0xffffffffu;
    IBH_HIP(hipMemsetAsync(first_r, 0xFF, sizeof(uint32_t) * (er + ec + 1), st));

    // dense numbering in emission order; each user-visible set is numbered by exactly one Ur matrix
    // (RegridMatrices_Dynamic.cpp:75-81, 86-90, 178-183, 187-190, 270-277), so the two are independent.
    Numbering rnum = number_set_prepare(rg, dims[0], key_extent(g, sp->row_key), sp->row_list, sp->row_key,
                                        (sp->row_list == LIST_EP ? 2 : 1) * g->nX, 0, first_r, st);
    Numbering cnum = number_set_prepare(rg, dims[1], key_extent(g, sp->col_key), sp->col_list, sp->col_key,
                                        (sp->col_list == LIST_EP ? 2 : 1) * g->nX, 2, first_c, st);
    const int T = 256;
    const dim3 grid(g->nX ? ceil_div(g->nX, T) : 1);
    uint32_t *pk = A.get<uint32_t>((size_t)g->nX);
    uint32_t *roff = A.get<uint32_t>((size_t)g->nX), *coff = A.get<uint32_t>((size_t)g->nX), *poff = A.get<uint32_t>((size_t)g->nX);
    rnum.args.off = roff; cnum.args.off = coff;
    if (uses_ep) {
        hipLaunchKernelGGL(k_first2<true>, grid, dim3(T), 0, st, rg, rnum.args, cnum.args, d_err);
        hipLaunchKernelGGL(k_flag2<true>, grid, dim3(T), 0, st, rg, rnum.args, cnum.args, *sp, pk);
    } else {
        hipLaunchKernelGGL(k_first2<false>, grid, dim3(T), 0, st, rg, rnum.args, cnum.args, d_err);
        hipLaunchKernelGGL(k_flag2<false>, grid, dim3(T), 0, st, rg, rnum.args, cnum.args, *sp, pk);
    }
    exclusive_scan3(pk, (size_t)g->nX, roff, coff, poff, d_cnt + 1, st);
    uint32_t h_cnt[4];
    readback_sync(h_cnt, d_cnt, sizeof(h_cnt), st);
    if (h_cnt[0] != big) fail_elevation_range(rm, h_cnt[0]);
    for (Numbering *nb : {&rnum, &cnum}) {
        const uint32_t n_new = nb == &rnum ? h_cnt[1] : h_cnt[2];
        IBH_CHECK((int64_t)n_new <= nb->max_new, "internal: more new keys (%u) than reserved (%ld)", n_new, (long)nb->max_new);
        IBH_CHECK((int64_t)nb->ds.n_old + n_new < (1ll << 31), "dense extent overflows int32");
    }
    const uint32_t ncontrib = h_cnt[3];
    Triplets t = triplets_in_arena(ncontrib);
    // emit also records the new keys' dense -> sparse entries, so it runs even with no contributions
    if (uses_ep) hipLaunchKernelGGL(k_contrib_emit<true>, grid, dim3(T), 0, st, rg, *sp, rnum.args, cnum.args, pk, poff, t.keys, t.idx, t.term);
    else hipLaunchKernelGGL(k_contrib_emit<false>, grid, dim3(T), 0, st, rg, *sp, rnum.args, cnum.args, pk, poff, t.keys, t.idx, t.term);
    IBH_HIP(hipGetLastError());
    number_set_finish(rnum, h_cnt[1], st);
    number_set_finish(cnum, h_cnt[2], st);
    const DeviceSet &rset = rnum.ds, &cset = cnum.ds;
    const int nrow = rset.n, ncol = cset.n;
    int32_t *row = nullptr;
    // ice-cell rows over shared columns (IvA, IvE): the re-visits of straddling ice cells are far apart
    // in the emission order, the pieces would span the whole sequence -> straight to the radix sort
    build_csr_from_contributions(w.get(), t, nrow, ncol, &row, st, sp->row_key != KEY_I);
    const long nnz = w->nnz;

    // weights
    double *rs = A.get<double>((size_t)nrow), *cs = A.get<double>((size_t)ncol);
    double *rowmul = A.get<double>((size_t)nrow), *colmul = A.get<double>((size_t)ncol);
    w->wM.alloc((size_t)nrow); w->Mw.alloc((size_t)ncol);
    seg_sums<true>(w->rowptr.p, nullptr, w->val.p, nrow, nnz, rs, st);
    uint32_t *colptr = nullptr, *lidx = nullptr;       // per-column slots (short-column path), reused by build_bands
    int32_t *lrow = nullptr;
    if (short_columns(nnz, ncol)) {
        // short columns: per-column slots + one thread per column (see k_col_sums)
        const ColSlots s = col_sums_by_slots(w.get(), row, ncol, cs, st);
        colptr = s.colptr; lrow = s.lrow; lidx = s.lidx;
    } else {
        col_sums_by_sort(w.get(), ncol, cs, st);
    }
    FinalizeArgs fa{sp->family, scale, correctA, sp->row_key, sp->col_key, nrow, ncol, rset.to_sparse, cset.to_sparse,
                    rs, cs, w->wM.p, w->Mw.p, rowmul, colmul};
    const int nmax = nrow > ncol ? nrow : ncol;
    if (nmax) hipLaunchKernelGGL(k_weights, dim3(ceil_div(nmax, T)), dim3(T), 0, st, rg, fa);
    const int apply_row = scale ? 1 : 0;
    const int apply_col = (correctA && sp->family != FAM_AEVI) ? 1 : 0;
    if (nnz && (apply_row || apply_col))
        hipLaunchKernelGGL(k_scale, dim3(ceil_div(nnz, T)), dim3(T), 0, st, row, w->colind.p, w->val.p, nnz, rowmul, colmul,
                           apply_row, apply_col);
    IBH_HIP(hipGetLastError());
    if (smooth) smooth_matrix(w.get(), rm, rset.to_sparse, sigma, st, comm);
    // E-row matrices over ice / exchange columns: band structure for the apply (after the scaling: exact
    // copies of M), when asked for (bands_at_build)
    const bool want_bands = bands_wanted && colptr != nullptr && ncol < (1 << 28);
    uint32_t nband_entries = 0;
    if (want_bands) {
        uint32_t *d_nb = A.get<uint32_t>(1);
        Bands b = build_bands(w.get(), rg, rset.to_sparse, row, colptr, lrow, lidx, d_nb, st);
        readback_sync(&nband_entries, d_nb, sizeof(uint32_t), st);
        b.n = nband_entries;
        w->st.bands = std::move(b);
    } else {
        IBH_HIP(hipStreamSynchronize(st));
    }
    *out = w.release();
    return true;
}

// ---- a batch of builds (the coupler's per-timestep set, IceCoupler.cpp:361-468) ----------------------------------
// Same results as calling matrix_d for the jobs one after the other, in order.  Jobs that share no set they could
// modify run CONCURRENTLY, each on a host thread of a small persistent pool and that thread's own stream: a 5 km build
// is ~250 workgroups, an eighth of the chip, so four of them overlap almost perfectly.  A job waits for every earlier
// job that may still append to one of its sets (EvI numbers dimE before IvE / XvE read it); jobs of one wave that share a
// pre-populated set run in fast-only mode (the fast path only reads such a set) and anything that needs the general
// pipeline -- which may append -- is redone sequentially afterwards, together with the later jobs that share its sets.
namespace {
class WorkerPool {
    // A coupling step at 5 km is ~0.2 ms in two waves of two builds: a worker that went to sleep on the condition variable between
    // the waves costs a futex wake-up (tens of us) each time.  Workers therefore poll for the next job for a short while after
    // finishing one, and wait() polls before it blocks; idle pools sleep as before.
    static constexpr long SPIN_NS = 400 * 1000;
    std::vector<std::thread> threads;
    std::mutex mu;
    std::condition_variable cv, done_cv;
    std::deque<std::function<void()>> queue;
    std::atomic<int> queued{0}, pending{0};
    bool stop = false;
    static long now_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
public:
    explicit WorkerPool(int n) {
        for (int i = 0; i < n; ++i)
            threads.emplace_back([this] {
                long spin_until = 0;
                for (;;) {
                    std::function<void()> job;
                    while (queued.load(std::memory_order_acquire) == 0 && now_ns() < spin_until) __builtin_ia32_pause();
                    {
                        std::unique_lock<std::mutex> lk(mu);
                        cv.wait(lk, [this] { return stop || !queue.empty(); });
                        if (stop && queue.empty()) return;
                        job = std::move(queue.front());
                        queue.pop_front();
                        queued.fetch_sub(1, std::memory_order_relaxed);
                    }
                    job();
                    if (pending.fetch_sub(1, std::memory_order_acq_rel) == 1) {
                        std::lock_guard<std::mutex> lk(mu);      // (pairs with wait(): no wake-up is lost)
                        done_cv.notify_all();
                    }
                    spin_until = now_ns() + SPIN_NS;
                }
            });
    }
    ~WorkerPool() {
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv.notify_all();
        for (auto &t : threads) t.detach();      // process exit: the HIP runtime may already be gone, do not join into it
    }
    void submit(std::function<void()> f) {
        { std::lock_guard<std::mutex> lk(mu); queue.push_back(std::move(f)); pending.fetch_add(1, std::memory_order_relaxed); queued.fetch_add(1, std::memory_order_release); }
        cv.notify_one();
    }
    void wait() {
        const long until = now_ns() + 4 * SPIN_NS;
        while (pending.load(std::memory_order_acquire) != 0 && now_ns() < until) __builtin_ia32_pause();
        std::unique_lock<std::mutex> lk(mu);
        done_cv.wait(lk, [this] { return pending.load(std::memory_order_acquire) == 0; });
    }
};
WorkerPool &pool() { static WorkerPool *p = new WorkerPool(3); return *p; }
}  // namespace

void assemble_batch(const ibh_regrid_matrices *rm, int n, const char *const *specs, ibh_sparse_set *const *dim0,
                    ibh_sparse_set *const *dim1, const int32_t *scale, const int32_t *correctA, const double sigma[3],
                    ibh_weighted **out) {
    IBH_CHECK(rm && n >= 0 && (n == 0 || (specs && scale && correctA && out)), "bad arguments");
    struct Job { const MatSpec *sp; ibh_sparse_set *d[2]; int wave; bool done; int code; std::string err; };
    std::vector<Job> jobs((size_t)n);
    for (int j = 0; j < n; ++j) {
        IBH_CHECK(specs[j] != nullptr, "null matrix name in batch");
        jobs[(size_t)j] = Job{find_spec(specs[j]), {dim0 ? dim0[j] : nullptr, dim1 ? dim1[j] : nullptr}, 0, false, IBH_OK, std::string()};
        IBH_CHECK(jobs[(size_t)j].d[0] == nullptr || jobs[(size_t)j].d[0] != jobs[(size_t)j].d[1], "dims[0] and dims[1] must be distinct sets");
        out[j] = nullptr;
    }
    const ibh_regridder *g = rm->rg;
    auto readonly = [&](const Job &jb, int k) {          // a set no build ever changes: the identity over its whole extent
        const ibh_sparse_set *s = jb.d[k];
        return s && s->identity() && s->n() == key_extent(g, k == 0 ? jb.sp->row_key : jb.sp->col_key);
    };
    // wave of a job: one after the PRODUCER of each of its sets -- the first job of the batch that uses a set which is
    // still empty numbers it; the later users of that set only read it (fast path) and do not wait for each other
    for (int j = 0; j < n; ++j)
        for (int a = 0; a < 2; ++a) {
            const ibh_sparse_set *s = jobs[(size_t)j].d[a];
            if (!s || s->n() != 0 || readonly(jobs[(size_t)j], a)) continue;
            for (int i = 0; i < j; ++i)
                if (jobs[(size_t)i].d[0] == s || jobs[(size_t)i].d[1] == s) {      // i is the producer (the first user)
                    jobs[(size_t)j].wave = std::max(jobs[(size_t)j].wave, jobs[(size_t)i].wave + 1);
                    break;
                }
        }
    int dev = 0;
    IBH_HIP(hipGetDevice(&dev));
    int nwaves = 0;
    for (auto &jb : jobs) nwaves = std::max(nwaves, jb.wave + 1);
    auto run = [&](int j, bool fast_only) {
        Job &jb = jobs[(size_t)j];
        try {
            jb.done = assemble_matrix(rm, specs[j], jb.d[0], jb.d[1], scale[j], correctA[j], sigma, &out[j], fast_only);
        } catch (const Error &e) { jb.code = e.code; jb.err = e.msg; }
        catch (const std::exception &e) { jb.code = IBH_EINVAL; jb.err = e.what(); }
    };
    auto shares = [&](int i, int j) {
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b)
                if (jobs[(size_t)i].d[a] && jobs[(size_t)i].d[a] == jobs[(size_t)j].d[b] && !readonly(jobs[(size_t)i], a)) return true;
        return false;
    };
    for (int wv = 0; wv < nwaves; ++wv) {
        std::vector<int> members;
        for (int j = 0; j < n; ++j) if (jobs[(size_t)j].wave == wv) members.push_back(j);
        // members that share a (by now pre-populated) set with another member: fast-only; the others are free to use either path
        std::vector<char> fo(members.size(), 0);
        for (size_t a = 0; a < members.size(); ++a)
            for (size_t b = 0; b < members.size(); ++b)
                if (a != b && shares(members[a], members[b])) fo[a] = 1;
        for (int j : members) { ibh_sparse_set *d[2] = {jobs[(size_t)j].d[0], jobs[(size_t)j].d[1]}; fast_prewarm(rm, jobs[(size_t)j].sp, d, hipStreamPerThread); }
        for (size_t a = 1; a < members.size(); ++a) {
            const int j = members[a];
            const bool f = fo[a] != 0;
            pool().submit([&, j, f, dev] { (void)hipSetDevice(dev); run(j, f); });
        }
        if (!members.empty()) run(members[0], fo[0] != 0);
        pool().wait();
        // anything the fast path declined is redone by the general pipeline, in order; a later member that shares a set
        // with it saw the set before that build could append to it and is redone too
        std::vector<int> redone;
        for (size_t a = 0; a < members.size(); ++a) {
            const int j = members[a];
            Job &jb = jobs[(size_t)j];
            if (jb.code != IBH_OK) continue;
            bool redo = !jb.done;
            for (int b : redone) redo = redo || shares(b, j);
            if (!redo) continue;
            if (out[j]) { delete out[j]; out[j] = nullptr; }
            redone.push_back(j);
            run(j, false);
        }
    }
    for (int j = 0; j < n; ++j)
        if (jobs[(size_t)j].code != IBH_OK) {
            const Job jb = jobs[(size_t)j];
            for (int q = 0; q < n; ++q) { delete out[q]; out[q] = nullptr; }
            throw Error(jb.code, jb.err);
        }
}

}  // namespace ibh
