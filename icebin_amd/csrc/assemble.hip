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
// bit-identical to the oracle.
#include "assemble.h"
#include "applystruct.h"
#include "asm_plan.h"
#include "csrbuild.h"
#include "prims.h"
#include "smooth.h"
#include "sparseset.h"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
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
// (GCM cell, class) of an E key (a regridder's strides are checked when it is made)
__device__ __forceinline__ void e_decode(const RgView &rg, int64_t e, long &a, long &hc) {
    HcIndexing{rg.sA, rg.sHC}.split<true>(e, a, hc);
}

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
    bool underflow;     // a weight != 0 and an area != 0 whose product is 0: fewer entries than the class pattern says
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
    c.underflow = false;
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
            c.underflow = c.a != 0 && ((w0 != 0 && !h0) || (w1 != 0 && !h1));
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
        Bands b = build_bands(w.get(), HcIndexing{g->hc_stride_A, g->hc_stride_HC}, rset.to_sparse, row, colptr, lrow, lidx, d_nb, st);
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
