// common.h -- internal helpers of libicebin_hip.so (error channel, device buffers, handle layouts).
#pragma once
#include <atomic>
#include <mutex>
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/icebin_hip.h"
#include "apply_plan.h"

namespace ibh {

// ---- error channel -------------------------------------------------------------------------
struct Error : std::exception {
    int code;
    std::string msg;
    Error(int c, std::string m) : code(c), msg(std::move(m)) {}
    const char *what() const noexcept override { return msg.c_str(); }
};
[[noreturn]] void fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void set_last_error(const char *msg);
// the status of a C-ABI call made from inside the library, as this call's own error
inline void rethrow(int rc) { if (rc != IBH_OK) throw Error(rc, ibh_last_error()); }
// there is a HIP device at all, else IBH_ENODEVICE: the library has no CPU fallback (defined in capi.hip, like the next one)
void require_device();
// a handle made on `device` is used on it: "<what> belongs to device %d, current device is %d"
void check_current_device(int device, const char *what);

#define IBH_HIP(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            ::ibh::fail(e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice ? IBH_ENODEVICE : IBH_EHIP, \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define IBH_CHECK(cond, ...)                                  \
    do {                                                      \
        if (!(cond)) ::ibh::fail(IBH_EINVAL, __VA_ARGS__);    \
    } while (0)

// Wrap a C-ABI body: exceptions -> status code + thread-local message.
template <class F>
int guarded(F &&f) noexcept {
    try {
        f();
        return IBH_OK;
    } catch (const Error &e) {
        set_last_error(e.msg.c_str());
        return e.code;
    } catch (const std::bad_alloc &) {
        set_last_error("out of host memory");
        return IBH_EINVAL;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return IBH_EINVAL;
    }
}

// ---- device memory -------------------------------------------------------------------------
// Caching allocator (capi.hip): freed blocks are kept per device and size class and handed out again,
// so that rebuilding the same matrices every coupling step does no hipMalloc/hipFree (both
// synchronise the device).  ibh_release_cached_memory() returns everything to the driver.
void *dev_alloc(size_t bytes, size_t *granted, int *device);
void dev_free(void *p, size_t granted, int device);     // filed under the device the block was allocated on
void release_cached_memory();

template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    size_t granted = 0;     // bytes actually reserved (size class)
    int device = 0;         // device the block lives on (the current one at alloc time)
    DevBuf() = default;
    explicit DevBuf(size_t count) { alloc(count); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n), granted(o.granted), device(o.device) { o.p = nullptr; o.n = 0; o.granted = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; n = o.n; granted = o.granted; device = o.device; o.p = nullptr; o.n = 0; o.granted = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void alloc(size_t count) {
        if (p && count * sizeof(T) <= granted) { n = count; return; }
        release();
        n = count;
        p = static_cast<T *>(dev_alloc((count ? count : 1) * sizeof(T), &granted, &device));
    }
    void release() {
        if (p) dev_free(p, granted, device);
        p = nullptr; n = 0; granted = 0;
    }
    void upload(const T *host, size_t count, hipStream_t s = nullptr) {
        if (count > n || !p) alloc(count);
        if (count) IBH_HIP(hipMemcpyAsync(p, host, count * sizeof(T), hipMemcpyHostToDevice, s));
    }
    void download(T *host, size_t count, hipStream_t s = nullptr) const {
        if (count) IBH_HIP(hipMemcpyAsync(host, p, count * sizeof(T), hipMemcpyDeviceToHost, s));
        IBH_HIP(hipStreamSynchronize(s));
    }
    void zero(hipStream_t s = nullptr) { if (n) IBH_HIP(hipMemsetAsync(p, 0, n * sizeof(T), s)); }
};

constexpr int IBH_GT_EP = IBH_GSLOTS + 2;   // u16 entry offsets of a tile: one per slot + the end, padded to whole dwords
inline int bits_for(uint64_t n) {   // bits needed to represent values in [0, n)
    int b = 0;
    while (b < 64 && (n > (1ull << b))) ++b;
    return b;
}

// indexingHC of an E index: iE = iA * sA + ihc * sHC, with (sA, sHC) = (1, nA) (the class slowest) or (nhc, 1) (the class
// fastest).  The one definition of the tuple for every unit, on the host and on the device.
struct HcIndexing {
    int64_t sA, sHC;
    // UNIT_CLASS_STRIDE: the caller has checked that the strides are one of the two pairs above, so the class stride of the
    // class-fastest order is 1 and its division is left out (the assembly's kernels decode once per matrix entry: with the
    // division the E-keyed builds measured 2 - 5 % slower)
    template <bool UNIT_CLASS_STRIDE = false>
    __host__ __device__ void split(int64_t iE, int64_t &iA, int64_t &ihc) const {
        if (sHC >= sA) { ihc = iE / sHC; iA = (iE % sHC) / sA; }
        else { iA = iE / sA; ihc = UNIT_CLASS_STRIDE ? iE % sA : (iE % sA) / sHC; }
    }
    __host__ __device__ int64_t index(int64_t iA, int64_t ihc) const { return iA * sA + ihc * sHC; }
    // indexingHC_change_nhc (modele/merge_topo.cpp:364-372): the class-slowest order keeps (1, nA), the class-fastest one becomes (nhc, 1)
    HcIndexing with_nhc(int64_t nhc) const { return sHC >= sA ? *this : HcIndexing{nhc, 1}; }
};

}  // namespace ibh

// ---- handle layouts (opaque to the C-ABI user) ----------------------------------------------
// A SparseSet (spsparse::SparseSet): the dense -> sparse table of a matrix dimension, in first-seen order.  A matrix build
// appends on the DEVICE; the host copy is completed lazily (ensure_host) so that a 10^7-entry dims table never crosses PCIe
// unless a caller actually reads it.  The copies and caches are changed by the members alone, so each decides in one place
// which of them stay valid (the longer ones: sparseset.hip).
struct ibh_sparse_set {
  public:
    ibh_sparse_set() = default;
    explicit ibh_sparse_set(int64_t sparse_extent) : sparse_extent_(sparse_extent) {}
    ibh_sparse_set(const ibh_sparse_set &o);            // the entries only: no device copy, no caches
    ibh_sparse_set &operator=(ibh_sparse_set &&o) = default;

    int32_t n() const { return n_; }
    int32_t dense_extent() const { return n_; }
    int64_t sparse_extent() const { return sparse_extent_; }
    bool identity() const { return identity_; }

    // host side (the C-ABI's SparseSet calls)
    void make_identity(int64_t n) { *this = ibh_sparse_set(n); n_ = (int32_t)n; identity_ = true; }
    void assign_host(int64_t sparse_extent, const int64_t *keys, int32_t n);
    int32_t add_dense_host(int64_t key);
    int32_t to_dense(int64_t key) const;                // -1: missing
    const int64_t *to_sparse_host() const { ensure_host(); return host_.data(); }
    void ensure_host() const;
    void ensure_inverse() const {
        ensure_host();
        for (int32_t i = inv_n_; i < n_; ++i) inv_[host_[(size_t)i]] = i;
        inv_n_ = n_;
    }
    // every entry the host holds lies in [0, extent), and there are no more entries than that; `what` names the set in the error
    void check_entries_within(int64_t extent, const char *what) const;
    // the sparse extent is unset (-1) or `extent`, the cells of the grid the set is used for
    void check_extent(int64_t extent, const char *what) const;

    // device side.  A set only READ by a build -- identity, pre-populated -- may be shared by builds running concurrently
    // (assemble_batch): the extent is written only when it changes, and a table that adds nothing changes nothing else.
    void set_sparse_extent(int64_t extent) { if (sparse_extent_ != extent) sparse_extent_ = extent; }
    // dense -> sparse of the first n entries into dst, enqueued on st: iota for an identity set, else the device copy, else an
    // upload of the host copy.  No synchronisation: the source is the set's own host copy, which every caller leaves alone
    // until it has synchronised the stream (they all read counts back, or synchronise, before returning or changing the set).
    void copy_to_sparse(int64_t *dst, int n, hipStream_t st) const;
    // the same table: the set's own device buffer when it holds the n entries, else a copy in the arena
    const int64_t *device_to_sparse(int n, hipStream_t st) const;
    bool on_device(int n) const { return !identity_ && dev_n_ >= n; }     // the first n entries are in the set's own device buffer
    // sparse -> dense (-1 missing) over [0, extent) on the device, built on demand and cached until the set changes
    const int32_t *device_to_dense(int64_t extent, hipStream_t st);
    // a build that writes that table itself (fastasm.inl): the buffer, then -- once the set has taken the build's entries --
    // the mark that it is valid
    int32_t *device_to_dense_for_write(int64_t extent) { tab_n_ = -1; tab_.alloc((size_t)extent); return tab_.p; }
    void mark_device_to_dense_written(int64_t extent) { tab_n_ = n_; tab_extent_ = extent; }
    // the set becomes table[0, n) over `extent`: the present entries followed by new ones (a set numbered by a build).  With
    // n <= dense extent nothing is new: only the extent is taken.  Cannot fail.
    void adopt_device(ibh::DevBuf<int64_t> &&table, int32_t n, int64_t extent) noexcept;

  private:
    int64_t sparse_extent_ = -1;
    int32_t n_ = 0;                         // dense extent
    bool identity_ = false;                 // to_sparse[i] == i for i < n; neither copy is materialised until asked for
    mutable std::vector<int64_t> host_;     // entries [0, host_n_) valid
    mutable int32_t host_n_ = 0;
    ibh::DevBuf<int64_t> dev_;              // entries [0, dev_n_) valid
    int32_t dev_n_ = 0;
    ibh::DevBuf<int32_t> tab_;              // device sparse -> dense table (-1 missing) of entries [0, tab_n_), built on demand
    int32_t tab_n_ = -1;
    int64_t tab_extent_ = -1;
    mutable std::unordered_map<int64_t, int32_t> inv_;   // sparse -> dense of entries [0, inv_n_): host-side to_dense / add_dense
    mutable int32_t inv_n_ = 0;
};

// Mask-independent structure of one exchange grid (fastasm.inl): built once, on the device, the first
// time a matrix of this sheet is assembled.  Only for grids sorted by (iA, iI) -- the order
// ExchangeGrid's constructor leaves them in (AbbrGrid.cpp:10-21).
struct ibh_plan {
    bool tried = false, ok = false;
    int32_t nAr = 0;                     // atmosphere cells with exchange cells ("ranges" of consecutive x)
    ibh::DevBuf<int32_t> arng;           // [nAr+1] first exchange cell of every range
    ibh::DevBuf<int32_t> aidx;           // [nX] range of every exchange cell
    ibh::DevBuf<int32_t> ilptr, ilist;   // [nI+1], [nX] exchange cells of every ice cell, ascending
    ibh::DevBuf<int32_t> ifirst;         // [nI] first exchange cell of the ice cell with area != 0, -1: none
    ibh::DevBuf<uint8_t> isdup;          // [nX] bit 0: same (iA, iI) as the cell before; bit 1: this is the ONLY exchange cell of
                                         //      its ice cell (the ice cell straddles no GCM-cell edge and has no duplicates); bit 2: this
                                         //      cell is the first-seen exchange cell of its ice cell (ifirst[iI] == x); bits 3 / 4: area > 0 /
                                         //      area != 0 and not > 0
    ibh::DevBuf<int32_t> mlist;          // [nmulti] ice cells with more than one exchange cell (several ranges, or duplicates)
    int32_t nmulti = 0;
    // [nI] matrix entries an UNMASKED ice cell has per elevation-class slot: groups of duplicate exchange cells (same (iA, iI))
    // with a member of area > 0 (IvA: rows of GvAp) / area != 0 (IvE: rows of GvI); static, so the I-row builds count their
    // rows without visiting the exchange cells.  Empty when an area is so small that area * weight could underflow
    // (the count would then depend on the elevation): the builds count by visiting, as before.
    ibh::DevBuf<uint8_t> icnt_pos, icnt_nz;
    // [nX] the ice-cell index of every exchange cell on its own (ex_indices interleaves it with the atmosphere index, which is
    // constant over a range): the per-range kernels and the streamed count read 4 bytes per cell instead of 8
    ibh::DevBuf<int32_t> exI;
    // for the streamed build (streamasm.inl): isdup bits 5 (first cell of its range), 6 (its ice cell was first seen in an
    // EARLIER range: a straddler) and 7 (the next cell is a duplicate of this one); the atmosphere cell of every range; the
    // longest range (positions inside a range's block of entries are stored in 16 bits when they fit); an area so small that
    // area * class weight could underflow was seen (the streamed elevation-class builds count by sign classes: not for it)
    ibh::DevBuf<int32_t> riA;
    int32_t maxrange = 0;
    bool tiny = false;
    // the ice cells with several exchange cells, split for the streamed build: PAIRS -- exactly two exchange cells, in two ranges,
    // the first one the first-seen cell (an ice cell across one GCM-cell edge: nearly all of them) -- as three parallel arrays
    // (first cell, second cell, ice cell), served by a lean kernel without list walks; the rest (corners, duplicates) in mlist3
    ibh::DevBuf<int32_t> px1, px2, piI, mlist3;
    ibh::DevBuf<double> pa1, pa2;        // the (static) overlap areas of a pair's two cells, beside them: no gathers in k_sa_pairs
    int32_t npair = 0, nmulti3 = 0;
    std::vector<int32_t> arng_h;         // host copy of arng (the sharded build deals ranges to ranks), filled on first use
};

struct ibh_regridder {
    int device = 0;
    mutable ibh_plan plan;
    int64_t nX = 0, nI = 0, nA = 0;
    int32_t nA_dense = 0, nhc = 0, interp_style = 0;
    int64_t hc_stride_A = 1, hc_stride_HC = 0;
    ibh::DevBuf<int32_t> ex_indices;    // [2*nX]
    ibh::DevBuf<double> ex_area;        // [nX]
    ibh::DevBuf<double> hcdefs;         // [nhc]
    ibh::DevBuf<double> A_ratio_s;      // [nA] native/proj by SPARSE A index, 0 where A cell not realised
    std::vector<int64_t> A_to_sparse;   // host copies for wA()
    std::vector<double> A_native, A_proj, hcdefs_h;
    double hc_last = 0;
    ibh::DevBuf<double> I_centroid;     // [2*nI] (x,y) by sparse ice index; empty when not supplied
    bool has_centroid = false;
    double cmin[2] = {0, 0}, cmax[2] = {0, 0};   // bounding box of the centroids
};

struct ibh_regrid_matrices {
    const ibh_regridder *rg = nullptr;
    ibh::DevBuf<double> elevmaskI;      // [nI] copy (RegridMatrices_Dynamic.cpp:352)
    int scale = 1, correctA = 0;
    double sigma[3] = {0, 0, 0};
    // one byte per ice cell, a function of its elevation and the regridder's elevation classes alone (ibh::elevmask_classes,
    // streamasm.inl): 0xFF masked, 0xFE elevation beyond the last class (linterp_1d_b's error), 0xFD a class weight below 1e-30, else first class | classes << 6.
    // Made once per elevmask -- at creation for grids the streamed build serves, else by the first build that wants it -- and read by
    // every matrix of this object in place of the 8-byte elevation wherever only the mask or the class pattern matters.
    mutable ibh::DevBuf<uint8_t> em_cls;
    mutable int em_cls_nhc = -1, em_cls_interp = -1;
    mutable std::mutex em_cls_mu;
};

namespace ibh {
inline uint64_t next_weighted_uid() {
    static std::atomic<uint64_t> n{0};
    return ++n;
}

// ---- apply structures: optional copies of a matrix's entries in the order one apply kernel family wants them ------------------
// Each is a value that owns its buffers: a builder (applystruct.hip) fills a local one and returns it, `x = {}` empties it,
// built() says whether it exists.

// rowdual (EvI, EvX): the CSR filtered to one entry per (GCM cell, ice cell) carrying the weights of BOTH elevation classes
// the cell lies between (applystruct.hip build_bands); band r = row r
struct Bands {
    int64_t n = 0;                          // band entries, 0: not built
    int32_t nrow = 0;                       // bands = rows of the matrix
    DevBuf<int32_t> ptr, col, rb1;          // [nrow+1]; [n] column | bit30 lower exists | bit31 upper exists; [nrow]
    DevBuf<double> v0, v1;                  // [n] lower-class / upper-class weight
    bool built() const { return n > 0; }
    // partial sums of an apply: [2: lower, upper][nbatch][nvar][part_ld()]
    long part_ld() const { return band_part_ld(nrow); }
    long part_stride(int nvar) const { return (long)nvar * part_ld(); }      // one batch's lower (or upper) sums
    size_t part_count(int nvar, int nbatch) const { return band_part_count(nrow, nvar, nbatch); }
};

// colsweep (EvI, EvX, and AvI, AvX in batched launches; sweep_kernel.inl): the entries in column order, paired per column into
// items, 64 items a block, tb blocks a task with its local row table (applystruct.hip build_sweep_from_csr)
struct Sweep {
    int32_t ntask = 0, nblk = 0, nprow = 0, nslot = 0;      // ntask == 0: not built
    int32_t tb = 0, nitems = 0, ident = 0;                  // blocks per task, items, column == item index
    DevBuf<int32_t> task_p0, task_ns, col;
    DevBuf<uint32_t> meta;
    DevBuf<double> v0, v1;
    DevBuf<int32_t> comb_ptr, comb_p;       // [nrow+1], [nprow]: the partial-sum rows that make up row r, in task order
    bool built() const { return ntask > 0; }
    // partial sums of an apply: [slices of 64 lanes, a lane = (batch, field)][nprow][part_ld()]
    long part_ld(int nvar) const { return sweep_part_ld(nvar); }
    long part_stride(int nvar) const { return (long)nprow * part_ld(nvar); }
    size_t part_count(int nvar, int nbatch) const { return sweep_part_count(nprow, nvar, nbatch); }
};

// fused pair (ibh_weighted_pair_prepare): a second matrix whose every row reads rows of ONE group of this matrix only (AvE
// after EvI: a GCM cell's value is a combination of that cell's elevation classes) rides in the row-group kernel's epilogue.
// w[g * IBH_GSLOTS + s]: the second matrix's weight of slot s of group g (mask[g] bit s: it has one); row[g]: the second
// matrix's row fed by group g, -1 none.
struct Pair {
    const ibh_weighted *second = nullptr;   // named by (address, uid); nullptr: not built
    uint64_t uid = 0;
    DevBuf<double> w;
    DevBuf<uint32_t> mask;
    DevBuf<int32_t> row;
    bool built() const { return second != nullptr; }
};

// rowgroup (EvI, EvX; spmm.hip): the rows of one GCM cell (its elevation classes) form a GROUP; the group's entries are
// listed once per distinct column, ascending, as ITEMS {col, meta = slot0 | slot1 << 8 | has-bits, v0, v1} -- the column set
// of a group is the AvI row of its GCM cell, so X is gathered once per (GCM cell, ice cell) instead of once per class; slot s
// of group g is row slotrow[g * IBH_GSLOTS + s] (applystruct.hip build_groups_from_csr).
struct RowGroups {
    int32_t n = 0, nslot = 0, nitems = 0;           // groups (0: not built), most rows in a group, items
    DevBuf<int32_t> ptr, ns, slotrow, col;          // [n+1] items of a group; [n] rows of a group; [n*IBH_GSLOTS]; [nitems]
    DevBuf<uint32_t> meta;
    DevBuf<double> v0, v1;
    // grouptile (spmm.hip): the items of a group cut into TILES of seg columns; per tile the columns (padded by repeating
    // the last) and the entries sorted by (slot, column) as {8 x local item index, weight} with u16 offsets per slot -- the rows
    // of the CSR restricted to the tile, in CSR order.  Entries of tile t start at ibh_gt_ecap(seg) * t.
    struct Tiles {
        int32_t ntile = 0, seg = 0;                 // 0: not built
        DevBuf<int32_t> ptr, col;                   // [n+1] tiles of a group; [ntile * seg]
        DevBuf<uint16_t> ek, eptr;                  // [ntile * ecap]; [ntile * IBH_GT_EP]
        DevBuf<double> ev;                          // [ntile * ecap]
        bool built() const { return ntile > 0; }
    };
    Tiles tiles;                                    // the tiles and a pairing index the group table: they exist, and go, with it
    Pair pair;
    bool built() const { return n > 0; }
};

// What the applies keep beside a matrix: the structures (with one flag each: a build that was declined or failed is not tried
// again), the per-apply scratch, and what the last apply launched.
struct ApplyState {
    Bands bands;
    Sweep sweep;
    RowGroups groups;
    bool bands_tried = false, sweep_tried = false, groups_tried = false;
    struct Scratch {
        DevBuf<double> scratch, tbuf, rowsum1;      // apply_transformed: fields + small transform, and M*1 (row sums) for the offset term
        DevBuf<double> consv;                       // force_conservation: the two dot products per variable [2*nvar] + chunk sums
        DevBuf<double> xt;                          // shortrow: transposed copy of the (small) input fields
        DevBuf<double> band_part, sweep_part;       // partial sums of one launch (Bands::part_count, Sweep::part_count)
        DevBuf<int32_t> rowperm;                    // rows by descending length (batched rowblock launches)
        bool have_rowsum1 = false, have_rowperm = false;
    } scr;
    int64_t napply = 0;                             // applies the matrix has seen (the lazy builds wait for the second)
    ApplyKernel last_kernel = KERNEL_AUTO;          // KERNEL_AUTO: no apply yet
    char last_sig[64] = {0};    // the kernel instantiation the last apply launched, as rocprofv3 names it (every apply kernel family records it)
    // per-handle launch options (ibh_weighted_set_option): looked up before the process-wide ibh_set_tuning map by every apply of
    // THIS matrix, so two host threads tuning different handles do not interfere
    std::unordered_map<std::string, int> opts;
    void fill(MatrixFacts &f) const {               // the structures' part of what the choice reads (facts_of)
        f.bands_built = bands.built(); f.bands_tried = bands_tried; f.bands_n = bands.n;
        f.sweep_built = sweep.built(); f.sweep_tried = sweep_tried;
        f.sweep_ntask = sweep.ntask; f.sweep_nprow = sweep.nprow; f.sweep_nslot = sweep.nslot; f.sweep_ident = sweep.ident;
        f.groups_built = groups.built(); f.groups_tried = groups_tried; f.groups_n = groups.n; f.groups_nslot = groups.nslot;
        f.tiles_built = groups.tiles.built(); f.tiles_seg = groups.tiles.seg;
        f.napply = napply;
    }
};

// One dimension of a matrix: its set, and whether the matrix owns it (and deletes it with itself) or the caller does.  Made
// by the named constructors alone, which are the cases there are.
class DimRef {
  public:
    DimRef() = default;
    DimRef(DimRef &&o) noexcept : set_(o.set_), owns_(o.owns_) { o.set_ = nullptr; o.owns_ = false; }
    DimRef &operator=(DimRef &&o) noexcept { std::swap(set_, o.set_); std::swap(owns_, o.owns_); return *this; }
    ~DimRef() { if (owns_) delete set_; }
    static DimRef borrowed(ibh_sparse_set *callers) { return DimRef(callers, false); }
    static DimRef owned(std::unique_ptr<ibh_sparse_set> set) { return DimRef(set.release(), true); }
    static DimRef owned_identity(int64_t n) {
        DimRef d = owned(std::make_unique<ibh_sparse_set>());
        d->make_identity(n);
        return d;
    }
    // the same set for a second matrix: the caller's is shared, one that `src`'s matrix owns is copied (the second matrix may
    // outlive the first)
    static DimRef borrow_or_copy(const DimRef &src) {
        return src.owns_ ? owned(std::make_unique<ibh_sparse_set>(*src.set_)) : borrowed(src.set_);
    }
    ibh_sparse_set *get() const { return set_; }
    ibh_sparse_set *operator->() const { return set_; }
    operator ibh_sparse_set *() const { return set_; }

  private:
    DimRef(ibh_sparse_set *set, bool owns) : set_(set), owns_(owns) {}
    ibh_sparse_set *set_ = nullptr;
    bool owns_ = false;
};

// The set a build numbers in place of the caller's (null: nobody's): a copy of the caller's entries, or a fresh set.  The
// caller's own set is untouched until commit(), which the build calls once nothing can fail any more and which cannot fail.
class WorkingSet {
  public:
    explicit WorkingSet(ibh_sparse_set *callers)
        : callers_(callers), work_(callers ? std::make_unique<ibh_sparse_set>(*callers) : std::make_unique<ibh_sparse_set>()) {}
    ibh_sparse_set *get() const { return work_.get(); }
    ibh_sparse_set *operator->() const { return work_.get(); }
    ibh_sparse_set &operator*() const { return *work_; }
    // the caller's set takes the entries and the matrix borrows it; without one the matrix owns the working set
    DimRef commit() noexcept {
        if (!callers_) return DimRef::owned(std::move(work_));
        *callers_ = std::move(*work_);
        return DimRef::borrowed(callers_);
    }

  private:
    ibh_sparse_set *callers_;
    std::unique_ptr<ibh_sparse_set> work_;
};
}  // namespace ibh
// The matrix proper is immutable once it is built; `st` is the cache the applies keep beside it.
struct ibh_weighted {
    const uint64_t uid = ibh::next_weighted_uid();     // never reused: a pairing names its second matrix by (address, uid)
    int device = 0;
    int32_t nrow = 0, ncol = 0;
    int64_t nnz = 0;
    ibh::DevBuf<int32_t> rowptr, colind;
    ibh::DevBuf<double> val, wM, Mw;
    ibh::DimRef dims[2];
    int conservative = 1, scaled = 1;
    int built_fast = 0;                 // assembled by the plan-based fast path (fastasm.inl); introspection only
    int smoothed_by = 0;                // the SmoothForm (smooth_plan.h) that smoothed it, 0: not smoothed; introspection only
    int composed_by = 0;                // the ComposeForm (csrops.h) a to_modele matrix was composed by, 0: not composed; introspection only
    ibh::ApplyKernel kernel_override = ibh::KERNEL_AUTO;    // SpMM dispatch (ibh_weighted_set_kernel)
    // E-row matrices over ice / exchange columns can get row groups, a column sweep or bands from their CSR (spmm.hip
    // build_structures): set by the matrix build, with how the row keys decode into (GCM cell, class)
    int band_eligible = 0;
    int64_t band_sA = 0, band_sHC = 0;
    mutable ibh::ApplyState st;
};

namespace ibh {
inline MatrixFacts facts_of(const ibh_weighted &w) {
    MatrixFacts f;
    f.nrow = w.nrow; f.ncol = w.ncol; f.nnz = w.nnz;
    f.band_eligible = w.band_eligible != 0; f.conservative = w.conservative != 0; f.kernel_override = w.kernel_override;
    w.st.fill(f);
    return f;
}
// a fresh handle on the current device
inline std::unique_ptr<ibh_weighted> new_weighted() {
    std::unique_ptr<ibh_weighted> w(new ibh_weighted);
    IBH_HIP(hipGetDevice(&w->device));
    return w;
}
}  // namespace ibh

struct ibh_exgrid {
    int64_t nX = 0;
    ibh::DevBuf<int32_t> indices;       // [2*nX] interleaved (iA, iI), sorted by (iA, iI)
    ibh::DevBuf<double> overlaps;       // [nX]
};

namespace ibh {
// spmm.hip
// comm.hip: the exchanges of the sharded assembly (streamasm.inl), enqueued on the caller's stream
int comm_world(const ibh_comm *c);
int comm_rank(const ibh_comm *c);
void comm_exchange_blocks(ibh_comm *c, double *base, int64_t count, int64_t stride, hipStream_t st);
void comm_gatherv(ibh_comm *c, int n, void *const *bases, const int64_t *const *offs, hipStream_t st);
void spmm_launch(const ibh_weighted *w, const double *dA, int nvar, int64_t lda, double *dB, int64_t ldb,
                 double fill, int force_conservation, hipStream_t stream);
void spmm_launch_many(const ibh_weighted *w, int nbatch, const double *const *dA, int nvar, int64_t lda,
                      double *const *dB, int64_t ldb, double fill, int force_conservation, hipStream_t stream);
void weighted_reserve(const ibh_weighted *w, int nvar);
// groups_asked: the caller needs the row groups whatever the rules say, and no other structure (weighted_pair_prepare)
void weighted_prepare(const ibh_weighted *w, int nvar, int nbatch, bool groups_asked = false);
void weighted_pair_prepare(const ibh_weighted *first, const ibh_weighted *second, int nvar);
void spmm_launch_pair(const ibh_weighted *first, const ibh_weighted *second, const double *dA, int nvar, int64_t lda, double *dB1,
                      int64_t ldb1, double *dB2, int64_t ldb2, double fill, hipStream_t stream);
void spmm_launch_chain(const ibh_weighted *first, const ibh_weighted *second, const ibh_weighted *third, const double *dA, int nvar, int64_t lda,
                       double *dB1, int64_t ldb1, double *dB2, int64_t ldb2, double *dB3, int64_t ldb3, double fill, hipStream_t stream);
void matvec_legacy_launch(const ibh_weighted *w, const double *dx, int nvar, int64_t ldx, double *dy, int64_t ldy,
                          int ignore_nan, hipStream_t stream);
void spmm_transformed_launch(const ibh_weighted *w, const double *dA, int nvar_in, int64_t lda, const double *T,
                              const double *b, int nvar_out, double *dB, int64_t ldb, double fill, hipStream_t stream);
void weight_dot_launch(const double *dw, int n, const double *dA, int nvar, int64_t lda, double *dout, double *part,
                       hipStream_t stream);
size_t weight_dot_scratch(int n, int nvar);
void set_launch_events(hipEvent_t start, hipEvent_t stop);
int get_tuning(const char *key, int dflt);
void set_tuning(const char *key, int value);
// gridgen.hip
// make_exchange_grid (gridgen/GridGen_Exchange.cpp:175-284) for a rectilinear XY ice grid
void exgrid_generate(const ibh_exgrid_desc *d, ibh_exgrid *out);
// the same from polygons already in HBM (d_*: device arrays, ascending iA; edges on the host), through the streamed clip
void exgrid_generate_polys(int nx, int ny, const double *xedges, const double *yedges, int x_fastest, int npoly, const int32_t *d_polyptr,
                           const double *d_vx, const double *d_vy, const int64_t *d_iA, ibh_exgrid *out, hipStream_t st);
}  // namespace ibh
