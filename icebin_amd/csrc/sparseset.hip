// sparseset.hip -- ibh_sparse_set's members (common.h) and the first-seen numbering of a key stream (sparseset.h).
#include "prims.h"
#include "sparseset.h"

#include <algorithm>

namespace ibh {

__global__ void k_fill_i32(int32_t *p, size_t n, int32_t v) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
__global__ void k_iota_i64(int64_t *p, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = (int64_t)i;
}
__global__ void k_scatter_existing(int32_t *tab, const int64_t *to_sparse, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) tab[to_sparse[i]] = i;
}
void fill_to_dense_table(int32_t *tab, int64_t extent, const int64_t *to_sparse, int n, hipStream_t st) {
    const int T = 256;
    if (extent) hipLaunchKernelGGL(k_fill_i32, dim3(ceil_div(extent, T)), dim3(T), 0, st, tab, (size_t)extent, -1);
    if (n) hipLaunchKernelGGL(k_scatter_existing, dim3(ceil_div(n, T)), dim3(T), 0, st, tab, to_sparse, n);
}
}  // namespace ibh

// ---- ibh_sparse_set (common.h) ------------------------------------------------------------------------------------------------
ibh_sparse_set::ibh_sparse_set(const ibh_sparse_set &o) : sparse_extent_(o.sparse_extent_), n_(o.n_), identity_(o.identity_) {
    if (identity_ || !n_) return;
    const int64_t *t = o.to_sparse_host();
    host_.assign(t, t + n_);
    host_n_ = n_;
}
void ibh_sparse_set::assign_host(int64_t sparse_extent, const int64_t *keys, int32_t n) {
    std::vector<int64_t> sorted(keys, keys + n);
    std::sort(sorted.begin(), sorted.end());
    for (int32_t i = 0; i < n; ++i) {
        IBH_CHECK(sorted[(size_t)i] >= 0 && (sparse_extent < 0 || sorted[(size_t)i] < sparse_extent),
                  "sparse index %ld outside extent %ld", (long)sorted[(size_t)i], (long)sparse_extent);
        IBH_CHECK(i == 0 || sorted[(size_t)i] != sorted[(size_t)i - 1], "duplicate sparse index %ld", (long)sorted[(size_t)i]);
    }
    *this = ibh_sparse_set(sparse_extent);
    host_.assign(keys, keys + n);
    n_ = host_n_ = n;
}
int32_t ibh_sparse_set::add_dense_host(int64_t key) {
    IBH_CHECK(key >= 0 && (sparse_extent_ < 0 || key < sparse_extent_), "sparse index %ld outside extent %ld", (long)key, (long)sparse_extent_);
    if (identity_ && key < n_) return (int32_t)key;
    ensure_inverse();                       // materialises an identity prefix on the host
    auto it = inv_.find(key);
    if (it != inv_.end()) return it->second;
    IBH_CHECK(n_ < 0x7fffffff, "dense extent overflows int32");
    identity_ = false;
    host_.push_back(key);
    inv_[key] = n_;
    host_n_ = inv_n_ = ++n_;                // the device copy (entries [0, dev_n_)) is completed by the next build
    return n_ - 1;
}
int32_t ibh_sparse_set::to_dense(int64_t key) const {
    if (identity_) return key >= 0 && key < n_ ? (int32_t)key : -1;
    ensure_inverse();
    auto it = inv_.find(key);
    return it == inv_.end() ? -1 : it->second;
}
void ibh_sparse_set::ensure_host() const {
    if (host_n_ >= n_) return;
    host_.resize((size_t)n_);
    if (identity_) {
        for (int32_t i = host_n_; i < n_; ++i) host_[(size_t)i] = i;
    } else {
        if (dev_n_ < n_) ibh::fail(IBH_EINVAL, "internal: sparse set has no valid copy of entries [%d,%d)", host_n_, n_);
        IBH_HIP(hipMemcpy(host_.data() + host_n_, dev_.p + host_n_, sizeof(int64_t) * (size_t)(n_ - host_n_), hipMemcpyDeviceToHost));
    }
    host_n_ = n_;
}
void ibh_sparse_set::check_entries_within(int64_t extent, const char *what) const {
    IBH_CHECK(n_ <= extent, "%s holds %d entries, more than its extent of %lld", what, n_, (long long)extent);
    if (identity_ || host_n_ < n_) return;          // (entries on the device only were checked when they were numbered)
    for (int32_t i = 0; i < n_; ++i)
        IBH_CHECK(host_[(size_t)i] >= 0 && host_[(size_t)i] < extent, "%s entry %lld outside [0, %lld)", what,
                  (long long)host_[(size_t)i], (long long)extent);
}
void ibh_sparse_set::check_extent(int64_t extent, const char *what) const {
    IBH_CHECK(sparse_extent_ == -1 || sparse_extent_ == extent, "%s has sparse extent %lld, the grid %lld cells", what,
              (long long)sparse_extent_, (long long)extent);
}
void ibh_sparse_set::copy_to_sparse(int64_t *dst, int n, hipStream_t st) const {
    if (n == 0) return;
    if (identity_) {
        hipLaunchKernelGGL(ibh::k_iota_i64, dim3(ibh::ceil_div(n, 256)), dim3(256), 0, st, dst, (size_t)n);
    } else if (dev_n_ >= n) {
        IBH_HIP(hipMemcpyAsync(dst, dev_.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToDevice, st));
    } else {
        ensure_host();
        IBH_HIP(hipMemcpyAsync(dst, host_.data(), sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, st));
    }
}
const int64_t *ibh_sparse_set::device_to_sparse(int n, hipStream_t st) const {
    if (n > 0 && on_device(n)) return dev_.p;
    int64_t *t = ibh::arena().get<int64_t>((size_t)n);
    copy_to_sparse(t, n, st);
    return t;
}
const int32_t *ibh_sparse_set::device_to_dense(int64_t extent, hipStream_t st) {
    if (tab_n_ == n_ && tab_extent_ == extent && tab_.p) return tab_.p;
    tab_.alloc((size_t)extent);
    if (dev_n_ < n_) {                      // complete the device copy of the dense -> sparse table first
        ibh::DevBuf<int64_t> grown((size_t)n_);
        copy_to_sparse(grown.p, n_, st);
        IBH_HIP(hipStreamSynchronize(st));
        dev_ = std::move(grown);
        dev_n_ = n_;
    }
    ibh::fill_to_dense_table(tab_.p, extent, dev_.p, n_, st);
    tab_n_ = n_; tab_extent_ = extent;
    return tab_.p;
}
void ibh_sparse_set::adopt_device(ibh::DevBuf<int64_t> &&table, int32_t n, int64_t extent) noexcept {
    set_sparse_extent(extent);
    if (n <= n_) return;
    // the host copy and the inverse map hold a prefix of the table and stay valid; the device inverse table does not
    dev_ = std::move(table);
    dev_n_ = n_ = n;
    identity_ = false;
    tab_n_ = -1;
}

namespace ibh {

// ---- first-seen numbering of a key stream (sparseset.h) -----------------------------------------------------------------------
// position p names a key this numbering sees: inside the mask and, when the range is checked, inside [0, extent) (else reported)
template <class K>
__device__ __forceinline__ bool key_at(const KeyNumbering &s, const K *__restrict__ key, int stride, long p, int64_t &k) {
    if (s.act && !s.act[p]) return false;
    k = key[p * stride];
    if (s.bad_range && (k < 0 || k >= s.extent)) { *s.bad_range = 1u; return false; }
    return true;
}
template <class K>
__global__ void k_key_first(KeyNumbering s, const K *__restrict__ key, int stride, long n) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t k;
    if (p < n && key_at(s, key, stride, p, k) && old_id(s, k) < 0) atomicMin(&s.first[k], (uint32_t)p);
}
template <class K>
__global__ void k_key_flag(KeyNumbering s, const K *__restrict__ key, int stride, long n, uint8_t *__restrict__ isnew) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    int64_t k;
    isnew[p] = key_at(s, key, stride, p, k) && old_id(s, k) < 0 && s.first[k] == (uint32_t)p ? 1 : 0;
}
template <class K>
__global__ void k_key_new(const K *__restrict__ key, int stride, long n, const uint8_t *__restrict__ isnew,
                          const uint32_t *__restrict__ rank, int64_t *__restrict__ out) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n && isnew[p]) out[rank[p]] = key[p * stride];
}
template <class K>
__global__ void k_key_dense(KeyNumbering s, const K *__restrict__ key, int stride, long n, int32_t *__restrict__ dense,
                            uint32_t *__restrict__ missing) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    int64_t k;
    int d = -1;
    if (key_at(s, key, stride, p, k)) {
        d = dense_of(s, k);
        if (d < 0 && s.transform == IBH_TO_DENSE) atomicOr(missing, 1u);
    }
    dense[p] = d;
}

template <class K>
KeyNumberingRun number_keys_prepare(ibh_sparse_set *set, int64_t extent, int transform, const K *key, int stride, long n,
                                    const uint8_t *act, bool check_range, hipStream_t st) {
    Arena &A = arena();
    KeyNumberingRun nb;
    nb.set = set;
    nb.status = A.get<uint32_t>(2);
    KeyNumbering &s = nb.s;
    s.transform = transform;
    s.act = act;
    s.extent = extent;
    s.n_old = set ? set->n() : (int)extent;
    s.ident_n = -1;
    if (!set || set->identity() || s.n_old == 0) s.ident_n = s.n_old;      // an empty set: the identity on [0, 0)
    else s.tab = set->device_to_dense(extent, st);
    if (check_range) {
        IBH_HIP(hipMemsetAsync(nb.status, 0, sizeof(uint32_t) * 2, st));
        s.bad_range = nb.status + 1;
    }
    if (transform == IBH_ADD_DENSE) {
        s.first = A.get<uint32_t>((size_t)extent);
        s.rank = A.get<uint32_t>((size_t)n);
        uint8_t *isnew = A.get<uint8_t>((size_t)n);
        if (extent) IBH_HIP(hipMemsetAsync(s.first, 0xFF, sizeof(uint32_t) * (size_t)extent, st));
        if (n) {
            hipLaunchKernelGGL(k_key_first<K>, dim3(ceil_div(n, 256)), dim3(256), 0, st, s, key, stride, n);
            hipLaunchKernelGGL(k_key_flag<K>, dim3(ceil_div(n, 256)), dim3(256), 0, st, s, key, stride, n, isnew);
        }
        exclusive_scan_u8(isnew, s.rank, (size_t)n, nb.status, st);
        nb.isnew = isnew;
    }
    IBH_HIP(hipGetLastError());
    return nb;
}
template <class K>
DevBuf<int64_t> number_keys_grow(const KeyNumberingRun &nb, const K *key, int stride, long n, uint32_t n_new, hipStream_t st) {
    DevBuf<int64_t> grown;
    if (!nb.set || !nb.adds() || n_new == 0) return grown;
    const int n_old = nb.s.n_old;
    grown.alloc((size_t)n_old + n_new);
    nb.set->copy_to_sparse(grown.p, n_old, st);
    hipLaunchKernelGGL(k_key_new<K>, dim3(ceil_div(n, 256)), dim3(256), 0, st, key, stride, n, nb.isnew, nb.s.rank, grown.p + n_old);
    IBH_HIP(hipGetLastError());
    return grown;
}
template <class K>
void number_keys_dense(const KeyNumberingRun &nb, const K *key, int stride, long n, int32_t *dense, uint32_t *missing, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_key_dense<K>, dim3(ceil_div(n, 256)), dim3(256), 0, st, nb.s, key, stride, n, dense, missing);
    IBH_HIP(hipGetLastError());
}
template void number_keys_dense(const KeyNumberingRun &, const int32_t *, int, long, int32_t *, uint32_t *, hipStream_t);
template void number_keys_dense(const KeyNumberingRun &, const int64_t *, int, long, int32_t *, uint32_t *, hipStream_t);
template KeyNumberingRun number_keys_prepare(ibh_sparse_set *, int64_t, int, const int32_t *, int, long, const uint8_t *, bool, hipStream_t);
template KeyNumberingRun number_keys_prepare(ibh_sparse_set *, int64_t, int, const int64_t *, int, long, const uint8_t *, bool, hipStream_t);
template DevBuf<int64_t> number_keys_grow(const KeyNumberingRun &, const int32_t *, int, long, uint32_t, hipStream_t);
template DevBuf<int64_t> number_keys_grow(const KeyNumberingRun &, const int64_t *, int, long, uint32_t, hipStream_t);

void number_stream(ibh_sparse_set &set, int64_t extent, const int64_t *keys, long n, int32_t *dense, const char *what, hipStream_t st) {
    IBH_CHECK(extent >= 0 && extent < (1ll << 31), "%s: a sparse extent of %lld cannot be numbered on the device", what, (long long)extent);
    IBH_CHECK(n < (1ll << 31), "%s: %ld entries overflow int32", what, n);
    if (n == 0 || extent == 0) {
        IBH_CHECK(n == 0, "%s: entries in a set of extent 0", what);
        set.set_sparse_extent(extent);
        return;
    }
    const int32_t n0 = set.n();
    const KeyNumberingRun nb = number_keys_prepare(&set, extent, IBH_ADD_DENSE, keys, 1, n, nullptr, true, st);
    number_keys_dense(nb, keys, 1, n, dense, nullptr, st);
    uint32_t h[2] = {0, 0};
    readback_sync(h, nb.status, sizeof(h), st);             // the one host wait of a numbering
    IBH_CHECK(h[1] == 0, "%s: an index outside [0, %lld)", what, (long long)extent);
    const uint32_t n_new = h[0];
    IBH_CHECK((int64_t)n0 + n_new < 0x7fffffffll, "dense extent overflows int32");
    DevBuf<int64_t> grown = number_keys_grow(nb, keys, 1, n, n_new, st);
    if (n_new) IBH_HIP(hipStreamSynchronize(st));
    set.adopt_device(std::move(grown), (int32_t)(n0 + n_new), extent);      // (nothing new: only the extent)
}

}  // namespace ibh
