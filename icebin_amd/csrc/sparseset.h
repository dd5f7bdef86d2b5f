// sparseset.h -- the device side of ibh_sparse_set (common.h) and the first-seen numbering of a key stream
// (spsparse::SparseSet::add_dense in stream order), sparseset.hip.  Three passes over n keys, key of position p = key[p * stride]:
//   1 first   first[key] = smallest position that names a key the set lacks (atomicMin over the sparse extent)
//   2 flag    isnew[p] = p is that position, as bytes; their exclusive scan is rank[], its total the number of new keys
//   3 new     the new keys at table[n_old + rank[p]]
// after which the dense id of any key is its old id, or n_old + rank[first[key]] (dense_of).  A position outside the `act`
// mask, or -- when the range is checked -- a key outside [0, extent), is skipped by every pass.
// Numberings of their own, on purpose: the assembly's (assemble.hip k_first2: two sets per exchange-cell visit), multivec.hip's
// sort-based grouping (unbounded sparse extents) and modele.hip's host loops.
#pragma once
#include "common.h"

namespace ibh {

// tab[0, extent) = -1, then tab[to_sparse[i]] = i for i < n: a sparse -> dense table on the device, enqueued on st
void fill_to_dense_table(int32_t *tab, int64_t extent, const int64_t *to_sparse, int n, hipStream_t st);

// what a kernel needs to give a key its dense id: the set's old part, and under ADD_DENSE the result of passes 1 and 2
struct KeyNumbering {
    int64_t ident_n;            // >= 0: the old part is the identity on [0, ident_n)
    const int32_t *tab;         // otherwise: old sparse -> dense (-1 missing), [extent]
    int32_t n_old, transform;
    uint32_t *first;            // ADD_DENSE: [extent] smallest stream position naming a missing key
    uint32_t *rank;             // ADD_DENSE: [n] exclusive scan of the new-key flags
    const uint8_t *act;         // positions this set sees (nullptr: all)
    int64_t extent;
    uint32_t *bad_range;        // non-null: keys are checked against [0, extent); one outside sets it and is skipped
};
__device__ __forceinline__ int old_id(const KeyNumbering &s, int64_t key) {
    if (s.ident_n >= 0) return key < s.ident_n ? (int)key : -1;
    return s.tab[key];
}
// the dense id of a key the numbering has seen (or any key of the old part); -1: missing under a TO_DENSE transform
__device__ __forceinline__ int dense_of(const KeyNumbering &s, int64_t key) {
    const int d = old_id(s, key);
    if (d >= 0 || s.transform != IBH_ADD_DENSE) return d;
    return s.n_old + (int)s.rank[s.first[key]];
}

// One numbering between its two host steps.  Both only enqueue; the caller reads the count back between them and, once
// everything of its own has succeeded, hands the grown table to the set (ibh_sparse_set::adopt_device).
struct KeyNumberingRun {
    KeyNumbering s{};
    ibh_sparse_set *set = nullptr;      // null: nobody's set, the identity over the whole extent
    const uint8_t *isnew = nullptr;     // ADD_DENSE: [n] the flags of pass 2
    uint32_t *status = nullptr;         // device uint32[2]: [0] the number of new keys (ADD_DENSE), [1] a key lay outside the range
    bool adds() const { return status && s.transform == IBH_ADD_DENSE; }      // (a default run adds nothing)
};
// the view, and under ADD_DENSE passes 1 and 2.  K: int32_t or int64_t.  Uses the arena (not reset).
template <class K>
KeyNumberingRun number_keys_prepare(ibh_sparse_set *set, int64_t extent, int transform, const K *key, int stride, long n,
                                    const uint8_t *act, bool check_range, hipStream_t st);
// pass 3: the set's grown dense -> sparse table (old entries, then the n_new new keys first-seen); empty when it gains nothing
template <class K>
DevBuf<int64_t> number_keys_grow(const KeyNumberingRun &nb, const K *key, int stride, long n, uint32_t n_new, hipStream_t st);
// dense[p] = dense_of position p's key, -1 where the numbering does not see it or the key is missing; one missing under TO_DENSE
// raises *missing (not read under ADD_DENSE)
template <class K>
void number_keys_dense(const KeyNumberingRun &nb, const K *key, int stride, long n, int32_t *dense, uint32_t *missing, hipStream_t st);
// dense[i] = add_dense(keys[i]) for i ascending; the set takes the new keys and `extent`.  A key outside [0, extent) fails
// the call and leaves the set alone.  Uses the arena (not reset: the caller's arrays may live there); one host wait, and the
// adoption's when the set grows.
void number_stream(ibh_sparse_set &set, int64_t extent, const int64_t *keys, long n, int32_t *dense, const char *what, hipStream_t st);

}  // namespace ibh
