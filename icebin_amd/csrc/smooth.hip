// smooth.hip -- K5: the smoother on gfx950.  A finished CSR goes in, another comes out: it needs the matrix handle, the ice grid's
// centroids and elevations, the plan (smooth_plan.h), the scan and sort primitives (prims.h) and, for the triplet form, the
// triplets -> CSR layer (csrbuild.h).  The assembly (assemble.hip) calls it on the matrices of compute_IvAE.  Compiled with
// -ffp-contract=off like every bookkeeping unit.  Only smooth_check and smooth_matrix (smooth.h) are seen outside this file; the
// kernels and SmoothView, their argument, keep their names in namespace ibh.
#include "smooth.h"
#include "smooth_plan.h"
#include "csrbuild.h"
#include "prims.h"
#include <algorithm>
#include <mutex>
#include <vector>

namespace ibh {

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
static __device__ __forceinline__ bool smooth_tuple(const SmoothView &v, int d, double c[3]) {
    const int64_t s = v.row_s[d];
    const double e = v.em[s];
    if (e != e) return false;               // masked cells are not tuples (smoother.cpp:83-84)
    c[0] = v.cen[2 * s]; c[1] = v.cen[2 * s + 1]; c[2] = e;
    return true;
}
static __device__ __forceinline__ int smooth_bin(const SmoothView &v, const double c[3]) {
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
static __device__ __forceinline__ double smd_wave_sum(double v) {
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

void smooth_check(const ibh_regrid_matrices *rm, const double sigma[3]) {
    IBH_CHECK(rm->rg->has_centroid, "smoothing (sigma != 0) needs the ice grid's centroid_xy (ibh_regridder_desc.I_centroid_xy)");
    IBH_CHECK(sigma[0] > 0 && sigma[1] > 0 && sigma[2] > 0, "smoothing needs three positive sigmas, got (%g, %g, %g)", sigma[0], sigma[1], sigma[2]);
}
// ---- the smoothed build on the host: smooth_matrix (below) takes the plan (smooth_plan.h), bins the rows and tries the plan's forms in
// order; a form builds a new CSR beside the one it reads and returns false, with nothing touched, when its tables overflow
namespace {
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
    if (bf.nbits > 0) radix_sort_pairs_front(bkeys, bkeys2, brows, brows2, (size_t)n, &bf, 1, st);
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
    if (ns && sf[0].nbits > 0) radix_sort_pairs_front(sk, sk2, si, si2, ns, sf, 2, st);
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
}  // namespace
// (comm: smooth.h)
void smooth_matrix(ibh_weighted *w, const ibh_regrid_matrices *rm, const int64_t *row_s, const double sigma[3], hipStream_t st,
                   ibh_comm *comm) {
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

}  // namespace ibh
