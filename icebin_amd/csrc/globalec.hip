// globalec.hip -- the chunked half of modele/global_ec.cpp (main(), below "Check that I grid fits neatly into O grid",
// :752-893) and modele/combine_global_ec.cpp's combine_chunks (:94-262); DESIGN.md 19.
//
// Where things live.  The two int16 planes FGICE1m / ZICETOP1m stay on the device in their own width.  One pass over both
// (k_gec_scan) counts the ice cells of every ocean cell's tile and takes the elevation range of the ice; the ice fraction on
// the ocean grid is the existing typed regrid with the constant weight 1.  The chunk plan masks the counts with fgiceO != 0,
// scans them (prims.h) and reads the nO + 1 sums back once; the walk over them is host code.  A chunk's mask is one launch
// (k_gec_mask).  combine_chunks numbers the chunks' row and column keys first-seen (sparseset.h number_stream), adds the
// weights chunk by chunk with plain read-modify-write -- a key occurs once per chunk, so each launch touches a cell once and
// the launches are stream-ordered -- and hands the triplet stream to the triplets -> CSR layer (csrbuild.h).  The scan's 16-byte
// split of a row and its eight-cell loads are planetile.h's, shared with etopo1.hip and topoo.hip.
#include <algorithm>
#include <cmath>
#include <memory>

#include "common.h"
#include "csrbuild.h"
#include "csrops.h"
#include "planetile.h"
#include "prims.h"
#include "sparseset.h"

struct ibh_global_ec_scan {
    int device = 0;
    int32_t imO = 0, jmO = 0, imI = 0, jmI = 0, mult_i = 0, mult_j = 0;
    ibh::DevBuf<int16_t> fg_own, el_own;    // a host plane, uploaded once in its own width
    const int16_t *fg = nullptr, *el = nullptr;     // the planes: the copies above, or the caller's (which outlive the scan)
    ibh::DevBuf<double> fgiceO;             // [nO]
    ibh::DevBuf<int32_t> nice;              // [nO]
    ibh::DevBuf<uint32_t> cmask;            // [nO] fgiceO != 0 ? nice : 0
    ibh::DevBuf<uint32_t> excl;             // [nO + 1] exclusive scan of cmask, then the total
    std::vector<uint32_t> excl_h;           // read back by the first chunk plan
    int32_t range[2] = {10000, -10000};
    int64_t nO() const { return (int64_t)imO * jmO; }
    int64_t nI() const { return (int64_t)imI * jmI; }
};

namespace ibh {
namespace {

constexpr int GEC_T = 256;
constexpr int GEC_MAXCELLS = 2048;      // O cells of one workgroup's longitude slice (their counts live in LDS)

// ---- the ice scan (:805-813 and the tile counts of :876-886) ---------------------------------------------------------------------
// Workgroup (jO, slice) owns the O cells [o0, o0 + nc) of ocean row jO: mult_j ice rows, columns [o0 * mult_i, (o0 + nc) * mult_i).
// A row is read in 16-byte pieces (8 cells) between a head and a tail of fewer than 8 cells each, which go one cell a thread (the
// FGICE1m row's PlaneSplit); a piece may straddle O cells, so its cells are walked with the tile index carried along.  The elevation
// piece is read only where the piece holds ice.  Counts and the range are integers: LDS atomics give the same result in any order.
__global__ __launch_bounds__(GEC_T) void k_gec_scan(const int16_t *__restrict__ fg, const int16_t *__restrict__ el, int imI, int imO, int mult_i,
                                                    int mult_j, int cps, int nslice, int32_t *__restrict__ nice, int32_t *__restrict__ part) {
    __shared__ int s_cnt[GEC_MAXCELLS];
    __shared__ int s_mn, s_mx;
    const int tid = threadIdx.x;
    const int jO = blockIdx.x / nslice, sl = blockIdx.x - jO * nslice;
    const int o0 = sl * cps, nc = min(cps, imO - o0);
    for (int c = tid; c < nc; c += GEC_T) s_cnt[c] = 0;
    if (tid == 0) { s_mn = 10000; s_mx = -10000; }
    __syncthreads();
    const int len = nc * mult_i;
    int mn = 10000, mx = -10000;
    for (int r = 0; r < mult_j; ++r) {
        const size_t base = ((size_t)jO * mult_j + r) * (size_t)imI + (size_t)o0 * mult_i;
        const int16_t *f = fg + base, *e = el + base;
        const PlaneSplit S = plane_split(f, (unsigned)len);
        const int npiece = (int)S.npiece;
        const bool evec = (((uintptr_t)(e + S.head)) & 15) == 0;
        if (tid < (int)S.nloose((unsigned)len)) {
            const int x = (int)S.cell((unsigned)tid);
            if (f[x] != 0) {
                atomicAdd(&s_cnt[x / mult_i], 1);
                const int v = e[x];
                mn = min(mn, v); mx = max(mx, v);
            }
        }
        for (int p = tid; p < npiece; p += GEC_T) {
            const int x0 = (int)S.piece((unsigned)p);
            const short8 fv = load8(f + x0, true);
            bool any = false;
#pragma unroll
            for (int k = 0; k < 8; ++k) any |= fv[k] != 0;
            if (!any) continue;
            const short8 ev = load8(e + x0, evec);
            int o = x0 / mult_i, rem = x0 - o * mult_i, run = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (fv[k] != 0) {
                    ++run;
                    const int v = ev[k];
                    mn = min(mn, v); mx = max(mx, v);
                }
                if (++rem == mult_i) {
                    if (run) atomicAdd(&s_cnt[o], run);
                    run = 0; rem = 0; ++o;
                }
            }
            if (run) atomicAdd(&s_cnt[o], run);     // (rem != 0 here: o is still a cell of the slice)
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        mn = min(mn, __shfl_xor(mn, off, 64));
        mx = max(mx, __shfl_xor(mx, off, 64));
    }
    if ((tid & 63) == 0) { atomicMin(&s_mn, mn); atomicMax(&s_mx, mx); }
    __syncthreads();
    for (int c = tid; c < nc; c += GEC_T) nice[(size_t)jO * imO + o0 + c] = s_cnt[c];
    if (tid == 0) { part[2 * blockIdx.x] = s_mn; part[2 * blockIdx.x + 1] = s_mx; }
}

// the workgroups' ranges -> range[2]; one workgroup
__global__ __launch_bounds__(GEC_T) void k_gec_range(const int32_t *__restrict__ part, int npart, int32_t *__restrict__ range) {
    __shared__ int s_mn, s_mx;
    if (threadIdx.x == 0) { s_mn = 10000; s_mx = -10000; }
    __syncthreads();
    int mn = 10000, mx = -10000;
    for (int b = threadIdx.x; b < npart; b += GEC_T) { mn = min(mn, part[2 * b]); mx = max(mx, part[2 * b + 1]); }
    for (int off = 32; off > 0; off >>= 1) {
        mn = min(mn, __shfl_xor(mn, off, 64));
        mx = max(mx, __shfl_xor(mx, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { atomicMin(&s_mn, mn); atomicMax(&s_mx, mx); }
    __syncthreads();
    if (threadIdx.x == 0) { range[0] = s_mn; range[1] = s_mx; }
}

// c[k] = fgiceO[k] != 0 ? nice[k] : 0 (:878)
__global__ void k_gec_mask_counts(const double *__restrict__ fgiceO, const int32_t *__restrict__ nice, long nO, uint32_t *__restrict__ c) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nO) c[k] = fgiceO[k] != 0 ? (uint32_t)nice[k] : 0u;
}

// ---- a chunk's mask (:818-855) -----------------------------------------------------------------------------------------------------
// A thread takes GEC_MU pairs of consecutive cells of the flat plane, a workgroup's width apart: a pair is one 4-byte load from
// each int16 plane and one 16-byte store, so a wave's store covers 1 KiB of whole lines (pairs need the int16 bases 4-byte and
// the mask 16-byte aligned -- vec -- else the cells go one by one).  All loads of a thread are issued before its first store.
// cmask[k] != 0 stands for fgiceO[k] != 0: a tile whose masked count is 0 holds no ice cell that could pass.
constexpr int GEC_MU = 4;
typedef short short2v __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(GEC_T) void k_gec_mask(const int16_t *__restrict__ fg, const int16_t *__restrict__ el, const uint32_t *__restrict__ cmask,
                                                    unsigned nI, unsigned imI, unsigned imO, unsigned mult_i, unsigned mult_j, long k0, long k1, int vec,
                                                    double *__restrict__ out) {
    const unsigned base = blockIdx.x * (unsigned)(GEC_T * GEC_MU * 2) + threadIdx.x * 2;
    short2v fv[GEC_MU], ev[GEC_MU];
#pragma unroll
    for (int u = 0; u < GEC_MU; ++u) {
        const unsigned x0 = base + (unsigned)(u * GEC_T * 2);
        fv[u] = short2v{0, 0}; ev[u] = short2v{0, 0};
        if (x0 + 1 < nI && vec) {
            fv[u] = *reinterpret_cast<const short2v *>(fg + x0);
            ev[u] = *reinterpret_cast<const short2v *>(el + x0);
        } else if (x0 < nI) {
            fv[u][0] = fg[x0]; ev[u][0] = el[x0];
            if (x0 + 1 < nI) { fv[u][1] = fg[x0 + 1]; ev[u][1] = el[x0 + 1]; }
        }
    }
#pragma unroll
    for (int u = 0; u < GEC_MU; ++u) {
        const unsigned x0 = base + (unsigned)(u * GEC_T * 2);
        if (x0 >= nI) break;
        double o[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            o[k] = __builtin_nan("");
            if (fv[u][k] != 0) {            // (a cell past the end holds 0)
                const unsigned x = x0 + k, j = x / imI, i = x - j * imI;
                const long kk = (long)(j / mult_j) * imO + i / mult_i;
                if (kk >= k0 && kk < k1 && cmask[kk] != 0) o[k] = (double)ev[u][k];
            }
        }
        if (x0 + 1 < nI && vec) {
            *reinterpret_cast<double2 *>(out + x0) = make_double2(o[0], o[1]);
        } else {
            out[x0] = o[0];
            if (x0 + 1 < nI) out[x0 + 1] = o[1];
        }
    }
}

// ---- combine_chunks (combine_global_ec.cpp:152-249) --------------------------------------------------------------------------
// out[dense[i]] += w[i]: one chunk's weights; a key occurs once per chunk, so no two threads of a launch share a cell
__global__ void k_gec_accum(const int32_t *__restrict__ dense, const double *__restrict__ w, int n, double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[dense[i]] = out[dense[i]] + w[i];
}
// one chunk's entries in stored row-major order (:217-227): the dense ids of the combined sets, the sparse keys, the value
// (times sM of its row when scaling).  dB / kB and dA / kA are this chunk's parts of the key streams.
__global__ void k_gec_emit(Csr M, long nnz, const int32_t *__restrict__ dB, const int32_t *__restrict__ dA, const int64_t *__restrict__ kB,
                           const int64_t *__restrict__ kA, const double *__restrict__ sM, int32_t *__restrict__ drow, int32_t *__restrict__ dcol,
                           double *__restrict__ val, int64_t *__restrict__ sB, int64_t *__restrict__ sA) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    int lo = 0, hi = M.nrow;            // the last row r with rowptr[r] <= e
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (M.rowptr[mid] <= e) lo = mid; else hi = mid;
    }
    const int c = M.colind[e], d = dB[lo];
    drow[e] = d; dcol[e] = dA[c];
    sB[e] = kB[lo]; sA[e] = kA[c];
    val[e] = sM ? M.val[e] * sM[d] : M.val[e];
}

void check_nesting(int32_t imO, int32_t jmO, int32_t imI, int32_t jmI) {
    IBH_CHECK(imO > 0 && jmO > 0 && imI > 0 && jmI > 0, "hspecO / hspecI: grid sizes (%dx%d), (%dx%d) must be positive", imO, jmO, imI, jmI);
    IBH_CHECK((imI / imO) * imO == imI && (jmI / jmO) * jmO == jmI, "hspecI: Hntr grid (%dx%d) must be an even multiple of (%dx%d)", imI, jmI,
              imO, jmO);
}

std::unique_ptr<ibh_global_ec_scan> scan_create(int32_t imO, int32_t jmO, double offiO, double dlatO, int32_t imI, int32_t jmI, double offiI,
                                                double dlatI, const void *fgiceI, const void *elevI, int64_t nplane, int plane_type,
                                                int on_device, void *stream) {
    check_nesting(imO, jmO, imI, jmI);
    IBH_CHECK(fgiceI && elevI, "fgiceI / elevI: null plane");
    IBH_CHECK(plane_type == IBH_HNTR_I16, "fgiceI / elevI: plane type %d, the ice planes are int16 (IBH_HNTR_I16 = %d)", plane_type, IBH_HNTR_I16);
    IBH_CHECK((int64_t)imI * jmI < (1ll << 31), "hspecI: %lld ice cells overflow int32", (long long)imI * jmI);
    IBH_CHECK(nplane == (int64_t)imI * jmI, "fgiceI / elevI: the planes hold %lld cells, hspecI has %lld", (long long)nplane, (long long)imI * jmI);
    IBH_CHECK(on_device == 0 || on_device == 1, "on_device must be 0 or 1");
    IBH_CHECK((((uintptr_t)fgiceI | (uintptr_t)elevI) & 1) == 0, "fgiceI / elevI: a plane is not aligned to int16");
    require_device();
    std::unique_ptr<ibh_global_ec_scan> s(new ibh_global_ec_scan);
    IBH_HIP(hipGetDevice(&s->device));
    s->imO = imO; s->jmO = jmO; s->imI = imI; s->jmI = jmI; s->mult_i = imI / imO; s->mult_j = jmI / jmO;
    const int64_t nO = s->nO(), nI = s->nI();
    hipStream_t st = on_device ? (hipStream_t)stream : hipStreamPerThread;
    if (on_device) {
        s->fg = static_cast<const int16_t *>(fgiceI); s->el = static_cast<const int16_t *>(elevI);
    } else {
        s->fg_own.upload(static_cast<const int16_t *>(fgiceI), (size_t)nI, st);
        s->el_own.upload(static_cast<const int16_t *>(elevI), (size_t)nI, st);
        s->fg = s->fg_own.p; s->el = s->el_own.p;
    }
    // fgiceO = Hntr(17.17, hspecO, hspecI).regrid(const 1.0, fgiceI) (:778-780)
    s->fgiceO.alloc((size_t)nO);
    {
        ibh_hntr *hraw = nullptr;
        rethrow(ibh_hntr_create(&hraw, imI, jmI, offiI, dlatI, imO, jmO, offiO, dlatO, 0.));
        std::unique_ptr<ibh_hntr, int (*)(ibh_hntr *)> hntr(hraw, ibh_hntr_destroy);
        rethrow(ibh_hntr_regrid_typed_device(hntr.get(), nullptr, IBH_HNTR_F64, 0, 1.0, s->fg, IBH_HNTR_I16, 1, nI, s->fgiceO.p, nO, 0, 1., 0., st));
        IBH_HIP(hipStreamSynchronize(st));      // the regridder's tables go away
    }
    // the longitude slices: enough workgroups to fill the chip when jmO alone does not, and no more cells than LDS holds
    int nslice = (int)std::min<long>(imO, std::max<long>(cdiv(imO, GEC_MAXCELLS), cdiv(1024, jmO)));
    const int cps = (int)cdiv(imO, nslice);
    nslice = (int)cdiv(imO, cps);
    const long nwg = (long)jmO * nslice;
    IBH_CHECK(cps <= GEC_MAXCELLS && nwg < (1l << 31), "internal: scan slices");
    s->nice.alloc((size_t)nO); s->cmask.alloc((size_t)nO); s->excl.alloc((size_t)nO + 1);
    DevBuf<int32_t> part((size_t)(2 * nwg) + 2);
    hipLaunchKernelGGL(k_gec_scan, dim3((unsigned)nwg), dim3(GEC_T), 0, st, s->fg, s->el, imI, imO, s->mult_i, s->mult_j, cps, nslice, s->nice.p,
                       part.p);
    hipLaunchKernelGGL(k_gec_range, dim3(1), dim3(GEC_T), 0, st, part.p, (int)nwg, part.p + 2 * nwg);
    hipLaunchKernelGGL(k_gec_mask_counts, dim3((unsigned)cdiv(nO, GEC_T)), dim3(GEC_T), 0, st, s->fgiceO.p, s->nice.p, (long)nO, s->cmask.p);
    IBH_HIP(hipGetLastError());
    exclusive_scan_u32(s->cmask.p, s->excl.p, (size_t)nO, s->excl.p + nO, st);
    readback_sync(s->range, part.p + 2 * nwg, sizeof(s->range), st);
    return s;
}

// The walk of :868-893 over excl[nO + 1], the exclusive sums of the masked counts followed by their total.  Chunk n starts
// where chunk n - 1 ended and ends, exclusive, at the first cell whose running sum from the start (that cell included)
// reaches chunk_size -- the cell goes to the next chunk (goto endscan2 leaves iO where it is), its ice is in this one's
// reported nice -- or at nO.  chunk_size > mult_i * mult_j: a cell that holds chunk_size on its own would end every chunk
// where it starts, and the reference's loop would never finish.
int32_t chunk_walk(const uint32_t *excl, int32_t imO, int32_t jmO, int64_t chunk_size, int32_t cap, int32_t *chunks, int64_t *nice) {
    const int64_t nO = (int64_t)imO * jmO;
    int32_t n = 0;
    for (int64_t start = 0; start < nO; ++n) {
        const uint64_t target = (uint64_t)excl[start] + (uint64_t)chunk_size;
        // first k >= start with excl[k + 1] >= target
        const uint32_t *p = std::lower_bound(excl + start + 1, excl + nO + 1, target, [](uint32_t a, uint64_t b) { return (uint64_t)a < b; });
        const int64_t end = p == excl + nO + 1 ? nO : (int64_t)(p - excl) - 1;
        if (n < cap) {
            if (chunks) {
                int32_t *c = chunks + 5 * (size_t)n;
                c[0] = n; c[1] = (int32_t)(start / imO); c[2] = (int32_t)(start % imO); c[3] = (int32_t)(end / imO); c[4] = (int32_t)(end % imO);
            }
            if (nice) nice[n] = (int64_t)(end == nO ? excl[nO] : excl[end + 1]) - (int64_t)excl[start];
        }
        start = end;
        if (end == nO) { ++n; break; }
    }
    return n;
}

void check_plan_args(int32_t mult_i, int32_t mult_j, int64_t chunk_size, int32_t cap, const int32_t *nchunks) {
    IBH_CHECK(nchunks, "nchunks: null argument");
    IBH_CHECK(cap >= 0, "cap: negative capacity %d", cap);
    IBH_CHECK(chunk_size > (int64_t)mult_i * mult_j, "chunk_size: %lld must exceed the %lld ice cells of one ocean cell (%dx%d)",
              (long long)chunk_size, (long long)mult_i * mult_j, mult_i, mult_j);
}

// one chunk's part of the inputs
struct ChunkIn {
    const ibh_weighted *w;
    const int64_t *hdim[2];     // host dims the caller names in place of the handle's sets (null: the handle's)
    int64_t ext[2];
};

void combine_chunks(int32_t nchunks, const ibh_weighted *const *mats, const int64_t *const *dims_host, const int64_t *extents, int scale,
                    int64_t *stream_iB, int64_t *stream_iA, double *stream_val, ibh_weighted **out) {
    IBH_CHECK(out, "out: null argument");
    IBH_CHECK(nchunks >= 1 && mats, "mats: combine_chunks needs at least one chunk");
    IBH_CHECK(scale == 0 || scale == 1, "scale must be 0 or 1");
    IBH_CHECK((dims_host == nullptr) == (extents == nullptr), "dims_host / extents: give both or neither");
    std::vector<ChunkIn> ch((size_t)nchunks);
    int64_t nB = 0, nA = 0, nnz = 0;
    int conservative = 1;
    for (int c = 0; c < nchunks; ++c) {
        const ibh_weighted *w = mats[c];
        IBH_CHECK(w, "mats: chunk %d is null", c);
        IBH_CHECK(!w->scaled, "mats: chunk %d's matrix is scaled; combine_chunks takes the unscaled matrices of write_matrices", c);
        ChunkIn &k = ch[(size_t)c];
        k.w = w;
        for (int d = 0; d < 2; ++d) {
            k.hdim[d] = dims_host ? dims_host[2 * c + d] : nullptr;
            const int n = d == 0 ? w->nrow : w->ncol;
            if (dims_host) {
                IBH_CHECK(k.hdim[d] || n == 0, "dims_host: chunk %d, dimension %d is null", c, d);
                k.ext[d] = extents[2 * c + d];
                // a handle's own set holds a key once; a table from a file must too (k_gec_accum gives a key's cell to one thread)
                std::vector<int64_t> keys(k.hdim[d], k.hdim[d] + n);
                std::sort(keys.begin(), keys.end());
                const auto dup = std::adjacent_find(keys.begin(), keys.end());
                IBH_CHECK(dup == keys.end(), "dims_host: chunk %d, dimension %d names the sparse index %lld twice", c, d,
                          dup == keys.end() ? 0ll : (long long)*dup);
            } else {
                const ibh_sparse_set *s = w->dims[d].get();
                IBH_CHECK(s && s->n() >= n, "mats: chunk %d's matrix has %d %s, its set %d entries", c, n, d == 0 ? "rows" : "columns", s ? s->n() : 0);
                k.ext[d] = s->sparse_extent();
            }
        }
        IBH_CHECK(k.ext[0] == ch[0].ext[0] && k.ext[1] == ch[0].ext[1], "mats: chunk %d has sparse extents (%lld, %lld), chunk 0 (%lld, %lld)", c,
                  (long long)k.ext[0], (long long)k.ext[1], (long long)ch[0].ext[0], (long long)ch[0].ext[1]);
        nB += w->nrow; nA += w->ncol; nnz += w->nnz;
        conservative &= w->conservative != 0;
    }
    IBH_CHECK(ch[0].ext[0] >= 0 && ch[0].ext[1] >= 0, "mats: the chunks' sets have no sparse extent");
    IBH_CHECK(nB < (1ll << 31) && nA < (1ll << 31) && nnz < (1ll << 31), "mats: %lld rows, %lld columns, %lld entries overflow int32", (long long)nB,
              (long long)nA, (long long)nnz);
    IBH_CHECK(nnz == 0 || ((stream_iB == nullptr) == (stream_iA == nullptr) && (stream_iA == nullptr) == (stream_val == nullptr)),
              "stream_iB / stream_iA / stream_val: give all three or none");
    require_device();
    for (int c = 0; c < nchunks; ++c) check_current_device(mats[c]->device, "chunk matrix");
    hipStream_t st = hipStreamPerThread;

    // the two key streams: dimB_c[i] for i < len(wM_c), dimA_c[i] for i < len(Mw_c), chunks in order
    DevBuf<int64_t> key[2] = {DevBuf<int64_t>((size_t)nB), DevBuf<int64_t>((size_t)nA)};
    DevBuf<int32_t> dense[2] = {DevBuf<int32_t>((size_t)nB), DevBuf<int32_t>((size_t)nA)};
    for (int d = 0; d < 2; ++d) {
        int64_t off = 0;
        for (const ChunkIn &k : ch) {
            const int n = d == 0 ? k.w->nrow : k.w->ncol;
            if (n && k.hdim[d]) IBH_HIP(hipMemcpyAsync(key[d].p + off, k.hdim[d], sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, st));
            else if (n) k.w->dims[d]->copy_to_sparse(key[d].p + off, n, st);
            off += n;
        }
    }
    auto setB = std::make_unique<ibh_sparse_set>(), setA = std::make_unique<ibh_sparse_set>();
    arena().reset();
    number_stream(*setB, ch[0].ext[0], key[0].p, (long)nB, dense[0].p, "combine_chunks: rows (dimB)", st);
    number_stream(*setA, ch[0].ext[1], key[1].p, (long)nA, dense[1].p, "combine_chunks: columns (dimA)", st);
    const int nBo = setB->n(), nAo = setA->n();

    // wM_out / Mw_out: from 0.0, chunk by chunk (:197-200, :247-249); sM = 1 / the same sums (:152-174)
    DevBuf<double> wM((size_t)nBo), Mw((size_t)nAo), sM;
    wM.zero(st); Mw.zero(st);
    {
        int64_t offB = 0, offA = 0;
        for (const ChunkIn &k : ch) {
            const int nr = k.w->nrow, nc = k.w->ncol;
            if (nr) hipLaunchKernelGGL(k_gec_accum, dim3((unsigned)cdiv(nr, GEC_T)), dim3(GEC_T), 0, st, dense[0].p + offB, k.w->wM.p, nr, wM.p);
            if (nc) hipLaunchKernelGGL(k_gec_accum, dim3((unsigned)cdiv(nc, GEC_T)), dim3(GEC_T), 0, st, dense[1].p + offA, k.w->Mw.p, nc, Mw.p);
            offB += nr; offA += nc;
        }
        IBH_HIP(hipGetLastError());
    }
    if (scale) recip(wM.p, nBo, sM, st);

    // the triplet stream (:217-227)
    DevBuf<int32_t> drow((size_t)nnz), dcol((size_t)nnz);
    DevBuf<double> val((size_t)nnz);
    DevBuf<int64_t> sB((size_t)nnz), sA((size_t)nnz);
    {
        int64_t offB = 0, offA = 0, off = 0;
        for (const ChunkIn &k : ch) {
            const ibh_weighted &M = *k.w;
            if (M.nnz)
                hipLaunchKernelGGL(k_gec_emit, dim3((unsigned)cdiv(M.nnz, GEC_T)), dim3(GEC_T), 0, st, view(M), (long)M.nnz, dense[0].p + offB,
                                   dense[1].p + offA, key[0].p + offB, key[1].p + offA, scale ? sM.p : nullptr, drow.p + off, dcol.p + off,
                                   val.p + off, sB.p + off, sA.p + off);
            offB += M.nrow; offA += M.ncol; off += M.nnz;
        }
        IBH_HIP(hipGetLastError());
    }
    auto w = new_weighted();
    csr_from_device_triplets(w.get(), nBo, nAo, nnz, drow.p, dcol.p, val.p, st);
    if (stream_val && nnz) {
        IBH_HIP(hipMemcpyAsync(stream_iB, sB.p, sizeof(int64_t) * (size_t)nnz, hipMemcpyDeviceToHost, st));
        IBH_HIP(hipMemcpyAsync(stream_iA, sA.p, sizeof(int64_t) * (size_t)nnz, hipMemcpyDeviceToHost, st));
        IBH_HIP(hipMemcpyAsync(stream_val, val.p, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToHost, st));
    }
    w->wM = std::move(wM);
    w->Mw = std::move(Mw);
    w->conservative = conservative; w->scaled = scale;
    IBH_HIP(hipStreamSynchronize(st));
    w->dims[0] = DimRef::owned(std::move(setB));
    w->dims[1] = DimRef::owned(std::move(setA));
    *out = w.release();
}

}  // namespace
}  // namespace ibh

using namespace ibh;
extern "C" {

int ibh_global_ec_scan_create(int32_t imO, int32_t jmO, double offiO, double dlatO, int32_t imI, int32_t jmI, double offiI, double dlatI,
                              const void *fgiceI, const void *elevI, int64_t nplane, int plane_type, int on_device, void *stream,
                              ibh_global_ec_scan **out) {
    if (out) *out = nullptr;
    return guarded([&] {
        IBH_CHECK(out, "out: null argument");
        *out = scan_create(imO, jmO, offiO, dlatO, imI, jmI, offiI, dlatI, fgiceI, elevI, nplane, plane_type, on_device, stream).release();
    });
}

int ibh_global_ec_scan_destroy(ibh_global_ec_scan *s) {
    return guarded([&] { delete s; });
}

int ibh_global_ec_scan_get(const ibh_global_ec_scan *s, const double **d_fgiceO, const int32_t **d_nice, int16_t *elevI_range, double *fgiceO,
                           int32_t *nice) {
    return guarded([&] {
        IBH_CHECK(s, "scan: null argument");
        check_current_device(s->device, "scan");
        if (d_fgiceO) *d_fgiceO = s->fgiceO.p;
        if (d_nice) *d_nice = s->nice.p;
        if (elevI_range) { elevI_range[0] = (int16_t)s->range[0]; elevI_range[1] = (int16_t)s->range[1]; }
        if (fgiceO) s->fgiceO.download(fgiceO, (size_t)s->nO(), hipStreamPerThread);
        if (nice) s->nice.download(nice, (size_t)s->nO(), hipStreamPerThread);
    });
}

int ibh_global_ec_scan_copy_device(const ibh_global_ec_scan *s, double *d_fgiceO, int32_t *d_nice, void *stream) {
    return guarded([&] {
        IBH_CHECK(s, "scan: null argument");
        check_current_device(s->device, "scan");
        hipStream_t st = (hipStream_t)stream;
        if (d_fgiceO) IBH_HIP(hipMemcpyAsync(d_fgiceO, s->fgiceO.p, sizeof(double) * (size_t)s->nO(), hipMemcpyDeviceToDevice, st));
        if (d_nice) IBH_HIP(hipMemcpyAsync(d_nice, s->nice.p, sizeof(int32_t) * (size_t)s->nO(), hipMemcpyDeviceToDevice, st));
    });
}

int ibh_global_ec_ec_range(const int16_t *elevI_range, double ec_skip, double *ec_range) {
    return guarded([&] {
        IBH_CHECK(elevI_range && ec_range, "elevI_range / ec_range: null argument");
        IBH_CHECK(ec_skip > 0, "ec_skip: %g must be positive", ec_skip);
        ec_range[0] = ec_skip * std::floor((double)elevI_range[0] / ec_skip);
        ec_range[1] = ec_skip * std::ceil((double)elevI_range[1] / ec_skip);
    });
}

int ibh_global_ec_chunk_plan_counts(int32_t imO, int32_t jmO, int32_t mult_i, int32_t mult_j, const int32_t *counts, int64_t chunk_size,
                                    int32_t cap, int32_t *chunks, int64_t *nice, int32_t *nchunks) {
    return guarded([&] {
        IBH_CHECK(imO > 0 && jmO > 0 && mult_i > 0 && mult_j > 0, "imO / jmO / mult_i / mult_j must be positive");
        IBH_CHECK(counts, "counts: null argument");
        check_plan_args(mult_i, mult_j, chunk_size, cap, nchunks);
        const int64_t nO = (int64_t)imO * jmO;
        std::vector<uint32_t> excl((size_t)nO + 1, 0u);
        for (int64_t k = 0; k < nO; ++k) {
            IBH_CHECK(counts[k] >= 0 && counts[k] <= (int64_t)mult_i * mult_j, "counts: cell %lld holds %d ice cells of %lld", (long long)k, counts[k],
                      (long long)mult_i * mult_j);
            IBH_CHECK((uint64_t)excl[(size_t)k] + (uint32_t)counts[k] < (1ull << 32), "counts: the sum overflows 32 bits");
            excl[(size_t)k + 1] = excl[(size_t)k] + (uint32_t)counts[k];
        }
        *nchunks = chunk_walk(excl.data(), imO, jmO, chunk_size, cap, chunks, nice);
    });
}

int ibh_global_ec_chunk_plan(ibh_global_ec_scan *s, int64_t chunk_size, int32_t cap, int32_t *chunks, int64_t *nice, int32_t *nchunks) {
    return guarded([&] {
        IBH_CHECK(s, "scan: null argument");
        check_plan_args(s->mult_i, s->mult_j, chunk_size, cap, nchunks);
        check_current_device(s->device, "scan");
        if (s->excl_h.empty()) {        // the one download of the plan: nO sums and their total
            std::vector<uint32_t> h((size_t)s->nO() + 1);
            s->excl.download(h.data(), h.size(), hipStreamPerThread);
            s->excl_h.swap(h);
        }
        *nchunks = chunk_walk(s->excl_h.data(), s->imO, s->jmO, chunk_size, cap, chunks, nice);
    });
}

int ibh_global_ec_chunk_mask(const ibh_global_ec_scan *s, int32_t jO0, int32_t iO0, int32_t jO1, int32_t iO1, double *d_elevmaskI, int64_t nmask,
                             void *stream) {
    return guarded([&] {
        IBH_CHECK(s, "scan: null argument");
        IBH_CHECK(d_elevmaskI, "d_elevmaskI: null argument");
        IBH_CHECK(nmask == s->nI(), "d_elevmaskI: %lld cells, hspecI has %lld", (long long)nmask, (long long)s->nI());
        IBH_CHECK(((uintptr_t)d_elevmaskI & 7) == 0, "d_elevmaskI: not aligned to double");
        const int64_t k0 = (int64_t)jO0 * s->imO + iO0, k1 = (int64_t)jO1 * s->imO + iO1;
        IBH_CHECK(jO0 >= 0 && iO0 >= 0 && iO0 < s->imO && jO1 >= 0 && iO1 >= 0 && iO1 < s->imO && k0 <= k1 && k1 <= s->nO(),
                  "chunk: [(%d, %d), (%d, %d)) is no range of cells of the %dx%d ocean grid", jO0, iO0, jO1, iO1, s->imO, s->jmO);
        check_current_device(s->device, "scan");
        const int vec = ((((uintptr_t)s->fg | (uintptr_t)s->el) & 3) | ((uintptr_t)d_elevmaskI & 15)) == 0;
        const long nblock = cdiv(s->nI(), (long)GEC_T * GEC_MU * 2);
        hipLaunchKernelGGL(k_gec_mask, dim3((unsigned)nblock), dim3(GEC_T), 0, (hipStream_t)stream, s->fg, s->el, s->cmask.p, (unsigned)s->nI(),
                           (unsigned)s->imI, (unsigned)s->imO, (unsigned)s->mult_i, (unsigned)s->mult_j, (long)k0, (long)k1, vec, d_elevmaskI);
        IBH_HIP(hipGetLastError());
    });
}

int ibh_global_ec_chunk_mask_host(const ibh_global_ec_scan *s, int32_t jO0, int32_t iO0, int32_t jO1, int32_t iO1, double *elevmaskI,
                                  int64_t nmask) {
    return guarded([&] {
        IBH_CHECK(s, "scan: null argument");
        IBH_CHECK(elevmaskI, "elevmaskI: null argument");
        IBH_CHECK(nmask == s->nI(), "elevmaskI: %lld cells, hspecI has %lld", (long long)nmask, (long long)s->nI());
        check_current_device(s->device, "scan");
        DevBuf<double> d((size_t)nmask);
        rethrow(ibh_global_ec_chunk_mask(s, jO0, iO0, jO1, iO1, d.p, nmask, hipStreamPerThread));
        d.download(elevmaskI, (size_t)nmask, hipStreamPerThread);
    });
}

int ibh_global_ec_combine_chunks(int32_t nchunks, const ibh_weighted *const *mats, const int64_t *const *dims_host, const int64_t *extents,
                                 int scale, int64_t *stream_iB, int64_t *stream_iA, double *stream_val, ibh_weighted **out) {
    if (out) *out = nullptr;
    return guarded([&] { combine_chunks(nchunks, mats, dims_host, extents, scale, stream_iB, stream_iA, stream_val, out); });
}

}  // extern "C"
