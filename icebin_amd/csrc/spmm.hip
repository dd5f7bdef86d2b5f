// spmm.hip -- K1: CSR x dense-field products for Weighted::apply on gfx950.
//
// Replaces the Eigen SparseMatrix<ColMajor> * Dense product inside
// ibmisc::linear::Weighted_Eigen::apply (call sites modele/merge_topo.cpp:65,
// modele/icebin22m.cpp:153; inline products IceCoupler.cpp:237,445).
//
// Fields are field-major (X[f*ldx + col], Y[f*ldy + row]): one field is one
// contiguous vector, as blitz::Array<double,2>(nvar, n) is (icebin22m.cpp:142).
// fp64, HBM-bound (<= 0.25 flop/byte): no MFMA.  Two shapes, two kernels:
//
//  * rowblock  -- few long rows (AvI/EvI/AvE direction: 10^2..10^5 rows of
//    10^1..10^4 nnz).  One 256-thread workgroup per (row, chunk of fields).
//    The row segment (colind, vals) is staged once in LDS by all four waves
//    with coalesced loads, then every wave streams its own fields: lane k reads
//    X[f, col[k]], so a wave-load is 64 consecutive-ish doubles of one field
//    (dense column ids of one GCM cell are near-contiguous by construction of
//    the first-seen numbering).  Per-lane accumulators, one butterfly reduction
//    per (row, field) at the end, no atomics -> bitwise reproducible.
//    blockIdx is remapped so that the field-chunks of one row land on the same
//    XCD and share the row segment through that XCD's L2.
//
//  * shortrow  -- millions of rows of 1-3 nnz (IvA/IvE direction).  One thread
//    per row, looping over a chunk of fields with the row's entries held in
//    registers; lanes own consecutive rows, so the dominant traffic -- the
//    Y stores -- is fully coalesced (512 B per wave-store, non-temporal); the
//    small X (nf x nA_d) is served from L2.
#include "common.h"
#include "applystruct.h"
#include "sweep_kernel.inl"
#include <hip/hip_ext.h>
#include <mutex>
#include <set>
#include <type_traits>

namespace ibh {

// ---- tuning knobs (ibh_set_tuning) ---------------------------------------------------------
// Process-wide and read on every apply while another host thread may be calling ibh_set_tuning:
// guarded by a mutex (an uncontended lock is ~20 ns against a >= 3 us launch).
namespace {
struct Tuning {
    std::mutex mu;
    std::unordered_map<std::string, int> map;
};
Tuning &tuning() { static Tuning *t = new Tuning; return *t; }
}  // namespace
// the matrix whose apply is being set up on this thread: its own options (ibh_weighted_set_option) win over the process-wide map
static thread_local const ibh_weighted *tl_handle = nullptr;
struct HandleScope {
    const ibh_weighted *prev;
    explicit HandleScope(const ibh_weighted *w) : prev(tl_handle) { tl_handle = w; }
    ~HandleScope() { tl_handle = prev; }
};
int get_tuning(const char *key, int dflt) {
    if (tl_handle && !tl_handle->st.opts.empty()) {
        auto it = tl_handle->st.opts.find(key);
        if (it != tl_handle->st.opts.end()) return it->second;
    }
    Tuning &t = tuning();
    std::lock_guard<std::mutex> lk(t.mu);
    if (t.map.empty()) return dflt;
    auto it = t.map.find(key);
    return it == t.map.end() ? dflt : it->second;
}
void set_tuning(const char *key, int value) {
    Tuning &t = tuning();
    std::lock_guard<std::mutex> lk(t.mu);
    if (value == INT32_MIN) t.map.erase(key);       // back to the built-in default
    else t.map[key] = value;
}

// ---- launch timing (ibh_set_launch_events) ---------------------------------------------------------
// A caller that wants the duration of the SpMM kernel ITSELF (bench.py's roofline figure: the kernel's
// launch duration, not the host's submission latency in front of it) hands in a pair of HIP events; the
// next rowblock launch of this thread attaches them to its own dispatch (hipExtLaunchKernel: start =
// kernel begins, stop = kernel ends -- the interval rocprofv3's kernel trace reports).  One-shot.
static thread_local hipEvent_t g_ev_start = nullptr, g_ev_stop = nullptr;
void set_launch_events(hipEvent_t start, hipEvent_t stop) { g_ev_start = start; g_ev_stop = stop; }

// ---- helpers -------------------------------------------------------------------------------
// Sum over the 64 lanes of a wave, result valid in every lane.  DPP moves instead of ds_bpermute:
// the shuffle form is six dependent trips through the LDS crossbar (0.6 us measured at the end of
// every workgroup of the headline kernel, on its critical path); this is ~25 VALU instructions.
// Fixed combination order -> bitwise reproducible.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_move(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum(double v) {
    v += dpp_move<0xB1, 0xf>(v);     // quad_perm [1,0,3,2]: pairs
    v += dpp_move<0x4E, 0xf>(v);     // quad_perm [2,3,0,1]: quads
    v += dpp_move<0x141, 0xf>(v);    // row_half_mirror: 8 lanes
    v += dpp_move<0x140, 0xf>(v);    // row_mirror: 16 lanes (every lane of a row holds the row sum)
    v += dpp_move<0x142, 0xa>(v);    // row_bcast15 into rows 1,3: lanes 16-31 = rows 0+1, lanes 48-63 = rows 2+3
    v += dpp_move<0x143, 0xc>(v);    // row_bcast31 into rows 2,3: lanes 48-63 = total
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}

// Workgroups are dealt round-robin over the 8 XCDs (b and b+8 share one).  Give each
// XCD a contiguous range of logical ids, so neighbours in logical order share an L2.
__device__ __forceinline__ int xcd_contiguous(int b, int nb) {
    const int q = nb >> 3, rem = nb & 7;
    const int x = b & 7, slot = b >> 3;
    const int base = x < rem ? x * (q + 1) : rem * (q + 1) + (x - rem) * q;
    return base + slot;
}

// blockIdx -> (row, field chunk).  Workgroups are dealt round-robin over the 8 XCDs, each with its
// own L2.  Two rows that share X lines (an ice cell straddling two GCM cells is a column of both)
// read them for the SAME field chunk, so:
//   mode 1 (nfc a multiple of 8, or 1/2/4): an XCD owns whole field chunks and runs every row for
//           them -- no X line is fetched by two XCDs, all XCDs do identical work; the (small) CSR
//           is read by every XCD and served from the memory-side Infinity Cache after the first.
//   mode 0: contiguous ranges of (row, chunk) pairs per XCD (rows of one chunk share the staged
//           CSR segment through L2); used when the chunk count does not split over 8 XCDs.
__device__ __forceinline__ bool block_to_task(int b, int nrow, int nfc, int mode, int &r, int &fc) {
    if (mode == 1) {
        const int x = b & 7, slot = b >> 3;
        if (nfc >= 8) {                       // nfc % 8 == 0
            const int per = nfc >> 3;
            r = slot / per;
            fc = x + 8 * (slot - r * per);
        } else {                              // nfc in {1,2,4}: 8/nfc XCDs share one chunk, split by row range
            const int m = 8 / nfc;
            fc = x % nfc;
            const int part = x / nfc;
            const int r0 = (int)((long)nrow * part / m), r1 = (int)((long)nrow * (part + 1) / m);
            r = r0 + slot;
            if (r >= r1) return false;
        }
        return r < nrow;
    }
    const int logical = xcd_contiguous(b, (int)gridDim.x);     // gridDim.x = nrow*nfc rounded up to a multiple of 8
    if (logical >= nrow * nfc) return false;
    r = logical / nfc;
    fc = logical - r * nfc;
    return true;
}

constexpr int RB_SEG = 1024;    // nnz staged per pass: 12 KB of LDS

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// One field's X row through a buffer descriptor: 32-bit per-lane byte offset, SGPR base.  The
// same voffset (col << 3) serves every field of the wave, so a gathered element costs one
// buffer_load + one FMA instead of a 64-bit address computation per load; at the 40 MB headline
// size the kernel is as much instruction-issue- as bandwidth-limited.
__device__ __forceinline__ double xload(__amdgpu_buffer_rsrc_t rs, int byte_off) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, byte_off, 0, 0));
}

// The tail batch of a row kernel: the last NU <= UNROLL slots of a wave's share of a staged segment, k = k0 + u * STEP < n
// (k0 holds the lane).  Every lane issues its NU * FPW gathers before the first FMA; the weights are read from LDS when the
// gathered values are consumed.  Slots below NU - 1 are full in every lane; in the last one the lanes past the end re-read the
// last entry and are masked at the FMA (never multiplied by 0: 0*NaN must not leak into a row).
template <int FPW, int NU, int STEP>
__device__ __forceinline__ void tail_slots(const int *s_col, const double *s_val, const __amdgpu_buffer_rsrc_t (&rs)[FPW], int k0, int n,
                                           double (&acc)[FPW]) {
    double x[FPW][NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int k = k0 + u * STEP;
        const int off = s_col[u < NU - 1 || k < n ? k : n - 1] << 3;
#pragma unroll
        for (int j = 0; j < FPW; ++j) x[j][u] = xload(rs[j], off);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int k = k0 + u * STEP;
        const bool ok = u < NU - 1 || k < n;
        const double v = s_val[ok ? k : n - 1];
#pragma unroll
        for (int j = 0; j < FPW; ++j) acc[j] = ok ? fma(v, x[j][u], acc[j]) : acc[j];
    }
}
// f(integral_constant<nu>) for a wave-uniform nu in 1..N.  A row issues only the slots that hold entries of it (the 5 km rows
// need 11.0 of 14 on average, a one-entry row 1; the others re-read the last entry for nothing), and each count is its own
// straight-line body: the wait in front of FMA u is then the constant NU - 1 - u, as it is in a full batch.  (Skipping slots
// inside ONE unrolled body makes the first FMA wait for every load: leave the body early and the number of loads behind a slot
// is no constant any more; enter it late -- the last nu slots, which keeps that number -- and the compiler, as built, still
// waits vmcnt(0) per slot and spills the gathered values: 92 bytes of scratch in rowblock<1, 1, 14, 8>.)
template <int N, class F>
__device__ __forceinline__ void with_slot_count(int nu, F &&f) {
    if constexpr (N > 1) {
        if (nu < N) { with_slot_count<N - 1>(nu, f); return; }
    }
    f(std::integral_constant<int, N>{});
}

// Field batches of one launch (ibh_weighted_apply_many_device): batch q reads x[q] and writes y[q],
// all with the same nvar / leading dimensions.  Passed by value in the kernarg segment, so a launch
// needs no device-side pointer table and stays stream-ordered and graph-capturable.
struct BatchPtrs {
    const double *x[IBH_MAX_BATCH];
    double *y[IBH_MAX_BATCH];
};

// FPW = fields per wave, WK = waves that split the nnz range of the row, NW = waves per workgroup.
// The NW waves form WF = NW/WK groups over fields; a block covers FB = FPW*WF fields and stages
// the row segment once for all of them.
//
// Batched launches (nbatch > 1): blockIdx.y = batch group; a workgroup serves `qi` consecutive
// batches of its (row, field chunk) with the row segment staged ONCE (rows of <= RB_SEG entries).
// A 40 MB apply is a latency-sized problem on this chip (launch + rowptr -> segment -> X are
// ~4 us of an 11 us launch); in one launch over several batches the workgroups of batch q+1 start
// while those of batch q still stream, so the prologue and the drain are paid once per LAUNCH.
// (Tried and dropped: renumbering the workgroups so that the batch groups of one (row, chunk) follow each other on one XCD and
// the row's CSR segment comes from the fabric once per launch instead of once per group.  With a buffer of its own for every
// batch of the launch it is SLOWER, 6.89 -> 7.83 us per apply at the headline shape: sixteen different X streams at once per
// XCD instead of one cost more than the 0.1 x of re-read CSR the Infinity Cache serves.  It looks faster, 6.8 -> 5.2 us, only
// where a launch holds the same X several times, because the repeats then meet in L2.  DESIGN.md section 3.)
//
// DUAL (EvI, EvX; WK == 1): the "row" is a BAND -- the ice cells of one GCM cell whose elevation lies
// between two neighbouring classes.  Such a cell is a column of two rows of M (weights 1-r and r on
// the lower and the upper class); as a band entry it carries both values (vals, vals2; bits 30/31 of
// the column say which exist) and is read ONCE, feeding two accumulators.  Row by row every X element
// of these matrices is fetched twice (measured: 2.0 GB for 1.03 GB algorithmic at 1 km).  The kernel
// then stores the two partial sums of the band (Y = lower-class sums, Y2 = upper-class sums, no
// fill); dual_combine_kernel adds, for every row, its own lower sum and the upper sum of the band
// below it.  The band arrays are a filtered copy of the CSR (applystruct.hip build_bands).
template <int FPW, int WK, int UNROLL, int NW, bool DUAL = false>
__global__ __launch_bounds__(NW * 64, (FPW == 1 && !DUAL) ? 8 : 1) void spmm_rowblock_kernel(
    const int *__restrict__ rowptr, const int *__restrict__ colind, const double *__restrict__ vals,
    const BatchPtrs bp, int nbatch, int qi, long ldx, int ncol, long ldy, int nrow, int nf, int nfc,
    int xcd_mode, const double *__restrict__ wM, double fill,
    const double *__restrict__ vals2 = nullptr, double *__restrict__ Y2 = nullptr,
    const int *__restrict__ rowperm = nullptr, long y2_stride = 0)
{
    static_assert(!DUAL || WK == 1, "bands are not split across waves");
    constexpr int RB_THREADS = NW * 64;
    constexpr int RB_STAGE = RB_SEG / RB_THREADS;
    constexpr int WF = NW / WK;
    constexpr int FB = FPW * WF;
    constexpr int STEP = WK * 64;
    constexpr int BATCH = UNROLL * STEP;
    __shared__ int s_col[RB_SEG];
    __shared__ double s_val[RB_SEG];
    __shared__ double s_val2[DUAL ? RB_SEG : 1];
    __shared__ double s_part[WK][FB];

    int r, fc;
    if (!block_to_task(blockIdx.x, nrow, nfc, xcd_mode, r, fc)) return;
    if (rowperm) r = rowperm[r];        // longest rows first: the launch ends on short workgroups
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);    // provably wave-uniform
    const int wf = wave % WF, wk = wave / WF;
    const int f0 = fc * FB + wf * FPW;
    const int q0 = blockIdx.y * qi, q1 = min(nbatch, q0 + qi);

    const int beg = rowptr[r], end = rowptr[r + 1];
    const bool one_seg = end - beg <= RB_SEG;
    const bool dead = DUAL ? false : wM[r] == 0.0;     // mask_result, IceCoupler.cpp:186-201
    // The row is walked in segments of RB_SEG entries staged in LDS.  The loads of segment s+1 are
    // issued before segment s is processed (they fly while X streams) and written to LDS after it.
    int cc[RB_STAGE];
    double vv[RB_STAGE], vv2[DUAL ? RB_STAGE : 1];
    auto stage_load = [&](int seg, int n) {       // all loads first (clamped, unconditional)
#pragma unroll
        for (int i = 0; i < RB_STAGE; ++i) {
            const int k = min((int)threadIdx.x + i * RB_THREADS, n - 1);
            cc[i] = colind[seg + k];
            vv[i] = vals[seg + k];
            if (DUAL) vv2[i] = vals2[seg + k];
        }
    };
    auto stage_store = [&](int n) {
#pragma unroll
        for (int i = 0; i < RB_STAGE; ++i) {
            const int k = threadIdx.x + i * RB_THREADS;
            if (k < n) { s_col[k] = cc[i]; s_val[k] = vv[i]; if (DUAL) s_val2[k] = vv2[i]; }
        }
    };

    for (int q = q0; q < q1; ++q) {
        const double *__restrict__ X = bp.x[q];
        double *__restrict__ Y = bp.y[q];
        __amdgpu_buffer_rsrc_t rs[FPW];
#pragma unroll
        for (int j = 0; j < FPW; ++j) {
            const int f = f0 + j < nf ? f0 + j : nf - 1;    // clamp: tail fields read valid memory, never stored
            rs[j] = __builtin_amdgcn_make_buffer_rsrc((void *)(X + (long)f * ldx), 0, ncol * 8, 0x00020000);
        }
        double acc[FPW], acc2[DUAL ? FPW : 1];
#pragma unroll
        for (int j = 0; j < FPW; ++j) { acc[j] = 0.0; if (DUAL) acc2[j] = 0.0; }

        if (beg < end && (q == q0 || !one_seg)) {       // a row of one segment stays staged for every batch
            stage_load(beg, min(RB_SEG, end - beg));
            if (q != q0) __syncthreads();               // every wave is done with the previous batch's last segment
            stage_store(min(RB_SEG, end - beg));
            __syncthreads();
        }
        for (int seg = beg; seg < end; seg += RB_SEG) {
            const int n = min(RB_SEG, end - seg);
            const int nxt = seg + RB_SEG;
            const bool more = nxt < end;
            if (more) stage_load(nxt, min(RB_SEG, end - nxt));
            // Full batches: every lane issues UNROLL*FPW loads before the first FMA, no predication.
            // The weights are read from LDS when the gathered values are consumed, not before the loads are issued: a slot in
            // flight then holds only its x (2 VGPRs per field), so that 14-16 loads per lane fit the 64 registers at which all
            // workgroups of a single 64-field apply are resident at once (8 waves per SIMD).
            const int nfull = n - n % BATCH;
            int kb = 0;
            if constexpr (!DUAL) {
                for (; kb < nfull; kb += BATCH) {
                    double x[FPW][UNROLL];
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) {
                        const int off = s_col[kb + wk * 64 + lane + u * STEP] << 3;
#pragma unroll
                        for (int j = 0; j < FPW; ++j) x[j][u] = xload(rs[j], off);
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) {
                        const double v = s_val[kb + wk * 64 + lane + u * STEP];
#pragma unroll
                        for (int j = 0; j < FPW; ++j) acc[j] = fma(v, x[j][u], acc[j]);
                    }
                }
                // Tail batch (every row of the 5 km matrices is nothing else): the slots that hold entries of this wave.
                if (kb + wk * 64 < n) {
                    const int k0 = kb + wk * 64;
                    const int nu = __builtin_amdgcn_readfirstlane(min(UNROLL, (n - k0 + STEP - 1) / STEP));
                    with_slot_count<UNROLL>(nu, [&](auto c) { tail_slots<FPW, decltype(c)::value, STEP>(s_col, s_val, rs, k0 + lane, n, acc); });
                }
            } else {
            for (; kb < nfull; kb += BATCH) {
                int off[UNROLL];
                double v[UNROLL], v2[UNROLL];
                bool h0[UNROLL], h1[UNROLL];
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    const int k = kb + wk * 64 + lane + u * STEP;
                    const int c = s_col[k];
                    off[u] = (c & 0x3fffffff) << 3;
                    v[u] = s_val[k];
                    v2[u] = s_val2[k]; h0[u] = (c >> 30) & 1; h1[u] = c < 0;
                }
                double x[FPW][UNROLL];
#pragma unroll
                for (int j = 0; j < FPW; ++j)
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) x[j][u] = xload(rs[j], off[u]);
#pragma unroll
                for (int j = 0; j < FPW; ++j)
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) {     // a missing partner is never multiplied (0*NaN)
                        acc[j] = h0[u] ? fma(v[u], x[j][u], acc[j]) : acc[j];
                        acc2[j] = h1[u] ? fma(v2[u], x[j][u], acc2[j]) : acc2[j];
                    }
            }
            if (kb + wk * 64 < n) {
                int off[UNROLL];
                double v[UNROLL], v2[UNROLL];
                bool ok[UNROLL], ok2[UNROLL];
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    const int k = kb + wk * 64 + lane + u * STEP;
                    ok[u] = k < n;
                    const int kk = ok[u] ? k : n - 1;
                    const int c = s_col[kk];
                    off[u] = (c & 0x3fffffff) << 3;
                    v[u] = s_val[kk];
                    v2[u] = s_val2[kk]; ok2[u] = ok[u] && c < 0; ok[u] = ok[u] && ((c >> 30) & 1);
                }
                double x[FPW][UNROLL];
#pragma unroll
                for (int j = 0; j < FPW; ++j)
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) x[j][u] = xload(rs[j], off[u]);
#pragma unroll
                for (int j = 0; j < FPW; ++j)
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) {
                        acc[j] = ok[u] ? fma(v[u], x[j][u], acc[j]) : acc[j];
                        acc2[j] = ok2[u] ? fma(v2[u], x[j][u], acc2[j]) : acc2[j];
                    }
            }
            }
            if (more) {
                __syncthreads();                      // every wave is done reading this segment
                stage_store(min(RB_SEG, end - nxt));
                __syncthreads();
            }
        }
#pragma unroll
        for (int j = 0; j < FPW; ++j) acc[j] = wave_sum(acc[j]);
        if (DUAL) {                          // partial sums of the band; fill and the pairing happen in dual_combine_kernel
#pragma unroll
            for (int j = 0; j < FPW; ++j) acc2[j] = wave_sum(acc2[j]);
            if (lane == 0) {
#pragma unroll
                for (int j = 0; j < FPW; ++j)
                    if (f0 + j < nf) { Y[(long)(f0 + j) * ldy + r] = acc[j]; Y2[(long)q * y2_stride + (long)(f0 + j) * ldy + r] = acc2[j]; }
            }
            continue;
        }
        if (WK == 1) {
            if (lane == 0) {
#pragma unroll
                for (int j = 0; j < FPW; ++j)
                    if (f0 + j < nf) Y[(long)(f0 + j) * ldy + r] = dead ? fill : acc[j];
            }
        } else {
            if (lane == 0) {
#pragma unroll
                for (int j = 0; j < FPW; ++j) s_part[wk][wf * FPW + j] = acc[j];
            }
            __syncthreads();
            if (threadIdx.x < FB) {
                const int f = fc * FB + threadIdx.x;
                double s = s_part[0][threadIdx.x];
#pragma unroll
                for (int qq = 1; qq < WK; ++qq) s += s_part[qq][threadIdx.x];
                if (f < nf) Y[(long)f * ldy + r] = dead ? fill : s;
            }
            if (q + 1 < q1) __syncthreads();           // s_part is reused by the next batch
        }
    }
}

// ---- rowone: ONE apply per launch, one field per wave -- the lean form of rowblock for the reference's own call shape ----------
// (Weighted_Eigen::apply, one call per matrix: merge_topo.cpp:65, icebin22m.cpp:153).  Same staging, same per-lane order,
// same wave_sum as rowblock with FPW = WK = 1 -> the same bits; what is gone is everything a single launch does not need: the
// batch loop and its pointer table in the kernel arguments, the cross-segment prefetch registers, the full / tail batch split.
// A row of <= U*64 entries (every row of the 5 km matrices) is ONE staged segment and ONE batch of U gathers per lane; the
// weights are read from LDS when the gathers land, so a slot in flight holds two registers and U = 14..16 fits the 64
// registers at which all workgroups of a 64-field apply are resident at once.  Measured against rowblock on the headline
// shape (scratch/chain_bench.hip has the decomposition: empty launch 4.1 us, matrix-free stream 7.9, this chain 9.8).
template <int NW, int U>
__global__ __launch_bounds__(NW * 64, 8) void spmm_rowone_kernel(
    const int *__restrict__ rowptr, const int *__restrict__ colind, const double *__restrict__ vals,
    const double *__restrict__ X, double *__restrict__ Y, long ldx, int ncol, long ldy, int nrow, int nf, int nfc,
    int xcd_mode, const double *__restrict__ wM, double fill)
{
    constexpr int T = NW * 64, SEG = U * 64, ST = (SEG + T - 1) / T;
    __shared__ int s_col[SEG];
    __shared__ double s_val[SEG];
    int r, fc;
    if (!block_to_task(blockIdx.x, nrow, nfc, xcd_mode, r, fc)) return;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fw = fc * NW + wave;
    const int f = fw < nf ? fw : nf - 1;            // clamp: tail fields read valid memory, never stored
    const int beg = rowptr[r], end = rowptr[r + 1];
    const __amdgpu_buffer_rsrc_t rs[1] = {__builtin_amdgcn_make_buffer_rsrc((void *)(X + (long)f * ldx), 0, ncol * 8, 0x00020000)};
    double acc[1] = {0.0};
    for (int seg = beg; seg < end; seg += SEG) {
        const int n = min(SEG, end - seg);
        int cc[ST];
        double vv[ST];
#pragma unroll
        for (int i = 0; i < ST; ++i) {              // all loads first (clamped, unconditional)
            const int k = min((int)threadIdx.x + i * T, n - 1);
            cc[i] = colind[seg + k];
            vv[i] = vals[seg + k];
        }
        if (seg != beg) __syncthreads();            // every wave is done with the previous segment
#pragma unroll
        for (int i = 0; i < ST; ++i) {
            const int k = threadIdx.x + i * T;
            if (k < n) { s_col[k] = cc[i]; s_val[k] = vv[i]; }
        }
        __syncthreads();
        // the ceil(n / 64) slots that hold entries, and no others (tail_slots: the tail batch of rowblock)
        const int nu = __builtin_amdgcn_readfirstlane(min(U, (n + 63) >> 6));
        with_slot_count<U>(nu, [&](auto c) { tail_slots<1, decltype(c)::value, 64>(s_col, s_val, rs, lane, n, acc); });
    }
    const double sum = wave_sum(acc[0]);
    if (lane == 0 && fw < nf) Y[(long)fw * ldy + r] = wM[r] == 0.0 ? fill : sum;      // mask_result, IceCoupler.cpp:186-201
}
// Tried on top of this and dropped (measured on MI355X, 5 km AvI, 64 fields): RUN HINTS -- the first-seen numbering makes a
// row's columns a contiguous run behind ~18 scattered ones, so the gathers of the run were issued with arithmetic addresses
// together with the staging loads -- bought nothing (10.44 against 10.48 us): the FMA chain starts with chunk 0, whose gather
// still waits for the staged columns and then queues behind every other load of the CU.  In-kernel stamps
// (scratch/chain_bench.hip, CHAIN_TIMELINE) show why: the X phase is throughput-bound -- a wave needs a median 3.5 us just to
// ISSUE its 14 gathers because the memory pipeline is full -- so what a single launch can still gain is its 1.2 us prologue.
// A staging-free variant ("rowdirect": a wave owns (row, 4 fields) and reads colind / vals itself, all chunks of the row in
// flight at once, row pointers in the kernel arguments, no LDS, no barrier) was SLOWER at every size (5 km 12.6 against
// 11.7 us, 1 km 235 against 186): 1.5 x the vector-memory instructions per gathered element, and row pointers in the kernarg
// segment are a memory round trip like any other (12.64 against 12.60 us with / without).

// ---- rowgroup: E-row matrices (EvI, EvX), one workgroup per (GCM cell, chunk of fields) ------------------------------------------
// An ice cell between two elevation classes is a column of TWO rows of M -- (GCM cell a, class k) and (a, k+1) -- so row by row
// every X element is gathered twice, and each of the ~10 class rows of a GCM cell touches ~15 % of the cell's footprint: most
// of every line it fetches belongs to other classes (5 km EvI: ~100 MB effective for a 42 MB apply).  Here the rows of one GCM
// cell form a GROUP whose entries are listed once per distinct column, ascending, as items {col, slot0, slot1, v0, v1}
// (applystruct.hip build_groups_from_csr): the column set of a group is the AvI row of its GCM cell -- a contiguous run behind a
// few cells shared with earlier GCM cells -- so the gathers are those of the A-row kernel: every X element once, whole lines.
// Lane = column, wave = field (as rowone): lane L multiplies its column's value into the sums of the column's two classes,
// kept in a per-wave LDS table acc[slot][lane] (bank = lane: conflict-free whatever the slots); at the end one wave_sum per
// class.  A group holds ALL entries of its rows, so the result is final: no partial sums, no second kernel.  Fixed order
// throughout (per lane: items lane, lane + 64, ... ascending; then the wave sum) -> bitwise reproducible; entries are
// predicated by existence, never multiplied by a padded zero (0*NaN).
struct GroupView {
    const int *ptr, *ns, *slotrow, *col;
    const unsigned *meta;
    const double *v0, *v1;
    int ngrp, nslot;
};
static GroupView group_view(const RowGroups &g) { return {g.ptr.p, g.ns.p, g.slotrow.p, g.col.p, g.meta.p, g.v0.p, g.v1.p, g.n, g.nslot}; }
constexpr unsigned RG_HAS0 = 1u << 16, RG_HAS1 = 1u << 17;
// PAIR: a second matrix applied to this one's result in the epilogue (ibh_weighted_apply_pair_device; see ibh::Pair)
struct PairView {
    const double *w;
    const unsigned *mask;
    const int *row;
    const double *wM2;
    double *Y2;
    long ldy2;
};
static PairView pair_view(const Pair &p, double *Y2, long ldy2) { return {p.w.p, p.mask.p, p.row.p, p.second->wM.p, Y2, ldy2}; }
template <int NW, int U, int TW, bool PAIR = false>
__global__ __launch_bounds__(NW * 64) void spmm_rowgroup_kernel(const GroupView gv, const BatchPtrs bp, long ldx, int ncol, long ldy, int nf,
                                                               int nfc, int xcd_mode, const double *__restrict__ wM, double fill,
                                                               const PairView pv = PairView{})
{
    constexpr int T = NW * 64, SEG = U * 64, ST = SEG / T;
    static_assert(SEG % T == 0, "segment is a multiple of the workgroup");
    extern __shared__ double rg_lds[];
    double *s_v0 = rg_lds, *s_v1 = rg_lds + SEG;
    int *s_col = reinterpret_cast<int *>(rg_lds + 2 * SEG);
    unsigned *s_meta = reinterpret_cast<unsigned *>(s_col + SEG);
    double *s_tab = rg_lds + 3 * SEG;                       // [NW][nslot][64]
    int g, fc;
    if (!block_to_task(blockIdx.x, gv.ngrp, nfc, xcd_mode, g, fc)) return;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fw = fc * NW + wave;
    const int f = fw < nf ? fw : nf - 1;            // clamp: tail fields read valid memory, never stored
    const double *__restrict__ X = bp.x[blockIdx.y];
    double *__restrict__ Y = bp.y[blockIdx.y];
    const int beg = gv.ptr[g], end = gv.ptr[g + 1], ns = gv.ns[g];
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)(X + (long)f * ldx), 0, ncol * 8, 0x00020000);
    // TW = 32: lanes L and L + 32 share a table entry (half the LDS: all workgroups of a 64-field apply at 5 km are resident
    // at once instead of in two rounds); their adds are issued as two instructions, lower half first -- LDS operations of a wave
    // execute in issue order, so the sum of an entry is still formed in one fixed order
    double *tab = s_tab + (long)wave * gv.nslot * TW + (lane & (TW - 1));
    for (int s = 0; s < ns; ++s) tab[s * TW] = 0.0;
    // The group is walked in segments of SEG items staged in LDS; the loads of segment s+1 are issued before segment s is
    // processed (they fly while X streams) and written to LDS after it.
    int cc[ST];
    unsigned mm[ST];
    double a0[ST], a1[ST];
    auto stage_load = [&](int seg, int n) {         // all loads first (clamped, unconditional)
#pragma unroll
        for (int i = 0; i < ST; ++i) {
            const int k = seg + min((int)threadIdx.x + i * T, n - 1);
            cc[i] = gv.col[k]; mm[i] = gv.meta[k]; a0[i] = gv.v0[k]; a1[i] = gv.v1[k];
        }
    };
    auto stage_store = [&](int n) {
#pragma unroll
        for (int i = 0; i < ST; ++i) {
            const int k = threadIdx.x + i * T;
            if (k < n) { s_col[k] = cc[i]; s_meta[k] = mm[i]; s_v0[k] = a0[i]; s_v1[k] = a1[i]; }
        }
    };
    if (beg < end) {
        stage_load(beg, min(SEG, end - beg));
        stage_store(min(SEG, end - beg));
        __syncthreads();
    }
    for (int seg = beg; seg < end; seg += SEG) {
        const int n = min(SEG, end - seg);
        const int nxt = seg + SEG;
        const bool more = nxt < end;
        if (more) stage_load(nxt, min(SEG, end - nxt));
        double x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = lane + 64 * u;
            x[u] = xload(rs, s_col[k < n ? k : n - 1] << 3);
        }
        // the items' slots and weights come out of LDS while the gathers fly ...
        unsigned m[U];
        double w0[U], w1[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = lane + 64 * u;
            const int kk = k < n ? k : n - 1;
            m[u] = k < n ? s_meta[kk] : 0u;             // lanes past the end: no has-bit
            w0[u] = s_v0[kk]; w1[u] = s_v1[kk];
        }
        __builtin_amdgcn_sched_barrier(0);
        // ... and the products go to the LDS pipe as ds_add_f64 WITHOUT return, back to back: the sums of a lane are added in
        // program order (deterministic) and the wave never waits for a read-modify-write round trip
        if (TW == 64) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (m[u] & RG_HAS0) __hip_atomic_fetch_add(tab + (m[u] & 0xffu) * TW, w0[u] * x[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (m[u] & RG_HAS1) __hip_atomic_fetch_add(tab + ((m[u] >> 8) & 0xffu) * TW, w1[u] * x[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const double p0 = w0[u] * x[u], p1 = w1[u] * x[u];
                const bool lo = lane < 32;
                if ((m[u] & RG_HAS0) && lo) __hip_atomic_fetch_add(tab + (m[u] & 0xffu) * TW, p0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __builtin_amdgcn_sched_barrier(0);
                if ((m[u] & RG_HAS0) && !lo) __hip_atomic_fetch_add(tab + (m[u] & 0xffu) * TW, p0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __builtin_amdgcn_sched_barrier(0);
                if ((m[u] & RG_HAS1) && lo) __hip_atomic_fetch_add(tab + ((m[u] >> 8) & 0xffu) * TW, p1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __builtin_amdgcn_sched_barrier(0);
                if ((m[u] & RG_HAS1) && !lo) __hip_atomic_fetch_add(tab + ((m[u] >> 8) & 0xffu) * TW, p1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (more) {
            __syncthreads();                        // every wave is done reading this segment
            stage_store(min(SEG, end - nxt));
            __syncthreads();
        }
    }
    // class sums: lane L adds one half (32 lanes' worth) of slot L % 32, starting at a lane-dependent offset (bank = 2 x index:
    // two lanes per bank instead of all 64), then the two halves meet; fixed order per lane -> reproducible
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    const int sl = lane & 31, half = lane >> 5;
    double tot = 0.0;
    if (sl < ns) {
        constexpr int HW = TW / 2;
        const double *row = s_tab + ((long)wave * gv.nslot + sl) * TW + half * HW;
#pragma unroll 8
        for (int j = 0; j < HW; ++j) tot += row[(j + lane) & (HW - 1)];
    }
    tot += __shfl_xor(tot, 32, 64);
    double y1 = 0.0;
    if (half == 0 && sl < ns) {
        const int r = gv.slotrow[g * IBH_GSLOTS + sl];
        y1 = wM[r] == 0.0 ? fill : tot;                         // mask_result, IceCoupler.cpp:186-201
        if (fw < nf) Y[(long)fw * ldy + r] = y1;
    }
    if (PAIR) {
        // the second matrix's row of this group: lane s holds weight x (the value just stored for slot s), summed over the wave
        // in the fixed order of wave_sum -- entry k of the row in lane k, as the row kernel holds it when the second matrix's
        // columns are this group's rows in slot order
        const int a2 = pv.row[g];
        if (a2 >= 0) {
            double v = 0.0;
            if (half == 0 && sl < ns && ((pv.mask[g] >> sl) & 1u)) v = pv.w[g * IBH_GSLOTS + sl] * y1;
            const double s2 = wave_sum(v);
            if (lane == 0 && fw < nf) pv.Y2[(long)fw * pv.ldy2 + a2] = pv.wM2[a2] == 0.0 ? fill : s2;
        }
    }
}

// Measured on MI355X (us per apply, one launch / 16 per launch; rowblock in brackets): 5 km EvI 64 fields 17.1 / 14.8 (23.0 / 16.5),
// 16 fields 7.5 / 3.9 (8.8 / 4.9); 1 km EvI 64 fields 223 / 204 (colsweep 231 / 203).  The read-modify-write of the class table
// was the first bottleneck (32.5 us at 5 km with plain LDS loads and stores: a dependent round trip per item); a variant without
// staging (every wave reads its items from global memory, LDS = tables only, no barrier) lost at every size (21.4 / 16.3 us at
// 5 km, 322 at 1 km): as for the A-row kernel, extra vector-memory instructions cost more than barriers and LDS footprint.
// Two fields per wave (the items read once per 16 fields instead of 8: 1.45 -> 1.22 x traffic at 1 km) doubles the class tables:
// 250 against 217 us at 1 km with 8 waves, 216 with 4 (no gain), 20.3 against 17.1 us at 5 km.
// A lean form for groups that fit one staged segment (U = 12..16 gathers per lane, slots and weights read from LDS when the
// gathers land, no cross-segment prefetch -- what made rowone fast) does NOT carry over: 17.5 us at best (U = 14, half-width
// tables), 24-29 with full tables (two workgroups per CU).  What bounds this kernel is the LDS pipe, not the gathers: per item
// and field it moves ~56 bytes through LDS (col, meta, two weights, two read-modify-write adds) where the A-row kernel moves 12.

// ---- grouptile: the row groups with X staged through LDS and register sums (round 5) ---------------------------------------------
// What bounded the row-group kernel above was the LDS pipe: wave = field, lane = column, so every wave re-read each item's
// {col, meta, v0, v1} and issued two ds_add_f64 per item (~56 B through LDS per item and field).  Here the roles are turned:
// the columns of a group are cut into TILES of SEG = 256 or 128 items (applystruct.hip build_group_tiles); a workgroup serves (group, F
// fields, F = 16 or 32) and for every tile
//   1. gathers X[f, col[k]] for the tile's items -- lane = item, one field per load, exactly the gathers of the kernel above:
//      every X element once per GCM cell, whole lines -- into an LDS tile s_x[f][k];
//   2. walks the tile's ENTRIES, sorted by (slot, item) = the rows of the CSR restricted to the tile, in QUADS of four entries
//      of one slot (the lists are padded to fours with {zero column, weight 0}): lane = (sublane j, field f), J = 64 / F sublanes;
//      a sublane reads its entry of the quad -- {8 k, v}, two LDS reads broadcast within the sublane -- then x = s_x[f][k] (one
//      conflict-free ds_read_b64) and does one FMA into a REGISTER: the slot of a quad is wave-uniform.  ~20 B through LDS per
//      entry and field, no atomics, no read-modify-write, no predicate.
// Which wave sums what is static, so the sums stay in registers across tiles: every slot's list of a tile is cut into SP parts
// (SP = the largest power of two with SP * ns <= 16, by the group's number of rows ns -- a GCM cell of two classes keeps all
// waves busy as one of sixteen does); the units u = s * SP + part, in this order, are dealt to the waves in contiguous, balanced
// ranges -- consecutive units are consecutive quads of the tile's list, so a wave walks ONE run of quads per tile and only
// switches its accumulator on the way.
// Summation order of (row, field): entry e of a part's run of the tile goes to partial sum e mod 4, tiles ascending; per part
// (p0 + p1) + (p2 + p3); parts ascending -- fixed by the matrix alone, so one apply, a batch, every field count and both F
// agree bitwise.
struct TileView {
    const int *gptr, *tptr, *tcol;
    const unsigned short *ek, *eptr;
    const double *ev;
    const int *ns, *slotrow;
    int ngrp;
};
static TileView tile_view(const RowGroups &g) {
    return {g.ptr.p, g.tiles.ptr.p, g.tiles.col.p, g.tiles.ek.p, g.tiles.eptr.p, g.tiles.ev.p, g.ns.p, g.slotrow.p, g.n};
}
constexpr int GT_UNITS = 16;         // the SP bound above: a group's units (slot, part) number max(16, ns)
constexpr int GT_TABP = 65;          // row stride of the epilogue's table of partial sums [unit][lane]
// sums of the two 32-lane halves of a wave: lo = lanes 0..31, hi = lanes 32..63, each in the order wave_sum adds a wave whose
// other half is zero
__device__ __forceinline__ void wave_half_sums(double v, double &lo, double &hi) {
    v += dpp_move<0xB1, 0xf>(v);
    v += dpp_move<0x4E, 0xf>(v);
    v += dpp_move<0x141, 0xf>(v);
    v += dpp_move<0x140, 0xf>(v);
    v += dpp_move<0x142, 0xa>(v);    // row_bcast15 into rows 1,3: lane 31 = rows 0+1, lane 63 = rows 2+3
    lo = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 31), __builtin_amdgcn_readlane(__double2loint(v), 31));
    hi = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
template <int F, int NS, int SEG, int NW, bool PAIR = false>
__global__ __launch_bounds__(NW * 64, 4) void spmm_grouptile_kernel(const TileView tv, const BatchPtrs bp, long ldx, int ncol, long ldy, int nf,
                                                                            int nfc, int xcd_mode, const double *__restrict__ wM, double fill,
                                                                            const PairView pv = PairView{})
{
    constexpr int NB = SEG / 64, T = NW * 64, SEGP = SEG + 2, ECAP = ibh_gt_ecap(SEG);
    constexpr int FW = F / (NW / NB);                   // fields a wave gathers for its 64 items
    constexpr int EPT = (ECAP + T - 1) / T;      // entries staged per thread
    constexpr int J = 64 / F, R = 4 / J;                // sublanes; entries of a quad per sublane = partial sums per lane and unit
    constexpr int OS = ((NS > GT_UNITS ? NS : GT_UNITS) + NW - 1) / NW;     // most units (slot, part) of a wave: groups of <= NS rows
    static_assert(F == 16 || F == 32, "fields per workgroup");
    static_assert(NW % NB == 0 && F % (NW / NB) == 0, "shape");
    extern __shared__ double gt_lds[];
    double *s_x = gt_lds;                                                // [F][SEGP]; columns SEG, SEG + 1 stay zero
    double *s_ev = s_x + F * SEGP;                                       // [ECAP]
    unsigned short *s_ek = reinterpret_cast<unsigned short *>(s_ev + ECAP);      // [ECAP]
    double *s_tab = gt_lds;                                              // epilogue: [R][32 units][GT_TABP], over s_x
    int g, fc;
    if (!block_to_task(blockIdx.x, tv.ngrp, nfc, xcd_mode, g, fc)) return;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const double *__restrict__ X = bp.x[blockIdx.y];
    double *__restrict__ Y = bp.y[blockIdx.y];
    const int t0 = tv.tptr[g], t1 = tv.tptr[g + 1], ns = tv.ns[g];
    const int nitems = tv.gptr[g + 1] - tv.gptr[g];
    const int ib = wave % NB, fg = wave / NB;           // this wave gathers items [64 ib, 64 ib + 64) for fields [FW fg, FW fg + FW)
    const int j = lane / F, f = lane % F;
    // parts per slot: the largest power of two with sp * ns <= GT_UNITS; this wave's units [ub, ue)
    constexpr int UL = GT_UNITS;
    const int lsp = ns * 16 <= UL ? 4 : ns * 8 <= UL ? 3 : ns * 4 <= UL ? 2 : ns * 2 <= UL ? 1 : 0;
    const int nunit = ns << lsp;
    const int ub = (wave * nunit) / NW, ue = ((wave + 1) * nunit) / NW;
    if (threadIdx.x < 2 * F) s_x[(threadIdx.x >> 1) * SEGP + SEG + (threadIdx.x & 1)] = 0.0;

    double x[FW];
    double evv[EPT];
    unsigned short ekk[EPT];
    // The HEAD of a tile -- the columns of this wave's 64 items and the tile's row of entry offsets (one per slot, lane i of every
    // wave holds offset i) -- is fetched one tile BEFORE its X values and entries are: inside the loop a tile costs one memory
    // round trip (its gathers, issued with addresses already in registers), not two, and the unit boundaries come out of
    // registers (v_readlane) instead of LDS.
    int c_nxt = 0, ep_nxt = 0;
    auto tile_n = [&](int t) { return min(SEG, nitems - (t - t0) * SEG); };
    auto load_head = [&](int t) {
        if (ib * 64 < tile_n(t)) c_nxt = tv.tcol[(long)t * SEG + ib * 64 + lane];
        ep_nxt = tv.eptr[(long)t * IBH_GT_EP + min(lane, IBH_GT_EP - 1)];
    };
    auto load_tile = [&](int t, int c, int ne) {        // into registers; flies while the previous tile is summed
        if (ib * 64 < tile_n(t)) {
            const int off = c << 3;
#pragma unroll
            for (int i = 0; i < FW; ++i) {
                const int fw = fc * F + fg * FW + i;
                const __amdgpu_buffer_rsrc_t rs =
                    __builtin_amdgcn_make_buffer_rsrc((void *)(X + (long)(fw < nf ? fw : nf - 1) * ldx), 0, ncol * 8, 0x00020000);
                x[i] = xload(rs, off);
            }
        }
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
            const int e = threadIdx.x + i * T;
            if (e < ne) { ekk[i] = tv.ek[(long)t * ECAP + e]; evv[i] = tv.ev[(long)t * ECAP + e]; }
        }
    };
    auto store_tile = [&](int t) {
        if (ib * 64 < tile_n(t)) {
#pragma unroll
            for (int i = 0; i < FW; ++i) s_x[(fg * FW + i) * SEGP + ib * 64 + lane] = x[i];
        }
#pragma unroll
        for (int i = 0; i < EPT; ++i) {                 // (beyond the tile's entries: stale values nobody uses)
            const int e = threadIdx.x + i * T;
            if (e < ECAP) { s_ek[e] = ekk[i]; s_ev[e] = evv[i]; }
        }
    };

    double acc[OS][R];
#pragma unroll
    for (int o = 0; o < OS; ++o)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[o][r] = 0.0;
    // per lane: field f's row of the X tile; this sublane's entry of step 0 (weights); the entry whose item a lane fetches for a batch
    const char *a_x = reinterpret_cast<const char *>(s_x) + f * SEGP * 8;
    const char *a_ev = reinterpret_cast<const char *>(s_ev) + j * 8;
    const char *a_ek = reinterpret_cast<const char *>(s_ek) + (J * (lane & 15) + j) * 2;

    int ep_cur = 0;
    if (t0 < t1) {
        load_head(t0);
        const int c0 = c_nxt;
        ep_cur = ep_nxt;
        if (t0 + 1 < t1) load_head(t0 + 1);
        load_tile(t0, c0, __builtin_amdgcn_readlane(ep_cur, IBH_GSLOTS));
    }
    for (int t = t0; t < t1; ++t) {
        if (t != t0) __syncthreads();                   // every wave is done with the previous tile
        store_tile(t);
        __syncthreads();
        const int ep = ep_cur;
        if (t + 1 < t1) {
            const int c = c_nxt;
            ep_cur = ep_nxt;
            if (t + 2 < t1) load_head(t + 2);
            load_tile(t + 1, c, __builtin_amdgcn_readlane(ep_cur, IBH_GSLOTS));
        }
        __builtin_amdgcn_sched_barrier(0);              // (the loads above fly while the tile is summed: nothing of them sinks below)
        // Unit o of this wave = steps [B[o], B[o + 1]) of the tile's list (a step = J entries x F fields), walked in batches of
        // 4 steps: lane 16 r + i fetches the item index 8 k of the entry that step i of the batch hands to sublane r / (F / 16) --
        // one LDS read per lane and batch; a DPP row broadcast folded into the address add then gives every step its X
        // address, the weights come as broadcast reads at fixed offsets, and the 8 reads of a batch are in flight together.
        int B[OS + 1];
#pragma unroll
        for (int o = 0; o <= OS; ++o) {
            const int u = min(ub + o, ue);              // (o past this wave's units: the end of its run)
            const int uu = min(u, nunit - 1);
            const int sl = uu >> lsp, part = u >= nunit ? (1 << lsp) : (u & ((1 << lsp) - 1));
            const int lb = __builtin_amdgcn_readlane(ep, sl) >> 2, nq = (__builtin_amdgcn_readlane(ep, sl + 1) >> 2) - lb;
            B[o] = (lb + ((nq * part) >> lsp)) * R;
        }
#pragma unroll
        for (int o = 0; o < OS; ++o) {
            for (int p0 = B[o]; p0 < B[o + 1]; p0 += 4) {
                const int nb = B[o + 1] - p0;
                const int mk = *reinterpret_cast<const unsigned short *>(a_ek + p0 * J * 2);
                const char *pv = a_ev + p0 * J * 8;
                double xx[4], vv[4];
#define GT_XR(S)                                                                                                                          \
                xx[S] = *reinterpret_cast<const double *>(a_x + __builtin_amdgcn_update_dpp(0, mk, 0x150 + (S), 0xf, 0xf, false));        \
                vv[S] = *reinterpret_cast<const double *>(pv + (S) * J * 8)
#define GT_FM(S) if ((S) < nb) acc[o][(S) % R] = fma(vv[S], xx[S], acc[o][(S) % R])
                GT_XR(0); GT_XR(1); GT_XR(2); GT_XR(3);
                GT_FM(0); GT_FM(1); GT_FM(2); GT_FM(3);
#undef GT_XR
#undef GT_FM
            }
        }
    }
    __syncthreads();                                    // s_x is done: the partial sums take its place
#pragma unroll
    for (int o = 0; o < OS; ++o)
        if (ub + o < ue) {
#pragma unroll
            for (int r = 0; r < R; ++r) s_tab[(r * 32 + ub + o) * GT_TABP + lane] = acc[o][r];
        }
    __syncthreads();
    // thread -> (field, slot): lanes 0..31 of a wave are the slots of one field, lanes 32..63 those of the next
    const int sl = lane & 31, half = lane >> 5;
#pragma unroll
    for (int i = 0; i < F / (2 * NW); ++i) {
        const int fl = 2 * (wave * (F / (2 * NW)) + i) + half, fw = fc * F + fl;
        double y1 = 0.0;
        if (sl < ns) {
            double tot = 0.0;
            for (int p = 0; p < (1 << lsp); ++p) {
                const double *row = s_tab + ((sl << lsp) + p) * GT_TABP + fl;
                double pp;
                if constexpr (J == 4) pp = (row[0] + row[16]) + (row[32] + row[48]);
                else pp = (row[0] + row[32]) + (row[32 * GT_TABP] + row[32 * GT_TABP + 32]);
                tot = p == 0 ? pp : tot + pp;
            }
            const int r = tv.slotrow[g * IBH_GSLOTS + sl];
            y1 = wM[r] == 0.0 ? fill : tot;             // mask_result, IceCoupler.cpp:186-201
            if (fw < nf) Y[(long)fw * ldy + r] = y1;
        }
        if (PAIR) {                                     // the second matrix's row of this group, as in spmm_rowgroup_kernel
            const int a2 = pv.row[g];
            if (a2 >= 0) {
                double v2 = 0.0;
                if (sl < ns && ((pv.mask[g] >> sl) & 1u)) v2 = pv.w[g * IBH_GSLOTS + sl] * y1;
                double s_lo, s_hi;
                wave_half_sums(v2, s_lo, s_hi);
                const double s2 = half ? s_hi : s_lo;
                if (sl == 0 && fw < nf) pv.Y2[(long)fw * pv.ldy2 + a2] = pv.wM2[a2] == 0.0 ? fill : s2;
            }
        }
    }
}


// XT[c*ldt + f] = X[f*ldx + c]; pad columns f in [nf, ldt) are zeroed (read for tail fields, never stored)
__global__ void transpose_fields_kernel(const BatchPtrs bp, long ldx, int nf, int ncol,
                                        double *__restrict__ XT0, int ldt, long xt_stride) {
    __shared__ double tile[16][65];
    const double *__restrict__ X = bp.x[blockIdx.z];
    double *__restrict__ XT = XT0 + (long)blockIdx.z * xt_stride;
    const int cb = blockIdx.x * 64, fb = blockIdx.y * 16;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;          // 256 threads: 64 columns x 4
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int f = fb + ty * 4 + q, c = cb + tx;
        tile[ty * 4 + q][tx] = (f < nf && c < ncol) ? X[(long)f * ldx + c] : 0.0;
    }
    __syncthreads();
    const int fo = threadIdx.x & 15, co = threadIdx.x >> 4;          // 16 fields x 16 columns per pass
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = cb + co + q * 16;
        if (c < ncol && fb + fo < ldt) XT[(long)c * ldt + fb + fo] = tile[fo][co + q * 16];
    }
}

// REALIGN: the result planes Y[f, :] do not start on 64-byte lines (odd leading dimension: the
// reference's A_b(nvar, n) is contiguous, so ldy = nrow_d).  A wave's 512-byte store would then
// straddle nine lines and leave two of them partially written, to be completed by the neighbouring
// wave: measured 4.0 instead of 6.0 TB/s of store bandwidth on this chip.  The workgroup therefore
// computes 256 rows but OWNS, per plane, the line-aligned run of <= 255 rows that starts at the first
// 64-byte boundary at or after its first row (consecutive workgroups advance by 248 rows, so the
// runs tile the plane exactly); values cross lanes through LDS and every wave stores whole lines.
// XT: X is read from its transpose XT[c, f] (row stride ldx = fields padded to 16): the G fields of
// one entry are 8*G contiguous bytes per lane, fetched with 16-byte loads.  With the field-major X a
// wave gather touches up to 64 lines PER FIELD when the lanes' columns differ (IvE: the elevation
// class changes from cell to cell); transposed it is 64 lines per ENTRY.  The transpose of the
// (small: nf x nA_d or nE_d) input is a ~3 us pre-kernel.
typedef double sr_double2 __attribute__((ext_vector_type(2)));
template <bool NT, int G, bool REALIGN, bool XT>
__global__ __launch_bounds__(SR_THREADS) void spmm_shortrow_kernel(
    const int *__restrict__ rowptr, const int *__restrict__ colind, const double *__restrict__ vals,
    const BatchPtrs bp, const double *__restrict__ XT0, long xt_stride, long ldx, long ldy, int nrow, int nf, int fper,
    const double *__restrict__ wM, double fill)
{
    __shared__ double s_y[REALIGN ? G : 1][SR_THREADS];
    // blockIdx.y = field batch of a batched launch (ibh_weighted_apply_many_device): the workgroups of batch q+1 start while
    // those of batch q still store, so launch ramp and drain are paid once per launch
    const double *__restrict__ X = XT ? XT0 + (long)blockIdx.y * xt_stride : bp.x[blockIdx.y];
    double *__restrict__ Y = bp.y[blockIdx.y];
    // 1-D grid, field chunk fastest, contiguous ranges per XCD: the nfy workgroups that walk the same
    // 256 rows (one per field chunk) are neighbours on one XCD, so rowptr/colind/vals/wM of those rows
    // come from HBM once and from that XCD's L2 for the other chunks.
    const int nfy = (nf + fper - 1) / fper;
    const int logical = xcd_contiguous(blockIdx.x, gridDim.x);
    const int rb = logical / nfy, fy = logical - rb * nfy;
    const int rbase = rb * (REALIGN ? SR_STEP : SR_THREADS);
    const int r = rbase + threadIdx.x;
    const bool live = r < nrow;
    const int fbeg = fy * fper;
    const int fend = min(nf, fbeg + fper);
    if (!REALIGN && !live) return;
    int beg = 0, end = 0;
    bool dead = false;
    if (live) { beg = rowptr[r]; end = rowptr[r + 1]; dead = wM[r] == 0.0; }
    const int n = end - beg;
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    double v0 = 0, v1 = 0, v2 = 0, v3 = 0;
    if (n > 0) { c0 = colind[beg]; v0 = vals[beg]; }
    if (n > 1) { c1 = colind[beg + 1]; v1 = vals[beg + 1]; }
    if (n > 2) { c2 = colind[beg + 2]; v2 = vals[beg + 2]; }
    if (n > 3) { c3 = colind[beg + 3]; v3 = vals[beg + 3]; }
    // G fields in flight per thread: all G gathers are issued before the first store.  vmcnt counts
    // loads and stores together in issue order, so a gather issued after a store would wait for that
    // store's (long) write acknowledgement; with G == fields per thread there is one load phase and
    // one store phase per thread.
    // SHARED columns (XT, groups of <= 4 fields): rows of one GCM cell follow each other in a fresh ice dimension, so for every entry
    // slot most lanes of a wave name the SAME column.  That column's X values come through scalar loads and feed the FMAs as scalar
    // operands; only the lanes that differ (the ice cells along the cell's edge: two per grid-row segment) gather theirs, and a gather
    // costs the texture path by its ACTIVE lanes.  A full-wave gather of 16 bytes per lane is 16 cycles per CU whatever the addresses:
    // the time of this kernel followed the entries of the longest row of a wave, not the bytes (16.3 M rows, 128 fields: 3.0 / 4.0 /
    // 5.3 ms at 1 / 2 / 4 entries in every row; 4.9 with 2 and 4 in 7 % of the rows, scattered: the Antarctic IvE).
    constexpr bool SHARED = XT && G <= 4;
    int ucA[4] = {0, 0, 0, 0}, ucB[4] = {0, 0, 0, 0};
    bool mineA[4] = {false, false, false, false}, mineB[4] = {false, false, false, false};     // this lane's entry e sits in shared column A / B
    bool hasB[4] = {false, false, false, false};     // (wave-uniform) a second shared column
    bool leftover = false;                           // (wave-uniform) lanes in neither: the wave takes the gather form below
    int nmax = 0;
    bool shared_ok = SHARED && __ballot(n > 4) == 0;      // (a smoothed matrix has longer rows: the gather form, too)
    if (shared_ok) {
        const int cc[4] = {c0, c1, c2, c3};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned long long he = __ballot(n > e);
            if (!he) break;
            nmax = e + 1;
            // A: the column of the first or of the last lane that has the entry, whichever more lanes name; B: the column of the
            // first lane outside A (a class boundary or a cell edge inside the wave)
            const int ca = __builtin_amdgcn_readlane(cc[e], __builtin_ctzll(he)), cb = __builtin_amdgcn_readlane(cc[e], 63 - __builtin_clzll(he));
            const unsigned long long ma = __ballot(n > e && cc[e] == ca), mb = __ballot(n > e && cc[e] == cb);
            ucA[e] = __popcll(ma) >= __popcll(mb) ? ca : cb;
            mineA[e] = n > e && cc[e] == ucA[e];
            const unsigned long long rest = __ballot(n > e && !mineA[e]);
            if (rest) {
                hasB[e] = true;
                ucB[e] = __builtin_amdgcn_readlane(cc[e], __builtin_ctzll(rest));
                mineB[e] = n > e && !mineA[e] && cc[e] == ucB[e];
                leftover = leftover || __ballot(n > e && !mineA[e] && !mineB[e]) != 0;
            }
        }
    }
    shared_ok = shared_ok && !leftover;
    for (int f0 = fbeg; f0 < fend; f0 += G) {
        double acc[G];
        if (shared_ok) {
#pragma unroll
            for (int g = 0; g < G; ++g) acc[g] = 0.0;
            const double vv[4] = {v0, v1, v2, v3};
            // all loads of the group first (scalar: wave-uniform addresses)
            double sa[4][G], sb[4][G];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e >= nmax) break;
                const double *__restrict__ pa = X + (long)ucA[e] * ldx + f0;     // (wave-uniform addresses: scalar loads)
#pragma unroll
                for (int g = 0; g < G; ++g) sa[e][g] = pa[g];
                if (hasB[e]) {
                    const double *__restrict__ pb = X + (long)ucB[e] * ldx + f0;
#pragma unroll
                    for (int g = 0; g < G; ++g) sb[e][g] = pb[g];
                }
            }
            // the products, entry by entry in every lane (the row's order): never multiplied by a padded zero (0*NaN)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e >= nmax) break;
                if (mineA[e]) {
#pragma unroll
                    for (int g = 0; g < G; ++g) acc[g] = e == 0 ? vv[e] * sa[e][g] : fma(vv[e], sa[e][g], acc[g]);
                }
                if (hasB[e] && mineB[e]) {
#pragma unroll
                    for (int g = 0; g < G; ++g) acc[g] = e == 0 ? vv[e] * sb[e][g] : fma(vv[e], sb[e][g], acc[g]);
                }
            }
            if (dead) {
#pragma unroll
                for (int g = 0; g < G; ++g) acc[g] = fill;
            }
        } else if (XT) {
            // entry by entry, G fields at a time (f0 is a multiple of G, rows of XT are padded to 16 fields)
#pragma unroll
            for (int g = 0; g < G; ++g) acc[g] = 0.0;
            auto entry = [&](int c, double v, bool first) {
                const sr_double2 *p = reinterpret_cast<const sr_double2 *>(X + (long)c * ldx + f0);
#pragma unroll
                for (int g = 0; g < G; g += 2) {
                    const sr_double2 x = p[g >> 1];
                    acc[g] = first ? v * x.x : fma(v, x.x, acc[g]);
                    acc[g + 1] = first ? v * x.y : fma(v, x.y, acc[g + 1]);
                }
            };
            // predicated, never multiplied by a padded zero: 0*NaN must not leak into a row
            if (n > 0) entry(c0, v0, true);
            if (n > 1) entry(c1, v1, false);
            if (n > 2) entry(c2, v2, false);
            if (n > 3) entry(c3, v3, false);
            for (int k = beg + 4; k < end; ++k) entry(colind[k], vals[k], false);
            if (dead) {
#pragma unroll
                for (int g = 0; g < G; ++g) acc[g] = fill;
            }
        } else {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int f = f0 + g < fend ? f0 + g : fend - 1;
            const double *xf = X + (long)f * ldx;
            // predicated, never multiplied by a padded zero: 0*NaN must not leak into a row
            double a = 0.0;
            if (n > 0) a = v0 * xf[c0];
            if (n > 1) a = fma(v1, xf[c1], a);
            if (n > 2) a = fma(v2, xf[c2], a);
            if (n > 3) a = fma(v3, xf[c3], a);
            for (int k = beg + 4; k < end; ++k) a = fma(vals[k], xf[colind[k]], a);
            acc[g] = dead ? fill : a;
        }
        }
        if (!REALIGN) {
#pragma unroll
            for (int g = 0; g < G; ++g)
                if (f0 + g < fend) {
                    if (NT) __builtin_nontemporal_store(acc[g], &Y[(long)(f0 + g) * ldy + r]);
                    else Y[(long)(f0 + g) * ldy + r] = acc[g];
                }
        } else {
            if (f0 != fbeg) __syncthreads();               // the previous group's values have been read
#pragma unroll
            for (int g = 0; g < G; ++g) s_y[g][threadIdx.x] = acc[g];
            __syncthreads();
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (f0 + g >= fend) break;
                double *yf = Y + (long)(f0 + g) * ldy;
                // first row >= rbase whose address is a multiple of 64 bytes (the very first run starts at row 0)
                const long a8 = (long)(reinterpret_cast<uintptr_t>(yf) >> 3);
                const int s0 = rb == 0 ? 0 : rbase + (int)((-(a8 + rbase)) & 7);
                int s1 = rbase + SR_STEP + (int)((-(a8 + rbase + SR_STEP)) & 7);
                if (s1 > nrow || rbase + SR_STEP >= nrow) s1 = nrow;
                const int rr = s0 + (int)threadIdx.x;
                if (rr < s1) {
                    const double v = s_y[g][rr - rbase];
                    if (NT) __builtin_nontemporal_store(v, &yf[rr]); else yf[rr] = v;
                }
            }
        }
    }
}

// (Round 5, tried and removed -- "fieldlane": I-row matrices on >= 64 fields with lane = FIELD, a wave owning 16 rows, the row
// structure wave-uniform (columns and weights through v_readlane into the scalar offset of one coalesced 512-byte load of the
// transposed input per entry, one FMA, no masks), row sums through an LDS tile that leaves transposed.  Bitwise the row kernel on
// every matrix tried, smoothed ones included, and slower everywhere on the Antarctic sheet, 128 fields, IvE / IvA against 4.1 /
// 2.8 ms: a tile per wave stored as 16 or 8 rows per plane (128- / 64-byte pieces) 6.8 / 5.8 and 8.6-9.0 / 7.5-8.0 ms -- with 22
// scalar instructions per entry or with 4, the same; HBM traffic exact (16.9 GB written, 1.6 fetched) -- and a tile per workgroup
// with the row kernel's own 512-byte stores 7.1 / 6.1 ms: four workgroups of 33 KB per CU and six to eight dependent round trips
// per 64 rows.  The thread-per-row kernel keeps many more loads in flight per wave; it stays.)
// ---- conservation correction (non-conservative matrices only) ------------------------------
// out[k] = sum_j w[j] * A[k*lda + j] over j with w[j] != 0, in a fixed order: the vector is cut into <= WD_MAXCHUNK chunks
// (one workgroup each per variable: a single workgroup per variable reads 10^5..10^7 elements at one CU's bandwidth --
// measured 35 us of an 85 us corrected apply at 5 km), the chunk sums are added sequentially by the last stage.
constexpr int WD_MAXCHUNK = 256, WD_MINLEN = 4096;
static int weight_dot_chunks(int n) { return n <= WD_MINLEN ? 1 : std::min(WD_MAXCHUNK, ceil_div(n, WD_MINLEN)); }
__global__ __launch_bounds__(1024) void weight_dot_kernel(const double *__restrict__ w, int n, int chunk_len,
                                                          const double *__restrict__ A, long lda,
                                                          double *__restrict__ part)
{
    __shared__ double s[16];
    const double *a = A + (long)blockIdx.x * lda;
    const int j0 = blockIdx.y * chunk_len, j1 = min(n, j0 + chunk_len);
    double acc = 0.0;
    for (int j = j0 + threadIdx.x; j < j1; j += 1024) {
        const double wj = w[j];
        if (wj != 0.0) acc = fma(wj, a[j], acc);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int q = 0; q < 16; ++q) t += s[q];
        part[(long)blockIdx.x * gridDim.y + blockIdx.y] = t;
    }
}
__global__ void weight_dot_final_kernel(const double *__restrict__ part, int nchunk, double *__restrict__ out) {
    const int k = blockIdx.x;                      // one variable per (single-thread) workgroup: <= WD_MAXCHUNK additions, in chunk order
    double t = 0.0;
    for (int c = 0; c < nchunk; ++c) t += part[(long)k * nchunk + c];
    out[k] = t;
}
__global__ void conserve_scale_kernel(double *__restrict__ Y, long ldy, int nrow, const double *__restrict__ wM,
                                      const double *__restrict__ TA, const double *__restrict__ TB)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = blockIdx.y;
    if (r >= nrow || wM[r] == 0.0) return;
    Y[(long)k * ldy + r] *= TA[k] / TB[k];
}

// dout[nvar]; part: scratch of nvar * weight_dot_chunks(n) doubles (nullptr allowed when n <= WD_MINLEN: one chunk goes
// straight to dout)
void weight_dot_launch(const double *dw, int n, const double *dA, int nvar, int64_t lda, double *dout, double *part,
                       hipStream_t stream)
{
    if (nvar <= 0) return;
    const int nchunk = part ? weight_dot_chunks(n) : 1;
    const int len = ceil_div(n, nchunk);
    hipLaunchKernelGGL(weight_dot_kernel, dim3(nvar, nchunk), dim3(1024), 0, stream, dw, n, len, dA, (long)lda, nchunk == 1 ? dout : part);
    if (nchunk > 1) hipLaunchKernelGGL(weight_dot_final_kernel, dim3(nvar), dim3(1), 0, stream, part, nchunk, dout);
    IBH_HIP(hipGetLastError());
}
size_t weight_dot_scratch(int n, int nvar) { return (size_t)nvar * (size_t)weight_dot_chunks(n); }

// ---- dispatch ------------------------------------------------------------------------------
void ensure_rowsum1(const ibh_weighted *w, hipStream_t stream);
// Scratch owned by the handle grows OUTSIDE stream capture only (hipMalloc is illegal while capturing
// and synchronises the device): ibh_weighted_reserve() sizes it up front; an apply that still finds a
// buffer too small grows it after a device synchronisation (an earlier apply may be reading the old
// block), or fails when its stream is being captured.
static bool is_capturing(hipStream_t stream) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (stream) IBH_HIP(hipStreamIsCapturing(stream, &cs));
    return cs != hipStreamCaptureStatusNone;
}
template <class T>
static void grow_scratch(DevBuf<T> &b, size_t count, hipStream_t stream, const char *what) {
    if (b.p && count * sizeof(T) <= b.granted) { b.n = count; return; }
    IBH_CHECK(!is_capturing(stream),
              "apply inside a stream capture needs %zu more bytes of %s scratch: call ibh_weighted_reserve() before capturing",
              count * sizeof(T), what);
    if (b.p) IBH_HIP(hipDeviceSynchronize());
    b.alloc(count);
}

// rowperm[k] = the row with the k-th most entries (ties by index): longest-processing-time-first order
// of the (row, chunk) tasks.  Rank by counting, nrow <= LPT_MAX_ROWS.
constexpr int LPT_MAX_ROWS = 8192;
__global__ void rowperm_kernel(const int *__restrict__ rowptr, int nrow, int *__restrict__ perm) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrow) return;
    const int len = rowptr[r + 1] - rowptr[r];
    int rank = 0;
    for (int q = 0; q < nrow; ++q) {
        const int lq = rowptr[q + 1] - rowptr[q];
        rank += (lq > len || (lq == len && q < r)) ? 1 : 0;
    }
    perm[rank] = r;
}
static bool ensure_rowperm(const ibh_weighted *w, hipStream_t stream) {
    ApplyState::Scratch &scr = w->st.scr;
    if (scr.have_rowperm) return true;
    if (w->nrow > LPT_MAX_ROWS || w->nrow < 2) return false;
    if (is_capturing(stream) && !(scr.rowperm.p && (size_t)w->nrow * sizeof(int) <= scr.rowperm.granted)) return false;
    grow_scratch(scr.rowperm, (size_t)w->nrow, stream, "row-order");
    hipLaunchKernelGGL(rowperm_kernel, dim3(ceil_div(w->nrow, 256)), dim3(256), 0, stream, w->rowptr.p, w->nrow, scr.rowperm.p);
    IBH_HIP(hipGetLastError());
    scr.have_rowperm = true;
    return true;
}

// B[f, r] = lower-class sum of band r + upper-class sum of the band below it (rb1[r], -1: none)
__global__ void dual_combine_kernel(const double *__restrict__ P0, const double *__restrict__ P1, long ldp, long pstride,
                                    const int *__restrict__ rb1, const double *__restrict__ wM, double fill,
                                    const BatchPtrs bp, long ldy, int nrow, int nf) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    const int f = blockIdx.y, q = blockIdx.z;
    if (r >= nrow) return;
    const int b = rb1[r];
    double t = P0[(long)q * pstride + (long)f * ldp + r];
    if (b >= 0) t = t + P1[(long)q * pstride + (long)f * ldp + b];
    bp.y[q][(long)f * ldy + r] = wM[r] == 0.0 ? fill : t;
}

// ---- colsweep (sweep_kernel.inl): E-row matrices, >= 32 fields ------------------------------------------------
// Y[f, r] = the partial sums of the tasks that touch row r (comb_p[comb_ptr[r] .. comb_ptr[r+1])), in task order; rows no
// task touches are 0, rows with wM == 0 hold `fill` (mask_result, IceCoupler.cpp:186-201).
__global__ __launch_bounds__(256) void sweep_combine_kernel(const double *__restrict__ P, long pstride, long ldp,
                                                            const int *__restrict__ comb_ptr, const int *__restrict__ comb_p,
                                                            const double *__restrict__ wM, double fill, const BatchPtrs bp, long ldy,
                                                            int nrow, int nf, int lg)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int f = blockIdx.y * 64 + (threadIdx.x & 63);
    const int q = blockIdx.z;
    if (r >= nrow || f >= nf) return;
    const int k0 = comb_ptr[r], k1 = comb_ptr[r + 1];
    // the sweep's lanes are (batch, field) pairs (sweep_kernel.inl): lg = 6 -> one batch per slice, lane = field of the field
    // block; lg < 6 -> 64 >> lg batches per slice, lane = (batch % G) << lg | field
    const int G = 64 >> lg;
    const double *p = lg == 6 ? P + (long)q * pstride + f : P + (long)(q / G) * pstride + ((q % G) << lg) + f;
    // eight partial rows in flight (index, then value: two dependent loads each), added in task order
    double tot = 0.0;
    int k = k0;
    if (k < k1) { tot = p[(long)comb_p[k] * ldp]; ++k; }
    for (; k + 8 <= k1; k += 8) {
        int idx[8];
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) idx[u] = comb_p[k + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[(long)idx[u] * ldp];
#pragma unroll
        for (int u = 0; u < 8; ++u) tot += v[u];
    }
    for (; k < k1; ++k) tot += p[(long)comb_p[k] * ldp];
    bp.y[q][(long)f * ldy + r] = wM[r] == 0.0 ? fill : tot;
}
static SweepView sweep_view(const Sweep &s) { return {s.task_p0.p, s.task_ns.p, s.col.p, s.meta.p, s.v0.p, s.v1.p, s.tb, s.nblk, s.nitems}; }

// ---- launching a plan (apply_plan.h) --------------------------------------------------------------------------------------------
// One launcher per instantiation, in the order of apply_plan.h's lists; launch_plan walks a plan: scratch, the launch events, the
// grid check, the LDS limit and the name of the launch happen there, once.
struct Launch {
    const ibh_weighted *w; const ApplyPlan &p; const BatchPtrs &bp;
    int nbatch, nvar; long lda, ldb; double fill; hipStream_t stream; const PairView *pair;
    hipEvent_t ev0, ev1;            // launch timing (ibh_set_launch_events): attached to the first and the last dispatch of the apply
    dim3 grid() const { return dim3(p.grid[0], p.grid[1], p.grid[2]); }
};
struct Launcher { const void *kernel; void (*run)(const Launch &); };

template <int F, int NS, int SEG, int NW, bool PAIR>
static void run_grouptile(const Launch &l) {
    const RowGroups &grp = l.w->st.groups;
    IBH_CHECK(grp.nslot <= NS && grp.tiles.seg == SEG, "row groups of %d rows / tiles of %d in a kernel for %d / %d", grp.nslot, grp.tiles.seg, NS, SEG);
    static_assert(grouptile_lds(F, SEG) <= 64 * 1024, "within the default dynamic-LDS limit");
    IBH_CHECK(!PAIR || l.nbatch == 1, "fused pair apply: %d batches not supported", l.nbatch);
    hipExtLaunchKernelGGL((spmm_grouptile_kernel<F, NS, SEG, NW, PAIR>), l.grid(), dim3(NW * 64), l.p.lds, l.stream, l.ev0, l.ev1, 0, tile_view(grp), l.bp,
                          l.lda, l.w->ncol, l.ldb, l.nvar, l.p.nfc, l.p.xcd_mode, l.w->wM.p, l.fill, PAIR ? *l.pair : PairView{});
}
template <bool FULL, bool IDENT>
static void run_sweep(const Launch &l) {
    const ibh_weighted *w = l.w;
    const Sweep &sweep = w->st.sweep;
    const int lg = sweep_lg(l.nvar);
    const long ldp = sweep.part_ld(l.nvar), pstride = sweep.part_stride(l.nvar);
    double *part = w->st.scr.sweep_part.p;
    SweepBatch sb{};
    for (int q = 0; q < l.nbatch; ++q) sb.x[q] = l.bp.x[q];
    for (unsigned zz = 0; zz < l.p.grid[2]; ++zz) sb.p[zz] = part + (size_t)zz * (size_t)pstride;
    // launch timing: start = the sweep kernel begins, stop = the combine kernel ends (both belong to the apply)
    hipExtLaunchKernelGGL((spmm_sweep_kernel<FULL, IDENT, 0>), l.grid(), dim3(SWEEP_NW * 64), l.p.lds, l.stream, l.ev0, nullptr, 0, sweep_view(sweep), sb,
                          l.lda, l.nvar, sweep.nslot, ldp, lg, l.nbatch);
    hipExtLaunchKernelGGL(sweep_combine_kernel, dim3((unsigned)ceil_div(w->nrow, 4), l.p.grid[1], (unsigned)l.nbatch), dim3(256), 0, l.stream, nullptr, l.ev1, 0,
                          part, pstride, ldp, sweep.comb_ptr.p, sweep.comb_p.p, w->wM.p, l.fill, l.bp, l.ldb, w->nrow, l.nvar, lg);
}
template <int NW, int U, int TW, bool PAIR>
static void run_rowgroup(const Launch &l) {
    IBH_CHECK(!PAIR || (l.p.lds <= 64 * 1024 && l.nbatch == 1), "fused pair apply: %zu bytes of LDS / %d batches not supported", l.p.lds, l.nbatch);
    hipExtLaunchKernelGGL((spmm_rowgroup_kernel<NW, U, TW, PAIR>), l.grid(), dim3(NW * 64), l.p.lds, l.stream, l.ev0, l.ev1, 0, group_view(l.w->st.groups), l.bp,
                          l.lda, l.w->ncol, l.ldb, l.nvar, l.p.nfc, l.p.xcd_mode, l.w->wM.p, l.fill, PAIR ? *l.pair : PairView{});
}
// bands + combine: the events are recorded around the sequence
template <int FPW, int WK, int U, int NW, bool DUAL>
static void run_rowdual(const Launch &l) {
    const ibh_weighted *w = l.w;
    const Bands &bands = w->st.bands;
    const long ldp = bands.part_ld(), pstride = bands.part_stride(l.nvar);
    double *P0 = w->st.scr.band_part.p, *P1 = P0 + (size_t)l.nbatch * (size_t)pstride;
    BatchPtrs bq{};
    for (int q = 0; q < l.nbatch; ++q) { bq.x[q] = l.bp.x[q]; bq.y[q] = P0 + (size_t)q * (size_t)pstride; }
    if (l.ev0) IBH_HIP(hipEventRecord(l.ev0, l.stream));
    hipLaunchKernelGGL((spmm_rowblock_kernel<FPW, WK, U, NW, DUAL>), l.grid(), dim3(NW * 64), 0, l.stream, bands.ptr.p, bands.col.p, bands.v0.p, bq, l.nbatch, 1,
                       l.lda, w->ncol, ldp, w->nrow, l.nvar, l.p.nfc, l.p.xcd_mode, w->wM.p, l.fill, bands.v1.p, P1, (const int *)nullptr, pstride);
    hipLaunchKernelGGL(dual_combine_kernel, dim3((unsigned)ceil_div(w->nrow, 256), (unsigned)l.nvar, (unsigned)l.nbatch), dim3(256), 0, l.stream,
                       P0, P1, ldp, pstride, bands.rb1.p, w->wM.p, l.fill, l.bp, l.ldb, w->nrow, l.nvar);
    if (l.ev1) IBH_HIP(hipEventRecord(l.ev1, l.stream));
}
template <int NW, int U>
static void run_rowone(const Launch &l) {
    const ibh_weighted *w = l.w;
    hipExtLaunchKernelGGL((spmm_rowone_kernel<NW, U>), l.grid(), dim3(NW * 64), 0, l.stream, l.ev0, l.ev1, 0, w->rowptr.p, w->colind.p, w->val.p,
                          l.bp.x[0], l.bp.y[0], l.lda, w->ncol, l.ldb, w->nrow, l.nvar, l.p.nfc, l.p.xcd_mode, w->wM.p, l.fill);
}
template <int FPW, int WK, int U, int NW, bool DUAL>
static void run_rowblock(const Launch &l) {
    const ibh_weighted *w = l.w;
    const int *rowperm = l.p.lpt && ensure_rowperm(w, l.stream) ? w->st.scr.rowperm.p : nullptr;
    hipExtLaunchKernelGGL((spmm_rowblock_kernel<FPW, WK, U, NW, DUAL>), l.grid(), dim3(NW * 64), 0, l.stream, l.ev0, l.ev1, 0, w->rowptr.p, w->colind.p, w->val.p,
                          l.bp, l.nbatch, l.p.qi, l.lda, w->ncol, l.ldb, w->nrow, l.nvar, l.p.nfc, l.p.xcd_mode, w->wM.p, l.fill,
                          (const double *)nullptr, (double *)nullptr, rowperm, 0l);
}
// the I-row path: the events go to its first and last dispatch (transposed input + row kernel)
template <bool NT, int G, bool REALIGN, bool XT>
static void run_shortrow(const Launch &l) {
    const ibh_weighted *w = l.w;
    DevBuf<double> &xt = w->st.scr.xt;
    const long xt_stride = (long)w->ncol * l.p.ldt;
    hipEvent_t e_first = l.ev0;
    if (XT) {
        grow_scratch(xt, (size_t)xt_stride * (size_t)l.nbatch, l.stream, "transposed-input");
        hipExtLaunchKernelGGL(transpose_fields_kernel, dim3((unsigned)ceil_div(w->ncol, 64), (unsigned)(l.p.ldt / 16), (unsigned)l.nbatch), dim3(256), 0, l.stream,
                              e_first, nullptr, 0, l.bp, l.lda, l.nvar, w->ncol, xt.p, l.p.ldt, xt_stride);
        e_first = nullptr;
    }
    hipExtLaunchKernelGGL((spmm_shortrow_kernel<NT, G, REALIGN, XT>), l.grid(), dim3(SR_THREADS), 0, l.stream, e_first, l.ev1, 0, w->rowptr.p, w->colind.p, w->val.p,
                          l.bp, (const double *)xt.p, xt_stride, XT ? (long)l.p.ldt : l.lda, l.ldb, w->nrow, l.nvar, l.p.fper, w->wM.p, l.fill);
}
#define IBH_L_GT(...) {(const void *)spmm_grouptile_kernel<__VA_ARGS__>, run_grouptile<__VA_ARGS__>},
#define IBH_L_SW(...) {(const void *)spmm_sweep_kernel<__VA_ARGS__, 0>, run_sweep<__VA_ARGS__>},
#define IBH_L_RG(...) {(const void *)spmm_rowgroup_kernel<__VA_ARGS__>, run_rowgroup<__VA_ARGS__>},
#define IBH_L_RD(...) {(const void *)spmm_rowblock_kernel<__VA_ARGS__>, run_rowdual<__VA_ARGS__>},
#define IBH_L_R1(...) {(const void *)spmm_rowone_kernel<__VA_ARGS__>, run_rowone<__VA_ARGS__>},
#define IBH_L_RB(...) {(const void *)spmm_rowblock_kernel<__VA_ARGS__>, run_rowblock<__VA_ARGS__>},
#define IBH_L_SR(...) {(const void *)spmm_shortrow_kernel<__VA_ARGS__>, run_shortrow<__VA_ARGS__>},
static const Launcher RUN_GROUPTILE[] = {IBH_GROUPTILE_INSTS(IBH_L_GT)}, RUN_SWEEP[] = {IBH_SWEEP_INSTS(IBH_L_SW)}, RUN_ROWGROUP[] = {IBH_ROWGROUP_INSTS(IBH_L_RG)},
                      RUN_ROWDUAL[] = {IBH_ROWDUAL_INSTS(IBH_L_RD)}, RUN_ROWONE[] = {IBH_ROWONE_INSTS(IBH_L_R1)}, RUN_ROWBLOCK[] = {IBH_ROWBLOCK_INSTS(IBH_L_RB)},
                      RUN_SHORTROW[] = {IBH_SHORTROW_INSTS(IBH_L_SR)};
static const Launcher *const RUN[T_COUNT] = {RUN_GROUPTILE, RUN_SWEEP, RUN_ROWGROUP, RUN_ROWDUAL, RUN_ROWONE, RUN_ROWBLOCK, RUN_SHORTROW};

// nbatch <= IBH_MAX_BATCH batches by plan p (of the same nbatch), p.per_launch at a time
static void launch_plan(const ibh_weighted *w, const MatrixFacts &f, ApplyPlan p, const BatchPtrs &bp, int nbatch, int nvar, long lda, long ldb, double fill,
                        hipStream_t stream, const PairView *pair = nullptr)
{
    ApplyState::Scratch &scr = w->st.scr;
    if (p.band_part) grow_scratch(scr.band_part, p.band_part, stream, "band");
    if (p.sweep_part) grow_scratch(scr.sweep_part, p.sweep_part, stream, "column-sweep");
    // the transposed copies of a deep launch do not fit the scratch the handle owns: the launcher grows it -- unless the stream is
    // being captured (no allocation there): then as many batches per launch as fit
    if (p.xt * sizeof(double) > scr.xt.granted && p.per_launch > 1 && is_capturing(stream)) clamp_shortrow(p, f, nbatch, scr.xt.granted);
    hipEvent_t ev0 = g_ev_start, ev1 = g_ev_stop;
    g_ev_start = g_ev_stop = nullptr;
    for (int q0 = 0; q0 < nbatch; q0 += p.per_launch) {
        const int nq = std::min(p.per_launch, nbatch - q0);
        BatchPtrs bq{};
        bool misaligned = (ldb & 7) != 0;
        for (int q = 0; q < nq; ++q) {
            bq.x[q] = bp.x[q0 + q]; bq.y[q] = bp.y[q0 + q];
            misaligned = misaligned || (reinterpret_cast<uintptr_t>(bq.y[q]) & 63) != 0;
        }
        if (p.family == KERNEL_SHORTROW) align_shortrow(p, f, nvar, misaligned, nq);
        IBH_CHECK(p.inst >= 0 && p.inst < INSTS[p.table].n, "no apply kernel for this plan (table %d)", p.table);
        IBH_CHECK(p.nblocks < (1l << 31), "spmm grid too large (%ld blocks)", p.nblocks);
        IBH_CHECK(p.table == T_SHORTROW || p.table == T_SWEEP || (long)w->ncol * 8 < (1l << 31), "ncol too large for 32-bit buffer offsets");
        const Launcher &run = RUN[p.table][p.inst];
        if (p.lds > 64 * 1024) {                             // beyond the default dynamic-LDS limit: raise it once per device and kernel
            static std::mutex mu;
            static std::set<std::pair<int, const void *>> raised;
            std::lock_guard<std::mutex> lk(mu);
            if (!raised.count({w->device, run.kernel})) {
                IBH_HIP(hipFuncSetAttribute(run.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
                raised.insert({w->device, run.kernel});
            }
        }
        snprintf(w->st.last_sig, sizeof(w->st.last_sig), "%s", INSTS[p.table].v[p.inst].sig);
        run.run(Launch{w, p, bq, nq, nvar, lda, ldb, fill, stream, pair, q0 == 0 ? ev0 : nullptr, q0 + p.per_launch >= nbatch ? ev1 : nullptr});
    }
    IBH_HIP(hipGetLastError());
}

// A structure that cannot be built (out of memory, not representable) is no reason to fail an apply the row-by-row kernel
// serves: the failure is swallowed, the structure marked as tried, the matrix keeps its kernel.  Never inside a capture.
// `groups_asked`: the caller needs the row groups whatever the rules say (ibh_weighted_pair_prepare), and nothing else.
static void build_structures(const ibh_weighted *w, int nvar, int nbatch, bool seen, hipStream_t stream, long nseen = 1l << 30,
                             bool groups_asked = false) {
    ApplyState &st = w->st;
    const long ns = seen ? nseen : 0;
    auto groups = [&] { return wants_groups(facts_of(*w), nvar, nbatch, ns, groups_asked); };
    auto sweep = [&] { return !groups_asked && wants_sweep(facts_of(*w), nvar, nbatch, seen); };
    auto bands = [&] { return !groups_asked && !st.groups.built() && wants_bands(facts_of(*w), nvar, seen); };
    if ((!groups() && !sweep() && !bands()) || is_capturing(stream)) return;
    // (a builder hands over a finished structure or none: nothing to undo when it throws)
    auto attempt = [](bool &tried, auto &&build) {
        tried = true;
        try { build(); } catch (const Error &) { (void)hipGetLastError(); }
    };
    if (groups()) attempt(st.groups_tried, [&] { st.groups = build_groups_from_csr(w, stream); });
    if (sweep()) attempt(st.sweep_tried, [&] { st.sweep = build_sweep_from_csr(w, stream); });      // (also: an E-row matrix whose groups were declined just now)
    if (bands()) attempt(st.bands_tried, [&] { st.bands = build_bands_from_csr(w, stream); });
}

// Scratch of the launches that applies of (nvar, <= nbatch per launch) can make, by the family the rules pick and by those whose structure exists: a
// later set_kernel or tuning change must not turn a captured apply into an allocation.  (Shortrow's transposed input: where shortrow is the pick only.)
static size_t consv_count(const ibh_weighted *w, int nvar) { return 2 * (size_t)nvar + weight_dot_scratch(std::max(w->nrow, w->ncol), nvar); }
static void size_scratch(const ibh_weighted *w, int nvar, int nbatch) {
    ApplyState::Scratch &scr = w->st.scr;
    const MatrixFacts f = facts_of(*w);
    for (int nb : {1, nbatch})
        for (ApplyKernel k : {plan_apply(f, nvar, nb, false).family, KERNEL_ROWDUAL, KERNEL_COLSWEEP}) {
            if ((k == KERNEL_ROWDUAL && !f.bands_built) || (k == KERNEL_COLSWEEP && !f.sweep_built)) continue;
            const ApplyPlan p = plan_launch(f, k, nvar, nb, false);
            if (p.band_part) grow_scratch(scr.band_part, p.band_part, nullptr, "band");
            if (p.sweep_part) grow_scratch(scr.sweep_part, p.sweep_part, nullptr, "column-sweep");
            if (p.xt) grow_scratch(scr.xt, p.xt, nullptr, "transposed-input");
        }
    grow_scratch(scr.consv, consv_count(w, nvar), nullptr, "conservation");
    // apply_transformed: the small side holds nvar fields
    grow_scratch(scr.scratch, (size_t)nvar * (size_t)std::min(w->nrow, w->ncol), nullptr, "transform");
    ensure_rowsum1(w, nullptr);
    if (get_tuning("rowblock_lpt", 0)) (void)ensure_rowperm(w, nullptr);
}

void weighted_reserve(const ibh_weighted *w, int nvar) {
    HandleScope hs_(w);
    if (nvar > 0) size_scratch(w, nvar, 1);
}

void weighted_prepare(const ibh_weighted *w, int nvar, int nbatch, bool groups_asked) {
    HandleScope hs_(w);
    if (nvar <= 0 || nbatch <= 0 || w->nrow == 0) return;
    const int nb = std::min(nbatch, IBH_MAX_BATCH);           // deeper batches are split into launches of IBH_MAX_BATCH
    build_structures(w, nvar, nb, true, nullptr, 1l << 30, groups_asked);
    size_scratch(w, nvar, nb);
    IBH_HIP(hipStreamSynchronize(nullptr));
}
// ---- fused pair: B1 = first * A, B2 = second * B1 in one launch (BASELINE config 3: EvI then AvE) --------------------------------
// Possible when every row of `second` reads rows of ONE row group of `first` only -- AvE after EvI: the value of a GCM cell is a
// combination of that cell's own elevation classes -- so the group's workgroup has all inputs of the second row in hand when
// it has its class sums.  The pairing is worked out on the host (the second matrix is tiny: one entry per class) through the
// SPARSE indices of the two matrices' shared dimension, so the two need not share a SparseSet object or a numbering.
void weighted_pair_prepare(const ibh_weighted *first, const ibh_weighted *second, int nvar) {
    HandleScope hs_(first);
    IBH_CHECK(first && second && first != second, "pair: two different matrices expected");
    IBH_CHECK(first->device == second->device, "pair: matrices live on different devices");
    IBH_CHECK(second->ncol == first->nrow || second->dims[1], "pair: the second matrix's columns are not the first one's rows");
    IBH_CHECK(second->nnz <= (1 << 22), "pair: the second matrix is too large (%ld entries) to be paired on the host", (long)second->nnz);
    RowGroups &grp = first->st.groups;
    grp.pair = {};
    if (!grp.built()) weighted_prepare(first, nvar > 0 ? nvar : 16, 1, true);       // row groups first (small matrices get them from an explicit request only)
    if (!grp.built()) fail(IBH_ENOTIMPL, "pair: the first matrix has no row groups (not an elevation-class-row matrix, or its structure was declined)");
    const int ngrp = grp.n;
    std::vector<int32_t> slotrow((size_t)ngrp * IBH_GSLOTS), gns((size_t)ngrp), rp2((size_t)second->nrow + 1), ci2((size_t)second->nnz);
    std::vector<double> v2((size_t)second->nnz);
    IBH_HIP(hipMemcpy(slotrow.data(), grp.slotrow.p, slotrow.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    IBH_HIP(hipMemcpy(gns.data(), grp.ns.p, gns.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    IBH_HIP(hipMemcpy(rp2.data(), second->rowptr.p, rp2.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (second->nnz) {
        IBH_HIP(hipMemcpy(ci2.data(), second->colind.p, ci2.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        IBH_HIP(hipMemcpy(v2.data(), second->val.p, v2.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    // first row (dense) -> (group, slot)
    std::vector<int32_t> where_g((size_t)first->nrow, -1), where_s((size_t)first->nrow, -1);
    for (int g = 0; g < ngrp; ++g)
        for (int sl = 0; sl < gns[(size_t)g]; ++sl) {
            const int r = slotrow[(size_t)g * IBH_GSLOTS + sl];
            IBH_CHECK(r >= 0 && r < first->nrow, "pair: corrupt group table");
            where_g[(size_t)r] = g; where_s[(size_t)r] = sl;
        }
    // second column (dense) -> first row (dense), through the sparse indices of the shared dimension
    const ibh_sparse_set *d1 = first->dims[0], *d2 = second->dims[1];
    const bool same_numbering = d1 == d2 || !d1 || !d2;
    if (same_numbering) IBH_CHECK(second->ncol == first->nrow, "pair: extents differ (%d columns, %d rows)", second->ncol, first->nrow);
    else if (d1->sparse_extent() != d2->sparse_extent())
        fail(IBH_ENOTIMPL, "pair: the second matrix's columns (extent %ld) are not the first one's rows (extent %ld)",
             (long)d2->sparse_extent(), (long)d1->sparse_extent());
    const int64_t *cols2 = same_numbering ? nullptr : d2->to_sparse_host();     // the second matrix's columns, sparse
    std::vector<double> pw((size_t)ngrp * IBH_GSLOTS, 0.0);
    std::vector<uint32_t> pm((size_t)ngrp, 0u);
    std::vector<int32_t> pr((size_t)ngrp, -1);
    for (int a = 0; a < second->nrow; ++a) {
        if (rp2[(size_t)a] == rp2[(size_t)a + 1]) fail(IBH_ENOTIMPL, "pair: row %d of the second matrix has no entries", a);
        int grp = -1;
        for (int k = rp2[(size_t)a]; k < rp2[(size_t)a + 1]; ++k) {
            int r1 = ci2[(size_t)k];
            if (!same_numbering) {
                r1 = d1->to_dense(cols2[(size_t)r1]);
                if (r1 < 0) fail(IBH_ENOTIMPL, "pair: a column of the second matrix is no row of the first");
            }
            IBH_CHECK(r1 >= 0 && r1 < first->nrow, "pair: column out of range");
            const int g = where_g[(size_t)r1], sl = where_s[(size_t)r1];
            if (g < 0 || (grp >= 0 && g != grp)) fail(IBH_ENOTIMPL, "pair: row %d of the second matrix reads rows of more than one group of the first", a);
            grp = g;
            pw[(size_t)g * IBH_GSLOTS + sl] = v2[(size_t)k];
            pm[(size_t)g] |= 1u << sl;
        }
        if (pr[(size_t)grp] >= 0) fail(IBH_ENOTIMPL, "pair: two rows of the second matrix read the same group of the first");
        pr[(size_t)grp] = a;
    }
    Pair pair;
    pair.w.alloc(pw.size()); pair.mask.alloc(pm.size()); pair.row.alloc(pr.size());
    IBH_HIP(hipMemcpy(pair.w.p, pw.data(), pw.size() * sizeof(double), hipMemcpyHostToDevice));
    IBH_HIP(hipMemcpy(pair.mask.p, pm.data(), pm.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    IBH_HIP(hipMemcpy(pair.row.p, pr.data(), pr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    pair.second = second;
    pair.uid = second->uid;
    grp.pair = std::move(pair);
}

void spmm_launch_pair(const ibh_weighted *first, const ibh_weighted *second, const double *dA, int nvar, int64_t lda, double *dB1,
                      int64_t ldb1, double *dB2, int64_t ldb2, double fill, hipStream_t stream)
{
    HandleScope hs_(first);
    const Pair &pair = first->st.groups.pair;
    IBH_CHECK(pair.second == second && pair.uid == second->uid && first->st.groups.built(),
              "pair apply: call ibh_weighted_pair_prepare(first, second, nvar) first");
    if (nvar <= 0 || first->nrow == 0) return;
    IBH_CHECK(lda >= first->ncol && ldb1 >= first->nrow && ldb2 >= second->nrow, "pair apply: leading dimensions (%ld, %ld, %ld) too small",
              (long)lda, (long)ldb1, (long)ldb2);
    IBH_CHECK(first->conservative && second->conservative, "pair apply: smoothed (non-conservative) matrices take separate applies");
    BatchPtrs bp{};
    bp.x[0] = dA; bp.y[0] = dB1;
    const PairView pv = pair_view(pair, dB2, (long)ldb2);
    const MatrixFacts f = facts_of(*first);
    launch_plan(first, f, plan_apply(f, nvar, 1, true), bp, 1, nvar, (long)lda, (long)ldb1, fill, stream, &pv);
    first->st.last_kernel = KERNEL_ROWGROUP;
    second->st.last_kernel = KERNEL_ROWGROUP;
    ++first->st.napply; ++second->st.napply;
}
// B1 = first * A, B2 = second * B1 (the fused pair), B3 = third * B2: the chain ice -> elevation classes -> atmosphere -> ice of
// BASELINE config 3 (EvI, AvE, IvA): the pair launch and the third matrix's apply, stream-ordered.
void spmm_launch_chain(const ibh_weighted *first, const ibh_weighted *second, const ibh_weighted *third, const double *dA, int nvar, int64_t lda,
                       double *dB1, int64_t ldb1, double *dB2, int64_t ldb2, double *dB3, int64_t ldb3, double fill, hipStream_t stream)
{
    IBH_CHECK(third->ncol == second->nrow, "chain: the third matrix reads %d columns, the second makes %d rows", third->ncol, second->nrow);
    if (nvar <= 0 || first->nrow == 0) return;
    spmm_launch_pair(first, second, dA, nvar, lda, dB1, ldb1, dB2, ldb2, fill, stream);
    spmm_launch(third, dB2, nvar, ldb2, dB3, ldb3, fill, 0, stream);
}

void spmm_launch_many(const ibh_weighted *w, int nbatch, const double *const *dA, int nvar, int64_t lda,
                      double *const *dB, int64_t ldb, double fill, int force_conservation, hipStream_t stream)
{
    HandleScope hs_(w);
    if (nvar <= 0 || w->nrow == 0 || nbatch <= 0) return;
    IBH_CHECK(lda >= w->ncol && ldb >= w->nrow, "apply: leading dimensions (%ld, %ld) smaller than (%d, %d)",
              (long)lda, (long)ldb, w->ncol, w->nrow);
    // A matrix that is applied again gets the structures its applies want now (wants_bands, wants_sweep, wants_groups: apply_plan.h).
    // This is the one place where an apply synchronises and allocates: ibh_weighted_prepare() does it up front,
    // ibh_set_tuning("lazy_structures", 0) switches it off.
    if (get_tuning("lazy_structures", 1)) build_structures(w, nvar, std::min(nbatch, IBH_MAX_BATCH), w->st.napply >= 1, stream, (long)w->st.napply);
    ++w->st.napply;
    const MatrixFacts f = facts_of(*w);
    // the family is chosen once, by the whole call's nbatch; a last launch of fewer batches keeps it and plans its own shape
    ApplyPlan plan = plan_apply(f, nvar, nbatch, false, lda);
    w->st.last_kernel = plan.family;
    w->st.last_sig[0] = 0;
    const bool correct = !w->conservative && force_conservation;
    if (correct) grow_scratch(w->st.scr.consv, consv_count(w, nvar), stream, "conservation");
    for (int b0 = 0; b0 < nbatch; b0 += IBH_MAX_BATCH) {
        const int nb = std::min(IBH_MAX_BATCH, nbatch - b0);
        BatchPtrs bp{};
        for (int q = 0; q < nb; ++q) {
            IBH_CHECK(dA[b0 + q] && dB[b0 + q], "apply: null field pointer in batch %d", b0 + q);
            bp.x[q] = dA[b0 + q]; bp.y[q] = dB[b0 + q];
        }
        if (nb != std::min(nbatch, IBH_MAX_BATCH)) plan = plan_launch(f, plan.family, nvar, nb, false);
        launch_plan(w, f, plan, bp, nb, nvar, (long)lda, (long)ldb, fill, stream);
        if (correct) {
            // factor_k = (Mw . A_k) / (wM . B_k); rows with wM == 0 hold `fill` and are skipped.  The two
            // dot products live in handle-owned scratch: stream-ordered, no allocation, no host sync.
            for (int q = 0; q < nb; ++q) {
                double *T = w->st.scr.consv.p;
                weight_dot_launch(w->Mw.p, w->ncol, bp.x[q], nvar, lda, T, T + 2 * nvar, stream);
                weight_dot_launch(w->wM.p, w->nrow, bp.y[q], nvar, ldb, T + nvar, T + 2 * nvar, stream);
                dim3 grid((unsigned)ceil_div(w->nrow, 256), (unsigned)nvar);
                hipLaunchKernelGGL(conserve_scale_kernel, grid, dim3(256), 0, stream, bp.y[q], (long)ldb, w->nrow, w->wM.p,
                                   T, T + nvar);
            }
            IBH_HIP(hipGetLastError());
        }
    }
}

void spmm_launch(const ibh_weighted *w, const double *dA, int nvar, int64_t lda, double *dB, int64_t ldb,
                 double fill, int force_conservation, hipStream_t stream)
{
    spmm_launch_many(w, 1, &dA, nvar, lda, &dB, ldb, fill, force_conservation, stream);
}

// ---- legacy coo_matvec contract (pylib/icebin_cython.cpp:158-192) ----------------------------------
// yy = M xx with "REPLACE" semantics: a row is written only if at least one of its terms survives;
// with ignore_nan, terms whose input is NaN are skipped; rows with no surviving term keep whatever
// the caller put in yy (icebin.coo_multiply presets `fill`).  No wM involved.  One wave per (row,
// field) for long rows, one thread for short ones; fixed summation order.
template <bool WAVE>
__global__ void matvec_legacy_kernel(const int *__restrict__ rowptr, const int *__restrict__ colind,
                                     const double *__restrict__ vals, const double *__restrict__ X, long ldx,
                                     double *__restrict__ Y, long ldy, int nrow, int ignore_nan)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int r = (int)(WAVE ? t >> 6 : t);
    const int lane = WAVE ? (int)(threadIdx.x & 63) : 0;
    if (r >= nrow) return;
    const double *x = X + (long)blockIdx.y * ldx;
    double acc = 0.0;
    int live = 0;
    for (int k = rowptr[r] + lane; k < rowptr[r + 1]; k += WAVE ? 64 : 1) {
        const double xv = x[colind[k]];
        if (ignore_nan && xv != xv) continue;
        acc = fma(vals[k], xv, acc);
        ++live;
    }
    if (WAVE) {
        acc = wave_sum(acc);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) live += __shfl_xor(live, off, 64);
    }
    if (lane == 0 && live > 0) Y[(long)blockIdx.y * ldy + r] = acc;
}
void matvec_legacy_launch(const ibh_weighted *w, const double *dx, int nvar, int64_t ldx, double *dy, int64_t ldy,
                          int ignore_nan, hipStream_t stream)
{
    if (nvar <= 0 || w->nrow == 0) return;
    IBH_CHECK(ldx >= w->ncol && ldy >= w->nrow, "coo_matvec: leading dimensions too small");
    const bool wave = w->nnz >= 8 * (int64_t)w->nrow;
    if (wave)
        hipLaunchKernelGGL(matvec_legacy_kernel<true>, dim3((unsigned)ceil_div((long)w->nrow * 64, 256), (unsigned)nvar), dim3(256), 0,
                           stream, w->rowptr.p, w->colind.p, w->val.p, dx, (long)ldx, dy, (long)ldy, w->nrow, ignore_nan);
    else
        hipLaunchKernelGGL(matvec_legacy_kernel<false>, dim3((unsigned)ceil_div(w->nrow, 256), (unsigned)nvar), dim3(256), 0,
                           stream, w->rowptr.p, w->colind.p, w->val.p, dx, (long)ldx, dy, (long)ldy, w->nrow, ignore_nan);
    IBH_HIP(hipGetLastError());
}

// ---- coupler-shaped product M * (V*T + b) ---------------------------------------------------
// out[k, j] = sum_l T[l,k] * in[l, j] + b[k] * (scale ? scale[j] : 1): the variable transform, applied
// on whichever side of M is small.  T entries that are exactly 0 are structural (skipped: a NaN in an
// unused input variable must not reach the outputs).  One thread per column j.
// T (row-major nvar_in x nvar_out) and b travel in the kernarg segment (TB_MAX doubles): the caller's
// host arrays are consumed at launch time, nothing is copied asynchronously from them and the call
// stays stream-ordered and graph-capturable.  Larger transforms go through a device copy.
constexpr int TB_MAX = 384;
struct TransformArgs { double tb[TB_MAX]; };
template <bool INLINE>
__global__ void transform_kernel(const double *__restrict__ in, long ldin, int nin, const TransformArgs ta,
                                 const double *__restrict__ Tdev, const double *__restrict__ scale,
                                 const double *__restrict__ wM, double fill, double *__restrict__ out, long ldout,
                                 int nout, int n)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = blockIdx.y;
    if (j >= n) return;
    const double *Tm = INLINE ? ta.tb : Tdev;
    const double *b = Tm + (size_t)nin * nout;
    double acc = 0.0;
    for (int l = 0; l < nin; ++l) {
        const double t = Tm[l * nout + k];
        if (t != 0.0) acc = fma(t, in[(long)l * ldin + j], acc);
    }
    acc += scale ? b[k] * scale[j] : b[k];
    if (wM && wM[j] == 0.0) acc = fill;
    out[(long)k * ldout + j] = acc;
}
// rowsum1[r] = sum of row r of M (= M * 1, the factor of the offset term b): one wave per row
__global__ void rowsum_kernel(const int *__restrict__ rowptr, const double *__restrict__ vals, int nrow,
                              double *__restrict__ out)
{
    const int r = (int)(((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= nrow) return;
    double acc = 0.0;
    for (int k = rowptr[r] + lane; k < rowptr[r + 1]; k += 64) acc += vals[k];
    acc = wave_sum(acc);
    if (lane == 0) out[r] = acc;
}
void ensure_rowsum1(const ibh_weighted *w, hipStream_t stream) {
    ApplyState::Scratch &scr = w->st.scr;
    if (scr.have_rowsum1 || w->nrow == 0) return;
    grow_scratch(scr.rowsum1, (size_t)w->nrow, stream, "row-sum");
    hipLaunchKernelGGL(rowsum_kernel, dim3(ceil_div((long)w->nrow * 64, 256)), dim3(256), 0, stream, w->rowptr.p, w->val.p,
                       w->nrow, scr.rowsum1.p);
    IBH_HIP(hipGetLastError());
    scr.have_rowsum1 = true;
}

void spmm_transformed_launch(const ibh_weighted *w, const double *dA, int nvar_in, int64_t lda, const double *T,
                             const double *b, int nvar_out, double *dB, int64_t ldb, double fill, hipStream_t stream)
{
    if (nvar_out <= 0 || w->nrow == 0) return;
    IBH_CHECK(nvar_in > 0 && T && b, "apply_transformed: empty transform");
    IBH_CHECK(lda >= w->ncol && ldb >= w->nrow, "apply_transformed: leading dimensions too small");
    const size_t ntb = (size_t)nvar_in * nvar_out + nvar_out;
    const bool inl = ntb <= (size_t)TB_MAX;
    ApplyState::Scratch &scr = w->st.scr;
    TransformArgs ta;
    const double *dT = nullptr;
    if (inl) {
        std::copy(T, T + (size_t)nvar_in * nvar_out, ta.tb);
        std::copy(b, b + nvar_out, ta.tb + (size_t)nvar_in * nvar_out);
    } else {
        // more than TB_MAX coefficients: staged through a device copy (synchronises; not capturable)
        std::vector<double> tb(ntb);
        std::copy(T, T + (size_t)nvar_in * nvar_out, tb.begin());
        std::copy(b, b + nvar_out, tb.begin() + (size_t)nvar_in * nvar_out);
        grow_scratch(scr.tbuf, ntb, stream, "transform-coefficient");
        IBH_HIP(hipStreamSynchronize(stream));      // an earlier apply may still read tbuf
        IBH_HIP(hipMemcpyAsync(scr.tbuf.p, tb.data(), sizeof(double) * ntb, hipMemcpyHostToDevice, stream));
        IBH_HIP(hipStreamSynchronize(stream));      // tb is a stack-lifetime staging buffer
        dT = scr.tbuf.p;
    }
    auto transform = [&](const double *in, long ldin, const double *scale, const double *wM, double *out, long ldout, int n) {
        dim3 grid((unsigned)ceil_div(n, 256), (unsigned)nvar_out);
        if (inl) hipLaunchKernelGGL(transform_kernel<true>, grid, dim3(256), 0, stream, in, ldin, nvar_in, ta, dT, scale, wM, fill, out, ldout, nvar_out, n);
        else hipLaunchKernelGGL(transform_kernel<false>, grid, dim3(256), 0, stream, in, ldin, nvar_in, ta, dT, scale, wM, fill, out, ldout, nvar_out, n);
        IBH_HIP(hipGetLastError());
    };
    if (w->ncol <= w->nrow) {
        // inputs are the small side: X' = V*T + b, then B = M * X'
        grow_scratch(scr.scratch, (size_t)nvar_out * (size_t)w->ncol, stream, "transform");
        transform(dA, (long)lda, nullptr, nullptr, scr.scratch.p, (long)w->ncol, w->ncol);
        spmm_launch(w, scr.scratch.p, nvar_out, w->ncol, dB, ldb, fill, 0, stream);
    } else {
        // outputs are the small side: Z = M * V, then B = T^T Z + b * (M * 1), rows with wM == 0 -> fill
        ensure_rowsum1(w, stream);
        grow_scratch(scr.scratch, (size_t)nvar_in * (size_t)w->nrow, stream, "transform");
        spmm_launch(w, dA, nvar_in, lda, scr.scratch.p, w->nrow, 0.0, 0, stream);
        transform(scr.scratch.p, (long)w->nrow, scr.rowsum1.p, w->wM.p, dB, (long)ldb, w->nrow);
    }
}

}  // namespace ibh
