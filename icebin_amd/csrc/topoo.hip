// topoo.hip -- modele/topo_base.cpp's _make_topoO (:263-809) with its callZ (:20-221) from arrays: the base ocean-grid TOPO planes
// from the four 1' planes FGICE1m / ZICETOP1m / ZSOLG1m / FOCEAN1m and the lake plane FLAKES; DESIGN.md 21.
//
// Where things live.  The int16 planes stay in HBM in their own width, the 20 output planes are doubles [jmO, imO] at
// planes + k * ld in the reference's order of out.add (:275-377).  One call enqueues, stream-ordered:
//   six typed Hntr regrids (:392, :399, :575, :646, :661, :663), straight into FOCEANF, FGICEF, FLAKE, dZOCEN and two work planes
//   k_to_cells   every ocean cell from its own values: the south-pole row (:498-502), the rounding under SET_TO (:506-531), FLAKE's
//                bands, wedge, apportioning and clamp (:578-623), FGRND (:633-641), dZOCEN (:646-655), ZSOLDG (:723) and the cell's
//                own half of dZGICE (:681-692)
//   k_to_gice    one workgroup: a lane per row for the sums over I, one lane for the chain over J and CONSTK, then the fill (:694-710)
//   k_to_tiles   callZ, one workgroup per ocean cell (one per pole row): the tile staged in LDS, its land cells as 32-bit keys, a
//                bitonic sort, and every chain of :92-205 walked by one wave in lockstep
//   k_to_tiles<LONG>  the same for tiles above IBH_MAKE_TOPOO_MAX_TILE cells, with a counting sort in global scratch
//   k_to_resets, k_to_blocks   :747-758 and :761-795
// The row areas (make_dxyp, libm sin) are host tables uploaded by the handle, so a call only enqueues.  The 16-byte split of a tile's
// row, the eight-cell loads, the LDS sort and the argument checks are planetile.h's, shared with globalec.hip and etopo1.hip.
#include <algorithm>
#include <climits>
#include <memory>
#include <vector>

#include "planetile.h"

namespace ibh {
namespace {
enum ToPlane {
    P_FOCEAN, P_FLAKE, P_FGRND, P_FGICE, P_FGICE_GREENLAND, P_ZATMO, P_DZOCEN, P_DZLAKE, P_DZGICE, P_ZSOLDG, P_ZICETOP, P_ZLAND_MIN, P_ZLAND_MAX,
    P_ZSGLO, P_ZLAKE, P_ZGRND, P_ZSGHI, P_FOCEANF, P_FGICEF, P_ZATMOF, P_N
};
static_assert(P_N == IBH_MAKE_TOPOO_NPLANE, "plane count");
// the status words on the device
enum ToStat { S_OCEAN_FLAG, S_OCEAN_MIN, S_CONT_FLAG, S_CONT_MIN, S_FGICE_LOW, S_FGICE_HIGH, S_FLAKE_REDUCED, S_FGRND_RANGE, S_DZOCEN_NONPOS, S_FLAKE_ONE, S_N };
static_assert(S_N == IBH_MAKE_TOPOO_NSTATUS, "status count");
constexpr int TO_T = 256;
constexpr int TO_BINS = 65536;      // the depths of an int16
}  // namespace
}  // namespace ibh

struct ibh_make_topoo {
    int device = 0;
    int32_t imI = 0, jmI = 0, imO = 0, jmO = 0, imS = 0, jmS = 0, mult_i = 0, mult_j = 0;
    ibh::DevBuf<double> dxypI, dxypO;           // [jmI], [jmO]: make_dxyp with a 0-based row
    ibh_hntr *hntrI = nullptr, *hntrS = nullptr;    // Hntr(17.17, hspecO, hspecI) (:391), Hntr(17.17, hspecO, hspecS) (:574)
    ibh::DevBuf<int8_t> set_to;                 // [nO] 0 none, 1 ocean, 2 land (:403-494)
    ibh::DevBuf<int32_t> reset_x;               // [nreset] 0-based cells (:231-248)
    ibh::DevBuf<double> reset_elev;
    int32_t nreset = 0;
    ibh::DevBuf<double> work;                   // zictop, zsolg, pow(RGICE, .3) [3 * nO], the row sums [2 * jmO]
    ibh::DevBuf<uint32_t> scratch;              // the long path: per tile TO_BINS counts and the sorted cells
    ibh::DevBuf<int32_t> status;                // [S_N]
    bool long_interior = false, long_poles = false;
    int64_t nI() const { return (int64_t)imI * jmI; }
    int64_t nO() const { return (int64_t)imO * jmO; }
    int64_t nS() const { return (int64_t)imS * jmS; }
    ~ibh_make_topoo() {
        if (hntrI) ibh_hntr_destroy(hntrI);
        if (hntrS) ibh_hntr_destroy(hntrS);
    }
};

namespace ibh {
namespace {

// ---- :498-655, :681-692, :723: everything a cell takes from its own values ------------------------------------------------------
__global__ __launch_bounds__(TO_T) void k_to_cells(double *__restrict__ planes, long ld, const double *__restrict__ zictop,
                                                   const double *__restrict__ zsolg, double *__restrict__ powp,
                                                   const int8_t *__restrict__ set_to, int IM, int JM, int *__restrict__ status) {
    const long x = (long)blockIdx.x * TO_T + threadIdx.x;
    if (x >= (long)IM * JM) return;
    const int J = (int)(x / IM) + 1, I = (int)(x - (long)(J - 1) * IM) + 1;
    const double foceanf = planes[P_FOCEANF * ld + x];
    double fgicef = planes[P_FGICEF * ld + x];
    double focean, fgice;
    if (J == 1) {       // :498-502
        focean = 0; fgice = 1; fgicef = 1;
        planes[P_FGICEF * ld + x] = fgicef;
    } else {            // :506-531
        const int s = set_to[x];
        const bool to_ocean = s == 1 ? true : s == 2 ? false : foceanf >= .5;
        if (to_ocean) {
            focean = 1.; fgice = 0;
        } else {
            const double fact = 1. / (1. - foceanf);
            focean = 0.; fgice = fgicef * fact;
        }
    }
    // :578-586
    double flake = planes[P_FLAKE * ld + x];
    if (J <= JM / 6 || J >= JM * 14 / 15 + 1 || (I <= IM / 2 && J >= JM * 41 / 45 + 1)) flake = 0;
    if (J >= (JM * 5) / 6 && J <= (JM * 11) / 12 && I >= IM / 3 + 1 && I <= (int)(.5 + .75 * IM * (J - JM * .3) / JM)) flake = 0;
    // :589-600
    const double fcont = 1. - focean, fcontf = 1. - foceanf;
    if (fcontf != 0.) {
        flake = flake * fcont / (fcontf + 1e-20);
        flake = round(flake * 256.) / 256.;
    }
    // :608-623
    if (J >= JM / 6 + 1) {
        if (fgice < 0) { atomicAdd(&status[S_FGICE_LOW], 1); fgice = 0; }
        if (fgice > 1) { atomicAdd(&status[S_FGICE_HIGH], 1); fgice = 1; }
        if (flake + fgice + focean > 1) { atomicAdd(&status[S_FLAKE_REDUCED], 1); flake = 1. - fgice - focean; }
    }
    // :633-641
    double fgrnd = 1.0 - focean - flake - fgice;
    if (fabs(fgrnd) < 1.e-14) fgrnd = 0;
    if (fgrnd < 0 || fgrnd > 1) atomicAdd(&status[S_FGRND_RANGE], 1);
    // :646-655, :723
    const double dzocen = -planes[P_DZOCEN * ld + x] * focean;
    if (focean == 1 && dzocen <= 0) atomicAdd(&status[S_DZOCEN_NONPOS], 1);
    // :681-692
    const double dzgice = zictop[x] - zsolg[x];
    double pw = 0;
    if (!(dzgice != 0)) pw = pow(fgice / (fcont + 1e-20), .3);
    powp[x] = pw;
    planes[P_FOCEAN * ld + x] = focean;
    planes[P_FGICE * ld + x] = fgice;
    planes[P_FLAKE * ld + x] = flake;
    planes[P_FGRND * ld + x] = fgrnd;
    planes[P_DZOCEN * ld + x] = dzocen;
    planes[P_ZSOLDG * ld + x] = -dzocen;
    planes[P_DZGICE * ld + x] = dzgice != 0 ? dzgice : 0;
}

// ---- :671-711 -------------------------------------------------------------------------------------------------------------------
// One workgroup.  A lane per row J sums its cells over I in order (:680-693), one lane then walks J in order (:694-698), and every
// thread fills its share of cells (:701-710).  A cell took :688-691 iff zictop - zsolg is not != 0, which is recomputed here.
__global__ __launch_bounds__(TO_T) void k_to_gice(double *__restrict__ planes, long ld, const double *__restrict__ zictop,
                                                  const double *__restrict__ zsolg, const double *__restrict__ powp,
                                                  const double *__restrict__ dxypO, double *__restrict__ rowsum, int IM, int JM) {
    __shared__ double s_constk;
    const int tid = threadIdx.x;
    const double *fgice = planes + P_FGICE * ld;
    for (int j = tid; j < JM; j += TO_T) {
        double sum_dfr = 0, sum_df = 0;
        for (int i = 0; i < IM; ++i) {
            const long x = (long)j * IM + i;
            if (zictop[x] - zsolg[x] != 0) continue;
            sum_dfr += fgice[x] * powp[x];
            sum_df += fgice[x];
        }
        rowsum[j] = sum_dfr; rowsum[JM + j] = sum_df;
    }
    __syncthreads();
    if (tid == 0) {
        double SUMDFR = 0, SUMDF = 0;
        for (int j = 0; j < JM; ++j) {
            SUMDFR += dxypO[j] * rowsum[j];
            SUMDF += dxypO[j] * rowsum[JM + j];
        }
        s_constk = 264.7 * SUMDF / SUMDFR;
    }
    __syncthreads();
    const double CONSTK = s_constk;
    double *dzg = planes + P_DZGICE * ld;
    for (long x = tid; x < (long)IM * JM; x += TO_T) {
        if (fgice[x] == 0) dzg[x] = 0;
        else if (dzg[x] == 0) dzg[x] = CONSTK * powp[x];
    }
}

// ---- callZ (:20-221) ---------------------------------------------------------------------------------------------------------------
// a fine cell as the chains want it: the biased elevation in the high half, bit 1: FGICE1m != 0, bit 0: FOCEAN1m == 1
__device__ __forceinline__ uint32_t to_pack(int zt, int fg, int fo) {
    return (uint32_t)(zt + 32768) << 16 | (fg != 0 ? 2u : 0u) | (fo == 1 ? 1u : 0u);
}

struct ToTiles {
    const int16_t *fg, *zt, *fo;        // FGICE1m, ZICETOP1m, FOCEAN1m (callZ never reads ZSOLG1m)
    const double *dxypI;
    double *planes;
    long ld;
    int *status;
    uint32_t *scratch;                  // LONG: per workgroup TO_BINS + w * mult_j words
    int imI, imO, mult_j;
    int w;                              // fine columns of a tile: mult_i, or imI on the pole rows (IMAX = 1, :64-67)
    int imax, jO0, jstep;               // workgroup b owns ocean cell (jO0 + (b / imax) * jstep, b % imax)
};

// Workgroup b owns one ocean cell and its tile of w x mult_j fine cells, traversal position c = (J1m - J11) * w + (I1m - I11).
// Short path: the tile is staged in LDS (elevation and two flag bits a cell, read in 16-byte pieces between a row's unaligned head
// and tail); a land cell becomes the key (ZICETOP1m + 32768) << 16 | c, so ascending keys are (depth, traversal position); the keys
// are appended in any order and sorted by planetile.h's lds_sort_keys.  Long path: nothing is staged; the
// land cells are counted per depth in global scratch, the counts scanned, and the cells placed 256 at a time in traversal order --
// a cell goes to its depth's cursor plus the number of equal depths before it in its chunk -- which gives the same order.
// Wave 0 then walks every chain in lockstep: 64 cells a step are fetched one a lane and broadcast lane by lane, and every lane
// carries the same sums, so each chain is the reference's, term by term in its order.
template <bool LONG>
__global__ __launch_bounds__(TO_T) void k_to_tiles(ToTiles A) {
    extern __shared__ uint32_t s_key[];
    __shared__ int s_n, s_min;
    __shared__ int s_d[LONG ? TO_T : 1];
    __shared__ uint32_t s_part[LONG ? TO_T : 1];
    const int tid = threadIdx.x;
    const int q = (int)(blockIdx.x / (unsigned)A.imax), iO = (int)(blockIdx.x - (unsigned)q * (unsigned)A.imax), jO = A.jO0 + q * A.jstep;
    const long xO = (long)jO * A.imO + iO;
    const int w = A.w, h = A.mult_j, ncell = w * h;
    const size_t jrow0 = (size_t)jO * h;
    const size_t base = jrow0 * (size_t)A.imI + (size_t)iO * w;
    const bool ocean = A.planes[P_FOCEAN * A.ld + xO] != 0;     // :69
    const int n2 = pow2_ceil(ncell);
    uint16_t *s_z = reinterpret_cast<uint16_t *>(s_key + (LONG ? 0 : n2));
    uint8_t *s_f = reinterpret_cast<uint8_t *>(s_z + (LONG ? 0 : ncell));
    uint32_t *cnt = LONG ? A.scratch + (size_t)blockIdx.x * ((size_t)TO_BINS + ncell) : nullptr, *ord = LONG ? cnt + TO_BINS : nullptr;
    if (tid == 0) { s_n = 0; s_min = INT_MAX; }

    auto cell = [&](int c) -> uint32_t {
        if (LONG) {
            const int r = c / w;
            const size_t x = base + (size_t)r * A.imI + (size_t)(c - r * w);
            return to_pack(A.zt[x], A.fg[x], A.fo[x]);
        }
        return (uint32_t)s_z[c] << 16 | s_f[c];
    };

    if (!LONG) {
        // a row is FOCEAN1m's PlaneSplit: work items [0, P8) of a row are its pieces, the 16 after them its loose cells
        const int P8 = w >> 3, per = P8 + 16;
        for (int it = tid; it < h * per; it += TO_T) {
            const int r = it / per, k = it - r * per;
            const size_t x0 = base + (size_t)r * A.imI;
            const PlaneSplit S = plane_split(A.fo + x0, (unsigned)w);
            if (k < P8) {
                if (k >= (int)S.npiece) continue;
                const int c0 = (int)S.piece((unsigned)k);
                const int16_t *pzt = A.zt + x0 + c0, *pfg = A.fg + x0 + c0;
                const short8 fo = load8(A.fo + x0 + c0, true);
                const short8 zt = load8(pzt, ((uintptr_t)pzt & 15) == 0), fg = load8(pfg, ((uintptr_t)pfg & 15) == 0);
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    const uint32_t p = to_pack(zt[m], fg[m], fo[m]);
                    s_z[r * w + c0 + m] = (uint16_t)(p >> 16); s_f[r * w + c0 + m] = (uint8_t)(p & 3u);
                }
            } else {
                const int s = k - P8;
                if (s >= (int)S.nloose((unsigned)w)) continue;
                const int c = (int)S.cell((unsigned)s);
                const uint32_t p = to_pack(A.zt[x0 + c], A.fg[x0 + c], A.fo[x0 + c]);
                s_z[r * w + c] = (uint16_t)(p >> 16); s_f[r * w + c] = (uint8_t)(p & 3u);
            }
        }
    } else if (!ocean) {
        for (int k = tid; k < TO_BINS; k += TO_T) cnt[k] = 0;
    }
    __syncthreads();

    if (ocean) {        // :78-83: the lowest ocean fine cell
        int m = INT_MAX;
        for (int c = tid; c < ncell; c += TO_T) {
            const uint32_t p = cell(c);
            if (p & 1u) m = min(m, (int)(p >> 16));
        }
        if (m != INT_MAX) atomicMin(&s_min, m);
    } else if (!LONG) {
        for (int c = tid; c < ncell; c += TO_T) {
            const uint32_t p = cell(c);
            if (!(p & 1u)) s_key[atomicAdd(&s_n, 1)] = (p & 0xFFFF0000u) | (uint32_t)c;
        }
        __syncthreads();
        lds_sort_keys<TO_T>(s_key, s_n, tid);
    } else {
        for (int c = tid; c < ncell; c += TO_T) {
            const uint32_t p = cell(c);
            if (!(p & 1u)) atomicAdd(&cnt[p >> 16], 1u);
        }
        __syncthreads();
        // exclusive scan of the counts: 256 bins a thread
        uint32_t mine = 0;
        for (int k = 0; k < TO_BINS / TO_T; ++k) mine += cnt[tid * (TO_BINS / TO_T) + k];
        s_part[tid] = mine;
        __syncthreads();
        if (tid == 0) {
            uint32_t run = 0;
            for (int k = 0; k < TO_T; ++k) { const uint32_t v = s_part[k]; s_part[k] = run; run += v; }
            s_n = (int)run;
        }
        __syncthreads();
        uint32_t run = s_part[tid];
        for (int k = 0; k < TO_BINS / TO_T; ++k) {
            const uint32_t v = cnt[tid * (TO_BINS / TO_T) + k];
            cnt[tid * (TO_BINS / TO_T) + k] = run;
            run += v;
        }
        __syncthreads();
        for (int c0 = 0; c0 < ncell; c0 += TO_T) {
            const int c = c0 + tid;
            int d = -1;
            if (c < ncell) {
                const uint32_t p = cell(c);
                if (!(p & 1u)) d = (int)(p >> 16);
            }
            s_d[tid] = d;
            __syncthreads();
            int rank = 0, total = 0;
            if (d >= 0) {
                for (int u = 0; u < TO_T; ++u) {
                    const int same = s_d[u] == d;
                    total += same;
                    rank += same & (u < tid);
                }
                ord[cnt[d] + (uint32_t)rank] = (uint32_t)c;
            }
            __syncthreads();
            if (d >= 0 && rank == total - 1) cnt[d] += (uint32_t)total;
            __syncthreads();
        }
    }
    __syncthreads();
    if (tid >= 64) return;

    // ---- the four sums of :92-108 / :124-142, in traversal order ----
    double SAREA = 0, SAZSG = 0, SAREA_li = 0, SAZSG_li = 0;
    {
        auto fetch = [&](int b, uint32_t &p, double &a) {
            const int c = b + tid;
            p = c < ncell ? cell(c) : 1u;
            a = c < ncell ? A.dxypI[jrow0 + (size_t)(c / w)] : 0.;
        };
        uint32_t pn; double an;
        fetch(0, pn, an);
        for (int b0 = 0; b0 < ncell; b0 += 64) {
            const uint32_t pm = pn; const double am = an;
            fetch(b0 + 64, pn, an);
            const int cnt64 = min(64, ncell - b0);
            for (int t = 0; t < cnt64; ++t) {
                const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)pm, t);
                const double area = lane_bcast(am, t);
                const double z = (double)((int)(p >> 16) - 32768);
                if (ocean) SAREA += area;
                if (p & 1u) continue;
                if (!ocean) SAREA += area;
                SAZSG += area * z;
                if (p & 2u) { SAREA_li += area; SAZSG_li += area * z; }
            }
        }
    }
    double *P = A.planes;
    const long ld = A.ld;
    double ZATMO = 0, dZLAKE = 0, ZSOLDG = P[P_ZSOLDG * ld + xO], ZICETOP = 0, ZSGLO = 0, ZLAKE = 0, ZGRND = 0, ZSGHI = 0;
    if (ocean) {
        const int m = s_min;
        if (m == INT_MAX) {     // :85
            if (tid == 0) { atomicAdd(&A.status[S_OCEAN_FLAG], 1); atomicMin(&A.status[S_OCEAN_MIN], (int)xO); }
            ZSGLO = 999999;
        } else {
            ZSGLO = (double)(m - 32768);
        }
        ZICETOP = SAREA_li > 0 ? SAZSG_li / SAREA_li : 0;
    } else {
        const int n = s_n;
        if (n == 0) {           // :146
            if (tid == 0) { atomicAdd(&A.status[S_CONT_FLAG], 1); atomicMin(&A.status[S_CONT_MIN], (int)xO); }
            return;
        }
        ZSOLDG = SAZSG / SAREA;
        ZICETOP = SAREA_li > 0 ? SAZSG_li / SAREA_li : 0;
        const double FLAKE = P[P_FLAKE * ld + xO], FGRND = P[P_FGRND * ld + xO];
        const double thr1 = SAREA * FLAKE, thr2 = SAREA * (FLAKE + FGRND);
        // sorted cell k: its depth as an int and its row's area
        auto fetch = [&](int b, int &d, double &a) {
            const int k = b + tid;
            d = 0; a = 0.;
            if (k >= n) return;
            if (LONG) {
                const int c = (int)ord[k], r = c / w;
                d = A.zt[base + (size_t)r * A.imI + (size_t)(c - r * w)];
                a = A.dxypI[jrow0 + (size_t)r];
            } else {
                const uint32_t key = s_key[k];
                d = (int)(key >> 16) - 32768;
                a = A.dxypI[jrow0 + (size_t)((int)(key & 0xFFFFu) / w)];
            }
        };
        // :159-205 in one pass over the sorted cells.  lake: the NLAKE walk (:164-172) has not ended; grnd: nor has the NGRND walk
        double ANSUM = 0, VNSUM = 0, AZATMO = 0, G = 0, dlake = 0, dgrnd = 0, dlast = 0;
        bool lake = true, grnd = true;
        int dn; double an;
        fetch(0, dn, an);
        for (int b0 = 0; b0 < n; b0 += 64) {
            const int dm = dn; const double am = an;
            fetch(b0 + 64, dn, an);
            const int cnt64 = min(64, n - b0);
            for (int t = 0; t < cnt64; ++t) {
                const double depth = (double)__builtin_amdgcn_readlane(dm, t);
                const double area = lane_bcast(am, t);
                const int k = b0 + t;
                if (k == 0) ZSGLO = depth;
                dlast = depth;
                if (lake) {
                    ANSUM += area;
                    VNSUM += area * depth;
                    if (ANSUM > thr1 || k == n - 1) {       // :171, or the --NLAKE end of :165-168
                        lake = false;
                        dlake = depth;
                        AZATMO = ANSUM * depth;             // :185
                        G = ANSUM - area;                   // :192
                        G += area;                          // :200 for NGRND = NLAKE
                        if (G > thr2) { grnd = false; dgrnd = depth; }
                    }
                } else {
                    AZATMO += area * depth;                 // :186-188
                    if (grnd) {
                        G += area;
                        if (G > thr2) { grnd = false; dgrnd = depth; }
                    }
                }
            }
        }
        if (grnd) dgrnd = dlast;        // :196-199
        ZLAKE = dlake;
        if (FLAKE > 0) {
            const double ZLBOT = (VNSUM - (ANSUM - thr1) * dlake) / thr1;
            const double thick = dlake - ZLBOT;
            dZLAKE = thick < 1.0 ? 1.0 : thick;       // std::max(thick, 1.0)
        }
        ZATMO = AZATMO / SAREA;
        ZGRND = dgrnd;
        ZSGHI = dlast;
    }
    // :211-218: a pole row's tile is the whole row's, except for ZATMOF
    const int nrep = A.imax == 1 ? A.imO : 1;
    for (int i = tid; i < nrep; i += 64) {
        const long x = xO + i;
        P[P_ZATMO * ld + x] = ZATMO; P[P_DZLAKE * ld + x] = dZLAKE; P[P_ZSOLDG * ld + x] = ZSOLDG; P[P_ZICETOP * ld + x] = ZICETOP;
        P[P_ZSGLO * ld + x] = ZSGLO; P[P_ZLAKE * ld + x] = ZLAKE; P[P_ZGRND * ld + x] = ZGRND; P[P_ZSGHI * ld + x] = ZSGHI;
    }
    if (tid == 0) P[P_ZATMOF * ld + xO] = SAZSG / SAREA;
}

// ---- :747-758: in the list's order, by one thread (a cell may be listed twice) -----------------------------------------------
__global__ void k_to_resets(double *__restrict__ planes, long ld, const int32_t *__restrict__ rx, const double *__restrict__ relev, int n) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int k = 0; k < n; ++k) {
        const long x = rx[k];
        const double elev = relev[k];
        planes[P_DZLAKE * ld + x] += (elev - planes[P_ZLAKE * ld + x]);
        planes[P_ZATMO * ld + x] = elev;
        planes[P_ZLAKE * ld + x] = elev;
    }
}

// ---- :761-795: a thread per 2 x 2 block ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TO_T) void k_to_blocks(double *__restrict__ planes, long ld, int IM, int JM, int *__restrict__ status) {
    const int IMB = IM / 2, JMB = JM / 2;
    const long b = (long)blockIdx.x * TO_T + threadIdx.x;
    if (b >= (long)IMB * JMB) return;
    const int jb = (int)(b / IMB), ib = (int)(b - (long)jb * IMB);
    double foceanb = 0;
    int ones = 0;
    for (int j = jb * 2; j < jb * 2 + 2; ++j)
        for (int i = ib * 2; i < ib * 2 + 2; ++i) {
            foceanb += planes[P_FOCEAN * ld + (long)j * IM + i];
            ones += planes[P_FLAKE * ld + (long)j * IM + i] == 1 ? 1 : 0;
        }
    if (ones) atomicAdd(&status[S_FLAKE_ONE], ones);
    if (!(foceanb > 0)) return;
    for (int j = jb * 2; j < jb * 2 + 2; ++j)
        for (int i = ib * 2; i < ib * 2 + 2; ++i) {
            const long x = (long)j * IM + i;
            const double flake = planes[P_FLAKE * ld + x];
            if (flake > 0) {
                planes[P_FGRND * ld + x] += flake;
                planes[P_FLAKE * ld + x] = 0;
                planes[P_DZLAKE * ld + x] = 0;
            }
        }
}

__global__ __launch_bounds__(TO_T) void k_to_pow03(const double *__restrict__ x, long n, double *__restrict__ out) {
    const long g = (long)blockIdx.x * TO_T + threadIdx.x;
    if (g < n) out[g] = pow(x[g], .3);
}

// NULL planes, alignment, ld, the outputs over an input: all before a device is touched
void check_planes(const ibh_make_topoo *h, const void *fgice, const void *zicetop, const void *zsolg, const void *focean, const void *flakes,
                  const void *planes, int64_t ld) {
    IBH_CHECK(h, "make_topoo: null handle");
    IBH_CHECK(ld >= h->nO(), "make_topoo: ld=%lld < %lld cells of hspecO", (long long)ld, (long long)h->nO());
    const size_t pb = sizeof(int16_t) * (size_t)h->nI();
    const PlaneArg a[] = {{fgice, pb, "FGICE1m", 2, false, false}, {zicetop, pb, "ZICETOP1m", 2, false, false}, {zsolg, pb, "ZSOLG1m", 2, false, false},
                          {focean, pb, "FOCEAN1m", 2, false, false}, {flakes, sizeof(double) * (size_t)h->nS(), "FLAKES", 8, false, false},
                          {planes, sizeof(double) * ((size_t)(P_N - 1) * (size_t)ld + (size_t)h->nO()), "the output planes", 8, true, false}};
    check_plane_args("make_topoo", a, (int)(sizeof(a) / sizeof(a[0])), "%s: %s overlap %s");
}

size_t tiles_lds(int ncell) {
    return sizeof(uint32_t) * (size_t)pow2_ceil(ncell) + sizeof(uint16_t) * (size_t)ncell + (size_t)ncell + 16;
}

// the enqueue proper; every pointer is a device pointer
void run_device(ibh_make_topoo *h, const int16_t *fg, const int16_t *zt, const int16_t *zs, const int16_t *fo, const double *flakes, double *planes,
                int64_t ld, hipStream_t st) {
    const int64_t nO = h->nO(), nI = h->nI();
    double *zictop = h->work.p, *zsolg = zictop + nO, *powp = zsolg + nO, *rowsum = powp + nO;
    IBH_HIP(hipMemsetAsync(h->status.p, 0, sizeof(int32_t) * S_N, st));
    IBH_HIP(hipMemsetD32Async((hipDeviceptr_t)(h->status.p + S_OCEAN_MIN), INT_MAX, 1, st));
    IBH_HIP(hipMemsetD32Async((hipDeviceptr_t)(h->status.p + S_CONT_MIN), INT_MAX, 1, st));
    IBH_HIP(hipMemset2DAsync(planes, sizeof(double) * (size_t)ld, 0, sizeof(double) * (size_t)nO, P_N, st));
    auto regrid = [&](ibh_hntr *hn, const void *wta, const void *a, int a_type, int64_t nA, double *out) {
        rethrow(ibh_hntr_regrid_typed_device(hn, wta, IBH_HNTR_I16, 0, 1.0, a, a_type, 1, nA, out, nO, 1, 1., 0., st));
    };
    regrid(h->hntrI, nullptr, fo, IBH_HNTR_I16, nI, planes + P_FOCEANF * ld);   // :392
    regrid(h->hntrI, nullptr, fg, IBH_HNTR_I16, nI, planes + P_FGICEF * ld);    // :399
    regrid(h->hntrS, nullptr, flakes, IBH_HNTR_F64, h->nS(), planes + P_FLAKE * ld);    // :575
    regrid(h->hntrI, fo, zs, IBH_HNTR_I16, nI, planes + P_DZOCEN * ld);         // :646
    regrid(h->hntrI, fg, zt, IBH_HNTR_I16, nI, zictop);                         // :661
    regrid(h->hntrI, fg, zs, IBH_HNTR_I16, nI, zsolg);                          // :663
    hipLaunchKernelGGL(k_to_cells, dim3((unsigned)cdiv(nO, TO_T)), dim3(TO_T), 0, st, planes, (long)ld, zictop, zsolg, powp, h->set_to.p, h->imO,
                       h->jmO, h->status.p);
    hipLaunchKernelGGL(k_to_gice, dim3(1), dim3(TO_T), 0, st, planes, (long)ld, zictop, zsolg, powp, h->dxypO.p, rowsum, h->imO, h->jmO);
    ToTiles A{fg, zt, fo, h->dxypI.p, planes, (long)ld, h->status.p, h->scratch.p, h->imI, h->imO, h->mult_j, 0, 0, 0, 0};
    // the interior rows, then the two pole rows; the long path's scratch holds the interior tiles first
    const unsigned nint = (unsigned)(h->jmO - 2) * (unsigned)h->imO;
    if (nint) {
        A.w = h->mult_i; A.imax = h->imO; A.jO0 = 1; A.jstep = 1;
        if (h->long_interior) hipLaunchKernelGGL(k_to_tiles<true>, dim3(nint), dim3(TO_T), 0, st, A);
        else hipLaunchKernelGGL(k_to_tiles<false>, dim3(nint), dim3(TO_T), tiles_lds(A.w * h->mult_j), st, A);
    }
    A.w = h->imI; A.imax = 1; A.jO0 = 0; A.jstep = h->jmO - 1;
    if (h->long_poles) {
        if (h->long_interior) A.scratch += (size_t)nint * ((size_t)TO_BINS + (size_t)h->mult_i * h->mult_j);
        hipLaunchKernelGGL(k_to_tiles<true>, dim3(2), dim3(TO_T), 0, st, A);
    } else {
        hipLaunchKernelGGL(k_to_tiles<false>, dim3(2), dim3(TO_T), tiles_lds(A.w * h->mult_j), st, A);
    }
    if (h->nreset) hipLaunchKernelGGL(k_to_resets, dim3(1), dim3(64), 0, st, planes, (long)ld, h->reset_x.p, h->reset_elev.p, h->nreset);
    hipLaunchKernelGGL(k_to_blocks, dim3((unsigned)cdiv(nO / 4, TO_T)), dim3(TO_T), 0, st, planes, (long)ld, h->imO, h->jmO, h->status.p);
    IBH_HIP(hipGetLastError());
}

void read_status(const ibh_make_topoo *h, int64_t *out, hipStream_t st) {
    int32_t s[S_N];
    IBH_HIP(hipMemcpyAsync(s, h->status.p, sizeof(s), hipMemcpyDeviceToHost, st));
    IBH_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < S_N; ++k) out[k] = s[k];
    if (!s[S_OCEAN_FLAG]) out[S_OCEAN_MIN] = -1;
    if (!s[S_CONT_FLAG]) out[S_CONT_MIN] = -1;
}

}  // namespace
}  // namespace ibh

using namespace ibh;
extern "C" {

int ibh_make_topoo_create(ibh_make_topoo **out, int32_t imI, int32_t jmI, double offiI, double dlatI, int32_t imO, int32_t jmO, double offiO,
                          double dlatO, int32_t imS, int32_t jmS, double offiS, double dlatS, int32_t nland, const int32_t *land_ij, int32_t nocean,
                          const int32_t *ocean_ij, int32_t nreset, const int32_t *reset_ij, const double *reset_elev) {
    if (out) *out = nullptr;
    return guarded([&] {
        IBH_CHECK(out, "out: null argument");
        IBH_CHECK(imI > 0 && jmI > 0 && imO > 0 && jmO > 0 && imS > 0 && jmS > 0,
                  "hspecI / hspecO / hspecS: grid sizes (%dx%d), (%dx%d), (%dx%d) must be positive", imI, jmI, imO, jmO, imS, jmS);
        IBH_CHECK(imI % imO == 0 && jmI % jmO == 0, "hspecI: the fine grid (%dx%d) must be an even multiple of the ocean grid (%dx%d)", imI, jmI,
                  imO, jmO);
        IBH_CHECK(imO % 2 == 0 && jmO % 2 == 0, "hspecO: (%dx%d); the 2 x 2 block pass needs even sizes", imO, jmO);
        IBH_CHECK((int64_t)imI * jmI < (1ll << 31), "hspecI: %lld cells overflow int32", (long long)imI * jmI);
        IBH_CHECK(nland >= 0 && nocean >= 0 && nreset >= 0, "cell lists: negative length (%d, %d, %d)", nland, nocean, nreset);
        IBH_CHECK((nland == 0 || land_ij) && (nocean == 0 || ocean_ij) && (nreset == 0 || (reset_ij && reset_elev)), "cell lists: null list with a length");
        auto check_ij = [&](const int32_t *ij, int n, const char *what) {
            for (int k = 0; k < n; ++k)
                IBH_CHECK(ij[2 * k] >= 1 && ij[2 * k] <= imO && ij[2 * k + 1] >= 1 && ij[2 * k + 1] <= jmO,
                          "%s: entry %d is (%d, %d), outside the ocean grid (%dx%d)", what, k, ij[2 * k], ij[2 * k + 1], imO, jmO);
        };
        check_ij(land_ij, nland, "set_to_land");
        check_ij(ocean_ij, nocean, "set_to_ocean");
        check_ij(reset_ij, nreset, "resets");
        std::unique_ptr<ibh_make_topoo> h(new ibh_make_topoo);
        h->imI = imI; h->jmI = jmI; h->imO = imO; h->jmO = jmO; h->imS = imS; h->jmS = jmS; h->mult_i = imI / imO; h->mult_j = jmI / jmO;
        const size_t nO = (size_t)h->nO();
        std::vector<int8_t> set_to(nO, 0);
        for (int k = 0; k < nland; ++k) set_to[(size_t)(land_ij[2 * k + 1] - 1) * imO + (land_ij[2 * k] - 1)] = 2;      // :416-446
        for (int k = 0; k < nocean; ++k) set_to[(size_t)(ocean_ij[2 * k + 1] - 1) * imO + (ocean_ij[2 * k] - 1)] = 1;   // :449-494, after
        std::vector<int32_t> rx((size_t)nreset);
        for (int k = 0; k < nreset; ++k) rx[(size_t)k] = (reset_ij[2 * k + 1] - 1) * imO + (reset_ij[2 * k] - 1);
        const std::vector<double> dI = dxyp_rows(imI, jmI), dO = dxyp_rows(imO, jmO);
        // the regridders check their grids on the host before they look for a device
        rethrow(ibh_hntr_create(&h->hntrI, imI, jmI, offiI, dlatI, imO, jmO, offiO, dlatO, 0.));
        rethrow(ibh_hntr_create(&h->hntrS, imS, jmS, offiS, dlatS, imO, jmO, offiO, dlatO, 0.));
        require_device();
        IBH_HIP(hipGetDevice(&h->device));
        hipStream_t st = hipStreamPerThread;
        h->dxypI.upload(dI.data(), dI.size(), st);
        h->dxypO.upload(dO.data(), dO.size(), st);
        h->set_to.upload(set_to.data(), nO, st);
        h->nreset = nreset;
        h->reset_x.upload(rx.data(), rx.size(), st);
        h->reset_elev.upload(reset_elev, (size_t)nreset, st);
        h->work.alloc(3 * nO + 2 * (size_t)jmO);
        h->status.alloc(S_N);
        const size_t tile = (size_t)h->mult_i * h->mult_j, pole = (size_t)imI * h->mult_j;
        h->long_interior = tile > IBH_MAKE_TOPOO_MAX_TILE;
        h->long_poles = pole > IBH_MAKE_TOPOO_MAX_TILE;
        size_t words = 0;
        if (h->long_interior) words += (size_t)(jmO - 2) * imO * (TO_BINS + tile);
        if (h->long_poles) words += 2 * (TO_BINS + pole);
        if (words) h->scratch.alloc(words);
        IBH_HIP(hipStreamSynchronize(st));
        *out = h.release();
    });
}

int ibh_make_topoo_destroy(ibh_make_topoo *h) {
    return guarded([&] { delete h; });
}

int ibh_make_topoo_device(ibh_make_topoo *h, const int16_t *d_FGICE1m, const int16_t *d_ZICETOP1m, const int16_t *d_ZSOLG1m,
                          const int16_t *d_FOCEAN1m, const double *d_FLAKES, double *d_planes, int64_t ld, void *stream) {
    return guarded([&] {
        check_planes(h, d_FGICE1m, d_ZICETOP1m, d_ZSOLG1m, d_FOCEAN1m, d_FLAKES, d_planes, ld);
        check_current_device(h->device, "make_topoo handle");
        run_device(h, d_FGICE1m, d_ZICETOP1m, d_ZSOLG1m, d_FOCEAN1m, d_FLAKES, d_planes, ld, (hipStream_t)stream);
    });
}

int ibh_make_topoo_status(const ibh_make_topoo *h, void *stream, int64_t *status) {
    return guarded([&] {
        IBH_CHECK(h && status, "make_topoo_status: null argument");
        check_current_device(h->device, "make_topoo handle");
        read_status(h, status, (hipStream_t)stream);
    });
}

int ibh_make_topoo_host(ibh_make_topoo *h, const int16_t *FGICE1m, const int16_t *ZICETOP1m, const int16_t *ZSOLG1m, const int16_t *FOCEAN1m,
                        const double *FLAKES, double *planes, int64_t ld, int64_t *status) {
    return guarded([&] {
        check_planes(h, FGICE1m, ZICETOP1m, ZSOLG1m, FOCEAN1m, FLAKES, planes, ld);
        check_current_device(h->device, "make_topoo handle");
        hipStream_t st = hipStreamPerThread;
        const size_t nI = (size_t)h->nI(), nO = (size_t)h->nO();
        DevBuf<int16_t> in[4];
        const int16_t *src[4] = {FGICE1m, ZICETOP1m, ZSOLG1m, FOCEAN1m};
        for (int k = 0; k < 4; ++k) in[k].upload(src[k], nI, st);
        DevBuf<double> fl, o;
        fl.upload(FLAKES, (size_t)h->nS(), st);
        o.alloc((size_t)P_N * nO);
        run_device(h, in[0].p, in[1].p, in[2].p, in[3].p, fl.p, o.p, (int64_t)nO, st);
        IBH_HIP(hipMemcpy2DAsync(planes, sizeof(double) * (size_t)ld, o.p, sizeof(double) * nO, sizeof(double) * nO, P_N, hipMemcpyDeviceToHost, st));
        int64_t s[S_N];
        read_status(h, s, st);      // (waits for the stream)
        if (status) std::copy(s, s + S_N, status);
    });
}

int ibh_selftest_pow03(const double *d_x, int64_t n, double *d_out, void *stream) {
    return guarded([&] {
        IBH_CHECK(d_x && d_out && n >= 0, "selftest_pow03: null argument");
        if (n) hipLaunchKernelGGL(k_to_pow03, dim3((unsigned)cdiv(n, TO_T)), dim3(TO_T), 0, (hipStream_t)stream, d_x, (long)n, d_out);
        IBH_HIP(hipGetLastError());
    });
}

}  // extern "C"
