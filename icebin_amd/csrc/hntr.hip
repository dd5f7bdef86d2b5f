// hntr.hip -- Hntr, the conservative lat-lon -> lat-lon regridder (GISS HNTR4), on the GPU.
//
// Replaces icebin::modele::Hntr (slib/icebin/modele/hntr.{hpp,cpp}): the constructor's partition
// (hntr.cpp:63-168) runs on the host with libm sin, exactly as the reference writes it, and is uploaded
// once; Hntr::regrid (hntr.hpp:204-244 RegridAccum, :341-435) is one launch for nvar fields plus, with
// mean_polar, a small sequential kernel for the two polar rows.
//
// Results are bitwise the reference's: every B cell's WEIGHT and VALUE chains are summed by ONE lane in
// the reference's loop order (JA outer, IAREV inner), with the reference's expressions and roundings
// (the build passes -ffp-contract=off; no fma anywhere on the chains), the host's SINA values and no
// atomics.  So the output does not depend on nvar, on the field grouping or on the launch shape.
//
// Kernel shape.  A workgroup is one wave; it owns the B cells of ONE B column IB and L consecutive B rows
// (lane t < L runs the chains of row jb0 + t).  All its cells share the A columns [IMIN(IB), IMAX(IB)]
// (wrapping past the date line), and lane t walks its own A rows JMIN..JMAX.  Step (r, c) stages, for
// every lane t, the K columns of chunk c of A row JMIN(jb0+t) + r -- of WTA and of each field of the
// group -- into LDS with coalesced loads (consecutive lanes load consecutive columns), then every lane
// runs K terms of its chains out of LDS.  LDS rows are padded to an odd number of doubles so that the
// lanes' ds_read_b64 fall on distinct banks.  The host picks L (fewer lanes per wave, more workgroups when
// the B grid has few cells) and K (the widest chunk that 20 KiB of LDS per workgroup holds, or 40 KiB when 20 would
// leave fewer than 16 columns); the LDS a workgroup asks for is what its tile needs, so small tiles leave room for more
// workgroups per CU.  A lane holds at most HNTR_STAGE staged doubles, which keeps the kernel within 141 VGPRs (no
// spills to AGPRs or scratch).
//
// Typed planes and a constant weight (the reference's template regrid<WeightT, SrcT, DestT>, hntr.hpp:385-391, as its TOPO
// tools instantiate it: int16 planes, const_array(shape, c) as the weight).  The kernel is a template over the weight form
// (double, float, int16_t planes or HntrConstW) and the source element type (double, float, int16_t); B stays double.  An
// element is converted to double, exactly, as it is loaded, and staged into LDS as a double: the LDS layout, the odd row
// stride S = K | 1 in doubles and the chains are those of the double kernel, so the bits are those of the double kernel on
// the widened planes.  K depends on the number of staged planes P alone, not on the element size: P = 1 + NV with a weight
// plane, P = NV under a constant weight, where no weight plane is loaded or staged and wta = wtm*c + wtb is computed per term
// in the same place (the bits of a plane filled with c); there the larger LDS budget is 32 KiB, not 40 (hntr_shape).  Loads are one element per lane (2, 4 or 8 bytes), consecutive lanes
// on consecutive columns: no load is wider than an element, so a plane base aligned to its element only (an odd lda of int16
// planes, a pointer at an odd element offset), a window that starts at any column or wraps the date line, and an odd imA need
// no special case, and no load touches an element outside [0, imA*jmA) of its plane.
#include <algorithm>
#include <cmath>
#include <memory>

#include "common.h"
#include "csrbuild.h"
#include "csrops.h"
#include "prims.h"
#include "sparseset.h"

namespace ibh {

constexpr int HNTR_LDS = 5056;      // most doubles of LDS per workgroup: with the row windows, 40 KiB (four workgroups per CU)
constexpr int HNTR_LDS_SMALL = 2496;    // the same for 20 KiB (eight workgroups per CU)
constexpr int HNTR_LDS_CONST = 4032;    // under a constant weight, in place of HNTR_LDS: 32 KiB (five workgroups per CU)
constexpr int HNTR_STAGE = 32;      // doubles a lane holds between its global loads and its LDS writes

// ---- partition (hntr.cpp:63-168), host side ----------------------------------------------------
struct HntrPartition {
    std::vector<double> SINA, SINB, FMIN, FMAX, GMIN, GMAX;     // SINA[0..jmA], SINB[0..jmB]; the rest 0-based by IB-1 / JB-1
    std::vector<int32_t> IMIN, IMAX, JMIN, JMAX;
};

static void check_spec(const char *g, int im, int jm, double offi, double dlat) {
    IBH_CHECK(im >= 1 && jm >= 1, "Hntr: grid %s has im=%d jm=%d (both must be >= 1)", g, im, jm);
    IBH_CHECK((int64_t)im * jm < (1ll << 31), "Hntr: grid %s has %lld cells (at most 2^31-1)", g, (long long)im * jm);
    IBH_CHECK(std::isfinite(dlat) && dlat > 0, "Hntr: grid %s has dlat=%g (must be > 0)", g, dlat);
    IBH_CHECK(std::isfinite(offi), "Hntr: grid %s has offi=%g (must be finite)", g, offi);
}

// IAREV runs past 2*imA in the reference when grid B starts east of grid A (offiB = 0.5 on a coarse B puts IMIN(1) past imA);
// its IA = 1 + (IAREV-1) % imA wraps that.  The device windows are moved back by whole turns so that IMIN(1) lies in
// [1, imA]: IA and every F (IAREV == IMIN / IMAX) stay the same, and IAREV <= 2*imA, so IA = IAREV - imA past imA.
static int hntr_column_shift(HntrPartition const &p, int imA) { return (p.IMIN[0] - 1) / imA * imA; }

static void hntr_partition(int imA, int jmA, double offiA, double dlatA, int imB, int jmB, double offiB, double dlatB,
                           HntrPartition &p) {
    check_spec("A", imA, jmA, offiA, dlatA);
    check_spec("B", imB, jmB, offiB, dlatB);
    p.SINA.assign((size_t)jmA + 1, 0.); p.SINB.assign((size_t)jmB + 1, 0.);
    p.FMIN.assign((size_t)imB, 0.); p.FMAX.assign((size_t)imB, 0.); p.IMIN.assign((size_t)imB, 0); p.IMAX.assign((size_t)imB, 0);
    p.GMIN.assign((size_t)jmB, 0.); p.GMAX.assign((size_t)jmB, 0.); p.JMIN.assign((size_t)jmB, 0); p.JMAX.assign((size_t)jmB, 0);

    // partition_east_west (hntr.cpp:84-117).  The walk is bounded: with absurd offsets the reference's loop runs for
    // as long as RIA < RIB.
    const double DIA = imB;
    int64_t IA = 1;
    double RIA = (IA + offiA - imA) * imB;
    int IB = imB;
    for (int IBp1 = 1; IBp1 <= imB; ++IBp1) {
        const double RIB = (IBp1 - 1 + offiB) * imA;
        while (RIA < RIB) {
            IA += 1;
            RIA += DIA;
            IBH_CHECK(IA <= 4 * (int64_t)imA, "Hntr: east-west partition runs past IA=4*imA (offiA=%g, offiB=%g)", offiA, offiB);
        }
        if (RIA == RIB) {
            p.IMAX[IB - 1] = (int32_t)IA; p.FMAX[IB - 1] = 0;
            IA += 1;
            RIA += DIA;
            p.IMIN[IBp1 - 1] = (int32_t)IA; p.FMIN[IBp1 - 1] = 0;
        } else {
            p.IMAX[IB - 1] = (int32_t)IA; p.FMAX[IB - 1] = (RIA - RIB) / DIA;
            p.IMIN[IBp1 - 1] = (int32_t)IA; p.FMIN[IBp1 - 1] = 1 - p.FMAX[IB - 1];
        }
        IB = IBp1;
    }
    p.IMAX[imB - 1] += imA;

    // partition_north_south (hntr.cpp:120-168)
    const double MIN_TO_RAD = (2. * M_PI) / (360 * 60);
    const double FJEQA = .5 * (1 + jmA);
    for (int JA = 1; JA <= jmA - 1; ++JA) {
        const double RJA = (JA + .5 - FJEQA) * dlatA;
        p.SINA[JA] = sin(RJA * MIN_TO_RAD);
    }
    p.SINA[0] = -1;
    p.SINA[jmA] = 1;
    const double FJEQB = .5 * (1 + jmB);
    for (int JB = 1; JB <= jmB - 1; ++JB) {
        const double RJB = (JB + .5 - FJEQB) * dlatB;
        p.SINB[JB] = sin(RJB * MIN_TO_RAD);
    }
    p.SINB[0] = -1;
    p.SINB[jmB] = 1;
    p.JMIN[0] = 1;
    p.GMIN[0] = 0;
    int JA = 1;
    for (int JB = 1; JB <= jmB - 1; ++JB) {
        // SINA(jmA) = 1 stops this walk; the coincident branch below can step past jmA, which the reference then reads
        while (p.SINA[JA] < p.SINB[JB]) ++JA;
        if (p.SINA[JA] == p.SINB[JB]) {
            p.JMAX[JB - 1] = JA; p.GMAX[JB - 1] = 0;
            JA += 1;
            IBH_CHECK(JA <= jmA, "Hntr: north-south partition leaves [1, jmA] at JB=%d", JB);
            p.JMIN[JB] = JA; p.GMIN[JB] = 0;
        } else {
            p.JMAX[JB - 1] = JA; p.GMAX[JB - 1] = p.SINA[JA] - p.SINB[JB];
            p.JMIN[JB] = JA; p.GMIN[JB] = p.SINB[JB] - p.SINA[JA - 1];
        }
    }
    p.JMAX[jmB - 1] = jmA;
    p.GMAX[jmB - 1] = 0;

    // Every index the regrid reads must lie in range: windows non-empty and in [1, 2*imA] x [1, jmA] once the column
    // windows are shifted by whole turns (hntr_column_shift), and both window ends non-decreasing.
    const int shift = hntr_column_shift(p, imA);
    for (int i = 0; i < imB; ++i) {
        IBH_CHECK(p.IMIN[i] - shift >= 1 && p.IMIN[i] <= p.IMAX[i] && p.IMAX[i] - shift <= 2 * imA,
                  "Hntr: column window %d..%d of IB=%d is outside [1, 2*imA=%d]", p.IMIN[i] - shift, p.IMAX[i] - shift, i + 1, 2 * imA);
        IBH_CHECK(p.IMAX[i] - p.IMIN[i] < 2 * imA, "Hntr: column window of IB=%d is wider than 2*imA", i + 1);
        IBH_CHECK(i == 0 || (p.IMIN[i] >= p.IMIN[i - 1] && p.IMAX[i] >= p.IMAX[i - 1]), "Hntr: column windows not ordered at IB=%d", i + 1);
    }
    for (int j = 0; j < jmB; ++j) {
        IBH_CHECK(p.JMIN[j] >= 1 && p.JMIN[j] <= p.JMAX[j] && p.JMAX[j] <= jmA,
                  "Hntr: row window %d..%d of JB=%d is outside [1, jmA=%d]", p.JMIN[j], p.JMAX[j], j + 1, jmA);
        IBH_CHECK(j == 0 || (p.JMIN[j] >= p.JMIN[j - 1] && p.JMAX[j] >= p.JMAX[j - 1]), "Hntr: row windows not ordered at JB=%d", j + 1);
    }
}

// ---- kernels -----------------------------------------------------------------------------------
struct HntrArgs {
    const double *SINA, *FMIN, *FMAX, *GMIN, *GMAX;
    const int32_t *IMIN, *IMAX, *JMIN, *JMAX;
    const void *WTA;        // planes of the kernel's weight type; unused under a constant weight
    int64_t wta_ld;         // 0: one WTA plane shared by all fields; in elements of the weight type
    double wconst;          // the constant weight (HntrConstW)
    const void *A;          // planes of the kernel's source type
    int64_t lda;            // in elements of the source type
    double *B;
    int64_t ldb;
    int imA, imB, jmB, nvar;
    int L, K, S;            // chain lanes per wave, columns per chunk, LDS row stride (odd, >= K)
    double wtm, wtb, datmis;
};

struct HntrConstW {};       // the weight type of a constant weight: no plane is loaded or staged

// One wave per workgroup: column IB = blockIdx.x % imB, rows jb0 .. jb0+L-1, fields NV*blockIdx.y .. (at most NV).
// A shared weight feeds the NV VALUE chains from one wt / WEIGHT chain; per-field weights run with NV = 1.
// WT: double, float, int16_t or HntrConstW; ST: double, float or int16_t.  An element becomes a double as it is loaded.
template <int NV, class WT, class ST>
__global__ __launch_bounds__(64) void hntr_regrid_kernel(HntrArgs a) {
    constexpr bool CW = std::is_same<WT, HntrConstW>::value;
    constexpr int PW = CW ? 0 : 1;                  // staged weight planes
    constexpr int P = PW + NV;                      // staged planes: WTA (if any), then the fields
    constexpr int U = HNTR_STAGE / (1 + NV) > 1 ? HNTR_STAGE / (1 + NV) : 1;   // staged items per lane in flight (a constant weight: as with a plane)
    using WE = typename std::conditional<CW, double, WT>::type;
    extern __shared__ double lds[];                 // [P][L][S], L*S*P <= HNTR_LDS
    __shared__ int sj0[64], sj1[64];

    const int lane = threadIdx.x;
    const int ib = blockIdx.x % a.imB;
    const int jb0 = (blockIdx.x / a.imB) * a.L;
    const int f0 = blockIdx.y * NV;
    const int nv = min(NV, a.nvar - f0);
    const WE *__restrict__ W = static_cast<const WE *>(a.WTA) + (a.wta_ld ? (int64_t)f0 * a.wta_ld : 0);
    const ST *__restrict__ Af = static_cast<const ST *>(a.A) + (int64_t)f0 * a.lda;
    const int L = a.L, S = a.S, K = a.K, imA = a.imA;
    const int64_t plane = (int64_t)L * S;

    const bool mine = lane < L && jb0 + lane < a.jmB;
    const int jb = jb0 + lane;
    int jmn = 1, jmx = 0;
    double gmn = 0, gmx = 0;
    if (mine) { jmn = a.JMIN[jb]; jmx = a.JMAX[jb]; gmn = a.GMIN[jb]; gmx = a.GMAX[jb]; }
    sj0[lane] = jmn;
    sj1[lane] = jmx;
    int nrows = jmx - jmn + 1;
    for (int o = 32; o > 0; o >>= 1) nrows = max(nrows, __shfl_xor(nrows, o));   // steps of the tile: its longest window

    const int imn = a.IMIN[ib], imx = a.IMAX[ib];
    const double fmn = a.FMIN[ib], fmx = a.FMAX[ib];

    double WEIGHT = 0, VALUE[NV];
#pragma unroll
    for (int f = 0; f < NV; ++f) VALUE[f] = 0;

    for (int r = 0; r < nrows; ++r) {
        const int JA = jmn + r;
        const bool act = mine && JA <= jmx;
        double G = 0;
        if (act) {
            G = a.SINA[JA] - a.SINA[JA - 1];
            if (JA == jmn) G -= gmn;
            if (JA == jmx) G -= gmx;
        }
        for (int c0 = imn; c0 <= imx; c0 += K) {
            const int kw = min(K, imx - c0 + 1);
            const int nitem = L * kw;
            const int dq = 64 / kw, dr = 64 % kw;
            __syncthreads();                        // the previous step's reads of LDS are done
            int t = lane / kw, k = lane % kw;       // item lane + 64*i -> (row t, column k)
            for (int i0 = lane; i0 < nitem; i0 += 64 * U) {
                int off[U];                         // element in the plane: < imA*jmA < 2^31
                int dst[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    off[u] = -1;
                    dst[u] = t * S + k;
                    if (i0 + 64 * u < nitem) {      // then t < L: rows whose window has ended are skipped
                        const int ja = sj0[t] + r;
                        if (ja <= sj1[t]) {
                            const int iarev = c0 + k;
                            const int ia = iarev > imA ? iarev - imA : iarev;
                            off[u] = (ja - 1) * imA + (ia - 1);
                        }
                    }
                    t += dq; k += dr;
                    if (k >= kw) { k -= kw; ++t; }
                }
                double v[U][P];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (off[u] >= 0) {
                        if (!CW) v[u][0] = (double)W[off[u]];
#pragma unroll
                        for (int f = 0; f < NV; ++f)
                            if (f < nv) v[u][PW + f] = (double)Af[(int64_t)f * a.lda + off[u]];
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (off[u] >= 0) {
#pragma unroll
                        for (int p = 0; p < P; ++p)
                            if (p < PW + nv) lds[p * plane + dst[u]] = v[u][p];
                    }
                }
            }
            __syncthreads();
            if (act) {
                const double *__restrict__ row = lds + lane * S;
#pragma unroll 4
                for (int kk = 0; kk < kw; ++kk) {
                    const int IAREV = c0 + kk;
                    double F = 1;
                    if (IAREV == imn) F -= fmn;
                    if (IAREV == imx) F -= fmx;
                    const double FG = F * G;
                    const double wta = a.wtm * (CW ? a.wconst : row[kk]) + a.wtb;
                    const double wt = FG * wta;
                    WEIGHT += wt;
#pragma unroll
                    for (int f = 0; f < NV; ++f)
                        if (f < nv) VALUE[f] += wt * row[(PW + f) * plane + kk];
                }
            }
        }
    }
    if (mine) {
        const int64_t ijb = (int64_t)jb * a.imB + ib;
#pragma unroll
        for (int f = 0; f < NV; ++f)
            if (f < nv) a.B[(int64_t)(f0 + f) * a.ldb + ijb] = WEIGHT == 0 ? a.datmis : VALUE[f] / WEIGHT;
    }
}

// mean_polar (hntr.hpp:404-423): one thread per (field, polar row), sequential in IB.  A NaN DATMIS never
// compares equal, so such rows average their NaNs in, as the reference does.
__global__ void hntr_mean_polar_kernel(double *B, int64_t ldb, int nvar, int imB, int jmB, double datmis) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 2 * nvar) return;
    double *row = B + (int64_t)(idx >> 1) * ldb + (int64_t)((idx & 1) ? jmB - 1 : 0) * imB;
    double BMEAN = datmis, WEIGHT = 0, VALUE = 0;
    for (int IB = 0;; ++IB) {
        if (IB >= imB) {
            if (WEIGHT != 0) BMEAN = VALUE / WEIGHT;
            break;
        }
        if (row[IB] == datmis) break;
        WEIGHT += 1;
        VALUE += row[IB];
    }
    for (int IB = 0; IB < imB; ++IB) row[IB] = BMEAN;
}

}  // namespace ibh

using namespace ibh;

struct ibh_hntr {
    int imA, jmA, imB, jmB;
    double offiA, dlatA, offiB, dlatB;      // the grid specs, for make_grid_spec (ibh_regridder_create_hntr)
    double datmis;
    int device = 0, ncu = 256;
    int wmax = 1;       // widest column window
    DevBuf<double> SINA, FMIN, FMAX, GMIN, GMAX;
    DevBuf<int32_t> IMIN, IMAX, JMIN, JMAX;
    // for the matrix forms (ibh_hntr_triplets / ibh_hntr_matrix_d): the windows on the host (column windows shifted as on the
    // device), dxyp of grid B, and the B cells whose windows hold each A row / each column position IAREV in [1, 2*imA]
    std::vector<int32_t> hIMIN, hIMAX, hJMIN, hJMAX;
    DevBuf<double> dxypB;
    DevBuf<int32_t> jbr, ibr;       // [2*jmA] first / last JB (1-based) per JA; [2*2*imA] first / last IB per IAREV (lo > hi: none)
};

namespace ibh {

// The shape of one launch, decided from the handle, nvar and the weight form alone: the planes are staged as doubles, so the
// element types play no part.
struct HntrShape {
    int NV, L, K, S;        // fields per group, chain lanes per wave, columns per chunk, LDS row stride in doubles (odd, >= K)
    int ngroups;
    size_t lds_bytes;       // dynamic LDS of a workgroup: the staged planes, 8 * P * L * S
};

static HntrShape hntr_shape(const ibh_hntr *h, int nvar, bool const_weight, bool per_field) {
    // fields per group: per-field weights run one field per group; a shared or constant weight serves up to 8
    const int NV = per_field || nvar <= 1 ? 1 : nvar == 2 ? 2 : nvar <= 4 ? 4 : 8;
    const int P = (const_weight ? 0 : 1) + NV;      // staged planes
    const int ngroups = (nvar + NV - 1) / NV;
    // lanes per wave: all 64 when there are B cells enough for four waves per CU, fewer (more workgroups, so more
    // CUs streaming at once) for small B grids
    int L = 64;
    while (L > 1 && (int64_t)ceil_div(h->jmB, L) * h->imB * ngroups < 4 * (int64_t)h->ncu) L >>= 1;
    if (L > h->jmB) { L = 1; while (L < h->jmB) L <<= 1; }
    // LDS per workgroup: 20 KiB (eight one-wave workgroups per CU) while that still leaves chunks of 16 columns, else up
    // to 40 KiB.  Measured from a 1' field: one field 1.38 ms at 20 KiB against 1.79 ms at 40 KiB (1/2 deg); eight fields,
    // whose chunks would shrink to 3 columns at 20 KiB, 9.2 ms at 40 KiB against 15.3 ms.  Under a constant weight the large
    // budget is 32 KiB: eight double fields onto 1 deg ran 18.5 ms with 9 columns in 36.5 KiB (four workgroups per CU) and
    // 12.6 ms with 7 columns in 28.5 KiB (five).
    int smax = HNTR_LDS_SMALL / (L * P);
    if (smax < std::min(h->wmax, 16)) smax = (const_weight ? HNTR_LDS_CONST : HNTR_LDS) / (L * P);
    if (!(smax & 1)) --smax;
    const int K = std::min(h->wmax, smax);
    const int S = K | 1;
    return HntrShape{NV, L, K, S, ngroups, (size_t)L * S * P * sizeof(double)};
}

template <int NV, class WT, class ST>
static void hntr_launch_nv(const ibh_hntr *h, HntrShape const &sh, HntrArgs a, hipStream_t s) {
    a.L = sh.L; a.K = sh.K; a.S = sh.S;
    dim3 grid((unsigned)(ceil_div(h->jmB, sh.L) * h->imB), (unsigned)sh.ngroups);
    hipLaunchKernelGGL((hntr_regrid_kernel<NV, WT, ST>), grid, dim3(64), sh.lds_bytes, s, a);
    IBH_HIP(hipGetLastError());
}
template <class WT, class ST>
static void hntr_launch_types(const ibh_hntr *h, HntrShape const &sh, HntrArgs const &a, hipStream_t s) {
    if (sh.NV == 1) hntr_launch_nv<1, WT, ST>(h, sh, a, s);
    else if (sh.NV == 2) hntr_launch_nv<2, WT, ST>(h, sh, a, s);
    else if (sh.NV == 4) hntr_launch_nv<4, WT, ST>(h, sh, a, s);
    else hntr_launch_nv<8, WT, ST>(h, sh, a, s);
}
template <class WT>
static void hntr_launch_weight(const ibh_hntr *h, HntrShape const &sh, HntrArgs const &a, int a_type, hipStream_t s) {
    if (a_type == IBH_HNTR_F64) hntr_launch_types<WT, double>(h, sh, a, s);
    else if (a_type == IBH_HNTR_F32) hntr_launch_types<WT, float>(h, sh, a, s);
    else hntr_launch_types<WT, int16_t>(h, sh, a, s);
}

static size_t hntr_elem_size(int type) { return type == IBH_HNTR_F64 ? 8 : type == IBH_HNTR_F32 ? 4 : 2; }
static void check_elem_type(int type, const char *which) {
    IBH_CHECK(type == IBH_HNTR_F64 || type == IBH_HNTR_I16 || type == IBH_HNTR_F32,
              "Hntr regrid: type code %d of %s is not IBH_HNTR_F64 (0), IBH_HNTR_I16 (1) or IBH_HNTR_F32 (2)", type, which);
}

// dWTA == nullptr: the constant weight wta_const (wta_type and wta_ld are not read)
static void hntr_regrid(const ibh_hntr *h, const void *dWTA, int wta_type, int64_t wta_ld, double wta_const, const void *dA, int a_type,
                        int32_t nvar, int64_t lda, double *dB, int64_t ldb, int mean_polar, double wtm, double wtb, hipStream_t s) {
    HntrArgs a{};
    a.SINA = h->SINA.p; a.FMIN = h->FMIN.p; a.FMAX = h->FMAX.p; a.GMIN = h->GMIN.p; a.GMAX = h->GMAX.p;
    a.IMIN = h->IMIN.p; a.IMAX = h->IMAX.p; a.JMIN = h->JMIN.p; a.JMAX = h->JMAX.p;
    a.WTA = dWTA; a.wta_ld = dWTA ? wta_ld : 0; a.wconst = wta_const; a.A = dA; a.lda = lda; a.B = dB; a.ldb = ldb;
    a.imA = h->imA; a.imB = h->imB; a.jmB = h->jmB; a.nvar = nvar;
    a.wtm = wtm; a.wtb = wtb; a.datmis = h->datmis;
    const HntrShape sh = hntr_shape(h, nvar, dWTA == nullptr, a.wta_ld != 0);
    if (!dWTA) hntr_launch_weight<HntrConstW>(h, sh, a, a_type, s);
    else if (wta_type == IBH_HNTR_F64) hntr_launch_weight<double>(h, sh, a, a_type, s);
    else if (wta_type == IBH_HNTR_F32) hntr_launch_weight<float>(h, sh, a, a_type, s);
    else hntr_launch_weight<int16_t>(h, sh, a, a_type, s);
    if (mean_polar) {
        hipLaunchKernelGGL(hntr_mean_polar_kernel, dim3((unsigned)ceil_div(2 * (int64_t)nvar, 64)), dim3(64), 0, s,
                           dB, ldb, nvar, h->imB, h->jmB, h->datmis);
        IBH_HIP(hipGetLastError());
    }
}

// const_weight: the typed entries' WTA == nullptr, where no weight plane is read and wta_ld is ignored
static void check_regrid_args(const ibh_hntr *h, const void *WTA, int64_t wta_ld, const void *A, int32_t nvar, int64_t lda,
                              const void *B, int64_t ldb, int mean_polar, bool const_weight = false) {
    IBH_CHECK(h != nullptr, "null Hntr handle");
    check_current_device(h->device, "Hntr handle");
    const int64_t nA = (int64_t)h->imA * h->jmA, nB = (int64_t)h->imB * h->jmB;
    IBH_CHECK(nvar >= 0 && (nvar == 0 || ((WTA || const_weight) && A && B)), "Hntr regrid: bad arguments (nvar=%d or a null array)", nvar);
    IBH_CHECK(lda >= nA && ldb >= nB, "Hntr regrid: leading dimensions too small (lda=%lld < %lld or ldb=%lld < %lld)",
              (long long)lda, (long long)nA, (long long)ldb, (long long)nB);
    IBH_CHECK(const_weight || wta_ld == 0 || wta_ld >= nA, "Hntr regrid: wta_ld=%lld must be 0 (shared weight) or >= %lld",
              (long long)wta_ld, (long long)nA);
    IBH_CHECK(!mean_polar || h->jmB >= 2, "Hntr regrid: mean_polar needs jmB >= 2 (the reference loops forever on jmB=1)");
}
static void check_typed_args(const ibh_hntr *h, const void *WTA, int wta_type, int64_t wta_ld, const void *A, int a_type, int32_t nvar,
                             int64_t lda, const void *B, int64_t ldb, int mean_polar) {
    check_elem_type(a_type, "A");
    if (WTA) check_elem_type(wta_type, "WTA");
    check_regrid_args(h, WTA, wta_ld, A, nvar, lda, B, ldb, mean_polar, WTA == nullptr);
}

// ---- matrix forms (hntr.hpp:205-338 Hntr::matrix, OverlapMatAccum, ScaledRegridMatAccum; hntr.cpp:33-52 make_dxyp) ----
// Hntr::matrix visits the included B cells in stream order (JB, then IB, ascending) and, inside a cell, JA from JMIN(JB) to
// JMAX(JB), then IAREV from IMIN(IB) to IMAX(IB), with the term FG = F*G; the accumulators emit ((IJB-1, IJA-1), FG *
// (1/WEIGHT) [* R2*dxyp(JB)]) once the cell's WEIGHT (the sum of its FG, in that order) is known.  On the device:
//   count     one thread per B cell: its triplets (JMAX-JMIN+1) * (IMAX-IMIN+1), or its distinct columns (CSR)
//   scan      prims' exclusive scan: the triplet offsets or the CSR row pointer
//   weight    one lane per B cell: the WEIGHT chain in stream order (loads nothing but the partition), 1/WEIGHT stored
//   fill      TPR lanes per row: the CSR in column order straight from the partition (no sort).  A window that wraps the
//             date line becomes two ascending IA runs per A row, listed low run first; a column visited twice (a window wider
//             than imA) is summed in stream order (IAREV = IA, then IA + imA), the first term assigned (setFromTriplets).
//             Quads of entries aligned to the whole array are stored as int4 / 2 x double2.
//   wM        one lane per row: the row's values again, from 0 in column order (spsparse sum(M, 0, '+')); no loads
//   Mw        one thread per A column: the B cells whose windows hold it, rows ascending, from 0
// All values are recomputed with the same expressions wherever they are needed, so fill, wM and Mw agree bit for bit.
// Other dims (ADD_DENSE onto a partial set, TO_DENSE through a pre-populated or permuted one, transpose) take the triplets
// through a first-seen numbering on the device and the triplets -> CSR layer's setFromTriplets (weighted_from_device_triplets).
static void hntr_dxyp(int im, int jm, double *dxyp) {
    const double dLON = (2. * M_PI) / im;
    const double dLAT = M_PI / jm;
    for (int j = 1; j <= jm; ++j) {
        const double SINS = sin(dLAT * (j - jm / 2 - 1));
        const double SINN = sin(dLAT * (j - jm / 2));
        dxyp[j - 1] = dLON * (SINN - SINS);
    }
}

static void hntr_matrix_tables(ibh_hntr *h, HntrPartition const &p) {
    // p: column windows already shifted
    h->hIMIN = p.IMIN; h->hIMAX = p.IMAX; h->hJMIN = p.JMIN; h->hJMAX = p.JMAX;
    std::vector<double> dx((size_t)h->jmB);
    hntr_dxyp(h->imB, h->jmB, dx.data());
    h->dxypB.upload(dx.data(), dx.size());
    std::vector<int32_t> jbr(2 * (size_t)h->jmA), ibr(4 * (size_t)h->imA);
    for (int ja = 0; ja < h->jmA; ++ja) { jbr[2 * ja] = 1 << 30; jbr[2 * ja + 1] = -1; }
    for (int v = 0; v < 2 * h->imA; ++v) { ibr[2 * v] = 1 << 30; ibr[2 * v + 1] = -1; }
    for (int jb = 1; jb <= h->jmB; ++jb)
        for (int ja = p.JMIN[jb - 1]; ja <= p.JMAX[jb - 1]; ++ja) {
            jbr[2 * (ja - 1)] = std::min(jbr[2 * (ja - 1)], jb);
            jbr[2 * (ja - 1) + 1] = std::max(jbr[2 * (ja - 1) + 1], jb);
        }
    for (int ib = 1; ib <= h->imB; ++ib)
        for (int v = p.IMIN[ib - 1]; v <= p.IMAX[ib - 1]; ++v) {
            ibr[2 * (v - 1)] = std::min(ibr[2 * (v - 1)], ib);
            ibr[2 * (v - 1) + 1] = std::max(ibr[2 * (v - 1) + 1], ib);
        }
    h->jbr.upload(jbr.data(), jbr.size());
    h->ibr.upload(ibr.data(), ibr.size());
}

struct HmArgs {
    const double *SINA, *FMIN, *FMAX, *GMIN, *GMAX, *dxyp;
    const int32_t *IMIN, *IMAX, *JMIN, *JMAX, *jbr, *ibr;
    const uint8_t *mask;        // includeB, nullptr: every cell
    const double *winv;         // [nB] 1/WEIGHT of included cells
    int imA, jmA, imB, jmB;
    int overlap;
    double R2;
};
// one B cell's part of the partition
struct HmCell {
    int imn, imx, jmn, jmx, W, D, lo;
    double fmn, fmx, gmn, gmx, winv, s;
};
__device__ __forceinline__ bool hm_included(const HmArgs &a, long r) { return !a.mask || a.mask[r]; }
__device__ __forceinline__ HmCell hm_cell(const HmArgs &a, int ib, int jb, bool with_w) {
    HmCell c;
    c.imn = a.IMIN[ib]; c.imx = a.IMAX[ib]; c.fmn = a.FMIN[ib]; c.fmx = a.FMAX[ib];
    c.jmn = a.JMIN[jb]; c.jmx = a.JMAX[jb]; c.gmn = a.GMIN[jb]; c.gmx = a.GMAX[jb];
    c.W = c.imx - c.imn + 1;
    c.D = min(c.W, a.imA);
    c.lo = c.imn > a.imA ? c.imn - a.imA : c.imn;
    c.winv = with_w ? a.winv[(long)jb * a.imB + ib] : 0.;
    c.s = a.overlap ? a.R2 * a.dxyp[jb] : 1.;
    return c;
}
__device__ __forceinline__ double hm_G(const HmArgs &a, const HmCell &c, int JA) {
    double G = a.SINA[JA] - a.SINA[JA - 1];
    if (JA == c.jmn) G -= c.gmn;
    if (JA == c.jmx) G -= c.gmx;
    return G;
}
__device__ __forceinline__ double hm_F(const HmCell &c, int IAREV) {
    double F = 1;
    if (IAREV == c.imn) F -= c.fmn;
    if (IAREV == c.imx) F -= c.fmx;
    return F;
}
// the accumulators' value of one term: FG * (1/WEIGHT) [* (R2*dxyp(JB))], left to right
__device__ __forceinline__ double hm_val(const HmArgs &a, const HmCell &c, double FG) {
    const double v = FG * c.winv;
    return a.overlap ? v * c.s : v;
}
// IA (1-based) of the k-th distinct column of an A row of the cell, columns ascending
__device__ __forceinline__ int hm_col(const HmArgs &a, const HmCell &c, int k) {
    if (c.W >= a.imA) return k + 1;
    const int n2 = c.lo + c.W - 1 - a.imA;      // > 0: the window wraps, IA 1..n2 come first
    if (n2 <= 0) return c.lo + k;
    return k < n2 ? k + 1 : c.lo + (k - n2);
}
// the stored value at (cell, JA, IA): the terms of IAREV = IA, then IA + imA, that lie in the window, the first assigned
__device__ __forceinline__ double hm_entry(const HmArgs &a, const HmCell &c, double G, int IA) {
    double v = 0;
    bool any = false;
    if (IA >= c.imn && IA <= c.imx) { v = hm_val(a, c, hm_F(c, IA) * G); any = true; }
    const int IA2 = IA + a.imA;
    if (IA2 >= c.imn && IA2 <= c.imx) {
        const double t = hm_val(a, c, hm_F(c, IA2) * G);
        v = any ? v + t : t;
    }
    return v;
}

__global__ void k_hm_count(HmArgs a, int csr, uint32_t *__restrict__ cnt) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (long)a.imB * a.jmB) return;
    const int ib = (int)(r % a.imB), jb = (int)(r / a.imB);
    uint32_t n = 0;
    if (hm_included(a, r)) {
        const int W = a.IMAX[ib] - a.IMIN[ib] + 1;
        n = (uint32_t)(a.JMAX[jb] - a.JMIN[jb] + 1) * (uint32_t)(csr ? min(W, a.imA) : W);
    }
    cnt[r] = n;
}

__global__ void k_hm_weight(HmArgs a, double *__restrict__ winv) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (long)a.imB * a.jmB || !hm_included(a, r)) return;
    const HmCell c = hm_cell(a, (int)(r % a.imB), (int)(r / a.imB), false);
    double WEIGHT = 0;
    for (int JA = c.jmn; JA <= c.jmx; ++JA) {
        const double G = hm_G(a, c, JA);
        for (int IAREV = c.imn; IAREV <= c.imx; ++IAREV) WEIGHT += hm_F(c, IAREV) * G;
    }
    winv[r] = 1. / WEIGHT;
}

// rows handled by teams of TPR lanes (a power of two dividing 256)
__device__ __forceinline__ bool hm_team(const HmArgs &a, int TPR, long &r, int &t) {
    r = (long)blockIdx.x * (256 / TPR) + threadIdx.x / TPR;
    t = threadIdx.x % TPR;
    return r < (long)a.imB * a.jmB;
}

// stream-order triplets (iB, iA) sparse, 0-based, at offsets tptr[r]
__global__ __launch_bounds__(256) void k_hm_triplets(HmArgs a, int TPR, const uint32_t *__restrict__ tptr, int32_t *__restrict__ iB,
                                                     int32_t *__restrict__ iA, double *__restrict__ val) {
    long r; int t;
    if (!hm_team(a, TPR, r, t)) return;
    const uint32_t p0 = tptr[r], p1 = tptr[r + 1];
    if (p0 == p1) return;
    const HmCell c = hm_cell(a, (int)(r % a.imB), (int)(r / a.imB), true);
    for (uint32_t e = t; e < p1 - p0; e += TPR) {
        const int jr = (int)(e / (uint32_t)c.W), k = (int)(e % (uint32_t)c.W);
        const int JA = c.jmn + jr, IAREV = c.imn + k;
        const int IA = IAREV > a.imA ? IAREV - a.imA : IAREV;
        iB[p0 + e] = (int32_t)r;
        iA[p0 + e] = (JA - 1) * a.imA + (IA - 1);
        val[p0 + e] = hm_val(a, c, hm_F(c, IAREV) * hm_G(a, c, JA));
    }
}

// the CSR in column order; quads of the whole array that lie inside the row are stored 16 bytes at a time
__global__ __launch_bounds__(256) void k_hm_fill(HmArgs a, int TPR, const int32_t *__restrict__ rowptr, int32_t *__restrict__ colind,
                                                 double *__restrict__ val) {
    long r; int t;
    if (!hm_team(a, TPR, r, t)) return;
    const int p0 = rowptr[r], p1 = rowptr[r + 1];
    if (p0 == p1) return;
    const HmCell c = hm_cell(a, (int)(r % a.imB), (int)(r / a.imB), true);
    // positions in 64 bits: p1 may be INT32_MAX, and base runs up to 4*TPR past it
    for (long base = (p0 & ~3) + 4l * t; base < p1; base += 4l * TPR) {
        const long q0 = max(base, (long)p0), q1 = min(base + 4, (long)p1);
        int e = (int)(q0 - p0);
        int jr = e / c.D, k = e - jr * c.D;
        int cc[4] = {0, 0, 0, 0};
        double vv[4] = {0, 0, 0, 0};
        int JA = c.jmn + jr;
        double G = hm_G(a, c, JA);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (base + u < q0 || base + u >= q1) continue;
            const int IA = hm_col(a, c, k);
            cc[u] = (JA - 1) * a.imA + (IA - 1);
            vv[u] = hm_entry(a, c, G, IA);
            if (++k == c.D) { k = 0; ++JA; if (JA <= c.jmx) G = hm_G(a, c, JA); }
        }
        if (q0 == base && q1 == base + 4) {
            *reinterpret_cast<int4 *>(colind + base) = make_int4(cc[0], cc[1], cc[2], cc[3]);
            *reinterpret_cast<double2 *>(val + base) = make_double2(vv[0], vv[1]);
            *reinterpret_cast<double2 *>(val + base + 2) = make_double2(vv[2], vv[3]);
        } else {
            for (int u = 0; u < 4; ++u)
                if (base + u >= q0 && base + u < q1) { colind[base + u] = cc[u]; val[base + u] = vv[u]; }
        }
    }
}

// wM: sum(M, 0, '+') of every row, from 0 in column order, recomputed (rows without entries: 0)
__global__ void k_hm_rowsum(HmArgs a, double *__restrict__ wM) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (long)a.imB * a.jmB) return;
    double s = 0;
    if (hm_included(a, r)) {
        const HmCell c = hm_cell(a, (int)(r % a.imB), (int)(r / a.imB), true);
        for (int JA = c.jmn; JA <= c.jmx; ++JA) {
            const double G = hm_G(a, c, JA);
            for (int k = 0; k < c.D; ++k) s = s + hm_entry(a, c, G, hm_col(a, c, k));
        }
    }
    wM[r] = s;
}

// Mw: sum(M, 1, '+') of every A column: the B cells that hold it, JB then IB ascending, from 0.  The cells whose column
// window holds IA + imA but not IA come after those that hold IA (windows are ordered), so the two IB ranges are walked
// in turn, the second past the end of the first.
__global__ void k_hm_colsum(HmArgs a, double *__restrict__ Mw) {
    const long col = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= (long)a.imA * a.jmA) return;
    const int JA = (int)(col / a.imA) + 1, IA = (int)(col % a.imA) + 1;
    const int jb0 = a.jbr[2 * (JA - 1)], jb1 = a.jbr[2 * (JA - 1) + 1];
    const int i10 = a.ibr[2 * (IA - 1)], i11 = a.ibr[2 * (IA - 1) + 1];
    const int i20 = max(a.ibr[2 * (IA - 1 + a.imA)], i11 + 1), i21 = a.ibr[2 * (IA - 1 + a.imA) + 1];
    double s = 0;
    for (int JB = jb0; JB <= jb1; ++JB) {
        for (int pass = 0; pass < 2; ++pass) {
            const int b0 = pass ? i20 : i10, b1 = pass ? i21 : i11;
            for (int IB = b0; IB <= b1; ++IB) {
                const long r = (long)(JB - 1) * a.imB + (IB - 1);
                if (!hm_included(a, r)) continue;
                const HmCell c = hm_cell(a, IB - 1, JB - 1, true);
                s = s + hm_entry(a, c, hm_G(a, c, JA), IA);
            }
        }
    }
    Mw[col] = s;
}

// ---- the to-dense transforms of the triplets (the numbering itself: sparseset.h) ----------------------------------------------
// An entry's indices are transformed in order, B then A, and the entry stops at the first index that
// TO_DENSE_IGNORE_MISSING drops: its A index is then neither numbered (ADD_DENSE) nor looked up (TO_DENSE).  So B is
// numbered over every entry and A over the entries whose B index survived (`act`).
// act[p]: the B index has a dense id; keep[p]: so has the A index of an active entry.  A key missing under TO_DENSE
// raises *bad.
__global__ void k_hm_gate(KeyNumbering sb, const int32_t *__restrict__ iB, long n, uint8_t *__restrict__ act, uint32_t *__restrict__ bad) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int db = dense_of(sb, iB[p]);
    if (db < 0 && sb.transform == IBH_TO_DENSE) atomicOr(bad, 1u);
    act[p] = db >= 0;
}
__global__ void k_hm_keep(KeyNumbering sa, const int32_t *__restrict__ iA, long n, uint32_t *__restrict__ keep, uint32_t *__restrict__ bad) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (!sa.act[p]) { keep[p] = 0; return; }
    const int da = dense_of(sa, iA[p]);
    if (da < 0 && sa.transform == IBH_TO_DENSE) atomicOr(bad, 1u);
    keep[p] = da >= 0 ? 1u : 0u;
}
__global__ void k_hm_compact(KeyNumbering sb, KeyNumbering sa, const int32_t *__restrict__ iB, const int32_t *__restrict__ iA,
                             const double *__restrict__ v, long n, const uint32_t *__restrict__ kpos, int transpose,
                             int32_t *__restrict__ row, int32_t *__restrict__ col, double *__restrict__ val) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || kpos[p + 1] == kpos[p]) return;
    const int db = dense_of(sb, iB[p]), da = dense_of(sa, iA[p]);
    const uint32_t q = kpos[p];
    row[q] = transpose ? da : db;
    col[q] = transpose ? db : da;
    val[q] = v[p];
}
static int hm_tpr(int64_t nnz, int64_t nrow) {
    const int64_t avg = nrow ? nnz / nrow : 0;
    int tpr = 4;
    while (tpr < 256 && 4 * (int64_t)tpr < avg) tpr <<= 1;
    return tpr;
}

// the number of triplets (or CSR entries) of the included cells, in 64 bits, from the host copy of the windows
static int64_t hm_count_host(const ibh_hntr *h, const uint8_t *mask, bool csr) {
    std::vector<int64_t> wi((size_t)h->imB);
    for (int ib = 0; ib < h->imB; ++ib) {
        const int64_t W = h->hIMAX[ib] - h->hIMIN[ib] + 1;
        wi[ib] = csr ? std::min<int64_t>(W, h->imA) : W;
    }
    int64_t n = 0;
    int64_t sw = 0;
    if (!mask) for (int ib = 0; ib < h->imB; ++ib) sw += wi[ib];
    for (int jb = 0; jb < h->jmB; ++jb) {
        const int64_t nj = h->hJMAX[jb] - h->hJMIN[jb] + 1;
        if (!mask) { n += nj * sw; continue; }
        int64_t s = 0;
        const uint8_t *m = mask + (size_t)jb * h->imB;
        for (int ib = 0; ib < h->imB; ++ib) if (m[ib]) s += wi[ib];
        n += nj * s;
    }
    return n;
}

static void hm_check_kind(int kind) { IBH_CHECK(kind == IBH_HNTR_OVERLAP || kind == IBH_HNTR_SCALED, "Hntr matrix: kind %d is not IBH_HNTR_OVERLAP or IBH_HNTR_SCALED", kind); }

// Everything up to the triplets or the CSR: mask upload, count, scan, weights.  Returns the args; ptr = the scan [nB+1].
static HmArgs hm_prepare(const ibh_hntr *h, int kind, double eq_rad, const uint8_t *includeB, bool csr, uint32_t *ptr,
                         hipStream_t st) {
    Arena &A = arena();
    const long nB = (long)h->imB * h->jmB;
    HmArgs a{};
    a.SINA = h->SINA.p; a.FMIN = h->FMIN.p; a.FMAX = h->FMAX.p; a.GMIN = h->GMIN.p; a.GMAX = h->GMAX.p; a.dxyp = h->dxypB.p;
    a.IMIN = h->IMIN.p; a.IMAX = h->IMAX.p; a.JMIN = h->JMIN.p; a.JMAX = h->JMAX.p; a.jbr = h->jbr.p; a.ibr = h->ibr.p;
    a.imA = h->imA; a.jmA = h->jmA; a.imB = h->imB; a.jmB = h->jmB;
    a.overlap = kind == IBH_HNTR_OVERLAP;
    a.R2 = eq_rad * eq_rad;
    if (includeB) {
        uint8_t *m = A.get<uint8_t>((size_t)nB);
        IBH_HIP(hipMemcpyAsync(m, includeB, (size_t)nB, hipMemcpyHostToDevice, st));
        a.mask = m;
    }
    double *winv = A.get<double>((size_t)nB);
    a.winv = winv;
    hipLaunchKernelGGL(k_hm_count, dim3(ceil_div(nB, 256)), dim3(256), 0, st, a, (int)csr, ptr);
    exclusive_scan_u32(ptr, ptr, (size_t)nB, ptr + nB, st);
    hipLaunchKernelGGL(k_hm_weight, dim3(ceil_div(nB, 64)), dim3(64), 0, st, a, winv);
    IBH_HIP(hipGetLastError());
    return a;
}

static void hm_check(const ibh_hntr *h, int kind) {
    IBH_CHECK(h != nullptr, "null Hntr handle");
    hm_check_kind(kind);
    check_current_device(h->device, "Hntr handle");
}

// the set a matrix_d call uses for one side: the caller's (sparse extent -1 takes the grid's) or a fresh identity
static void hm_check_transform(int transform, const char *which) {
    IBH_CHECK(transform == IBH_ADD_DENSE || transform == IBH_TO_DENSE || transform == IBH_TO_DENSE_IGNORE_MISSING,
              "Hntr matrix_d: transform %d of %s is not IBH_ADD_DENSE, IBH_TO_DENSE or IBH_TO_DENSE_IGNORE_MISSING", transform, which);
}
static ibh_sparse_set *hm_dims(ibh_sparse_set *set, int64_t extent, const char *which) {
    if (!set) return nullptr;
    const std::string what = std::string("Hntr matrix_d: ") + which;
    set->check_extent(extent, what.c_str());
    set->check_entries_within(extent, what.c_str());
    return set;
}
static bool hm_full_identity(const ibh_sparse_set *set, int64_t extent) {
    return !set || (set->identity() && set->n() == extent);
}

static void hntr_matrix(const ibh_hntr *h, int kind, double eq_rad, const uint8_t *includeB, ibh_sparse_set *dimB, int tB,
                        ibh_sparse_set *dimA, int tA, int transpose, ibh_weighted **out) {
    IBH_CHECK(out != nullptr, "null argument");
    hm_check_kind(kind);
    hm_check_transform(tB, "dimB");
    hm_check_transform(tA, "dimA");
    hm_check(h, kind);
    const int64_t nB = (int64_t)h->imB * h->jmB, nA = (int64_t)h->imA * h->jmA;
    dimB = hm_dims(dimB, nB, "dimB");
    dimA = hm_dims(dimA, nA, "dimA");
    IBH_CHECK(dimB == nullptr || dimB != dimA, "Hntr matrix_d: dimB and dimA must be distinct sets");
    const bool fast = !transpose && hm_full_identity(dimB, nB) && hm_full_identity(dimA, nA);
    const int64_t n = hm_count_host(h, includeB, fast);
    IBH_CHECK(n <= INT32_MAX, "Hntr matrix_d: %lld entries exceed INT32_MAX (the row pointer is int32)", (long long)n);
    hipStream_t st = nullptr;
    Arena &A = arena();
    A.reset();
    auto w = new_weighted();
    w->conservative = 1;
    w->scaled = kind == IBH_HNTR_SCALED;
    KeyNumberingRun nbB, nbA;   // the fast path numbers nothing: the sets only take their sparse extent
    DevBuf<int64_t> grownB, grownA;
    if (fast) {
        w->nrow = (int32_t)nB; w->ncol = (int32_t)nA; w->nnz = n;
        w->rowptr.alloc((size_t)nB + 1); w->colind.alloc((size_t)n); w->val.alloc((size_t)n);
        w->wM.alloc((size_t)nB); w->Mw.alloc((size_t)nA);
        uint32_t *ptr = reinterpret_cast<uint32_t *>(w->rowptr.p);
        HmArgs a = hm_prepare(h, kind, eq_rad, includeB, true, ptr, st);
        const int tpr = hm_tpr(n, nB);
        if (n) hipLaunchKernelGGL(k_hm_fill, dim3(ceil_div(nB, 256 / tpr)), dim3(256), 0, st, a, tpr, w->rowptr.p, w->colind.p, w->val.p);
        hipLaunchKernelGGL(k_hm_rowsum, dim3(ceil_div(nB, 64)), dim3(64), 0, st, a, w->wM.p);
        hipLaunchKernelGGL(k_hm_colsum, dim3(ceil_div(nA, 256)), dim3(256), 0, st, a, w->Mw.p);
        IBH_HIP(hipGetLastError());
        IBH_HIP(hipStreamSynchronize(st));
    } else {
        uint32_t *ptr = A.get<uint32_t>((size_t)nB + 1);
        HmArgs a = hm_prepare(h, kind, eq_rad, includeB, false, ptr, st);
        int32_t *iB = A.get<int32_t>((size_t)n), *iA = A.get<int32_t>((size_t)n);
        double *v = A.get<double>((size_t)n);
        const int tpr = hm_tpr(n, nB);
        if (n) hipLaunchKernelGGL(k_hm_triplets, dim3(ceil_div(nB, 256 / tpr)), dim3(256), 0, st, a, tpr, ptr, iB, iA, v);
        uint32_t *keep = A.get<uint32_t>((size_t)n + 1), *bad = A.get<uint32_t>(1);
        uint8_t *act = A.get<uint8_t>((size_t)n);
        IBH_HIP(hipMemsetAsync(bad, 0, sizeof(uint32_t), st));
        nbB = number_keys_prepare(dimB, nB, tB, iB, 1, (long)n, nullptr, false, st);
        if (n) hipLaunchKernelGGL(k_hm_gate, dim3(ceil_div(n, 256)), dim3(256), 0, st, nbB.s, iB, (long)n, act, bad);
        nbA = number_keys_prepare(dimA, nA, tA, iA, 1, (long)n, act, false, st);
        if (n) hipLaunchKernelGGL(k_hm_keep, dim3(ceil_div(n, 256)), dim3(256), 0, st, nbA.s, iA, (long)n, keep, bad);
        exclusive_scan_u32(keep, keep, (size_t)n, keep + n, st);
        struct { uint32_t kept, bad, newB, newA; } rb{0, 0, 0, 0};
        readback_sync(&rb.kept, keep + n, sizeof(uint32_t), st);
        readback_sync(&rb.bad, bad, sizeof(uint32_t), st);
        if (nbB.adds()) readback_sync(&rb.newB, nbB.status, sizeof(uint32_t), st);
        if (nbA.adds()) readback_sync(&rb.newA, nbA.status, sizeof(uint32_t), st);
        IBH_CHECK(!rb.bad, "Hntr matrix_d: a key is missing from a TO_DENSE set");
        const int nrowB = (nbB.set ? nbB.s.n_old : (int)nB) + (int)rb.newB;
        const int ncolA = (nbA.set ? nbA.s.n_old : (int)nA) + (int)rb.newA;
        int32_t *row = A.get<int32_t>(rb.kept), *col = A.get<int32_t>(rb.kept);
        double *val = A.get<double>(rb.kept);
        if (n) hipLaunchKernelGGL(k_hm_compact, dim3(ceil_div(n, 256)), dim3(256), 0, st, nbB.s, nbA.s, iB, iA, v, (long)n, keep,
                                  transpose, row, col, val);
        IBH_HIP(hipGetLastError());
        weighted_from_device_triplets(w.get(), transpose ? ncolA : nrowB, transpose ? nrowB : ncolA, rb.kept, row, col, val, st);
        // both grown tables exist before either set changes: an error up to here leaves both sets as they were
        grownB = number_keys_grow(nbB, iB, 1, (long)n, rb.newB, st);
        grownA = number_keys_grow(nbA, iA, 1, (long)n, rb.newA, st);
        IBH_HIP(hipStreamSynchronize(st));
    }
    // the fresh identities first (they allocate), then the caller's sets take their tables: that cannot fail
    DimRef dB = dimB ? DimRef::borrowed(dimB) : DimRef::owned_identity(nB), dA = dimA ? DimRef::borrowed(dimA) : DimRef::owned_identity(nA);
    if (dimB) dimB->adopt_device(std::move(grownB), (int32_t)grownB.n, nB);
    if (dimA) dimA->adopt_device(std::move(grownA), (int32_t)grownA.n, nA);
    w->dims[transpose ? 1 : 0] = std::move(dB);
    w->dims[transpose ? 0 : 1] = std::move(dA);
    *out = w.release();
}

static void hntr_triplets(const ibh_hntr *h, int kind, double eq_rad, const uint8_t *includeB, int64_t *n, int32_t *iB, int32_t *iA,
                          double *val) {
    hm_check_kind(kind);
    IBH_CHECK(h != nullptr && n != nullptr, "null argument");
    const int64_t cnt = hm_count_host(h, includeB, false);
    *n = cnt;
    IBH_CHECK(cnt <= INT32_MAX, "Hntr triplets: %lld entries exceed INT32_MAX", (long long)cnt);
    if (!iB && !iA && !val) return;
    IBH_CHECK(iB && iA && val, "Hntr triplets: iB, iA and val must all be given (or all NULL)");
    hm_check(h, kind);
    hipStream_t st = nullptr;
    Arena &A = arena();
    A.reset();
    const long nB = (long)h->imB * h->jmB;
    uint32_t *ptr = A.get<uint32_t>((size_t)nB + 1);
    HmArgs a = hm_prepare(h, kind, eq_rad, includeB, false, ptr, st);
    int32_t *dB = A.get<int32_t>((size_t)cnt), *dA = A.get<int32_t>((size_t)cnt);
    double *dv = A.get<double>((size_t)cnt);
    const int tpr = hm_tpr(cnt, nB);
    if (cnt) hipLaunchKernelGGL(k_hm_triplets, dim3(ceil_div(nB, 256 / tpr)), dim3(256), 0, st, a, tpr, ptr, dB, dA, dv);
    IBH_HIP(hipGetLastError());
    if (cnt) {
        IBH_HIP(hipMemcpyAsync(iB, dB, sizeof(int32_t) * (size_t)cnt, hipMemcpyDeviceToHost, st));
        IBH_HIP(hipMemcpyAsync(iA, dA, sizeof(int32_t) * (size_t)cnt, hipMemcpyDeviceToHost, st));
        IBH_HIP(hipMemcpyAsync(val, dv, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost, st));
    }
    IBH_HIP(hipStreamSynchronize(st));
}

// ---- global_ec: the exchange grid of Hntr's overlap under an ice mask (modele/global_ec.cpp:296-322 ExchAccum, :384-432
// new_gcmA_standard) ------------------------------------------------------------------------------------------------------
// Grid A of the handle is the ice grid, B the GCM grid.  The overlap's stream-order entries (iB, iA, v) whose ice cell has a
// non-NaN mask are appended as exchange cells (iB, iA, v); WEIGHT (k_hm_weight, no includeB) sums every term of the B cell,
// the mask only filters.  On the device:
//   count     TPR lanes per B cell (grid-stride): the cell's kept terms (mask reads only), cnt[r]; a 64-bit grand total
//   scan      prims' exclusive scan of cnt (only once the total is known to fit in int32)
//   fill      TPR lanes per B cell: the terms in stream order, TPR at a time; a ballot over the team ranks the kept ones
//   dims      dimA = the cells with cnt > 0 (a flag scan); dimI = ice cells first-seen in stream order (sparseset.h)
constexpr int HX_T = 256;
__global__ __launch_bounds__(HX_T) void k_hx_count(HmArgs a, const double *__restrict__ mask, int TPR, uint32_t *__restrict__ cnt,
                                                   unsigned long long *__restrict__ total) {
    __shared__ unsigned long long part[HX_T / 64];
    const long nB = (long)a.imB * a.jmB;
    const int t = threadIdx.x % TPR;
    const long teams = (long)gridDim.x * (HX_T / TPR);
    unsigned long long acc = 0;
    for (long r = (long)blockIdx.x * (HX_T / TPR) + threadIdx.x / TPR; r < nB; r += teams) {      // team-uniform trip counts
        const int ib = (int)(r % a.imB), jb = (int)(r / a.imB);
        const int imn = a.IMIN[ib], W = a.IMAX[ib] - imn + 1, jmn = a.JMIN[jb];
        const uint32_t nt = (uint32_t)(a.JMAX[jb] - jmn + 1) * (uint32_t)W;
        uint32_t n = 0;
        for (uint32_t e = t; e < nt; e += TPR) {
            const int JA = jmn + (int)(e / (uint32_t)W), IAREV = imn + (int)(e % (uint32_t)W);
            const int IA = IAREV > a.imA ? IAREV - a.imA : IAREV;
            n += isnan(mask[(long)(JA - 1) * a.imA + (IA - 1)]) ? 0u : 1u;
        }
        for (int o = TPR / 2; o > 0; o >>= 1) n += __shfl_xor(n, o, TPR);
        if (t == 0) {
            if (cnt) cnt[r] = n;
            acc += n;
        }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x / 64] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < HX_T / 64; ++w) s += part[w];
        if (s) atomicAdd(total, s);
    }
}

// the exchange cells of B cell r at pos[r]: (iB, iI) pairs and their overlaps, stream order
__global__ __launch_bounds__(HX_T) void k_hx_fill(HmArgs a, const double *__restrict__ mask, int TPR, const uint32_t *__restrict__ pos,
                                                  int2 *__restrict__ idx, double *__restrict__ area) {
    long r; int t;
    if (!hm_team(a, TPR, r, t)) return;          // whole teams
    const uint32_t p0 = pos[r], p1 = pos[r + 1];
    if (p0 == p1) return;                         // whole teams
    const HmCell c = hm_cell(a, (int)(r % a.imB), (int)(r / a.imB), true);
    const uint32_t nt = (uint32_t)(c.jmx - c.jmn + 1) * (uint32_t)c.W;
    const int tb = (threadIdx.x & 63) & ~(TPR - 1);
    const unsigned long long tmask = TPR == 64 ? ~0ull : ((1ull << TPR) - 1);
    const unsigned long long below = (1ull << t) - 1;
    uint32_t p = p0;
    for (uint32_t base = 0; base < nt; base += TPR) {
        const uint32_t e = base + t;
        int JA = 0, IAREV = 0;
        long iI = 0;
        bool keep = false;
        if (e < nt) {
            JA = c.jmn + (int)(e / (uint32_t)c.W);
            IAREV = c.imn + (int)(e % (uint32_t)c.W);
            const int IA = IAREV > a.imA ? IAREV - a.imA : IAREV;
            iI = (long)(JA - 1) * a.imA + (IA - 1);
            keep = !isnan(mask[iI]);
        }
        const unsigned long long b = (__ballot(keep) >> tb) & tmask;
        if (keep) {
            const uint32_t q = p + (uint32_t)__popcll(b & below);
            idx[q] = make_int2((int)r, (int)iI);
            area[q] = hm_val(a, c, hm_F(c, IAREV) * hm_G(a, c, JA));
        }
        p += (uint32_t)__popcll(b);
    }
}

__global__ void k_hx_cellflag(const uint32_t *__restrict__ pos, long nB, uint32_t *__restrict__ flag) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < nB) flag[r] = pos[r + 1] != pos[r] ? 1u : 0u;
}
__global__ void k_hx_cells(const uint32_t *__restrict__ rank, long nB, int64_t *__restrict__ to_sparse) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < nB && rank[r + 1] != rank[r]) to_sparse[rank[r]] = r;
}
static const ibh_hntr *hx_check_desc(const ibh_hntr_regridder_desc *d) {
    IBH_CHECK(d != nullptr, "null argument");
    const ibh_hntr *h = d->hntr;
    IBH_CHECK(h != nullptr, "global_ec: null Hntr handle");
    check_current_device(h->device, "Hntr handle");
    const int64_t nI = (int64_t)h->imA * h->jmA, nA = (int64_t)h->imB * h->jmB;
    IBH_CHECK(d->elevmaskI != nullptr, "global_ec: null elevmaskI");
    IBH_CHECK(d->nmask == nI, "global_ec: elevmaskI has %lld elements, the ice grid (Hntr grid A) has nI=%lld", (long long)d->nmask,
              (long long)nI);
    IBH_CHECK(d->nhc >= 0, "global_ec: negative nhc");
    IBH_CHECK(nA * (int64_t)(d->nhc > 0 ? d->nhc : 1) < (1ll << 31), "global_ec: nE = nA*nhc = %lld overflows int32 dense ids",
              (long long)(nA * (int64_t)d->nhc));
    IBH_CHECK(d->interp_style == 0 || d->interp_style == 1, "unknown interp_style %d", d->interp_style);
    if (d->nhc > 0) {
        IBH_CHECK(d->hcdefs != nullptr, "null hcdefs");
        for (int k = 1; k < d->nhc; ++k) IBH_CHECK(d->hcdefs[k] > d->hcdefs[k - 1], "hcdefs must be ascending");
        const bool hc_slowest = d->hc_stride_A == 1 && d->hc_stride_HC == nA;
        const bool hc_fastest = d->hc_stride_HC == 1 && d->hc_stride_A == d->nhc;
        IBH_CHECK(hc_slowest || hc_fastest, "indexingHC strides (%ld,%ld) are neither (1,nA) nor (nhc,1)", (long)d->hc_stride_A,
                  (long)d->hc_stride_HC);
    }
    IBH_CHECK(std::isfinite(d->eq_rad), "global_ec: eq_rad=%g is not finite", d->eq_rad);
    return h;
}

// the device copy of the mask (the caller's pointer when it is on the device), on st
static const double *hx_mask(const ibh_hntr_regridder_desc *d, int64_t nI, hipStream_t st) {
    if (d->mask_on_device) return d->elevmaskI;
    double *m = arena().get<double>((size_t)nI);
    IBH_HIP(hipMemcpyAsync(m, d->elevmaskI, sizeof(double) * (size_t)nI, hipMemcpyHostToDevice, st));
    return m;
}

static HmArgs hx_args(const ibh_hntr *h, double eq_rad) {
    HmArgs a{};
    a.SINA = h->SINA.p; a.FMIN = h->FMIN.p; a.FMAX = h->FMAX.p; a.GMIN = h->GMIN.p; a.GMAX = h->GMAX.p; a.dxyp = h->dxypB.p;
    a.IMIN = h->IMIN.p; a.IMAX = h->IMAX.p; a.JMIN = h->JMIN.p; a.JMAX = h->JMAX.p; a.jbr = h->jbr.p; a.ibr = h->ibr.p;
    a.imA = h->imA; a.jmA = h->jmA; a.imB = h->imB; a.jmB = h->jmB;
    a.overlap = 1;
    a.R2 = eq_rad * eq_rad;
    return a;
}

// the kept terms in 64 bits (cnt != nullptr: also per B cell)
static int64_t hx_count(const ibh_hntr *h, const HmArgs &a, const double *mask, uint32_t *cnt, int TPR, hipStream_t st) {
    const long nB = (long)h->imB * h->jmB;
    unsigned long long *tot = arena().get<unsigned long long>(1);
    IBH_HIP(hipMemsetAsync(tot, 0, sizeof(unsigned long long), st));
    const long blocks = std::min<long>(ceil_div(nB, HX_T / TPR), 16l * h->ncu);
    hipLaunchKernelGGL(k_hx_count, dim3((unsigned)std::max(blocks, 1l)), dim3(HX_T), 0, st, a, mask, TPR, cnt, tot);
    IBH_HIP(hipGetLastError());
    unsigned long long n = 0;
    readback_sync(&n, tot, sizeof(n), st);
    return (int64_t)n;
}

// lanes per B cell: from the mean window size (a power of two, 4..64: a team lives inside one wave)
static int hx_tpr(const ibh_hntr *h) {
    return std::min(hm_tpr(hm_count_host(h, nullptr, false), (int64_t)h->imB * h->jmB), 64);
}

static void hntr_exgrid_count(const ibh_hntr_regridder_desc *d, int64_t *nX) {
    IBH_CHECK(nX != nullptr, "null argument");
    const ibh_hntr *h = hx_check_desc(d);
    hipStream_t st = static_cast<hipStream_t>(d->stream);
    Arena &A = arena();
    A.reset();
    const double *mask = hx_mask(d, (int64_t)h->imA * h->jmA, st);
    *nX = hx_count(h, hx_args(h, d->eq_rad), mask, nullptr, hx_tpr(h), st);
}

// make_grid_spec (GridSpec.cpp:80-122) with pole_caps = false: lonb [im+1], latb [2*(jm/2)+1], degrees
static void hx_grid_spec(int im, int jm, double offi, double dlat, std::vector<double> &lonb, std::vector<double> &latb) {
    const double deg_by_im = 360. / (double)im;
    lonb.clear(); latb.clear();
    for (int i = 0; i < im; ++i) lonb.push_back(-180. + (offi + (double)i) * deg_by_im);
    lonb.push_back(lonb[0] + 360.);
    latb.push_back(0);
    const double dlat_d = dlat / 60.;
    for (int j = 1; j < jm / 2; ++j) {
        const double lat = j * dlat_d;
        latb.push_back(lat);
        latb.push_back(-lat);
    }
    double lat = jm / 2 * dlat_d;
    if (std::abs(lat - 90.) < 1.e-10) lat = 90.;
    latb.push_back(lat);
    latb.push_back(-lat);
    std::sort(latb.begin(), latb.end());
}

static void regridder_create_hntr(const ibh_hntr_regridder_desc *d, ibh_sparse_set *dimA_out, ibh_sparse_set *dimI_out,
                                  ibh_regridder **out) {
    IBH_CHECK(out != nullptr, "null argument");
    const ibh_hntr *h = hx_check_desc(d);
    // make_grid_spec(hspecA) has 2*(jm/2) rows: an odd jm would leave the last GCM row without boundaries.  (The reference
    // also refuses an odd im there; its areas are well defined, so an odd im is accepted.)
    IBH_CHECK(h->jmB % 2 == 0, "global_ec: the GCM grid (Hntr grid B) has jm=%d; make_grid_spec needs an even jm", h->jmB);
    IBH_CHECK(!dimA_out || dimA_out->n() == 0, "global_ec: dimA_out must be an empty set");
    IBH_CHECK(!dimI_out || dimI_out->n() == 0, "global_ec: dimI_out must be an empty set");
    IBH_CHECK(!dimA_out || dimA_out != dimI_out, "global_ec: dimA_out and dimI_out must be distinct sets");
    const int64_t nI = (int64_t)h->imA * h->jmA, nB = (int64_t)h->imB * h->jmB;
    hipStream_t st = static_cast<hipStream_t>(d->stream);
    Arena &A = arena();
    A.reset();
    const HmArgs a0 = hx_args(h, d->eq_rad);
    const double *mask = hx_mask(d, nI, st);
    const int tpr = hx_tpr(h);
    // the kept cells in 64 bits before anything is allocated; when every term of the overlap fits in int32 the per-cell
    // counts come from the same pass (the mask is read once for the counts)
    uint32_t *pos = nullptr;
    if (hm_count_host(h, nullptr, false) <= INT32_MAX) pos = A.get<uint32_t>((size_t)nB + 1);
    const int64_t nX = hx_count(h, a0, mask, pos, tpr, st);
    // the bound of ibh_regridder_create (capi.hip): nX < 2^31 - 1
    IBH_CHECK(nX < INT32_MAX, "global_ec: %lld exchange cells exceed the regridder's limit (INT32_MAX - 1)", (long long)nX);

    std::unique_ptr<ibh_regridder> g(new ibh_regridder);
    g->device = h->device;
    g->nX = nX; g->nI = nI; g->nA = nB; g->nhc = d->nhc;
    g->interp_style = d->interp_style; g->hc_stride_A = d->hc_stride_A; g->hc_stride_HC = d->hc_stride_HC;
    g->hcdefs_h.assign(d->hcdefs, d->hcdefs + d->nhc);
    g->hcdefs.upload(d->hcdefs, (size_t)d->nhc, st);
    // count again per cell, scan, weights, fill
    if (!pos) {
        pos = A.get<uint32_t>((size_t)nB + 1);
        hx_count(h, a0, mask, pos, tpr, st);
    }
    exclusive_scan_u32(pos, pos, (size_t)nB, pos + nB, st);
    HmArgs a = a0;
    double *winv = A.get<double>((size_t)nB);
    a.winv = winv;
    hipLaunchKernelGGL(k_hm_weight, dim3(ceil_div(nB, 64)), dim3(64), 0, st, a, winv);
    g->ex_indices.alloc(2 * (size_t)nX);
    g->ex_area.alloc((size_t)nX);
    int2 *idx = reinterpret_cast<int2 *>(g->ex_indices.p);
    if (nX) hipLaunchKernelGGL(k_hx_fill, dim3(ceil_div(nB, HX_T / tpr)), dim3(HX_T), 0, st, a, mask, tpr, pos, idx, g->ex_area.p);
    // dimA: the B cells with exchange cells, ascending
    uint32_t *rank = A.get<uint32_t>((size_t)nB + 1);
    hipLaunchKernelGGL(k_hx_cellflag, dim3(ceil_div(nB, HX_T)), dim3(HX_T), 0, st, pos, (long)nB, rank);
    exclusive_scan_u32(rank, rank, (size_t)nB, rank + nB, st);
    uint32_t nAd = 0;
    readback_sync(&nAd, rank + nB, sizeof(nAd), st);
    DevBuf<int64_t> dA((size_t)nAd);
    if (nAd) hipLaunchKernelGGL(k_hx_cells, dim3(ceil_div(nB, HX_T)), dim3(HX_T), 0, st, rank, (long)nB, dA.p);
    // dimI: first-seen over the ice index (.y) of the exchange indices
    DevBuf<int64_t> dI;
    uint32_t nId = 0;
    if (dimI_out) {
        const int32_t *iI = reinterpret_cast<const int32_t *>(idx) + 1;
        const KeyNumberingRun nb = number_keys_prepare(dimI_out, nI, IBH_ADD_DENSE, iI, 2, (long)nX, nullptr, false, st);
        readback_sync(&nId, nb.status, sizeof(nId), st);
        dI = number_keys_grow(nb, iI, 2, (long)nX, nId, st);
    }
    IBH_HIP(hipGetLastError());
    // agridA on the host: make_abbr_grid's areas (GridGen_LonLat.cpp:234-275) from make_grid_spec(hspecA, false)
    g->nA_dense = (int32_t)nAd;
    g->A_to_sparse.resize(nAd);
    dA.download(g->A_to_sparse.data(), nAd, st);
    std::vector<double> lonb, latb;
    hx_grid_spec(h->imB, h->jmB, h->offiB, h->dlatB, lonb, latb);
    const double D2R = M_PI / 180.0;
    const double D2R_R2 = D2R * d->eq_rad * d->eq_rad;
    std::vector<double> dxyp((size_t)h->jmB);
    for (int j = 0; j < h->jmB; ++j) dxyp[j] = sin(latb[j + 1]) - sin(latb[j]);      // degrees into sin, as the reference
    g->A_native.resize(nAd);
    std::vector<double> ratio((size_t)nB, 0.0);
    for (uint32_t id = 0; id < nAd; ++id) {
        const int64_t s = g->A_to_sparse[id];
        const int i = (int)(s % h->imB), j = (int)(s / h->imB);
        g->A_native[id] = dxyp[j] * (lonb[i + 1] - lonb[i]) * D2R_R2;
        const double r = g->A_native[id] / g->A_native[id];      // projected area == native (IceRegridder.cpp:106-108)
        IBH_CHECK(std::isfinite(r) && r > 0, "global_ec: GCM cell %ld: native/proj area ratio %g is not positive", (long)s, r);
        ratio[(size_t)s] = r;
    }
    g->A_proj = g->A_native;
    g->A_ratio_s.upload(ratio.data(), ratio.size(), st);
    IBH_HIP(hipStreamSynchronize(st));
    // nothing below can fail: adopt the sets
    if (dimA_out) dimA_out->adopt_device(std::move(dA), (int32_t)nAd, nB);
    if (dimI_out) dimI_out->adopt_device(std::move(dI), (int32_t)nId, nI);
    *out = g.release();
}

// make_I2vX (modele/global_ec.cpp:345-376): I2vI from the Hntr overlap (as I2vI's columns: no transpose), then the products
// on the device (csrops.hip i2vx_compute).  dimI2 is numbered on a copy that replaces it only once everything succeeded.
static void make_i2vx(const ibh_weighted *IvX, const ibh_hntr *h, double eq_rad, const uint8_t *includeI, int64_t nincl,
                      ibh_sparse_set *dimI2, ibh_weighted **out) {
    IBH_CHECK(out != nullptr && IvX != nullptr, "null argument");
    hm_check(h, IBH_HNTR_OVERLAP);
    IBH_CHECK(IvX->device == h->device, "make_I2vX: IvX and the Hntr handle live on different devices");
    ibh_sparse_set *dimI = IvX->dims[0], *dimX = IvX->dims[1];
    const int64_t nI = (int64_t)h->imB * h->jmB, nI2 = (int64_t)h->imA * h->jmA;
    IBH_CHECK(dimI && dimX, "make_I2vX: IvX has no dims");
    IBH_CHECK(dimI->sparse_extent() == nI, "make_I2vX: IvX's ice dim has sparse extent %lld, the Hntr handle's grid B (hspecI) %lld cells",
              (long long)dimI->sparse_extent(), (long long)nI);
    IBH_CHECK(dimI->n() == IvX->nrow, "make_I2vX: IvX's ice dim holds %d entries, IvX has %d rows", dimI->n(), IvX->nrow);
    IBH_CHECK(includeI == nullptr || nincl == nI, "make_I2vX: includeI has %lld entries, the ice grid %lld cells", (long long)nincl,
              (long long)nI);
    IBH_CHECK(dimI2 == nullptr || (dimI2 != dimI && dimI2 != dimX), "make_I2vX: dimI2 must be a set of its own");
    IBH_CHECK(dimI2 == nullptr || dimI2->sparse_extent() == -1 || dimI2->sparse_extent() == nI2,
              "make_I2vX: dimI2 has sparse extent %lld, the Hntr handle's grid A (hspecI2) %lld cells",
              (long long)(dimI2 ? dimI2->sparse_extent() : 0), (long long)nI2);
    WorkingSet workI2(dimI2);
    ibh_weighted *raw = nullptr;
    hntr_matrix(h, IBH_HNTR_OVERLAP, eq_rad, includeI, dimI, IBH_TO_DENSE_IGNORE_MISSING, workI2.get(), IBH_ADD_DENSE, 0, &raw);
    std::unique_ptr<ibh_weighted> IvI2(raw);
    auto w = new_weighted();           // (hm_check: the handle's device)
    i2vx_compute(IvI2.get(), IvX, w.get());
    w->dims[1] = DimRef::borrow_or_copy(IvX->dims[1]);
    IvI2.reset();
    // nothing below can fail
    w->dims[0] = workI2.commit();
    *out = w.release();
}

}  // namespace ibh

extern "C" {

int ibh_hntr_partition(int32_t imA, int32_t jmA, double offiA, double dlatA, int32_t imB, int32_t jmB, double offiB, double dlatB,
                       double *SINA, double *SINB, int32_t *IMIN, int32_t *IMAX, double *FMIN, double *FMAX,
                       int32_t *JMIN, int32_t *JMAX, double *GMIN, double *GMAX) {
    return guarded([&] {
        IBH_CHECK(SINA && SINB && IMIN && IMAX && FMIN && FMAX && JMIN && JMAX && GMIN && GMAX, "null output array");
        HntrPartition p;
        hntr_partition(imA, jmA, offiA, dlatA, imB, jmB, offiB, dlatB, p);
        std::copy(p.SINA.begin(), p.SINA.end(), SINA); std::copy(p.SINB.begin(), p.SINB.end(), SINB);
        std::copy(p.IMIN.begin(), p.IMIN.end(), IMIN); std::copy(p.IMAX.begin(), p.IMAX.end(), IMAX);
        std::copy(p.FMIN.begin(), p.FMIN.end(), FMIN); std::copy(p.FMAX.begin(), p.FMAX.end(), FMAX);
        std::copy(p.JMIN.begin(), p.JMIN.end(), JMIN); std::copy(p.JMAX.begin(), p.JMAX.end(), JMAX);
        std::copy(p.GMIN.begin(), p.GMIN.end(), GMIN); std::copy(p.GMAX.begin(), p.GMAX.end(), GMAX);
    });
}

int ibh_hntr_create(ibh_hntr **out, int32_t imA, int32_t jmA, double offiA, double dlatA, int32_t imB, int32_t jmB, double offiB,
                    double dlatB, double datmis) {
    return guarded([&] {
        IBH_CHECK(out != nullptr, "null argument");
        HntrPartition p;
        hntr_partition(imA, jmA, offiA, dlatA, imB, jmB, offiB, dlatB, p);
        require_device();
        std::unique_ptr<ibh_hntr> h(new ibh_hntr);
        h->imA = imA; h->jmA = jmA; h->imB = imB; h->jmB = jmB; h->datmis = datmis;
        h->offiA = offiA; h->dlatA = dlatA; h->offiB = offiB; h->dlatB = dlatB;
        IBH_HIP(hipGetDevice(&h->device));
        IBH_HIP(hipDeviceGetAttribute(&h->ncu, hipDeviceAttributeMultiprocessorCount, h->device));
        const int shift = hntr_column_shift(p, imA);
        for (int i = 0; i < imB; ++i) {
            h->wmax = std::max(h->wmax, p.IMAX[i] - p.IMIN[i] + 1);
            p.IMIN[i] -= shift;
            p.IMAX[i] -= shift;
        }
        h->SINA.upload(p.SINA.data(), p.SINA.size()); h->FMIN.upload(p.FMIN.data(), p.FMIN.size());
        h->FMAX.upload(p.FMAX.data(), p.FMAX.size()); h->GMIN.upload(p.GMIN.data(), p.GMIN.size());
        h->GMAX.upload(p.GMAX.data(), p.GMAX.size()); h->IMIN.upload(p.IMIN.data(), p.IMIN.size());
        h->IMAX.upload(p.IMAX.data(), p.IMAX.size()); h->JMIN.upload(p.JMIN.data(), p.JMIN.size());
        h->JMAX.upload(p.JMAX.data(), p.JMAX.size());
        hntr_matrix_tables(h.get(), p);
        IBH_HIP(hipStreamSynchronize(nullptr));
        *out = h.release();
    });
}

int ibh_hntr_destroy(ibh_hntr *h) { delete h; return IBH_OK; }

int ibh_hntr_regrid_device(const ibh_hntr *h, const double *dWTA, int64_t wta_ld, const double *dA, int32_t nvar, int64_t lda,
                           double *dB, int64_t ldb, int mean_polar, double wtm, double wtb, void *stream) {
    return guarded([&] {
        check_regrid_args(h, dWTA, wta_ld, dA, nvar, lda, dB, ldb, mean_polar);
        if (nvar == 0) return;
        hntr_regrid(h, dWTA, IBH_HNTR_F64, wta_ld, 0., dA, IBH_HNTR_F64, nvar, lda, dB, ldb, mean_polar, wtm, wtb,
                    static_cast<hipStream_t>(stream));
    });
}

int ibh_hntr_regrid_typed_device(const ibh_hntr *h, const void *dWTA, int wta_type, int64_t wta_ld, double wta_const, const void *dA,
                                 int a_type, int32_t nvar, int64_t lda, double *dB, int64_t ldb, int mean_polar, double wtm, double wtb,
                                 void *stream) {
    return guarded([&] {
        check_typed_args(h, dWTA, wta_type, wta_ld, dA, a_type, nvar, lda, dB, ldb, mean_polar);
        if (nvar == 0) return;
        hntr_regrid(h, dWTA, wta_type, wta_ld, wta_const, dA, a_type, nvar, lda, dB, ldb, mean_polar, wtm, wtb,
                    static_cast<hipStream_t>(stream));
    });
}

int ibh_hntr_regrid_shape(const ibh_hntr *h, int32_t nvar, int wta_is_const, int wta_type, int64_t wta_ld, int a_type, int32_t *NV,
                          int32_t *L, int32_t *K, int64_t *lds_bytes) {
    return guarded([&] {
        IBH_CHECK(h != nullptr, "null Hntr handle");
        check_elem_type(a_type, "A");
        if (!wta_is_const) check_elem_type(wta_type, "WTA");
        IBH_CHECK(nvar >= 1, "Hntr regrid shape: nvar=%d (must be >= 1)", nvar);
        IBH_CHECK(NV && L && K && lds_bytes, "Hntr regrid shape: null output");
        const HntrShape sh = hntr_shape(h, nvar, wta_is_const != 0, !wta_is_const && wta_ld != 0);
        *NV = sh.NV; *L = sh.L; *K = sh.K; *lds_bytes = (int64_t)sh.lds_bytes;
    });
}

// The host forms, after their checks: every plane is copied in its own width and packed on the device, regridded there, and B
// copied back.  WTA == nullptr: the constant weight.
static void hntr_regrid_from_host(const ibh_hntr *h, const void *WTA, int wta_type, int64_t wta_ld, double wta_const, const void *A,
                                  int a_type, int32_t nvar, int64_t lda, double *B, int64_t ldb, int mean_polar, double wtm, double wtb) {
    if (nvar == 0) return;
    const size_t nA = (size_t)h->imA * h->jmA, nB = (size_t)h->imB * h->jmB;
    const size_t sS = hntr_elem_size(a_type), sW = WTA ? hntr_elem_size(wta_type) : 0;
    const size_t nw = !WTA ? 0 : wta_ld ? (size_t)nvar : 1;
    DevBuf<uint8_t> dW(sW * nw * nA), dA(sS * (size_t)nvar * nA);
    DevBuf<double> dB((size_t)nvar * nB);
    if (WTA)
        IBH_HIP(hipMemcpy2DAsync(dW.p, sW * nA, WTA, sW * (size_t)(wta_ld ? wta_ld : (int64_t)nA), sW * nA, nw, hipMemcpyHostToDevice, nullptr));
    IBH_HIP(hipMemcpy2DAsync(dA.p, sS * nA, A, sS * (size_t)lda, sS * nA, (size_t)nvar, hipMemcpyHostToDevice, nullptr));
    hntr_regrid(h, WTA ? dW.p : nullptr, wta_type, wta_ld ? (int64_t)nA : 0, wta_const, dA.p, a_type, nvar, (int64_t)nA, dB.p, (int64_t)nB,
                mean_polar, wtm, wtb, nullptr);
    IBH_HIP(hipMemcpy2DAsync(B, sizeof(double) * (size_t)ldb, dB.p, sizeof(double) * nB, sizeof(double) * nB, (size_t)nvar,
                             hipMemcpyDeviceToHost, nullptr));
    IBH_HIP(hipStreamSynchronize(nullptr));
}

int ibh_hntr_regrid_typed_host(const ibh_hntr *h, const void *WTA, int wta_type, int64_t wta_ld, double wta_const, const void *A,
                               int a_type, int32_t nvar, int64_t lda, double *B, int64_t ldb, int mean_polar, double wtm, double wtb) {
    return guarded([&] {
        check_typed_args(h, WTA, wta_type, wta_ld, A, a_type, nvar, lda, B, ldb, mean_polar);
        hntr_regrid_from_host(h, WTA, wta_type, WTA ? wta_ld : 0, wta_const, A, a_type, nvar, lda, B, ldb, mean_polar, wtm, wtb);
    });
}

int ibh_hntr_regrid_host(const ibh_hntr *h, const double *WTA, int64_t wta_ld, const double *A, int32_t nvar, int64_t lda,
                         double *B, int64_t ldb, int mean_polar, double wtm, double wtb) {
    return guarded([&] {
        check_regrid_args(h, WTA, wta_ld, A, nvar, lda, B, ldb, mean_polar);
        hntr_regrid_from_host(h, WTA, IBH_HNTR_F64, wta_ld, 0., A, IBH_HNTR_F64, nvar, lda, B, ldb, mean_polar, wtm, wtb);
    });
}

int ibh_hntr_dxyp(int32_t im, int32_t jm, double *dxyp) {
    return guarded([&] {
        IBH_CHECK(dxyp != nullptr, "null output array");
        IBH_CHECK(im >= 1 && jm >= 1, "Hntr dxyp: im=%d jm=%d (both must be >= 1)", im, jm);
        hntr_dxyp(im, jm, dxyp);
    });
}

int ibh_hntr_triplets(const ibh_hntr *h, int kind, double eq_rad, const uint8_t *includeB, int64_t *n, int32_t *iB, int32_t *iA,
                      double *val) {
    return guarded([&] { hntr_triplets(h, kind, eq_rad, includeB, n, iB, iA, val); });
}

int ibh_hntr_matrix_d(const ibh_hntr *h, int kind, double eq_rad, const uint8_t *includeB, ibh_sparse_set *dimB, int tB,
                      ibh_sparse_set *dimA, int tA, int transpose, ibh_weighted **out) {
    return guarded([&] {
        if (out) *out = nullptr;
        hntr_matrix(h, kind, eq_rad, includeB, dimB, tB, dimA, tA, transpose, out);
    });
}

}  // extern "C"

extern "C" {

int ibh_weighted_make_I2vX(const ibh_weighted *IvX, const ibh_hntr *hIvI2, double eq_rad, const uint8_t *includeI, int64_t nincl,
                           ibh_sparse_set *dimI2, ibh_weighted **out) {
    return guarded([&] {
        if (out) *out = nullptr;
        make_i2vx(IvX, hIvI2, eq_rad, includeI, nincl, dimI2, out);
    });
}

int ibh_hntr_exgrid_count(const ibh_hntr_regridder_desc *desc, int64_t *nX) {
    return guarded([&] { hntr_exgrid_count(desc, nX); });
}

int ibh_regridder_create_hntr(const ibh_hntr_regridder_desc *desc, ibh_sparse_set *dimA_out, ibh_sparse_set *dimI_out,
                              ibh_regridder **out) {
    return guarded([&] {
        if (out) *out = nullptr;
        regridder_create_hntr(desc, dimA_out, dimI_out, out);
    });
}

}  // extern "C"
