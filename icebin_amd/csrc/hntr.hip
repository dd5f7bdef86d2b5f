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
#include <algorithm>
#include <cmath>
#include <memory>

#include "common.h"

namespace ibh {

void require_device();      // capi.hip

constexpr int HNTR_LDS = 5056;      // most doubles of LDS per workgroup: with the row windows, 40 KiB (four workgroups per CU)
constexpr int HNTR_LDS_SMALL = 2496;    // the same for 20 KiB (eight workgroups per CU)
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
    const double *WTA;
    int64_t wta_ld;         // 0: one WTA plane shared by all fields
    const double *A;
    int64_t lda;
    double *B;
    int64_t ldb;
    int imA, imB, jmB, nvar;
    int L, K, S;            // chain lanes per wave, columns per chunk, LDS row stride (odd, >= K)
    double wtm, wtb, datmis;
};

// One wave per workgroup: column IB = blockIdx.x % imB, rows jb0 .. jb0+L-1, fields NV*blockIdx.y .. (at most NV).
// A shared weight feeds the NV VALUE chains from one wt / WEIGHT chain; per-field weights run with NV = 1.
template <int NV>
__global__ __launch_bounds__(64) void hntr_regrid_kernel(HntrArgs a) {
    constexpr int P = 1 + NV;                       // staged planes: WTA, then the fields
    constexpr int U = HNTR_STAGE / P > 1 ? HNTR_STAGE / P : 1;    // staged items per lane in flight
    extern __shared__ double lds[];                 // [P][L][S], L*S*P <= HNTR_LDS
    __shared__ int sj0[64], sj1[64];

    const int lane = threadIdx.x;
    const int ib = blockIdx.x % a.imB;
    const int jb0 = (blockIdx.x / a.imB) * a.L;
    const int f0 = blockIdx.y * NV;
    const int nv = min(NV, a.nvar - f0);
    const double *__restrict__ W = a.wta_ld ? a.WTA + (int64_t)f0 * a.wta_ld : a.WTA;
    const double *__restrict__ Af = a.A + (int64_t)f0 * a.lda;
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
                        v[u][0] = W[off[u]];
#pragma unroll
                        for (int f = 0; f < NV; ++f)
                            if (f < nv) v[u][1 + f] = Af[(int64_t)f * a.lda + off[u]];
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (off[u] >= 0) {
#pragma unroll
                        for (int p = 0; p < P; ++p)
                            if (p <= nv) lds[p * plane + dst[u]] = v[u][p];
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
                    const double wta = a.wtm * row[kk] + a.wtb;
                    const double wt = FG * wta;
                    WEIGHT += wt;
#pragma unroll
                    for (int f = 0; f < NV; ++f)
                        if (f < nv) VALUE[f] += wt * row[(1 + f) * plane + kk];
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
    double datmis;
    int device = 0, ncu = 256;
    int wmax = 1;       // widest column window
    DevBuf<double> SINA, FMIN, FMAX, GMIN, GMAX;
    DevBuf<int32_t> IMIN, IMAX, JMIN, JMAX;
};

namespace ibh {

template <int NV>
static void hntr_launch_nv(const ibh_hntr *h, HntrArgs a, hipStream_t s) {
    const int P = 1 + NV;
    const int ngroups = (a.nvar + NV - 1) / NV;
    // lanes per wave: all 64 when there are B cells enough for four waves per CU, fewer (more workgroups, so more
    // CUs streaming at once) for small B grids
    int L = 64;
    while (L > 1 && (int64_t)ceil_div(h->jmB, L) * h->imB * ngroups < 4 * (int64_t)h->ncu) L >>= 1;
    if (L > h->jmB) { L = 1; while (L < h->jmB) L <<= 1; }
    // LDS per workgroup: 20 KiB (eight one-wave workgroups per CU) while that still leaves chunks of 16 columns, else up
    // to 40 KiB.  Measured from a 1' field: one field 1.38 ms at 20 KiB against 1.79 ms at 40 KiB (1/2 deg); eight fields,
    // whose chunks would shrink to 3 columns at 20 KiB, 9.2 ms at 40 KiB against 15.3 ms.
    int smax = HNTR_LDS_SMALL / (L * P);
    if (smax < std::min(h->wmax, 16)) smax = HNTR_LDS / (L * P);
    if (!(smax & 1)) --smax;
    const int K = std::min(h->wmax, smax);
    a.L = L; a.K = K; a.S = K | 1;
    dim3 grid((unsigned)(ceil_div(h->jmB, L) * h->imB), (unsigned)ngroups);
    hipLaunchKernelGGL(hntr_regrid_kernel<NV>, grid, dim3(64), (size_t)L * a.S * P * sizeof(double), s, a);
    IBH_HIP(hipGetLastError());
}

static void hntr_regrid(const ibh_hntr *h, const double *dWTA, int64_t wta_ld, const double *dA, int32_t nvar, int64_t lda,
                        double *dB, int64_t ldb, int mean_polar, double wtm, double wtb, hipStream_t s) {
    HntrArgs a{};
    a.SINA = h->SINA.p; a.FMIN = h->FMIN.p; a.FMAX = h->FMAX.p; a.GMIN = h->GMIN.p; a.GMAX = h->GMAX.p;
    a.IMIN = h->IMIN.p; a.IMAX = h->IMAX.p; a.JMIN = h->JMIN.p; a.JMAX = h->JMAX.p;
    a.WTA = dWTA; a.wta_ld = wta_ld; a.A = dA; a.lda = lda; a.B = dB; a.ldb = ldb;
    a.imA = h->imA; a.imB = h->imB; a.jmB = h->jmB; a.nvar = nvar;
    a.wtm = wtm; a.wtb = wtb; a.datmis = h->datmis;
    if (wta_ld != 0 || nvar == 1) hntr_launch_nv<1>(h, a, s);
    else if (nvar == 2) hntr_launch_nv<2>(h, a, s);
    else if (nvar <= 4) hntr_launch_nv<4>(h, a, s);
    else hntr_launch_nv<8>(h, a, s);
    if (mean_polar) {
        hipLaunchKernelGGL(hntr_mean_polar_kernel, dim3((unsigned)ceil_div(2 * (int64_t)nvar, 64)), dim3(64), 0, s,
                           dB, ldb, nvar, h->imB, h->jmB, h->datmis);
        IBH_HIP(hipGetLastError());
    }
}

static void check_regrid_args(const ibh_hntr *h, const void *WTA, int64_t wta_ld, const void *A, int32_t nvar, int64_t lda,
                              const void *B, int64_t ldb, int mean_polar) {
    IBH_CHECK(h != nullptr, "null Hntr handle");
    int dev = -1;
    IBH_HIP(hipGetDevice(&dev));
    IBH_CHECK(dev == h->device, "Hntr handle belongs to device %d, current device is %d", h->device, dev);
    const int64_t nA = (int64_t)h->imA * h->jmA, nB = (int64_t)h->imB * h->jmB;
    IBH_CHECK(nvar >= 0 && (nvar == 0 || (WTA && A && B)), "Hntr regrid: bad arguments (nvar=%d or a null array)", nvar);
    IBH_CHECK(lda >= nA && ldb >= nB, "Hntr regrid: leading dimensions too small (lda=%lld < %lld or ldb=%lld < %lld)",
              (long long)lda, (long long)nA, (long long)ldb, (long long)nB);
    IBH_CHECK(wta_ld == 0 || wta_ld >= nA, "Hntr regrid: wta_ld=%lld must be 0 (shared weight) or >= %lld", (long long)wta_ld,
              (long long)nA);
    IBH_CHECK(!mean_polar || h->jmB >= 2, "Hntr regrid: mean_polar needs jmB >= 2 (the reference loops forever on jmB=1)");
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
        hntr_regrid(h, dWTA, wta_ld, dA, nvar, lda, dB, ldb, mean_polar, wtm, wtb, static_cast<hipStream_t>(stream));
    });
}

int ibh_hntr_regrid_host(const ibh_hntr *h, const double *WTA, int64_t wta_ld, const double *A, int32_t nvar, int64_t lda,
                         double *B, int64_t ldb, int mean_polar, double wtm, double wtb) {
    return guarded([&] {
        check_regrid_args(h, WTA, wta_ld, A, nvar, lda, B, ldb, mean_polar);
        if (nvar == 0) return;
        const size_t nA = (size_t)h->imA * h->jmA, nB = (size_t)h->imB * h->jmB;
        const size_t nw = wta_ld ? (size_t)nvar : 1;
        DevBuf<double> dW(nw * nA), dA((size_t)nvar * nA), dB((size_t)nvar * nB);
        IBH_HIP(hipMemcpy2DAsync(dW.p, sizeof(double) * nA, WTA, sizeof(double) * (size_t)(wta_ld ? wta_ld : (int64_t)nA),
                                 sizeof(double) * nA, nw, hipMemcpyHostToDevice, nullptr));
        IBH_HIP(hipMemcpy2DAsync(dA.p, sizeof(double) * nA, A, sizeof(double) * (size_t)lda, sizeof(double) * nA, (size_t)nvar,
                                 hipMemcpyHostToDevice, nullptr));
        hntr_regrid(h, dW.p, wta_ld ? (int64_t)nA : 0, dA.p, nvar, (int64_t)nA, dB.p, (int64_t)nB, mean_polar, wtm, wtb, nullptr);
        IBH_HIP(hipMemcpy2DAsync(B, sizeof(double) * (size_t)ldb, dB.p, sizeof(double) * nB, sizeof(double) * nB, (size_t)nvar,
                                 hipMemcpyDeviceToHost, nullptr));
        IBH_HIP(hipStreamSynchronize(nullptr));
    });
}

}  // extern "C"
