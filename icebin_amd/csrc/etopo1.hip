// etopo1.hip -- modele/etopo1_ice.cpp's etopo1_ice (:45-247) from arrays: the global ice extent FGICE1m and the planes FOCEAN1m /
// ZICETOP1m / ZSOLG1m on the fine grid, and their regrids onto the h grid (store_h, :17-29); DESIGN.md 20.
//
// Where things live.  The three int16 input planes and the four int16 output planes stay in HBM in their own width.  Three
// launches, stream-ordered:
//   k_et_planes   every output cell from its own three input cells: fgice = 0 (:51-52), the 78N band (:84-93), the south
//                 (:109-117), Greenland in the elevations (:121-140) and the FOCEAN1m half of :212-224
//   k_et_tiles    one workgroup per coarse cell of the north half (:166-209): the tile's land cells as 32-bit keys in LDS, a
//                 bitonic sort, the fill chain walked by one wave in lockstep, the taken cells' flags stored
//   k_et_unice    the transposed zeroing of :222, after the tiles
// then the typed Hntr regrid once per output plane.  The row areas (make_dxyp, libm sin) are host tables uploaded by the
// handle, so a call only enqueues.  The 16-byte split of a plane, the eight-cell loads and stores, the LDS sort and the argument
// checks are planetile.h's, shared with globalec.hip and topoo.hip.
#include <algorithm>
#include <memory>
#include <vector>

#include "planetile.h"

struct ibh_etopo1_ice {
    int device = 0;
    int32_t imI = 0, jmI = 0, imC = 0, jmC = 0, mult_i = 0, mult_j = 0, imH = 0, jmH = 0;
    ibh::DevBuf<double> dxypI, dxypC;       // [jmI], [jmC]: make_dxyp with a 0-based row
    ibh_hntr *hntrH = nullptr;              // Hntr(17.17, hspecH, hspecI); null: no h planes
    int64_t nI() const { return (int64_t)imI * jmI; }
    int64_t nH() const { return (int64_t)imH * jmH; }
    ~ibh_etopo1_ice() { if (hntrH) ibh_hntr_destroy(hntrH); }
};

namespace ibh {
namespace {

constexpr int ET_T = 256;
constexpr int16_t ET_GREENLAND = 2;         // GREENLAND_VAL (:14)
constexpr int ET_MIN_THK = 50;              // MIN_LANDICE_THK (:15)
constexpr int16_t ET_NO_GREENLAND = -300;   // :136-137

struct EtCell {
    int16_t fo, fg, zt, zs;
};
// one cell of :51-140 and of the FOCEAN1m half of :212-224; j is the cell's row
__device__ __forceinline__ EtCell et_cell(int fo, int zt, int zs, int j, int jband, int jhalf, int incl) {
    EtCell o{(int16_t)fo, 0, (int16_t)zt, (int16_t)zs};
    const bool thick = zt - zs >= ET_MIN_THK;       // in int (:113, :126)
    if (j >= jband && fo == 0) o.fg = 1;
    if (j < jhalf) {
        if (fo == 0 && thick) o.fg = 1;
    } else if (fo == ET_GREENLAND) {
        if (incl) {
            if (thick) o.fg = 1;
            o.fo = 0;
        } else {
            o.zt = ET_NO_GREENLAND; o.zs = ET_NO_GREENLAND;
            o.fo = 1;
        }
    }
    return o;
}

struct EtPlanes {
    const int16_t *fo, *zt, *zs;        // FOCEAN, ZICTOP, ZSOLID
    int16_t *ofo, *ofg, *ozt, *ozs;     // FOCEAN1m, FGICE1m, ZICETOP1m, ZSOLG1m
};

// The flat plane in 16-byte pieces (8 cells) between a head and a tail of fewer than 8 cells each, which go one cell a thread
// (S: FOCEAN's PlaneSplit).  The head is where FOCEAN becomes 16-byte aligned; avec bit p says that plane p (ZICTOP, ZSOLID, then
// the four outputs) is aligned there too, else its eight cells go one by one.  A piece may straddle rows: the row is carried
// along its cells.
__global__ __launch_bounds__(ET_T) void k_et_planes(EtPlanes P, unsigned nI, unsigned imI, int jband, int jhalf, int incl, PlaneSplit S,
                                                    unsigned avec) {
    const unsigned g = blockIdx.x * (unsigned)ET_T + threadIdx.x;
    if (g < S.nloose(nI)) {
        const unsigned x = S.cell(g);
        const EtCell o = et_cell(P.fo[x], P.zt[x], P.zs[x], (int)(x / imI), jband, jhalf, incl);
        P.ofo[x] = o.fo; P.ofg[x] = o.fg; P.ozt[x] = o.zt; P.ozs[x] = o.zs;
    }
    if (g >= S.npiece) return;
    const unsigned x0 = S.piece(g);
    const short8 fo = load8(P.fo + x0, true);
    const short8 zt = load8(P.zt + x0, avec & 1u), zs = load8(P.zs + x0, avec & 2u);
    unsigned j = x0 / imI, rem = x0 - j * imI;
    short8 ofo, ofg, ozt, ozs;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const EtCell o = et_cell(fo[k], zt[k], zs[k], (int)j, jband, jhalf, incl);
        ofo[k] = o.fo; ofg[k] = o.fg; ozt[k] = o.zt; ozs[k] = o.zs;
        if (++rem == imI) { rem = 0; ++j; }
    }
    store8(P.ofo + x0, ofo, avec & 4u); store8(P.ofg + x0, ofg, avec & 8u);
    store8(P.ozt + x0, ozt, avec & 16u); store8(P.ozs + x0, ozs, avec & 32u);
}

// ---- the downscaled ice fraction (:166-209) ----------------------------------------------------------------------------------------
// Workgroup b owns coarse cell (j1, i1) = (jC0 + b / imC, b % imC) and leaves at once when its fraction is 0 (:172).  A land
// cell (FOCEAN == 0; the Greenland clause of :179 is never true) becomes the key (32767 - ZICTOP) << 16 | local index, local =
// (j - j0) * mult_i + (i - i0): ascending keys are the reference's (-elev, j1m, i1m) order, the negation taken in int.  The keys
// are appended in any order (an LDS counter) and sorted by planetile.h's lds_sort_keys -- no key is ~0, its padding: a tile has
// fewer than 65536 cells.  Wave 0 then walks the chain of :190-207 in lockstep: 64 areas a step are fetched
// one a lane, broadcast lane by lane, and every lane carries the same `remain`, so the subtractions are the reference's, in its
// order; a cell is a compare and two selects, without a branch (the chain is the critical path: :190-207 once per tile).  The cells taken are the first ntake of the sorted keys; the workgroup stores their flags.
__global__ __launch_bounds__(ET_T) void k_et_tiles(const int16_t *__restrict__ fo, const int16_t *__restrict__ zt, const double *__restrict__ fgiceC,
                                                   const double *__restrict__ dxypI, const double *__restrict__ dxypC, int imI, int imC, int mult_i,
                                                   int mult_j, int jC0, int16_t *__restrict__ ofg) {
    extern __shared__ uint32_t s_key[];
    __shared__ int s_n, s_take;
    const int tid = threadIdx.x;
    const int j1 = jC0 + (int)(blockIdx.x / (unsigned)imC), i1 = (int)(blockIdx.x % (unsigned)imC);
    const double snow1 = fgiceC[(size_t)j1 * imC + i1];
    if (snow1 == 0) return;         // (uniform: the whole workgroup leaves)
    if (tid == 0) { s_n = 0; s_take = 0; }
    __syncthreads();
    const int ncell = mult_i * mult_j;
    const size_t base = (size_t)j1 * mult_j * (size_t)imI + (size_t)i1 * mult_i;
    for (int c = tid; c < ncell; c += ET_T) {
        const int r = c / mult_i;
        const size_t x = base + (size_t)r * imI + (size_t)(c - r * mult_i);
        if (fo[x] == 0) s_key[atomicAdd(&s_n, 1)] = (uint32_t)(32767 - (int)zt[x]) << 16 | (uint32_t)c;
    }
    __syncthreads();
    const int n = s_n;
    if (n == 0) return;             // :185
    lds_sort_keys<ET_T>(s_key, n, tid);
    if (tid < 64) {
        double remain = snow1 * dxypC[j1];      // :188
        const size_t jrow0 = (size_t)j1 * mult_j;
        int ntake = 0;
        bool alive = true;          // no cell has failed `area <= remain` yet
        // one cell of :196-206 without a branch: every lane holds the same values, and a lane that has stopped takes nothing
        auto step = [&](double area) {
            const bool le = alive && area <= remain;
            const bool rounded = alive && !le && remain >= area * .5;
            remain = le ? remain - area : remain;
            ntake += (le || rounded) ? 1 : 0;
            alive = le;
        };
        // lane l's area of sorted cell b + l; the next step's areas are asked for before this step's are walked
        auto area_of = [&](int b) { return b + tid < n ? dxypI[jrow0 + (size_t)((int)(s_key[b + tid] & 0xFFFFu) / mult_i)] : 0.; };
        double next = area_of(0);
        for (int b0 = 0; b0 < n; b0 += 64) {
            const double mine = next;
            next = area_of(b0 + 64);
            if (n - b0 >= 64) {
#pragma unroll
                for (int t = 0; t < 64; ++t) step(lane_bcast(mine, t));
            } else {
                for (int t = 0; t < n - b0; ++t) step(lane_bcast(mine, t));
            }
            if (!__builtin_amdgcn_readfirstlane((int)alive)) break;
        }
        if (tid == 0) s_take = ntake;
    }
    __syncthreads();
    const int ntake = s_take;
    for (int k = tid; k < ntake; k += ET_T) {
        const int c = (int)(s_key[k] & 0xFFFFu), r = c / mult_i;
        ofg[base + (size_t)r * imI + (size_t)(c - r * mult_i)] = 1;
    }
}

// ---- :212-224, the fgice half -------------------------------------------------------------------------------------------------
// Every Greenland cell (j, i) of the north half looks at the TRANSPOSED cell (r, c) = (i, j) of the ocean mask the reference's loop
// is rewriting in place: the new value g where that cell is Greenland of the north half itself and the loop has been there
// (i <= j, row-major), the input value elsewhere; where it reads 1 the transposed cell loses its ice.  (j, i) -> (i, j) is a
// bijection, so no two threads write one cell.  Outside the plane (i >= jmI or j >= imI) the reference's index leaves the array;
// nothing is read or written there.
// the check of one Greenland cell, x its flat index
__device__ __forceinline__ void et_unice_cell(const int16_t *__restrict__ fo, unsigned x, int imI, int jmI, int jhalf, int incl,
                                              int16_t *__restrict__ ofg) {
    const int j = (int)(x / (unsigned)imI), i = (int)(x - (unsigned)j * (unsigned)imI);
    if (i >= jmI || j >= imI) return;
    const size_t t = (size_t)i * imI + j;
    int v = fo[t];
    if (v == ET_GREENLAND && i >= jhalf && i <= j) v = incl ? 0 : 1;
    if (v == 1) ofg[t] = 0;
}
// The north half [x0, nI) of the flat ocean mask in 16-byte pieces between a head and a tail of fewer than 8 cells (S: the
// PlaneSplit of the nI - x0 cells from fo + x0), as k_et_planes reads it; few pieces hold a Greenland cell.
__global__ __launch_bounds__(ET_T) void k_et_unice(const int16_t *__restrict__ fo, unsigned nI, int imI, int jmI, int jhalf, int incl, unsigned x0,
                                                   PlaneSplit S, int16_t *__restrict__ ofg) {
    const unsigned g = blockIdx.x * (unsigned)ET_T + threadIdx.x;
    if (g < S.nloose(nI - x0)) {
        const unsigned x = x0 + S.cell(g);
        if (fo[x] == ET_GREENLAND) et_unice_cell(fo, x, imI, jmI, jhalf, incl, ofg);
    }
    if (g >= S.npiece) return;
    const unsigned xp = x0 + S.piece(g);
    const short8 v = load8(fo + xp, true);
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (v[k] == ET_GREENLAND) et_unice_cell(fo, xp + (unsigned)k, imI, jmI, jhalf, incl, ofg);
}

// NULL planes, alignment, an output over an input or another output: all before a device is touched
void check_planes(const ibh_etopo1_ice *h, const void *focean, const void *zictop, const void *zsolid, const void *fgiceC, const void *oFO,
                  const void *oFG, const void *oZT, const void *oZS, const void *planes_h, int64_t ldh) {
    IBH_CHECK(h, "etopo1_ice: null handle");
    const size_t pb = sizeof(int16_t) * (size_t)h->nI();
    IBH_CHECK(planes_h == nullptr || h->hntrH, "etopo1_ice: h planes asked for, the handle was made without hspecH");
    IBH_CHECK(planes_h == nullptr || ldh >= h->nH(), "etopo1_ice: ldh=%lld < %lld cells of hspecH", (long long)ldh, (long long)h->nH());
    const PlaneArg a[] = {{focean, pb, "focean", 2, false, false}, {zictop, pb, "zictop", 2, false, false}, {zsolid, pb, "zsolid", 2, false, false},
                          {fgiceC, sizeof(double) * (size_t)h->imC * h->jmC, "fgiceC", 8, false, false},
                          {oFO, pb, "FOCEAN1m", 2, true, false}, {oFG, pb, "FGICE1m", 2, true, false}, {oZT, pb, "ZICETOP1m", 2, true, false},
                          {oZS, pb, "ZSOLG1m", 2, true, false},
                          {planes_h, planes_h ? sizeof(double) * (size_t)(3 * ldh + h->nH()) : 0, "the h planes", 8, true, true}};
    check_plane_args("etopo1_ice", a, (int)(sizeof(a) / sizeof(a[0])));
}

// the enqueue proper; every pointer is a device pointer
void run_device(const ibh_etopo1_ice *h, const int16_t *fo, const int16_t *zt, const int16_t *zs, const double *fgiceC, int incl, int16_t *oFO,
                int16_t *oFG, int16_t *oZT, int16_t *oZS, double *planes_h, int64_t ldh, hipStream_t st) {
    const unsigned nI = (unsigned)h->nI();
    const int jband = (int)(((int64_t)h->jmI * 14) / 15), jhalf = h->jmI / 2;
    {
        const PlaneSplit S = plane_split(fo, nI);
        const void *others[6] = {zt, zs, oFO, oFG, oZT, oZS};
        unsigned avec = 0;
        for (int k = 0; k < 6; ++k)
            if ((((uintptr_t)others[k] + 2 * (uintptr_t)S.head) & 15) == 0) avec |= 1u << k;
        const long nthread = std::max<long>(S.npiece, S.nloose(nI));
        const EtPlanes P{fo, zt, zs, oFO, oFG, oZT, oZS};
        hipLaunchKernelGGL(k_et_planes, dim3((unsigned)cdiv(nthread, ET_T)), dim3(ET_T), 0, st, P, nI,
                           (unsigned)h->imI, jband, jhalf, incl, S, avec);
    }
    const int jC0 = h->jmC / 2;
    if (h->jmC > jC0) {
        const int n2 = pow2_ceil(h->mult_i * h->mult_j);
        hipLaunchKernelGGL(k_et_tiles, dim3((unsigned)(h->jmC - jC0) * (unsigned)h->imC), dim3(ET_T), sizeof(uint32_t) * (size_t)n2, st, fo, zt, fgiceC,
                           h->dxypI.p, h->dxypC.p, h->imI, h->imC, h->mult_i, h->mult_j, jC0, oFG);
    }
    if (h->jmI > jhalf) {
        const unsigned x0 = (unsigned)jhalf * (unsigned)h->imI, nN = nI - x0;
        const PlaneSplit S = plane_split(fo + x0, nN);
        const long nthread = std::max<long>(S.npiece, S.nloose(nN));
        hipLaunchKernelGGL(k_et_unice, dim3((unsigned)cdiv(nthread, ET_T)), dim3(ET_T), 0, st, fo, nI, h->imI, h->jmI, jhalf, incl, x0, S, oFG);
    }
    IBH_HIP(hipGetLastError());
    if (planes_h) {     // store_h (:17-29), in the reference's plane order of this library's outputs
        const int16_t *src[4] = {oFO, oFG, oZT, oZS};
        for (int k = 0; k < 4; ++k)
            rethrow(ibh_hntr_regrid_typed_device(h->hntrH, nullptr, IBH_HNTR_F64, 0, 1.0, src[k], IBH_HNTR_I16, 1, h->nI(), planes_h + (size_t)k * ldh,
                                                 h->nH(), 1, 1., 0., st));
    }
}

}  // namespace
}  // namespace ibh

using namespace ibh;
extern "C" {

int ibh_etopo1_ice_create(ibh_etopo1_ice **out, int32_t imI, int32_t jmI, double offiI, double dlatI, int32_t imC, int32_t jmC, int32_t imH,
                          int32_t jmH, double offiH, double dlatH) {
    if (out) *out = nullptr;
    return guarded([&] {
        IBH_CHECK(out, "out: null argument");
        IBH_CHECK(imI > 0 && jmI > 0 && imC > 0 && jmC > 0, "hspecI / hspecC: grid sizes (%dx%d), (%dx%d) must be positive", imI, jmI, imC, jmC);
        IBH_CHECK(imI % imC == 0 && jmI % jmC == 0, "hspecI: the fine grid (%dx%d) must be an even multiple of the coarse grid (%dx%d)", imI, jmI,
                  imC, jmC);
        IBH_CHECK((int64_t)imI * jmI < (1ll << 31), "hspecI: %lld cells overflow int32", (long long)imI * jmI);
        const int64_t tile = (int64_t)(imI / imC) * (jmI / jmC);
        IBH_CHECK(tile <= IBH_ETOPO1_MAX_TILE, "hspecI / hspecC: a coarse cell holds %lld fine cells (%dx%d), the limit is %d", (long long)tile,
                  imI / imC, jmI / jmC, IBH_ETOPO1_MAX_TILE);
        IBH_CHECK((imH == 0) == (jmH == 0), "hspecH: (%dx%d); give both sizes, or 0 and 0 for no h planes", imH, jmH);
        IBH_CHECK(imH == 0 || jmH >= 2, "hspecH: jm=%d; store_h's mean_polar needs at least two rows", jmH);
        std::unique_ptr<ibh_etopo1_ice> h(new ibh_etopo1_ice);
        h->imI = imI; h->jmI = jmI; h->imC = imC; h->jmC = jmC; h->mult_i = imI / imC; h->mult_j = jmI / jmC; h->imH = imH; h->jmH = jmH;
        const std::vector<double> dI = dxyp_rows(imI, jmI), dC = dxyp_rows(imC, jmC);
        // the regridder of store_h checks its grids on the host before it looks for a device
        if (imH) rethrow(ibh_hntr_create(&h->hntrH, imI, jmI, offiI, dlatI, imH, jmH, offiH, dlatH, 0.));
        require_device();
        IBH_HIP(hipGetDevice(&h->device));
        h->dxypI.upload(dI.data(), dI.size(), hipStreamPerThread);
        h->dxypC.upload(dC.data(), dC.size(), hipStreamPerThread);
        IBH_HIP(hipStreamSynchronize(hipStreamPerThread));
        *out = h.release();
    });
}

int ibh_etopo1_ice_destroy(ibh_etopo1_ice *h) {
    return guarded([&] { delete h; });
}

int ibh_etopo1_ice_device(const ibh_etopo1_ice *h, const int16_t *d_focean, const int16_t *d_zictop, const int16_t *d_zsolid, const double *d_fgiceC,
                          int include_greenland, int16_t *d_FOCEAN1m, int16_t *d_FGICE1m, int16_t *d_ZICETOP1m, int16_t *d_ZSOLG1m, double *d_planes_h,
                          int64_t ldh, void *stream) {
    return guarded([&] {
        check_planes(h, d_focean, d_zictop, d_zsolid, d_fgiceC, d_FOCEAN1m, d_FGICE1m, d_ZICETOP1m, d_ZSOLG1m, d_planes_h, ldh);
        check_current_device(h->device, "etopo1_ice handle");
        run_device(h, d_focean, d_zictop, d_zsolid, d_fgiceC, include_greenland != 0, d_FOCEAN1m, d_FGICE1m, d_ZICETOP1m, d_ZSOLG1m, d_planes_h, ldh,
                   (hipStream_t)stream);
    });
}

int ibh_etopo1_ice_host(const ibh_etopo1_ice *h, const int16_t *focean, const int16_t *zictop, const int16_t *zsolid, const double *fgiceC,
                        int include_greenland, int16_t *FOCEAN1m, int16_t *FGICE1m, int16_t *ZICETOP1m, int16_t *ZSOLG1m, double *planes_h,
                        int64_t ldh) {
    return guarded([&] {
        check_planes(h, focean, zictop, zsolid, fgiceC, FOCEAN1m, FGICE1m, ZICETOP1m, ZSOLG1m, planes_h, ldh);
        check_current_device(h->device, "etopo1_ice handle");
        hipStream_t st = hipStreamPerThread;
        const size_t nI = (size_t)h->nI(), nH = (size_t)h->nH();
        DevBuf<int16_t> in[3], o[4];
        const int16_t *src[3] = {focean, zictop, zsolid};
        for (int k = 0; k < 3; ++k) in[k].upload(src[k], nI, st);
        DevBuf<double> fC, dh;
        fC.upload(fgiceC, (size_t)h->imC * h->jmC, st);
        for (int k = 0; k < 4; ++k) o[k].alloc(nI);
        if (planes_h) dh.alloc(4 * nH);
        run_device(h, in[0].p, in[1].p, in[2].p, fC.p, include_greenland != 0, o[0].p, o[1].p, o[2].p, o[3].p, planes_h ? dh.p : nullptr, (int64_t)nH, st);
        int16_t *dst[4] = {FOCEAN1m, FGICE1m, ZICETOP1m, ZSOLG1m};
        for (int k = 0; k < 4; ++k) IBH_HIP(hipMemcpyAsync(dst[k], o[k].p, sizeof(int16_t) * nI, hipMemcpyDeviceToHost, st));
        if (planes_h)
            IBH_HIP(hipMemcpy2DAsync(planes_h, sizeof(double) * (size_t)ldh, dh.p, sizeof(double) * nH, sizeof(double) * nH, 4, hipMemcpyDeviceToHost, st));
        IBH_HIP(hipStreamSynchronize(st));
    });
}

}  // extern "C"
