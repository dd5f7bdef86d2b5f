// l1.hip -- L1 ice grids: a triangle mesh with piecewise-linear fields (GridParameterization::L1, ISSM) under convex GCM cells.
//
// Three pieces, all on the device:
//  * the exchange grid of a mesh: make_exchange_grid (slib/icebin/gridgen/GridGen_Exchange.cpp:175-284) with triangles in the
//    place of the rectilinear ice cells of gridgen.hip.  The reference pairs cells through an RTree and intersects with CGAL;
//    here the polygons' bounding boxes are binned into a uniform grid (count, scan, fill), one lane per triangle visits the
//    bins its own bounding box covers, takes every candidate polygon once and clips the triangle against the polygon's
//    half-planes (Sutherland-Hodgman), in the frame of the triangle's vertex 0.  Two passes (count, emit): the records come
//    out in ascending triangle order and a stable sort by (iA, iTri) -- prims' radix sort -- gives ExchangeGrid's order
//    (AbbrGrid.cpp:10-21).  The bin lists are filled with integer atomics: the order inside a list decides the order a
//    triangle emits its pieces in, and the sort key (iA, iTri) is unique, so nothing of it survives.
//  * the basis integrals: integrate_subelement (pylib/icebin/element_l1.py:27-93) for the three basis functions of the
//    cell's element over its exchange polygon.  The reference solves a 3x3 system in absolute coordinates per basis function and
//    sums cubic boundary terms; here the barycentric coefficients come from the element's edge cross products in the frame of
//    its vertex 0 and the polygon is fanned from its vertex 0: fan-triangle area x mean of the (linear) basis function at its
//    three corners, which is exact for a linear integrand.  Plain + - * / in a fixed order (the unit is compiled without
//    contraction): tests/l1_restatement.py states the same arithmetic in numpy, bit for bit.
//  * the matrix: compute_AvI (element_l1.py:96-148).  Three triplets per exchange cell stay on the device and go through the
//    triplets -> CSR layer's setFromTriplets (weighted_from_device_triplets): duplicates summed in stream order with the first term assigned,
//    wM / Mw in the canonical order.
#include "csrbuild.h"
#include "csrops.h"
#include "prims.h"

namespace ibh {
constexpr int L1_MAXV = 16;              // vertices of a GCM-cell polygon
constexpr int L1_CLIPV = L1_MAXV + 3;    // vertices of an exchange polygon: a triangle gains at most one per half-plane
constexpr int L1_LANES = 64;             // lanes of a clip block: one wave, 2 x 2 x L1_CLIPV doubles of LDS per lane
constexpr int L1_MAXBINS = 1024;         // bins per axis
}  // namespace ibh

struct ibh_l1_mesh {
    int32_t nvert = 0, ntri = 0;
    ibh::DevBuf<double> vx, vy;          // [nvert]
    ibh::DevBuf<int32_t> tri;            // [3*ntri] counter-clockwise
};
struct ibh_l1_exgrid {
    int64_t nX = 0, nq = 0;
    int64_t iA_extent = 0, iTri_extent = 0;     // one past the largest index of either kind
    ibh::DevBuf<int32_t> indices;        // [2*nX] interleaved (iA, iTri), sorted by (iA, iTri)
    ibh::DevBuf<double> area;            // [nX]
    ibh::DevBuf<int32_t> vptr;           // [nX+1]
    ibh::DevBuf<double> qx, qy;          // [nq] polygon vertices, counter-clockwise
};

namespace ibh {

// ---- mesh ---------------------------------------------------------------------------------------------------------------
__global__ void k_l1_check_mesh(const double *__restrict__ vx, const double *__restrict__ vy, const int32_t *__restrict__ tri,
                                int nvert, int ntri, uint32_t *__restrict__ first_bad) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntri) return;
    const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    bool ok = a >= 0 && a < nvert && b >= 0 && b < nvert && c >= 0 && c < nvert;
    if (ok) {
        const double e1x = vx[b] - vx[a], e1y = vy[b] - vy[a], e2x = vx[c] - vx[a], e2y = vy[c] - vy[a];
        ok = e1x * e2y - e1y * e2x > 0;          // false for NaN as well
    }
    if (!ok) atomicMin(first_bad, (uint32_t)t);  // an integer minimum: the same element whatever the order
}

static void l1_mesh_create(int32_t nvert, const double *vx, const double *vy, int32_t ntri, const int32_t *tri, ibh_l1_mesh **out) {
    IBH_CHECK(out != nullptr, "null argument");
    IBH_CHECK(nvert >= 0 && ntri >= 0 && (int64_t)ntri * 3 < (1ll << 31), "L1 mesh: bad sizes nvert=%d ntri=%d", nvert, ntri);
    IBH_CHECK((nvert == 0 || (vx && vy)) && (ntri == 0 || tri), "L1 mesh: null arrays");
    require_device();
    hipStream_t st = nullptr;
    std::unique_ptr<ibh_l1_mesh> m(new ibh_l1_mesh);
    m->nvert = nvert; m->ntri = ntri;
    m->vx.upload(vx, (size_t)nvert, st); m->vy.upload(vy, (size_t)nvert, st); m->tri.upload(tri, 3 * (size_t)ntri, st);
    if (ntri) {
        Arena &A = arena();
        A.reset();
        uint32_t *bad = A.get<uint32_t>(1);
        IBH_HIP(hipMemsetAsync(bad, 0xFF, sizeof(uint32_t), st));
        hipLaunchKernelGGL(k_l1_check_mesh, dim3(ceil_div(ntri, 256)), dim3(256), 0, st, m->vx.p, m->vy.p, m->tri.p, nvert, ntri, bad);
        IBH_HIP(hipGetLastError());
        uint32_t h = 0;
        readback_sync(&h, bad, sizeof(h), st);
        if (h != 0xFFFFFFFFu) {
            const int32_t *v = tri + 3 * (size_t)h;
            for (int k = 0; k < 3; ++k)
                IBH_CHECK(v[k] >= 0 && v[k] < nvert, "L1 mesh: element %u names vertex %d, outside [0, %d)", h, v[k], nvert);
            fail(IBH_EINVAL, "L1 mesh: element %u (vertices %d, %d, %d) is not counter-clockwise with positive area", h, v[0], v[1], v[2]);
        }
    }
    IBH_HIP(hipStreamSynchronize(st));
    *out = m.release();
}

// ---- polygon area -------------------------------------------------------------------------------------------------------
// Cell::proj_area (Grid.cpp:42-70) as gridgen.hip sums it, with the polygon's vertex 0 as the origin: in absolute
// coordinates the products lose the area of a cell far from the origin (polar-stereographic metres).  q: stride-s arrays.
template <class P>
__device__ __forceinline__ double l1_area(P qx, P qy, int n, int s) {
    const double ox = qx[0], oy = qy[0];
    double ret = 0;
    double x0 = qx[(n - 1) * s] - ox, y0 = qy[(n - 1) * s] - oy;
    for (int k = 0; k < n; ++k) {
        const double x1 = qx[k * s] - ox, y1 = qy[k * s] - oy;
        ret += (x0 * y1) - (x1 * y0);
        x0 = x1; y0 = y1;
    }
    return ret * .5;
}

// ---- candidate search: the polygons' bounding boxes in a uniform grid of bins ------------------------------------------------
struct L1Bins {
    double x0, y0, x1, y1;       // bounding box of all polygons
    double sx, sy;               // bins per unit length
    int nbx, nby;
};
__device__ __forceinline__ int l1_bin(double v, double lo, double scale, int nb) {
    const double f = (v - lo) * scale;
    int b = f > 0 ? (f < (double)nb ? (int)f : nb - 1) : 0;       // NaN -> 0
    return b;
}
struct L1Box { double xmin, ymin, xmax, ymax; };
struct L1BinRange { int bx0, bx1, by0, by1; };
__device__ __forceinline__ L1BinRange l1_bin_range(const L1Bins &g, const L1Box &b) {
    return L1BinRange{l1_bin(b.xmin, g.x0, g.sx, g.nbx), l1_bin(b.xmax, g.x0, g.sx, g.nbx), l1_bin(b.ymin, g.y0, g.sy, g.nby),
                      l1_bin(b.ymax, g.y0, g.sy, g.nby)};
}
// FILL = false: the polygon's box, and one count per bin it covers; true: the polygon into the list of each of those bins
template <bool FILL>
__global__ void k_l1_bin_polys(L1Bins g, const int32_t *__restrict__ polyptr, const double *__restrict__ px,
                               const double *__restrict__ py, int npoly, L1Box *__restrict__ box, uint32_t *__restrict__ cnt,
                               const uint32_t *__restrict__ binptr, int32_t *__restrict__ binlist) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npoly) return;
    L1Box b;
    if (!FILL) {
        b = L1Box{1e300, 1e300, -1e300, -1e300};
        for (int k = polyptr[p]; k < polyptr[p + 1]; ++k) {
            b.xmin = fmin(b.xmin, px[k]); b.xmax = fmax(b.xmax, px[k]);
            b.ymin = fmin(b.ymin, py[k]); b.ymax = fmax(b.ymax, py[k]);
        }
        box[p] = b;
    } else {
        b = box[p];
    }
    const L1BinRange r = l1_bin_range(g, b);
    for (int by = r.by0; by <= r.by1; ++by)
        for (int bx = r.bx0; bx <= r.bx1; ++bx) {
            const int bin = by * g.nbx + bx;
            const uint32_t k = atomicAdd(&cnt[bin], 1u);
            if (FILL) binlist[binptr[bin] + k] = p;
        }
}

// ---- clip: one lane per triangle ----------------------------------------------------------------------------------------------
struct L1ClipView {
    const double *vx, *vy;       // mesh
    const int32_t *tri;
    int ntri;
    const int32_t *polyptr;      // polygons
    const double *px, *py;
    const L1Box *box;
    L1Bins g;
    const uint32_t *binptr;
    const int32_t *binlist;
};
// the part of the subject polygon (in, n vertices, lane-strided LDS) on the inner side of the line a -> b of a counter-clockwise
// clip polygon: cross(b - a, s - a) >= 0.  A vertex ON the line is inside; the zero-area pieces that leaves are dropped by their area.
__device__ __forceinline__ int l1_clip_edge(const double *ix, const double *iy, int n, double *ox, double *oy, double ax, double ay,
                                            double bx, double by) {
    const double ex = bx - ax, ey = by - ay;
    int m = 0;
    for (int k = 0; k < n; ++k) {
        const int kn = k + 1 == n ? 0 : k + 1;
        const double sx = ix[k * L1_LANES], sy = iy[k * L1_LANES], tx = ix[kn * L1_LANES], ty = iy[kn * L1_LANES];
        const double ds = ex * (sy - ay) - ey * (sx - ax), dt = ex * (ty - ay) - ey * (tx - ax);
        const bool ins = ds >= 0, intt = dt >= 0;
        if (ins && m < L1_CLIPV) { ox[m * L1_LANES] = sx; oy[m * L1_LANES] = sy; ++m; }
        if (ins != intt && m < L1_CLIPV) {
            const double t = ds / (ds - dt);
            ox[m * L1_LANES] = sx + t * (tx - sx); oy[m * L1_LANES] = sy + t * (ty - sy);
            ++m;
        }
    }
    return m;
}
// EMIT = false: pieces and polygon vertices of every triangle (npiece, nvert_out); true: the records at the scanned offsets
template <bool EMIT>
__global__ void __launch_bounds__(L1_LANES)
k_l1_clip(L1ClipView c, uint32_t *__restrict__ npiece, uint32_t *__restrict__ nvert_out, const uint32_t *__restrict__ piece0,
          const uint32_t *__restrict__ vert0, const int64_t *__restrict__ iA, uint64_t *__restrict__ keys, uint32_t *__restrict__ idx,
          double *__restrict__ rec_area, uint32_t *__restrict__ rec_nv, uint32_t *__restrict__ rec_v0, double *__restrict__ qx, double *__restrict__ qy) {
    __shared__ double lds[4 * L1_CLIPV * L1_LANES];
    const int t = blockIdx.x * L1_LANES + threadIdx.x;
    if (t >= c.ntri) return;
    double *ax = lds + threadIdx.x, *ay = ax + L1_CLIPV * L1_LANES, *bx = ay + L1_CLIPV * L1_LANES, *by = bx + L1_CLIPV * L1_LANES;
    const int v0 = c.tri[3 * t], v1 = c.tri[3 * t + 1], v2 = c.tri[3 * t + 2];
    const double x0 = c.vx[v0], y0 = c.vy[v0];
    const double x1 = c.vx[v1], y1 = c.vy[v1], x2 = c.vx[v2], y2 = c.vy[v2];
    const L1Box tb{fmin(x0, fmin(x1, x2)), fmin(y0, fmin(y1, y2)), fmax(x0, fmax(x1, x2)), fmax(y0, fmax(y1, y2))};
    uint32_t np = 0, nv = 0;
    uint32_t rp = EMIT ? piece0[t] : 0, rv = EMIT ? vert0[t] : 0;
    if (tb.xmax >= c.g.x0 && tb.xmin <= c.g.x1 && tb.ymax >= c.g.y0 && tb.ymin <= c.g.y1) {
        const L1BinRange tr = l1_bin_range(c.g, tb);
        for (int biny = tr.by0; biny <= tr.by1; ++biny)
            for (int binx = tr.bx0; binx <= tr.bx1; ++binx) {
                const int bin = biny * c.g.nbx + binx;
                for (uint32_t j = c.binptr[bin]; j < c.binptr[bin + 1]; ++j) {
                    const int p = c.binlist[j];
                    const L1Box pb = c.box[p];
                    // each candidate once: in the first bin the two bin ranges share
                    const L1BinRange pr = l1_bin_range(c.g, pb);
                    if (binx != (pr.bx0 > tr.bx0 ? pr.bx0 : tr.bx0) || biny != (pr.by0 > tr.by0 ? pr.by0 : tr.by0)) continue;
                    if (pb.xmax < tb.xmin || pb.xmin > tb.xmax || pb.ymax < tb.ymin || pb.ymin > tb.ymax) continue;
                    // the triangle in the frame of its vertex 0, clipped by the polygon's edges in the same frame
                    ax[0] = 0; ay[0] = 0;
                    ax[L1_LANES] = x1 - x0; ay[L1_LANES] = y1 - y0;
                    ax[2 * L1_LANES] = x2 - x0; ay[2 * L1_LANES] = y2 - y0;
                    int n = 3;
                    const int pb0 = c.polyptr[p], pn = c.polyptr[p + 1] - pb0;
                    double *sx = ax, *sy = ay, *dx = bx, *dy = by;
                    for (int e = 0; e < pn && n > 0; ++e) {
                        const int en = e + 1 == pn ? 0 : e + 1;
                        n = l1_clip_edge(sx, sy, n, dx, dy, c.px[pb0 + e] - x0, c.py[pb0 + e] - y0, c.px[pb0 + en] - x0,
                                         c.py[pb0 + en] - y0);
                        double *tx = sx; sx = dx; dx = tx;
                        double *ty = sy; sy = dy; dy = ty;
                    }
                    if (n < 3) continue;
                    // back to the mesh's coordinates: these are the vertices the record holds, and the area is theirs
                    for (int k = 0; k < n; ++k) { sx[k * L1_LANES] = sx[k * L1_LANES] + x0; sy[k * L1_LANES] = sy[k * L1_LANES] + y0; }
                    const double area = l1_area(sx, sy, n, L1_LANES);
                    if (!(area > 0)) continue;       // an empty / degenerate overlap is no exchange cell (:183-184)
                    if (EMIT) {
                        keys[rp] = ((uint64_t)iA[p] << 32) | (uint32_t)t; idx[rp] = rp;
                        rec_area[rp] = area; rec_nv[rp] = (uint32_t)n; rec_v0[rp] = rv;
                        for (int k = 0; k < n; ++k) { qx[rv + k] = sx[k * L1_LANES]; qy[rv + k] = sy[k * L1_LANES]; }
                        ++rp; rv += (uint32_t)n;
                    }
                    ++np; nv += (uint32_t)n;
                }
            }
    }
    if (!EMIT) { npiece[t] = np; nvert_out[t] = nv; }
}
__global__ void k_l1_keys_given(const int32_t *__restrict__ iA, const int32_t *__restrict__ iTri, const int32_t *__restrict__ vptr,
                                uint32_t n, uint64_t *__restrict__ keys, uint32_t *__restrict__ idx, uint32_t *__restrict__ rec_nv,
                                uint32_t *__restrict__ rec_v0) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    keys[r] = ((uint64_t)(uint32_t)iA[r] << 32) | (uint32_t)iTri[r];
    idx[r] = r;
    rec_nv[r] = (uint32_t)(vptr[r + 1] - vptr[r]); rec_v0[r] = (uint32_t)vptr[r];
}
__global__ void k_l1_sorted_nv(const uint32_t *__restrict__ idx, const uint32_t *__restrict__ rec_nv, uint32_t n, uint32_t *__restrict__ nv) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) nv[r] = rec_nv[idx[r]];
}
// record idx[r] becomes exchange cell r; rec_area == nullptr: the area is taken here, from the polygon as given
__global__ void k_l1_gather(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ idx, uint32_t n,
                            const uint32_t *__restrict__ rec_nv, const uint32_t *__restrict__ rec_v0, const double *__restrict__ rec_area,
                            const double *__restrict__ sqx, const double *__restrict__ sqy, int32_t *__restrict__ vptr,
                            int32_t *__restrict__ indices, double *__restrict__ area, double *__restrict__ qx, double *__restrict__ qy,
                            uint32_t nq) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) { if (r == n) vptr[n] = (int32_t)nq; return; }
    const uint32_t s = idx[r], nv = rec_nv[s], src = rec_v0[s], dst = (uint32_t)vptr[r];
    for (uint32_t k = 0; k < nv; ++k) { qx[dst + k] = sqx[src + k]; qy[dst + k] = sqy[src + k]; }
    indices[2 * (size_t)r] = (int32_t)(keys[r] >> 32);
    indices[2 * (size_t)r + 1] = (int32_t)(uint32_t)keys[r];
    area[r] = rec_area ? rec_area[s] : l1_area(sqx + src, sqy + src, (int)nv, 1);
}

// the records (in the arena, unsorted, keys made) -> the exchange grid in (iA, iTri) order
static void l1_finish(ibh_l1_exgrid *ex, uint32_t n, uint64_t nq, uint64_t *keys, uint32_t *idx, const uint32_t *rec_nv,
                      const uint32_t *rec_v0, const double *rec_area, const double *sqx, const double *sqy, int64_t iA_extent,
                      int64_t iTri_extent, hipStream_t st) {
    Arena &A = arena();
    const int T = 256;
    uint64_t *keys_alt = A.get<uint64_t>(n);
    uint32_t *idx_alt = A.get<uint32_t>(n);
    const int lo_bits = bits_for((uint64_t)iTri_extent), hi_bits = bits_for((uint64_t)iA_extent);
    const KeyField f[2] = {{0, lo_bits > 0 ? lo_bits : 1}, {32, hi_bits > 0 ? hi_bits : 1}};
    if (radix_sort_pairs(keys, keys_alt, idx, idx_alt, n, f, 2, st)) { keys = keys_alt; idx = idx_alt; }
    ex->nX = n; ex->nq = (int64_t)nq; ex->iA_extent = iA_extent; ex->iTri_extent = iTri_extent;
    ex->indices.alloc(2 * (size_t)n); ex->area.alloc(n); ex->vptr.alloc((size_t)n + 1); ex->qx.alloc(nq); ex->qy.alloc(nq);
    uint32_t *nv = A.get<uint32_t>((size_t)n + 1);
    hipLaunchKernelGGL(k_l1_sorted_nv, dim3(ceil_div(n, T)), dim3(T), 0, st, idx, rec_nv, n, nv);
    exclusive_scan_u32(nv, reinterpret_cast<uint32_t *>(ex->vptr.p), n, nullptr, st);
    hipLaunchKernelGGL(k_l1_gather, dim3(ceil_div((long)n + 1, T)), dim3(T), 0, st, keys, idx, n, rec_nv, rec_v0, rec_area, sqx, sqy,
                       ex->vptr.p, ex->indices.p, ex->area.p, ex->qx.p, ex->qy.p, (uint32_t)nq);
    IBH_HIP(hipGetLastError());
    IBH_HIP(hipStreamSynchronize(st));
}

// k_l1_clip intersects the triangle with the half-plane of every polygon edge, which is the polygon only when the polygon is
// convex and counter-clockwise: a reflex vertex loses area and a clockwise polygon yields nothing, both silently.  So such a
// polygon is refused here.  A refusal must not trip on a side that carries computed collinear points (a projected lon/lat box
// with points_in_side > 1), so a turn counts as reflex only when it is more negative than rounding can make a straight one.
// The bound is derived, not measured.  With M the polygon's largest |coordinate|, u = ulp(M) <= eps M (eps = 2^-52), e = e_k,
// f = e_{k+1} and S = |e|_1 + |f|_1:
//   * moving every vertex by up to d in each coordinate moves each edge component by up to 2 d and
//     cross(e, f) = e_x f_y - e_y f_x by up to 2 d S + 8 d^2;  d = u (the stored coordinate is the exact one rounded at M's
//     binade) gives 2 u S + 8 u^2;
//   * evaluating the cross product in doubles (two differences, a product and the final difference, half an ulp each) is off by
//     up to 2 eps (|e_x f_y| + |e_y f_x|) <= 2 eps |e|_1 |f|_1 <= 4 eps M S, since an edge component is at most 2 M.
// Together 6 eps M S + 8 (eps M)^2.  The factor used is 16: it also covers a point computed as a + t (b - a), which carries
// three roundings (d up to 2.5 u: 5 + 4 = 9).  A turn more reflex than that is a property of the input.
// The edge directions must wind once as well (a star polygon turns left everywhere): at most two sign changes of the
// edges' x components and of their y components round the cycle, a component within 2 eps M of zero (both ends moved by u)
// counting as zero.
constexpr double L1_TURN_FACTOR = 16.0;
static void l1_check_convex_ccw(int p, const double *x, const double *y, int n) {
    const double eps = 2.220446049250313e-16;
    double M = 0;
    for (int k = 0; k < n; ++k) M = std::max(M, std::max(std::fabs(x[k]), std::fabs(y[k])));
    const double eM = eps * M;
    int chg[2] = {0, 0}, last[2] = {0, 0};      // per axis: sign changes so far, latest non-zero sign
    for (int k = 0; k < n; ++k) {
        const int k1 = k + 1 == n ? 0 : k + 1, k2 = k1 + 1 == n ? 0 : k1 + 1;
        const double e[2] = {x[k1] - x[k], y[k1] - y[k]}, f[2] = {x[k2] - x[k1], y[k2] - y[k1]};
        const double c = e[0] * f[1] - e[1] * f[0];
        const double S = (std::fabs(e[0]) + std::fabs(e[1])) + (std::fabs(f[0]) + std::fabs(f[1]));
        const double tol = L1_TURN_FACTOR * eM * (S + eM);
        IBH_CHECK(c >= -tol, "polygon %d is not counter-clockwise convex: the turn at vertex %d is reflex (cross product %.3e, rounding allows %.3e)",
                  p, k1, c, -tol);
        for (int a = 0; a < 2; ++a) {
            const int s = e[a] > 2 * eM ? 1 : e[a] < -2 * eM ? -1 : 0;
            if (!s) continue;
            if (last[a] && s != last[a]) ++chg[a];
            last[a] = s;
            // changes round the cycle come in pairs: a third one along the walk is the fourth of the cycle
            IBH_CHECK(chg[a] <= 2, "polygon %d is not convex: its edges wind more than once (the %c direction turns back a third time at vertex %d)",
                      p, a ? 'y' : 'x', k);
        }
    }
}

static void l1_exgrid_generate(const ibh_l1_mesh *m, int32_t npoly, const int32_t *polyptr, const double *px, const double *py,
                               const int64_t *iA, ibh_l1_exgrid **out) {
    IBH_CHECK(m && out, "null argument");
    IBH_CHECK(npoly >= 0 && (npoly == 0 || (polyptr && px && py && iA)), "null polygon arrays");
    L1Bins g{1e300, 1e300, -1e300, -1e300, 0, 0, 1, 1};
    for (int p = 0; p < npoly; ++p) {
        const int n = polyptr[p + 1] - polyptr[p];
        IBH_CHECK(polyptr[p] >= 0 && n >= 3 && n <= L1_MAXV, "polygon %d has %d vertices (3..%d supported)", p, n, L1_MAXV);
        IBH_CHECK(iA[p] >= 0 && iA[p] < (1ll << 31) - 1, "polygon %d: iA out of range", p);
        IBH_CHECK(p == 0 || iA[p] > iA[p - 1], "polygons must come in ascending iA order (cells.sorted(), AbbrGrid.cpp:15)");
        for (int k = polyptr[p]; k < polyptr[p + 1]; ++k) {
            IBH_CHECK(px[k] - px[k] == 0 && py[k] - py[k] == 0, "polygon %d: vertex %d is not finite", p, k - polyptr[p]);
            g.x0 = std::min(g.x0, px[k]); g.x1 = std::max(g.x1, px[k]);
            g.y0 = std::min(g.y0, py[k]); g.y1 = std::max(g.y1, py[k]);
        }
        l1_check_convex_ccw(p, px + polyptr[p], py + polyptr[p], n);
    }
    require_device();
    std::unique_ptr<ibh_l1_exgrid> ex(new ibh_l1_exgrid);
    ex->vptr.alloc(1); ex->vptr.zero();
    ex->iTri_extent = m->ntri;
    if (npoly == 0 || m->ntri == 0) { IBH_HIP(hipStreamSynchronize(nullptr)); *out = ex.release(); return; }
    // about one polygon per bin
    int nb = 1;
    while ((int64_t)nb * nb < npoly && nb < L1_MAXBINS) ++nb;
    g.nbx = g.nby = nb;
    g.sx = g.x1 > g.x0 ? nb / (g.x1 - g.x0) : 0;
    g.sy = g.y1 > g.y0 ? nb / (g.y1 - g.y0) : 0;
    hipStream_t st = nullptr;
    Arena &A = arena();
    A.reset();
    const int T = 256, nvp = polyptr[npoly], nbins = nb * nb, ntri = m->ntri;
    int32_t *dpp = A.get<int32_t>((size_t)npoly + 1);
    double *dpx = A.get<double>((size_t)nvp), *dpy = A.get<double>((size_t)nvp);
    int64_t *diA = A.get<int64_t>((size_t)npoly);
    IBH_HIP(hipMemcpyAsync(dpp, polyptr, sizeof(int32_t) * ((size_t)npoly + 1), hipMemcpyHostToDevice, st));
    IBH_HIP(hipMemcpyAsync(dpx, px, sizeof(double) * (size_t)nvp, hipMemcpyHostToDevice, st));
    IBH_HIP(hipMemcpyAsync(dpy, py, sizeof(double) * (size_t)nvp, hipMemcpyHostToDevice, st));
    IBH_HIP(hipMemcpyAsync(diA, iA, sizeof(int64_t) * (size_t)npoly, hipMemcpyHostToDevice, st));
    L1Box *box = A.get<L1Box>((size_t)npoly);
    uint32_t *cnt = A.get<uint32_t>((size_t)nbins + 1), *binptr = A.get<uint32_t>((size_t)nbins + 1);
    IBH_HIP(hipMemsetAsync(cnt, 0, sizeof(uint32_t) * ((size_t)nbins + 1), st));
    hipLaunchKernelGGL(k_l1_bin_polys<false>, dim3(ceil_div(npoly, T)), dim3(T), 0, st, g, dpp, dpx, dpy, npoly, box, cnt, nullptr, nullptr);
    exclusive_scan_u32(cnt, binptr, (size_t)nbins, binptr + nbins, st);
    uint32_t nlist = 0;
    readback_sync(&nlist, binptr + nbins, sizeof(uint32_t), st);
    IBH_CHECK(nlist < (1u << 31), "too many (polygon, bin) pairs");
    int32_t *binlist = A.get<int32_t>(nlist);
    IBH_HIP(hipMemsetAsync(cnt, 0, sizeof(uint32_t) * ((size_t)nbins + 1), st));
    hipLaunchKernelGGL(k_l1_bin_polys<true>, dim3(ceil_div(npoly, T)), dim3(T), 0, st, g, dpp, dpx, dpy, npoly, box, cnt, binptr, binlist);
    L1ClipView c{m->vx.p, m->vy.p, m->tri.p, ntri, dpp, dpx, dpy, box, g, binptr, binlist};
    uint32_t *npiece = A.get<uint32_t>((size_t)ntri + 1), *nvo = A.get<uint32_t>((size_t)ntri + 1);
    uint32_t *piece0 = A.get<uint32_t>((size_t)ntri + 1), *vert0 = A.get<uint32_t>((size_t)ntri + 1);
    hipLaunchKernelGGL(k_l1_clip<false>, dim3(ceil_div(ntri, L1_LANES)), dim3(L1_LANES), 0, st, c, npiece, nvo, nullptr, nullptr, nullptr,
                       nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    exclusive_scan_u32(npiece, piece0, (size_t)ntri, piece0 + ntri, st);
    exclusive_scan_u32(nvo, vert0, (size_t)ntri, vert0 + ntri, st);
    uint32_t nX = 0, nq = 0;
    readback_sync(&nX, piece0 + ntri, sizeof(uint32_t), st);
    readback_sync(&nq, vert0 + ntri, sizeof(uint32_t), st);
    IBH_CHECK(nX < (1u << 31) / 3 && nq < (1u << 31), "too many exchange cells");
    if (nX == 0) { *out = ex.release(); return; }
    double *rec_area = A.get<double>(nX), *sqx = A.get<double>(nq), *sqy = A.get<double>(nq);
    uint32_t *rec_nv = A.get<uint32_t>(nX), *rec_v0 = A.get<uint32_t>(nX), *idx = A.get<uint32_t>(nX);
    uint64_t *keys = A.get<uint64_t>(nX);
    hipLaunchKernelGGL(k_l1_clip<true>, dim3(ceil_div(ntri, L1_LANES)), dim3(L1_LANES), 0, st, c, nullptr, nullptr, piece0, vert0, diA, keys,
                       idx, rec_area, rec_nv, rec_v0, sqx, sqy);
    IBH_HIP(hipGetLastError());
    l1_finish(ex.get(), nX, nq, keys, idx, rec_nv, rec_v0, rec_area, sqx, sqy, iA[npoly - 1] + 1, ntri, st);
    *out = ex.release();
}

static void l1_exgrid_from_polygons(int64_t nX, const int32_t *iA, const int32_t *iTri, const int32_t *vptr, const double *qx,
                                    const double *qy, ibh_l1_exgrid **out) {
    IBH_CHECK(out != nullptr, "null argument");
    IBH_CHECK(nX >= 0 && nX < (1ll << 31) / 3, "nX=%lld out of range", (long long)nX);
    IBH_CHECK(vptr && (nX == 0 || (iA && iTri && qx && qy)), "null exchange-grid arrays");
    IBH_CHECK(vptr[0] == 0, "vptr[0] must be 0");
    int64_t iA_extent = 0, iTri_extent = 0;
    for (int64_t x = 0; x < nX; ++x) {
        const int n = vptr[x + 1] - vptr[x];
        IBH_CHECK(n >= 3 && n <= L1_CLIPV, "exchange cell %lld has %d vertices (3..%d supported)", (long long)x, n, L1_CLIPV);
        IBH_CHECK(iA[x] >= 0 && iA[x] < INT32_MAX && iTri[x] >= 0 && iTri[x] < INT32_MAX, "exchange cell %lld: negative index", (long long)x);
        iA_extent = std::max<int64_t>(iA_extent, (int64_t)iA[x] + 1); iTri_extent = std::max<int64_t>(iTri_extent, (int64_t)iTri[x] + 1);
    }
    require_device();
    std::unique_ptr<ibh_l1_exgrid> ex(new ibh_l1_exgrid);
    ex->vptr.alloc(1); ex->vptr.zero();
    if (nX == 0) { IBH_HIP(hipStreamSynchronize(nullptr)); *out = ex.release(); return; }
    hipStream_t st = nullptr;
    Arena &A = arena();
    A.reset();
    const uint32_t n = (uint32_t)nX, nq = (uint32_t)vptr[nX];
    int32_t *dA = A.get<int32_t>(n), *dT = A.get<int32_t>(n), *dv = A.get<int32_t>((size_t)n + 1);
    double *sqx = A.get<double>(nq), *sqy = A.get<double>(nq);
    IBH_HIP(hipMemcpyAsync(dA, iA, sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
    IBH_HIP(hipMemcpyAsync(dT, iTri, sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
    IBH_HIP(hipMemcpyAsync(dv, vptr, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyHostToDevice, st));
    IBH_HIP(hipMemcpyAsync(sqx, qx, sizeof(double) * nq, hipMemcpyHostToDevice, st));
    IBH_HIP(hipMemcpyAsync(sqy, qy, sizeof(double) * nq, hipMemcpyHostToDevice, st));
    uint64_t *keys = A.get<uint64_t>(n);
    uint32_t *idx = A.get<uint32_t>(n), *rec_nv = A.get<uint32_t>(n), *rec_v0 = A.get<uint32_t>(n);
    hipLaunchKernelGGL(k_l1_keys_given, dim3(ceil_div(n, 256)), dim3(256), 0, st, dA, dT, dv, n, keys, idx, rec_nv, rec_v0);
    IBH_HIP(hipGetLastError());
    l1_finish(ex.get(), n, nq, keys, idx, rec_nv, rec_v0, nullptr, sqx, sqy, iA_extent, iTri_extent, st);
    *out = ex.release();
}

// ---- basis integrals ------------------------------------------------------------------------------------------------------------
// One lane per exchange cell; the polygon is streamed from the ragged array (read once), nothing is indexed at run time but
// global memory.  With P0 the element's vertex 0, e1 = P1 - P0, e2 = P2 - P0, det = e1 x e2 and u = q - P0:
//   l1(u) = (u x e2) / det,   l2(u) = (e1 x u) / det,   l0(u) = (1 - l1) - l2
// and over the fan triangle (a, b, c), a = polygon vertex 0:  integral of l_k = area(a, b, c) * ((l_k(a) + l_k(b)) + l_k(c)) / 3.
// swap: rows are vertices and columns GCM cells (IvA).
struct L1Bary { double l0, l1, l2; };
__device__ __forceinline__ L1Bary l1_bary(double ux, double uy, double e1x, double e1y, double e2x, double e2y, double det) {
    L1Bary b;
    b.l1 = (ux * e2y - uy * e2x) / det;
    b.l2 = (e1x * uy - e1y * ux) / det;
    b.l0 = (1.0 - b.l1) - b.l2;
    return b;
}
__global__ void k_l1_integrals(const int32_t *__restrict__ indices, const int32_t *__restrict__ vptr, const double *__restrict__ qx,
                               const double *__restrict__ qy, int nX, const double *__restrict__ vx, const double *__restrict__ vy,
                               const int32_t *__restrict__ tri, int swap, int32_t *__restrict__ row, int32_t *__restrict__ col,
                               double *__restrict__ val) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nX) return;
    const int iA = indices[2 * (size_t)x], t = indices[2 * (size_t)x + 1];
    const int v0 = tri[3 * t], v1 = tri[3 * t + 1], v2 = tri[3 * t + 2];
    const double x0 = vx[v0], y0 = vy[v0];
    const double e1x = vx[v1] - x0, e1y = vy[v1] - y0, e2x = vx[v2] - x0, e2y = vy[v2] - y0;
    const double det = e1x * e2y - e1y * e2x;
    const int b = vptr[x], n = vptr[x + 1] - b;
    const double ax = qx[b] - x0, ay = qy[b] - y0;
    const L1Bary la = l1_bary(ax, ay, e1x, e1y, e2x, e2y, det);
    double bx = qx[b + 1] - x0, by = qy[b + 1] - y0;
    L1Bary lb = l1_bary(bx, by, e1x, e1y, e2x, e2y, det);
    double s0 = 0, s1 = 0, s2 = 0;
    for (int i = 2; i < n; ++i) {
        const double cx = qx[b + i] - x0, cy = qy[b + i] - y0;
        const L1Bary lc = l1_bary(cx, cy, e1x, e1y, e2x, e2y, det);
        const double fa = 0.5 * ((bx - ax) * (cy - ay) - (by - ay) * (cx - ax));
        const double t0 = fa * (((la.l0 + lb.l0) + lc.l0) / 3.0);
        const double t1 = fa * (((la.l1 + lb.l1) + lc.l1) / 3.0);
        const double t2 = fa * (((la.l2 + lb.l2) + lc.l2) / 3.0);
        if (i == 2) { s0 = t0; s1 = t1; s2 = t2; }          // the first term is assigned
        else { s0 = s0 + t0; s1 = s1 + t1; s2 = s2 + t2; }
        bx = cx; by = cy; lb = lc;
    }
    const size_t o = 3 * (size_t)x;
    int32_t *rA = swap ? col : row, *rV = swap ? row : col;
    rA[o] = iA; rA[o + 1] = iA; rA[o + 2] = iA;
    rV[o] = v0; rV[o + 1] = v1; rV[o + 2] = v2;
    val[o] = s0; val[o + 1] = s1; val[o + 2] = s2;
}
__global__ void k_l1_check_indices(const int32_t *__restrict__ indices, int nX, int nA, int ntri, uint32_t *__restrict__ first_bad) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nX) return;
    const int a = indices[2 * (size_t)x], t = indices[2 * (size_t)x + 1];
    if (a < 0 || a >= nA || t < 0 || t >= ntri) atomicMin(first_bad, (uint32_t)x);
}

static void l1_matrix(const ibh_l1_exgrid *ex, const ibh_l1_mesh *m, int64_t nA, const char *which, int scale, ibh_weighted **out,
                      int32_t *trow, int32_t *tcol, double *tval) {
    IBH_CHECK(ex && m && which, "null argument");
    const bool swap = !strcmp(which, "IvA");
    IBH_CHECK(swap || !strcmp(which, "AvI"), "L1 matrix: which must be \"AvI\" or \"IvA\", not \"%s\"", which);
    IBH_CHECK(nA > 0 && nA < (1ll << 31), "nA=%lld out of range", (long long)nA);
    IBH_CHECK(ex->iA_extent <= nA, "L1 matrix: the exchange grid names GCM cell %lld, nA is %lld", (long long)ex->iA_extent - 1, (long long)nA);
    IBH_CHECK(ex->iTri_extent <= m->ntri || ex->nX == 0, "L1 matrix: the exchange grid names element %lld, the mesh has %d",
              (long long)ex->iTri_extent - 1, m->ntri);
    require_device();
    hipStream_t st = nullptr;
    Arena &A = arena();
    A.reset();
    const int nX = (int)ex->nX;
    const size_t n = 3 * (size_t)nX;
    int32_t *row = A.get<int32_t>(n), *col = A.get<int32_t>(n);
    double *val = A.get<double>(n);
    if (nX) {
        uint32_t *bad = A.get<uint32_t>(1);
        IBH_HIP(hipMemsetAsync(bad, 0xFF, sizeof(uint32_t), st));
        hipLaunchKernelGGL(k_l1_check_indices, dim3(ceil_div(nX, 256)), dim3(256), 0, st, ex->indices.p, nX, (int)nA, m->ntri, bad);
        uint32_t h = 0;
        readback_sync(&h, bad, sizeof(h), st);
        IBH_CHECK(h == 0xFFFFFFFFu, "L1 matrix: exchange cell %u names a GCM cell or an element out of range", h);
        hipLaunchKernelGGL(k_l1_integrals, dim3(ceil_div(nX, 256)), dim3(256), 0, st, ex->indices.p, ex->vptr.p, ex->qx.p, ex->qy.p, nX,
                           m->vx.p, m->vy.p, m->tri.p, swap ? 1 : 0, row, col, val);
        IBH_HIP(hipGetLastError());
    }
    if (!out) {          // the terms themselves (ibh_l1_terms)
        if (n) {
            IBH_HIP(hipMemcpyAsync(trow, row, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
            IBH_HIP(hipMemcpyAsync(tcol, col, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
            IBH_HIP(hipMemcpyAsync(tval, val, sizeof(double) * n, hipMemcpyDeviceToHost, st));
        }
        IBH_HIP(hipStreamSynchronize(st));
        return;
    }
    auto w = new_weighted();
    w->conservative = 1;
    w->scaled = scale ? 1 : 0;
    const int nrow = swap ? m->nvert : (int)nA, ncol = swap ? (int)nA : m->nvert;
    weighted_from_device_triplets(w.get(), nrow, ncol, (int64_t)n, row, col, val, st);
    // M = diag(1 / wM) M  (fA = (1/weightsA) AvI fI, element_l1.py:100-102); rows without entries are left alone
    if (scale && w->nnz) scale_rows_recip(w->rowptr.p, nrow, w->wM.p, w->val.p, st);
    IBH_HIP(hipGetLastError());
    IBH_HIP(hipStreamSynchronize(st));
    w->dims[0] = DimRef::owned_identity(nrow); w->dims[1] = DimRef::owned_identity(ncol);
    *out = w.release();
}

}  // namespace ibh

using namespace ibh;

extern "C" {

int ibh_l1_mesh_create(int32_t nvert, const double *vx, const double *vy, int32_t ntri, const int32_t *tri, ibh_l1_mesh **out) {
    return guarded([&] {
        if (out) *out = nullptr;
        l1_mesh_create(nvert, vx, vy, ntri, tri, out);
    });
}
int ibh_l1_mesh_destroy(ibh_l1_mesh *mesh) { delete mesh; return IBH_OK; }

int ibh_l1_exgrid_generate(const ibh_l1_mesh *mesh, int32_t npoly, const int32_t *polyptr, const double *px, const double *py,
                           const int64_t *iA, ibh_l1_exgrid **out) {
    return guarded([&] {
        if (out) *out = nullptr;
        l1_exgrid_generate(mesh, npoly, polyptr, px, py, iA, out);
    });
}
int ibh_l1_exgrid_from_polygons(int64_t nX, const int32_t *iA, const int32_t *iTri, const int32_t *vptr, const double *qx,
                                const double *qy, ibh_l1_exgrid **out) {
    return guarded([&] {
        if (out) *out = nullptr;
        l1_exgrid_from_polygons(nX, iA, iTri, vptr, qx, qy, out);
    });
}
int ibh_l1_exgrid_size(const ibh_l1_exgrid *ex, int64_t *nX, int64_t *nq) {
    return guarded([&] {
        IBH_CHECK(ex && nX, "null argument");
        *nX = ex->nX;
        if (nq) *nq = ex->nq;
    });
}
int ibh_l1_exgrid_get(const ibh_l1_exgrid *ex, int32_t *indices, double *areas, int32_t *vptr, double *qx, double *qy) {
    return guarded([&] {
        IBH_CHECK(ex != nullptr, "null argument");
        if (vptr) ex->vptr.download(vptr, (size_t)ex->nX + 1);
        if (ex->nX == 0) return;
        if (indices) ex->indices.download(indices, 2 * (size_t)ex->nX);
        if (areas) ex->area.download(areas, (size_t)ex->nX);
        if (qx) ex->qx.download(qx, (size_t)ex->nq);
        if (qy) ex->qy.download(qy, (size_t)ex->nq);
    });
}
int ibh_l1_exgrid_destroy(ibh_l1_exgrid *ex) { delete ex; return IBH_OK; }

int ibh_l1_terms(const ibh_l1_exgrid *ex, const ibh_l1_mesh *mesh, int64_t nA, const char *which, int32_t *row, int32_t *col, double *val) {
    return guarded([&] {
        IBH_CHECK(ex && (ex->nX == 0 || (row && col && val)), "null argument");
        l1_matrix(ex, mesh, nA, which, 0, nullptr, row, col, val);
    });
}
int ibh_l1_matrix(const ibh_l1_exgrid *ex, const ibh_l1_mesh *mesh, int64_t nA, const char *which, int scale, ibh_weighted **out) {
    return guarded([&] {
        IBH_CHECK(out != nullptr, "null argument");
        *out = nullptr;
        l1_matrix(ex, mesh, nA, which, scale, out, nullptr, nullptr, nullptr);
    });
}

}  // extern "C"
