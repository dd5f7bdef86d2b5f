// gridgen.hip -- exchange-grid generation for a rectilinear XY ice grid under (projected) GCM cells: convex ones of up to 16
// vertices through k_gg_clip's per-lane arrays, anything else through the streamed clip (exgrid_generate decides per call).
//
// Replaces make_exchange_grid (slib/icebin/gridgen/GridGen_Exchange.cpp:175-284) for the case the
// regrid path is quoted on: ice cells are axis-aligned rectangles in the projected plane
// (gridgen/searise_grid.cpp), GCM cells are lon/lat boxes whose corners the caller has projected to
// that plane (OGrid, GridGen_Exchange.cpp:120-166) -- convex polygons of a few vertices.  The reference
// finds candidate pairs with an RTree over the ice cells and intersects polygons with CGAL; here the
// candidates of a GCM cell are the index ranges its bounding box covers (the ice grid is rectilinear:
// two binary searches), one thread clips the polygon against one ice cell (Sutherland-Hodgman against
// four axis-aligned half-planes) and takes the area with the reference's own formula
// (Cell::proj_area, Grid.cpp:42-70).  Cells are emitted ordered by (iA, iI) ascending -- the order of
// ExchangeGrid's constructor (AbbrGrid.cpp:10-21) -- by construction: candidates are enumerated in that
// order and compacted with a scan.  Byte/index work bound by HBM traffic; double arithmetic without
// contraction (the CGAL result is exact rationals rounded to double: areas agree to rounding).
#include <algorithm>

#include "prims.h"

namespace ibh {

constexpr int GG_MAXV = 16;          // vertices of a GCM-cell polygon
constexpr int GG_CLIPV = GG_MAXV + 4;

struct GridGenView {
    const double *xe, *ye;           // ice-cell edges [nx+1], [ny+1], ascending
    int nx, ny, x_fastest;
    const int32_t *polyptr;          // [npoly+1]
    const double *vx, *vy;           // polygon vertices, counter-clockwise
    int npoly;
};
struct CandRange { int ix0, nxr, iy0, nyr; };

__device__ __forceinline__ int first_edge_gt(const double *e, int n, double v) {     // first k with e[k] > v
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (e[mid] > v) hi = mid; else lo = mid + 1; }
    return lo;
}
__device__ __forceinline__ int first_edge_ge(const double *e, int n, double v) {     // first k with e[k] >= v
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (e[mid] >= v) hi = mid; else lo = mid + 1; }
    return lo;
}
// ice cells whose open interior can meet (lo, hi): cell k = [e[k], e[k+1]] needs e[k+1] > lo and e[k] < hi
__device__ __forceinline__ void cell_range(const double *e, int n, double lo, double hi, int &k0, int &cnt) {
    k0 = first_edge_gt(e, n + 1, lo) - 1;
    if (k0 < 0) k0 = 0;
    int k1 = first_edge_ge(e, n + 1, hi);        // cells k < k1 have e[k] < hi
    if (k1 > n) k1 = n;
    cnt = k1 > k0 ? k1 - k0 : 0;
}
__global__ void k_gg_ranges(GridGenView g, CandRange *__restrict__ rng, uint32_t *__restrict__ cnt) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= g.npoly) return;
    double xmin = 1e300, xmax = -1e300, ymin = 1e300, ymax = -1e300;
    for (int k = g.polyptr[p]; k < g.polyptr[p + 1]; ++k) {
        xmin = fmin(xmin, g.vx[k]); xmax = fmax(xmax, g.vx[k]);
        ymin = fmin(ymin, g.vy[k]); ymax = fmax(ymax, g.vy[k]);
    }
    CandRange r;
    cell_range(g.xe, g.nx, xmin, xmax, r.ix0, r.nxr);
    cell_range(g.ye, g.ny, ymin, ymax, r.iy0, r.nyr);
    rng[p] = r;
    cnt[p] = (uint32_t)r.nxr * (uint32_t)r.nyr;
}
// keep the part of the polygon on the inner side of one axis-aligned line: coordinate `axis` (0 x, 1 y),
// inside = (c >= bound) when lower, (c <= bound) otherwise
__device__ __forceinline__ int clip_axis(const double *ix, const double *iy, int n, double *ox, double *oy, int axis,
                                         double bound, bool lower) {
    int m = 0;
    for (int k = 0; k < n; ++k) {
        const int kn = k + 1 == n ? 0 : k + 1;
        const double ax = ix[k], ay = iy[k], bx = ix[kn], by = iy[kn];
        const double ca = axis ? ay : ax, cb = axis ? by : bx;
        const bool ina = lower ? ca >= bound : ca <= bound, inb = lower ? cb >= bound : cb <= bound;
        if (ina) { ox[m] = ax; oy[m] = ay; ++m; }
        if (ina != inb) {
            const double t = (bound - ca) / (cb - ca);
            if (axis) { ox[m] = ax + t * (bx - ax); oy[m] = bound; }
            else      { ox[m] = bound; oy[m] = ay + t * (by - ay); }
            ++m;
        }
    }
    return m;
}
__global__ void k_gg_clip(GridGenView g, const CandRange *__restrict__ rng, const uint32_t *__restrict__ candptr, uint32_t ncand,
                          double *__restrict__ area, uint32_t *__restrict__ keep, int32_t *__restrict__ cellI) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ncand) return;
    int lo = 0, hi = g.npoly;                      // polygon p with candptr[p] <= t < candptr[p+1]
    while (lo + 1 < hi) { const int mid = (lo + hi) >> 1; if (candptr[mid] <= t) lo = mid; else hi = mid; }
    const int p = lo;
    const CandRange r = rng[p];
    const uint32_t local = t - candptr[p];
    int ix, iy;
    if (g.x_fastest) { iy = r.iy0 + (int)(local / (uint32_t)r.nxr); ix = r.ix0 + (int)(local % (uint32_t)r.nxr); }
    else             { ix = r.ix0 + (int)(local / (uint32_t)r.nyr); iy = r.iy0 + (int)(local % (uint32_t)r.nyr); }
    double ax[GG_CLIPV], ay[GG_CLIPV], bx[GG_CLIPV], by[GG_CLIPV];
    int n = g.polyptr[p + 1] - g.polyptr[p];
    for (int k = 0; k < n; ++k) { ax[k] = g.vx[g.polyptr[p] + k]; ay[k] = g.vy[g.polyptr[p] + k]; }
    n = clip_axis(ax, ay, n, bx, by, 0, g.xe[ix], true);
    n = clip_axis(bx, by, n, ax, ay, 0, g.xe[ix + 1], false);
    n = clip_axis(ax, ay, n, bx, by, 1, g.ye[iy], true);
    n = clip_axis(bx, by, n, ax, ay, 1, g.ye[iy + 1], false);
    double ret = 0;                                // Cell::proj_area, Grid.cpp:42-70
    if (n >= 3) {
        double x0 = ax[n - 1], y0 = ay[n - 1];
        for (int k = 0; k < n; ++k) {
            const double x1 = ax[k], y1 = ay[k];
            ret += (x0 * y1) - (x1 * y0);
            x0 = x1; y0 = y1;
        }
        ret *= .5;
    }
    area[t] = ret;
    keep[t] = ret > 0 ? 1u : 0u;                   // an empty / degenerate overlap is no exchange cell (:183-184)
    cellI[t] = g.x_fastest ? iy * g.nx + ix : ix * g.ny + iy;
}
// ---- the streamed clip: any number of vertices, no per-lane arrays -----------------------------------------------------
// Sutherland-Hodgman in its re-entrant form (Sutherland & Hodgman 1974, "Reentrant polygon clipping"): the polygon goes vertex
// by vertex through four stages (x >= 0, x <= w, y >= 0, y <= h); a stage keeps its first point F and its previous point S and
// nothing else, and what it lets through is pushed into the next stage at once.  The fifth stage sums the shoelace terms.
// Coordinates are relative to the ice cell's lower-left corner, x - xe[ix] and y - ye[iy] (one rounding each), so the products
// of the shoelace carry the cell's size, not its distance from the projection's origin.  Operation order, each
// operation rounded on its own (-ffp-contract=off):
//   a point P reaching a stage with S set and S, P on different sides of the bound b (coordinate c = x or y, o the other one):
//       t = (b - c_S) / (c_P - c_S);  I = (c: b exactly, o: o_S + t * (o_P - o_S)) goes on first; then S = P; then P, if inside
//       (inside: c >= b for a lower bound, c <= b for an upper one);
//   at the end of the polygon every stage, in turn, treats the edge S -> F the same way and then closes the next stage;
//   the last stage: sum = 0; for every point after its first, sum += (x_S * y_P) - (x_P * y_S); at the end sum += (x_S * y_F) -
//   (x_F * y_S); area = .5 * sum when it saw >= 3 points, else 0.
// The points reach the last stage in the order k_gg_clip's arrays hold them; its sum starts with the closing edge and this one
// ends with it, so the two areas differ by rounding (and by the shift), not in which cells are kept beyond that.
struct ClipStage { double fx, fy, sx, sy; int has; };
struct ClipState {
    ClipStage s0, s1, s2, s3;
    double w, h;                    // the ice cell's extent: the upper bounds
    double fx, fy, sx, sy, sum;     // the shoelace stage
    int n;
};
template <int K> __device__ __forceinline__ ClipStage &clip_stage(ClipState &S) {
    if constexpr (K == 0) return S.s0;
    else if constexpr (K == 1) return S.s1;
    else if constexpr (K == 2) return S.s2;
    else return S.s3;
}
template <int K> __device__ __forceinline__ void clip_push(ClipState &S, double x, double y) {
    if constexpr (K == 4) {
        if (S.n) S.sum += (S.sx * y) - (x * S.sy);
        else { S.fx = x; S.fy = y; }
        S.sx = x; S.sy = y; ++S.n;
    } else {
        constexpr int axis = K >> 1;
        constexpr bool lower = (K & 1) == 0;
        ClipStage &st = clip_stage<K>(S);
        const double bound = lower ? 0.0 : (axis ? S.h : S.w);
        const double c = axis ? y : x;
        const bool in = lower ? c >= bound : c <= bound;
        if (st.has) {
            const double cs = axis ? st.sy : st.sx;
            const bool ins = lower ? cs >= bound : cs <= bound;
            if (ins != in) {
                const double t = (bound - cs) / (c - cs);
                if (axis) clip_push<K + 1>(S, st.sx + t * (x - st.sx), bound);
                else      clip_push<K + 1>(S, bound, st.sy + t * (y - st.sy));
            }
        } else { st.fx = x; st.fy = y; st.has = 1; }
        st.sx = x; st.sy = y;
        if (in) clip_push<K + 1>(S, x, y);
    }
}
template <int K> __device__ __forceinline__ void clip_close(ClipState &S) {
    if constexpr (K == 4) {
        if (S.n) S.sum += (S.sx * S.fy) - (S.fx * S.sy);
    } else {
        constexpr int axis = K >> 1;
        constexpr bool lower = (K & 1) == 0;
        ClipStage &st = clip_stage<K>(S);
        if (st.has) {
            const double bound = lower ? 0.0 : (axis ? S.h : S.w);
            const double cs = axis ? st.sy : st.sx, c = axis ? st.fy : st.fx;
            const bool ins = lower ? cs >= bound : cs <= bound, in = lower ? c >= bound : c <= bound;
            if (ins != in) {
                const double t = (bound - cs) / (c - cs);
                if (axis) clip_push<K + 1>(S, st.sx + t * (st.fx - st.sx), bound);
                else      clip_push<K + 1>(S, bound, st.sy + t * (st.fy - st.sy));
            }
        }
        clip_close<K + 1>(S);
    }
}
__global__ void k_gg_clip_stream(GridGenView g, const CandRange *__restrict__ rng, const uint32_t *__restrict__ candptr, uint32_t ncand,
                                 double *__restrict__ area, uint32_t *__restrict__ keep, int32_t *__restrict__ cellI) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ncand) return;
    int lo = 0, hi = g.npoly;                      // polygon p with candptr[p] <= t < candptr[p+1]
    while (lo + 1 < hi) { const int mid = (lo + hi) >> 1; if (candptr[mid] <= t) lo = mid; else hi = mid; }
    const int p = lo;
    const CandRange r = rng[p];
    const uint32_t local = t - candptr[p];
    int ix, iy;
    if (g.x_fastest) { iy = r.iy0 + (int)(local / (uint32_t)r.nxr); ix = r.ix0 + (int)(local % (uint32_t)r.nxr); }
    else             { ix = r.ix0 + (int)(local / (uint32_t)r.nyr); iy = r.iy0 + (int)(local % (uint32_t)r.nyr); }
    const double ox = g.xe[ix], oy = g.ye[iy];
    ClipState S;
    S.s0.has = S.s1.has = S.s2.has = S.s3.has = 0;
    S.w = g.xe[ix + 1] - ox; S.h = g.ye[iy + 1] - oy;
    S.sum = 0; S.n = 0;
    const int k1 = g.polyptr[p + 1];
    for (int k = g.polyptr[p]; k < k1; ++k) clip_push<0>(S, g.vx[k] - ox, g.vy[k] - oy);
    clip_close<0>(S);
    const double ret = S.n >= 3 ? S.sum * .5 : 0.0;
    area[t] = ret;
    keep[t] = ret > 0 ? 1u : 0u;
    cellI[t] = g.x_fastest ? iy * g.nx + ix : ix * g.ny + iy;
}
__global__ void k_gg_emit(const int64_t *__restrict__ iA, const uint32_t *__restrict__ candptr, int npoly, uint32_t ncand,
                          const double *__restrict__ area, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ pos,
                          const int32_t *__restrict__ cellI, int32_t *__restrict__ indices, double *__restrict__ overlaps) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ncand || !keep[t]) return;
    int lo = 0, hi = npoly;
    while (lo + 1 < hi) { const int mid = (lo + hi) >> 1; if (candptr[mid] <= t) lo = mid; else hi = mid; }
    const uint32_t q = pos[t];
    indices[2 * (size_t)q] = (int32_t)iA[lo];
    indices[2 * (size_t)q + 1] = cellI[t];
    overlaps[q] = area[t];
}

// The build from device arrays: candidate ranges, one clip per candidate pair, compaction.  g's arrays and iA [npoly] are in
// HBM and stay the caller's; work space comes from the arena, which the caller has reset.  stream_clip picks the clip kernel.
void exgrid_generate_device(const GridGenView &g, const int64_t *iA, bool stream_clip, ibh_exgrid *out, hipStream_t st) {
    Arena &A = arena();
    const int T = 256, np = g.npoly;
    out->nX = 0;
    if (np == 0) return;
    CandRange *rng = A.get<CandRange>((size_t)np);
    uint32_t *cnt = A.get<uint32_t>((size_t)np + 1), *candptr = A.get<uint32_t>((size_t)np + 1);
    hipLaunchKernelGGL(k_gg_ranges, dim3(ceil_div(np, T)), dim3(T), 0, st, g, rng, cnt);
    exclusive_scan_u32(cnt, candptr, (size_t)np, candptr + np, st);
    uint32_t ncand = 0;
    readback_sync(&ncand, candptr + np, sizeof(uint32_t), st);
    IBH_CHECK(ncand < (1u << 31), "too many candidate pairs");
    if (ncand == 0) return;
    double *area = A.get<double>(ncand);
    uint32_t *keep = A.get<uint32_t>((size_t)ncand + 1), *pos = A.get<uint32_t>((size_t)ncand + 1);
    int32_t *cellI = A.get<int32_t>(ncand);
    if (stream_clip) hipLaunchKernelGGL(k_gg_clip_stream, dim3(ceil_div(ncand, T)), dim3(T), 0, st, g, rng, candptr, ncand, area, keep, cellI);
    else hipLaunchKernelGGL(k_gg_clip, dim3(ceil_div(ncand, T)), dim3(T), 0, st, g, rng, candptr, ncand, area, keep, cellI);
    exclusive_scan_u32(keep, pos, ncand, pos + ncand, st);
    uint32_t nX = 0;
    readback_sync(&nX, pos + ncand, sizeof(uint32_t), st);
    out->nX = nX;
    out->indices.alloc(2 * (size_t)nX); out->overlaps.alloc(nX);
    if (nX) hipLaunchKernelGGL(k_gg_emit, dim3(ceil_div(ncand, T)), dim3(T), 0, st, iA, candptr, np, ncand, area, keep, pos, cellI,
                               out->indices.p, out->overlaps.p);
    IBH_HIP(hipGetLastError());
    IBH_HIP(hipStreamSynchronize(st));
}

void check_ice_edges(int nx, int ny, const double *xedges, const double *yedges) {
    IBH_CHECK(nx > 0 && ny > 0 && xedges && yedges, "ice grid: bad sizes / null edges");
    IBH_CHECK((int64_t)nx * ny < (1ll << 31), "nI overflows int32");
    for (int k = 0; k < nx; ++k) IBH_CHECK(xedges[k + 1] > xedges[k], "x edges must be ascending");
    for (int k = 0; k < ny; ++k) IBH_CHECK(yedges[k + 1] > yedges[k], "y edges must be ascending");
}

// Convex, as k_gg_clip's arrays need it: clip_axis adds one vertex per run of outside vertices, a convex n-gon has at most one
// such run per half-plane (n + 4 <= GG_CLIPV), a non-convex one can have n / 2.  The test: no two turn cross products of
// opposite strict sign, and the edge directions wind once -- at most two strict sign changes of the edges' x components and
// of their y components round the cycle (a {16/7} star turns the same way everywhere and winds seven times).  The count of
// runs follows from the sign changes alone, and the sign of a rounded difference is exact.  Zero tolerance, and a cross product
// that is not finite is "no": a wrong "no" only picks the streamed kernel.  Either orientation passes.
static bool gg_convex(const double *x, const double *y, int n) {
    bool pos = false, neg = false;
    int chg[2] = {0, 0}, first[2] = {0, 0}, last[2] = {0, 0};      // per axis: sign changes, first and latest non-zero sign
    for (int k = 0; k < n; ++k) {
        const int k1 = k + 1 == n ? 0 : k + 1, k2 = k1 + 1 == n ? 0 : k1 + 1;
        const double e[2] = {x[k1] - x[k], y[k1] - y[k]}, f[2] = {x[k2] - x[k1], y[k2] - y[k1]};
        const double c = e[0] * f[1] - e[1] * f[0];
        if (!(c - c == 0)) return false;
        pos |= c > 0; neg |= c < 0;
        for (int a = 0; a < 2; ++a) {
            const int s = e[a] > 0 ? 1 : e[a] < 0 ? -1 : 0;
            if (!s) continue;
            if (last[a] && s != last[a]) ++chg[a];
            if (!first[a]) first[a] = s;
            last[a] = s;
        }
    }
    for (int a = 0; a < 2; ++a)
        if (first[a] && last[a] != first[a]) ++chg[a];             // the cycle closes
    return !(pos && neg) && chg[0] <= 2 && chg[1] <= 2;
}

void exgrid_generate(const ibh_exgrid_desc *d, ibh_exgrid *out) {
    check_ice_edges(d->nx, d->ny, d->xedges, d->yedges);
    IBH_CHECK(d->npoly >= 0 && (d->npoly == 0 || (d->polyptr && d->vx && d->vy && d->iA)), "null polygon arrays");
    int maxv = 0, first_nonconvex = -1;
    for (int p = 0; p < d->npoly; ++p) {
        const int n = d->polyptr[p + 1] - d->polyptr[p];
        IBH_CHECK(n >= 3, "polygon %d has %d vertices (3 or more needed)", p, n);
        maxv = std::max(maxv, n);
        IBH_CHECK(d->iA[p] >= 0 && d->iA[p] < (1ll << 31), "polygon %d: iA out of range", p);
        IBH_CHECK(p == 0 || d->iA[p] > d->iA[p - 1], "polygons must come in ascending iA order (cells.sorted(), AbbrGrid.cpp:15)");
        if (first_nonconvex < 0 && n <= GG_MAXV && !gg_convex(d->vx + d->polyptr[p], d->vy + d->polyptr[p], n)) first_nonconvex = p;
    }
    // the array kernel for every call it can take (convex polygons of <= GG_MAXV vertices), the streamed one for the rest;
    // gridgen_stream_clip forces one
    const int forced = get_tuning("gridgen_stream_clip", -1);
    IBH_CHECK(forced != 0 || maxv <= GG_MAXV, "gridgen_stream_clip=0: a polygon has %d vertices, the array kernel takes 3..%d", maxv, GG_MAXV);
    IBH_CHECK(forced != 0 || first_nonconvex < 0, "gridgen_stream_clip=0: polygon %d is not convex, the array kernel takes convex polygons only",
              first_nonconvex);
    const bool stream_clip = forced >= 0 ? forced != 0 : maxv > GG_MAXV || first_nonconvex >= 0;
    hipStream_t st = nullptr;
    Arena &A = arena();
    A.reset();
    const int np = d->npoly;
    out->nX = 0;
    if (np == 0) return;
    const int nv = d->polyptr[np];
    double *xe = A.get<double>((size_t)d->nx + 1), *ye = A.get<double>((size_t)d->ny + 1);
    double *vx = A.get<double>((size_t)nv), *vy = A.get<double>((size_t)nv);
    int32_t *pp = A.get<int32_t>((size_t)np + 1);
    int64_t *iA = A.get<int64_t>((size_t)np);
    IBH_HIP(hipMemcpyAsync(xe, d->xedges, sizeof(double) * ((size_t)d->nx + 1), hipMemcpyHostToDevice, st));
    IBH_HIP(hipMemcpyAsync(ye, d->yedges, sizeof(double) * ((size_t)d->ny + 1), hipMemcpyHostToDevice, st));
    IBH_HIP(hipMemcpyAsync(vx, d->vx, sizeof(double) * (size_t)nv, hipMemcpyHostToDevice, st));
    IBH_HIP(hipMemcpyAsync(vy, d->vy, sizeof(double) * (size_t)nv, hipMemcpyHostToDevice, st));
    IBH_HIP(hipMemcpyAsync(pp, d->polyptr, sizeof(int32_t) * ((size_t)np + 1), hipMemcpyHostToDevice, st));
    IBH_HIP(hipMemcpyAsync(iA, d->iA, sizeof(int64_t) * (size_t)np, hipMemcpyHostToDevice, st));
    GridGenView g{xe, ye, d->nx, d->ny, d->x_fastest, pp, vx, vy, np};
    exgrid_generate_device(g, iA, stream_clip, out, st);
}

// the same under lon/lat cells already projected in HBM (lonlat.hip): always the streamed clip -- a cap has nlon * points_in_side vertices
void exgrid_generate_polys(int nx, int ny, const double *xedges, const double *yedges, int x_fastest, int npoly, const int32_t *d_polyptr,
                           const double *d_vx, const double *d_vy, const int64_t *d_iA, ibh_exgrid *out, hipStream_t st) {
    check_ice_edges(nx, ny, xedges, yedges);
    Arena &A = arena();
    A.reset();
    double *xe = A.get<double>((size_t)nx + 1), *ye = A.get<double>((size_t)ny + 1);
    IBH_HIP(hipMemcpyAsync(xe, xedges, sizeof(double) * ((size_t)nx + 1), hipMemcpyHostToDevice, st));
    IBH_HIP(hipMemcpyAsync(ye, yedges, sizeof(double) * ((size_t)ny + 1), hipMemcpyHostToDevice, st));
    GridGenView g{xe, ye, nx, ny, x_fastest, d_polyptr, d_vx, d_vy, npoly};
    exgrid_generate_device(g, d_iA, true, out, st);
}

}  // namespace ibh
