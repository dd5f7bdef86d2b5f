// lonlat.hip -- from grid specs to a regridder: the realised cells of a GridSpec_LonLat as projected polygons, with their areas.
//
// Replaces, for the regrid path, make_grid (slib/icebin/gridgen/GridGen_LonLat.cpp:109-232: the lon/lat polygons of the
// realised cells, points_in_side points per side, the polar caps), the projection the reference does through proj.4 (OCell,
// GridGen_Exchange.cpp:56-72; IceRegridder::init, IceRegridder.cpp:109-118) and the two areas every correctA branch reads:
// native_area (graticule_area_exact / polar_graticule_area_exact, GridGen_LonLat.cpp:79-102) and Cell::proj_area
// (Grid.cpp:42-71).  One lane per (cell, vertex) makes the lon/lat point with the reference's own expressions and projects
// it; one lane per cell takes the areas.  Everything stays in HBM: gridgen.hip's streamed clip reads the polygons where they
// lie and ibh_regridder_create_lonlat adopts the exchange grid it writes.
//
// The projection is proj.4's `stere` (Snyder 1987, ch. 21, in the form of PJ_stere.c), the only one the reference's grid
// generators name (gridgen/searise_grid.cpp:113,119, pism2_grid.cpp:97,104, mar_grid.cpp:116).  Operation order of
// stere_forward, every operation rounded on its own (-ffp-contract=off); D2R = M_PI / 180, angles in radians:
//   phi = lat * D2R;  dl = (lon - lon_0) * D2R;
//   ellipsoid, polar:    south pole: phi = -phi (dl is left alone: x keeps its sign, y changes it);  s = sin(phi);
//                        t = tan(pi/4 - .5*phi) / pow((1 - e*s) / (1 + e*s), .5*e);  r = a * (akm1 * t);
//                        x = r * sin(dl) + x_0;  y = (north: -(r * cos(dl)), south: r * cos(dl)) + y_0;
//   ellipsoid, oblique:  s = sin(phi);  X = 2 * atan(tan(pi/4 + .5*phi) * pow((1 - e*s) / (1 + e*s), .5*e)) - pi/2;
//                        sX = sin(X), cX = cos(X), cl = cos(dl);
//                        A = akm1 / (cosX1 * (1 + sinX1*sX + (cosX1*cX)*cl));
//                        x = ((a * A) * cX) * sin(dl) + x_0;  y = (a * A) * (cosX1*sX - (sinX1*cX)*cl) + y_0;
//   sphere, polar:       as the ellipsoid's with t = tan(pi/4 - .5*phi);
//   sphere, oblique:     s = sin(phi), c = cos(phi), cl = cos(dl);  k = akm1 / (1 + sinph0*s + (cosph0*c)*cl);
//                        x = ((a * k) * c) * sin(dl) + x_0;  y = (a * k) * (cosph0*s - (sinph0*c)*cl) + y_0.
// akm1, e, X1 are made once on the host (stere_setup).
#include <cmath>
#include <cstring>
#include <memory>
#include <string>

#include "prims.h"

struct ibh_lonlat_cells {
    int device = 0;
    int32_t ncell = 0;
    int64_t nvert = 0, nA = 0;
    bool has_lonlat = false;
    ibh::DevBuf<int64_t> iA;            // [ncell] the realised sparse indices, ascending
    ibh::DevBuf<int32_t> polyptr;       // [ncell+1]
    ibh::DevBuf<double> vx, vy;         // [nvert] projected
    ibh::DevBuf<double> lon, lat;       // [nvert] (keep_lonlat)
    ibh::DevBuf<double> native_area, proj_area;      // [ncell]
};

namespace ibh {

constexpr double LL_D2R = M_PI / 180.0;
constexpr double LL_HALFPI = M_PI / 2, LL_FORTPI = M_PI / 4;

enum { STERE_NORTH = 0, STERE_SOUTH = 1, STERE_OBLIQUE = 2 };
struct StereProj {
    int mode, sphere;
    double a, e, lon_0, akm1, sinX1, cosX1, x_0, y_0;      // sphere, oblique: sinX1 / cosX1 hold sin / cos of lat_0
};

__host__ __device__ inline void stere_forward(const StereProj &P, double lon, double lat, double &x, double &y) {
    double phi = lat * LL_D2R, dl = (lon - P.lon_0) * LL_D2R;
    if (P.mode != STERE_OBLIQUE) {
        if (P.mode == STERE_SOUTH) phi = -phi;      // PJ_stere.c S_POLE: phi and cos(lam) change sign, sin(lam) does not
        double t = tan(LL_FORTPI - .5 * phi);
        if (!P.sphere) {
            const double s = sin(phi);
            t = t / pow((1 - P.e * s) / (1 + P.e * s), .5 * P.e);
        }
        const double r = P.a * (P.akm1 * t);
        x = r * sin(dl) + P.x_0;
        const double rc = r * cos(dl);
        y = (P.mode == STERE_NORTH ? -rc : rc) + P.y_0;
    } else if (!P.sphere) {
        const double s = sin(phi);
        const double X = 2 * atan(tan(LL_FORTPI + .5 * phi) * pow((1 - P.e * s) / (1 + P.e * s), .5 * P.e)) - LL_HALFPI;
        const double sX = sin(X), cX = cos(X), cl = cos(dl);
        const double A = P.akm1 / (P.cosX1 * (1 + P.sinX1 * sX + (P.cosX1 * cX) * cl));
        x = ((P.a * A) * cX) * sin(dl) + P.x_0;
        y = (P.a * A) * (P.cosX1 * sX - (P.sinX1 * cX) * cl) + P.y_0;
    } else {
        const double s = sin(phi), c = cos(phi), cl = cos(dl);
        const double k = P.akm1 / (1 + P.sinX1 * s + (P.cosX1 * c) * cl);
        x = ((P.a * k) * c) * sin(dl) + P.x_0;
        y = (P.a * k) * (P.cosX1 * s - (P.sinX1 * c) * cl) + P.y_0;
    }
}

static double stere_tsfn(double phi, double e) {      // t(phi) of the polar form
    const double s = sin(phi);
    return tan(LL_FORTPI - .5 * phi) / pow((1 - e * s) / (1 + e * s), .5 * e);
}

static StereProj stere_setup(const ibh_stere_params *p) {
    IBH_CHECK(p != nullptr, "null projection");
    IBH_CHECK(std::isfinite(p->a) && std::isfinite(p->b) && p->a > 0 && p->b > 0 && p->b <= p->a, "stere: bad semi-axes a=%g b=%g", p->a, p->b);
    IBH_CHECK(std::isfinite(p->lat_0) && std::fabs(p->lat_0) <= 90, "stere: lat_0=%g outside [-90, 90]", p->lat_0);
    IBH_CHECK(std::isfinite(p->lon_0) && std::isfinite(p->x_0) && std::isfinite(p->y_0), "stere: non-finite lon_0 / x_0 / y_0");
    IBH_CHECK(std::isfinite(p->k_0) && p->k_0 > 0, "stere: k_0=%g is not positive", p->k_0);
    IBH_CHECK(!p->has_lat_ts || (std::isfinite(p->lat_ts) && std::fabs(p->lat_ts) <= 90), "stere: lat_ts=%g outside [-90, 90]", p->lat_ts);
    StereProj P{};
    P.a = p->a; P.lon_0 = p->lon_0; P.x_0 = p->x_0; P.y_0 = p->y_0;
    P.sphere = p->a == p->b;
    P.e = P.sphere ? 0.0 : sqrt(1 - (p->b * p->b) / (p->a * p->a));
    const double e = P.e, phi0 = p->lat_0 * LL_D2R;
    P.mode = std::fabs(p->lat_0) == 90 ? (p->lat_0 > 0 ? STERE_NORTH : STERE_SOUTH) : STERE_OBLIQUE;
    if (P.mode != STERE_OBLIQUE) {
        const bool ts = p->has_lat_ts && std::fabs(p->lat_ts) != 90;
        const double phits = std::fabs(p->lat_ts) * LL_D2R;
        if (P.sphere) P.akm1 = ts ? cos(phits) / tan(LL_FORTPI - .5 * phits) : 2 * p->k_0;
        else if (ts) {
            const double s = sin(phits);
            P.akm1 = cos(phits) / stere_tsfn(phits, e) / sqrt(1 - (e * e) * (s * s));
        } else P.akm1 = 2 * p->k_0 / sqrt(pow(1 + e, 1 + e) * pow(1 - e, 1 - e));
    } else if (P.sphere) {
        P.akm1 = 2 * p->k_0;
        P.sinX1 = sin(phi0); P.cosX1 = cos(phi0);
    } else {
        const double s = sin(phi0);
        const double X1 = 2 * atan(tan(LL_FORTPI + .5 * phi0) * pow((1 - e * s) / (1 + e * s), .5 * e)) - LL_HALFPI;
        P.akm1 = 2 * p->k_0 * cos(phi0) / sqrt(1 - (e * e) * (s * s));
        P.sinX1 = sin(X1); P.cosX1 = cos(X1);
    }
    return P;
}

// "+proj=stere +lat_0=90 ..." -> ibh_stere_params; anything it does not know is IBH_EINVAL, naming the key
static void parse_sproj(const char *sproj, ibh_stere_params *out) {
    IBH_CHECK(sproj && out, "null argument");
    ibh_stere_params p{};
    p.k_0 = 1;
    bool has_proj = false, has_a = false, has_b = false, has_R = false, wgs84 = false;
    const std::string s(sproj);
    size_t i = 0;
    while (i < s.size()) {
        while (i < s.size() && isspace((unsigned char)s[i])) ++i;
        size_t j = i;
        while (j < s.size() && !isspace((unsigned char)s[j])) ++j;
        if (j == i) break;
        std::string tok = s.substr(i, j - i);
        i = j;
        if (tok[0] == '+') tok.erase(0, 1);
        const size_t eq = tok.find('=');
        const std::string key = tok.substr(0, eq), val = eq == std::string::npos ? "" : tok.substr(eq + 1);
        auto num = [&](double &dst) {
            char *end = nullptr;
            dst = strtod(val.c_str(), &end);
            IBH_CHECK(!val.empty() && end && *end == 0 && std::isfinite(dst), "sproj: key '%s' has no numeric value ('%s')", key.c_str(), val.c_str());
        };
        if (key == "proj") { IBH_CHECK(val == "stere", "sproj: key 'proj' is '%s'; only stere is supported", val.c_str()); has_proj = true; }
        else if (key == "lat_0") num(p.lat_0);
        else if (key == "lon_0") num(p.lon_0);
        else if (key == "lat_ts") { num(p.lat_ts); p.has_lat_ts = 1; }
        else if (key == "k" || key == "k_0") num(p.k_0);
        else if (key == "x_0") num(p.x_0);
        else if (key == "y_0") num(p.y_0);
        else if (key == "ellps" || key == "datum") {
            IBH_CHECK(val == "WGS84", "sproj: key '%s' is '%s'; only WGS84 is supported", key.c_str(), val.c_str());
            wgs84 = true;
        }
        else if (key == "a") { num(p.a); has_a = true; }
        else if (key == "b") { num(p.b); has_b = true; }
        else if (key == "R") { num(p.a); p.b = p.a; has_R = true; }
        else if (key == "units") IBH_CHECK(val == "m", "sproj: key 'units' is '%s'; only m is supported", val.c_str());
        else if (key == "no_defs") IBH_CHECK(eq == std::string::npos, "sproj: key 'no_defs' takes no value");
        else fail(IBH_EINVAL, "sproj: unknown key '%s'", key.c_str());
    }
    IBH_CHECK(has_proj, "sproj: key 'proj' is missing");
    if (has_R) IBH_CHECK(!has_a && !has_b && !wgs84, "sproj: key 'R' excludes a, b, ellps and datum");
    else if (has_a || has_b) {
        IBH_CHECK(has_a && !wgs84, "sproj: key 'b' needs 'a' (and excludes ellps / datum)");
        if (!has_b) p.b = p.a;
    } else {
        p.a = 6378137.0;
        p.b = p.a * (1 - 1 / 298.257223563);
    }
    *out = p;
}

// ---- the cells -------------------------------------------------------------------------------------------------------
struct LonLatSpec {
    const double *lonb, *latb;      // device: [nlon+1], [nlatb]
    int nlon, nlatb, nlat;          // nlat = nlatb - 1 + sp + np (GridSpec.cpp:231-243)
    int lat_slowest;                // indices {1,0}: index = j*nlon + i; else {0,1}: index = i*nlat + j
    int sp, np, n;                  // caps; points_in_side
    double eq_rad;
};
enum { LL_CELL = 0, LL_SOUTH = 1, LL_NORTH = 2, LL_NONE = 3 };
// the cell a sparse index names (GridGen_LonLat.cpp:136-138,180-182,202): kind, and for an ordinary cell (ilon, ilat) into lonb / latb
__host__ __device__ inline int ll_decode(const LonLatSpec &S, int64_t idx, int &ilon, int &ilat) {
    if (S.np && idx == (int64_t)S.nlat * S.nlon + (S.nlon - 1)) return LL_NORTH;
    if (S.sp && idx == 0) return LL_SOUTH;
    if (idx < 0 || idx >= (int64_t)S.nlon * S.nlat) return LL_NONE;
    const int i = (int)(S.lat_slowest ? idx % S.nlon : idx / S.nlat), j = (int)(S.lat_slowest ? idx / S.nlon : idx % S.nlat);
    ilon = i; ilat = j - S.sp;
    return ilat >= 0 && ilat < S.nlatb - 1 ? LL_CELL : LL_NONE;
}
__host__ __device__ inline int ll_nvert(const LonLatSpec &S, int kind) { return kind == LL_CELL ? 4 * S.n : S.nlon * S.n; }

__global__ void k_ll_vertices(LonLatSpec S, StereProj P, const int64_t *__restrict__ iA, const int32_t *__restrict__ polyptr, int ncell,
                              int64_t nvert, double *__restrict__ vx, double *__restrict__ vy, double *__restrict__ olon,
                              double *__restrict__ olat) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nvert) return;
    int lo = 0, hi = ncell;                        // cell c with polyptr[c] <= v < polyptr[c+1]
    while (lo + 1 < hi) { const int mid = (lo + hi) >> 1; if (polyptr[mid] <= v) lo = mid; else hi = mid; }
    const int k = (int)(v - polyptr[lo]), n = S.n;
    int ilon = 0, ilat = 0;
    const int kind = ll_decode(S, iA[lo], ilon, ilat);
    double lon, lat;
    if (kind == LL_CELL) {                         // :144-169: lons[i] = lon0 + (lon1-lon0) * ((double)i/(double)n), four sides
        const double lon0 = S.lonb[ilon], lon1 = S.lonb[ilon + 1], lat0 = S.latb[ilat], lat1 = S.latb[ilat + 1];
        const int side = k / n, i = k % n;
        const int q = side < 2 ? i : n - i;
        const double f = (double)q / (double)n;
        if (side == 0)      { lon = lon0 + (lon1 - lon0) * f; lat = lat0; }
        else if (side == 1) { lon = lon1; lat = lat0 + (lat1 - lat0) * f; }
        else if (side == 2) { lon = lon0 + (lon1 - lon0) * f; lat = lat1; }
        else                { lon = lon0; lat = lat0 + (lat1 - lat0) * f; }
    } else {                                       // :184-193 north, :206-215 south (lonb walked downwards: counter-clockwise)
        const int seg = k / n, i = k % n;
        const int i0 = kind == LL_NORTH ? seg : S.nlon - seg, i1 = kind == LL_NORTH ? seg + 1 : S.nlon - seg - 1;
        const double lon0 = S.lonb[i0], lon1 = S.lonb[i1];
        lon = lon0 + (lon1 - lon0) * ((double)i / (double)n);
        lat = kind == LL_NORTH ? S.latb[S.nlatb - 1] : S.latb[0];
    }
    if (olon) { olon[v] = lon; olat[v] = lat; }
    double x, y;
    stere_forward(P, lon, lat, x, y);
    vx[v] = x; vy[v] = y;
}

__device__ __forceinline__ double ll_loncorrect(double lon, double min) {      // gridgen/gridutil.hpp:46-54
    const double max = min + 360.0;
    while (lon >= max) lon -= 360.0;
    while (lon < min) lon += 360.0;
    return lon;
}
__global__ void k_ll_areas(LonLatSpec S, const int64_t *__restrict__ iA, const int32_t *__restrict__ polyptr, int ncell,
                           const double *__restrict__ vx, const double *__restrict__ vy, double *__restrict__ native_area,
                           double *__restrict__ proj_area) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncell) return;
    int ilon = 0, ilat = 0;
    const int kind = ll_decode(S, iA[c], ilon, ilat);
    double nat;
    if (kind == LL_CELL) {                         // graticule_area_exact, :79-92
        const double dlon = ll_loncorrect(S.lonb[ilon + 1] - S.lonb[ilon], 0) * LL_D2R;
        const double lat0 = S.latb[ilat] * LL_D2R, lat1 = S.latb[ilat + 1] * LL_D2R;
        nat = dlon * (S.eq_rad * S.eq_rad) * (sin(lat1) - sin(lat0));
    } else {                                       // polar_graticule_area_exact, :96-102, radius 90 - lat (north), 90 + lat (south)
        const double theta = (kind == LL_NORTH ? 90.0 - S.latb[S.nlatb - 1] : 90.0 + S.latb[0]) * LL_D2R;
        nat = 2.0 * M_PI * (S.eq_rad * S.eq_rad) * (1.0 - cos(theta));
    }
    native_area[c] = nat;
    const int k0 = polyptr[c], k1 = polyptr[c + 1];      // Cell::proj_area, Grid.cpp:42-71: from the last vertex
    double ret = 0, x0 = vx[k1 - 1], y0 = vy[k1 - 1];
    for (int k = k0; k < k1; ++k) {
        const double x1 = vx[k], y1 = vy[k];
        ret += (x0 * y1) - (x1 * y0);
        x0 = x1; y0 = y1;
    }
    proj_area[c] = ret * .5;
}

__global__ void k_ll_project(StereProj P, int64_t n, const double *__restrict__ lon, const double *__restrict__ lat,
                             double *__restrict__ x, double *__restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double px, py;
    stere_forward(P, lon[i], lat[i], px, py);
    x[i] = px; y[i] = py;
}

__global__ void k_ll_centroids(const double *__restrict__ xe, const double *__restrict__ ye, int nx, int ny, int x_fastest,
                               double *__restrict__ cen) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)nx * ny) return;
    const int ix = (int)(x_fastest ? i % nx : i / ny), iy = (int)(x_fastest ? i / nx : i % ny);
    cen[2 * i] = .5 * (xe[ix] + xe[ix + 1]);
    cen[2 * i + 1] = .5 * (ye[iy] + ye[iy + 1]);
}

static void lonlat_cells_create(const ibh_lonlat_cells_desc *d, ibh_lonlat_cells **out) {
    IBH_CHECK(d != nullptr, "null argument");
    IBH_CHECK(d->nlonb >= 2 && d->nlatb >= 2 && d->lonb && d->latb, "lon/lat spec: needs at least two boundaries each");
    IBH_CHECK(d->points_in_side >= 1 && d->points_in_side <= 4096, "lon/lat spec: points_in_side=%d (1..4096)", d->points_in_side);
    IBH_CHECK((d->indices[0] == 0 && d->indices[1] == 1) || (d->indices[0] == 1 && d->indices[1] == 0),
              "lon/lat spec: indices {%d,%d} is neither {0,1} nor {1,0}", d->indices[0], d->indices[1]);
    IBH_CHECK(std::isfinite(d->eq_rad) && d->eq_rad > 0, "lon/lat spec: eq_rad=%g", d->eq_rad);
    for (int k = 0; k < d->nlonb; ++k) {
        IBH_CHECK(std::isfinite(d->lonb[k]) && std::fabs(d->lonb[k]) <= 720, "lon/lat spec: lonb[%d]=%g outside [-720, 720]", k, d->lonb[k]);
        IBH_CHECK(k == 0 || d->lonb[k] > d->lonb[k - 1], "lon/lat spec: lonb must be ascending");
    }
    for (int k = 0; k < d->nlatb; ++k) {
        IBH_CHECK(std::isfinite(d->latb[k]) && std::fabs(d->latb[k]) <= 90, "lon/lat spec: latb[%d]=%g outside [-90, 90]", k, d->latb[k]);
        IBH_CHECK(k == 0 || d->latb[k] > d->latb[k - 1], "lon/lat spec: latb must be ascending");
    }
    const StereProj P = stere_setup(d->proj);
    LonLatSpec S{};
    S.nlon = d->nlonb - 1; S.nlatb = d->nlatb;
    S.sp = d->south_pole ? 1 : 0; S.np = d->north_pole ? 1 : 0;
    S.nlat = d->nlatb - 1 + S.sp + S.np;
    S.lat_slowest = d->indices[0] == 1;
    S.n = d->points_in_side; S.eq_rad = d->eq_rad;
    const int64_t nA = (int64_t)S.nlon * (S.nlat + S.np);
    IBH_CHECK(nA < (1ll << 31), "lon/lat spec: %lld cells overflow int32", (long long)nA);
    IBH_CHECK(d->nrealised >= 0 && d->nrealised <= nA && (d->nrealised == 0 || d->realised), "realised: bad count / null array");
    const int32_t nc = (int32_t)d->nrealised;
    std::vector<int32_t> pp((size_t)nc + 1, 0);
    for (int32_t c = 0; c < nc; ++c) {
        IBH_CHECK(c == 0 || d->realised[c] > d->realised[c - 1], "realised must be strictly ascending (entry %d)", c);
        int ilon, ilat;
        const int kind = ll_decode(S, d->realised[c], ilon, ilat);
        IBH_CHECK(kind != LL_NONE, "realised[%d]=%lld is no cell of the spec", c, (long long)d->realised[c]);
        const int64_t next = (int64_t)pp[c] + ll_nvert(S, kind);
        IBH_CHECK(next < (1ll << 31), "too many polygon vertices");
        pp[(size_t)c + 1] = (int32_t)next;
    }
    require_device();
    std::unique_ptr<ibh_lonlat_cells> h(new ibh_lonlat_cells);
    IBH_HIP(hipGetDevice(&h->device));
    h->ncell = nc; h->nvert = pp[nc]; h->nA = nA; h->has_lonlat = d->keep_lonlat != 0;
    hipStream_t st = nullptr;
    DevBuf<double> lonb, latb;
    lonb.upload(d->lonb, (size_t)d->nlonb, st); latb.upload(d->latb, (size_t)d->nlatb, st);
    S.lonb = lonb.p; S.latb = latb.p;
    h->iA.upload(d->realised, (size_t)nc, st);
    h->polyptr.upload(pp.data(), pp.size(), st);
    h->vx.alloc((size_t)h->nvert); h->vy.alloc((size_t)h->nvert);
    h->native_area.alloc((size_t)nc); h->proj_area.alloc((size_t)nc);
    if (h->has_lonlat) { h->lon.alloc((size_t)h->nvert); h->lat.alloc((size_t)h->nvert); }
    if (nc) {
        const int T = 256;
        hipLaunchKernelGGL(k_ll_vertices, dim3(ceil_div(h->nvert, T)), dim3(T), 0, st, S, P, h->iA.p, h->polyptr.p, nc, h->nvert, h->vx.p,
                           h->vy.p, h->has_lonlat ? h->lon.p : nullptr, h->has_lonlat ? h->lat.p : nullptr);
        hipLaunchKernelGGL(k_ll_areas, dim3(ceil_div(nc, T)), dim3(T), 0, st, S, h->iA.p, h->polyptr.p, nc, h->vx.p, h->vy.p,
                           h->native_area.p, h->proj_area.p);
        IBH_HIP(hipGetLastError());
    }
    IBH_HIP(hipStreamSynchronize(st));      // lonb / latb go back to the pool below
    *out = h.release();
}

static void check_cells_device(const ibh_lonlat_cells *c) {
    IBH_CHECK(c != nullptr, "null cells handle");
    int dev = -1;
    IBH_HIP(hipGetDevice(&dev));
    IBH_CHECK(dev == c->device, "cells handle belongs to device %d, current device is %d", c->device, dev);
}

static void regridder_create_lonlat(const ibh_lonlat_regridder_desc *d, ibh_sparse_set *dimA_out, ibh_regridder **out) {
    IBH_CHECK(d && out, "null argument");
    const ibh_lonlat_cells *c = d->cells;
    check_cells_device(c);
    IBH_CHECK(!dimA_out || dimA_out->n() == 0, "dimA_out must be an empty set");
    IBH_CHECK(d->nhc >= 0 && (d->nhc == 0 || d->hcdefs), "null hcdefs");
    IBH_CHECK(c->nA * (int64_t)(d->nhc > 0 ? d->nhc : 1) < (1ll << 31), "nE = nA*nhc overflows int32 dense ids");
    IBH_CHECK(d->interp_style == 0 || d->interp_style == 1, "unknown interp_style %d", d->interp_style);
    for (int k = 1; k < d->nhc; ++k) IBH_CHECK(d->hcdefs[k] > d->hcdefs[k - 1], "hcdefs must be ascending");
    if (d->nhc > 0) {
        const bool hc_slowest = d->hc_stride_A == 1 && d->hc_stride_HC == c->nA;
        const bool hc_fastest = d->hc_stride_HC == 1 && d->hc_stride_A == d->nhc;
        IBH_CHECK(hc_slowest || hc_fastest, "indexingHC strides (%ld,%ld) are neither (1,nA) nor (nhc,1)", (long)d->hc_stride_A,
                  (long)d->hc_stride_HC);
    }
    hipStream_t st = nullptr;
    ibh_exgrid ex;
    exgrid_generate_polys(d->nx, d->ny, d->xedges, d->yedges, d->x_fastest, c->ncell, c->polyptr.p, c->vx.p, c->vy.p, c->iA.p, &ex, st);
    IBH_CHECK(ex.nX < (1ll << 31) - 1, "nX=%ld out of range", (long)ex.nX);
    const int64_t nI = (int64_t)d->nx * d->ny;
    std::unique_ptr<ibh_regridder> g(new ibh_regridder);
    g->device = c->device;
    g->nX = ex.nX; g->nI = nI; g->nA = c->nA; g->nA_dense = c->ncell; g->nhc = d->nhc;
    g->interp_style = d->interp_style; g->hc_stride_A = d->hc_stride_A; g->hc_stride_HC = d->hc_stride_HC;
    g->hcdefs_h.assign(d->hcdefs, d->hcdefs + d->nhc);
    g->hcdefs.upload(d->hcdefs, (size_t)d->nhc, st);
    // agridA on the host, as every regridder keeps it (wA()): per GCM cell, no polygon and no exchange cell
    const size_t nc = (size_t)c->ncell;
    g->A_to_sparse.resize(nc); g->A_native.resize(nc); g->A_proj.resize(nc);
    c->iA.download(g->A_to_sparse.data(), nc, st);
    c->native_area.download(g->A_native.data(), nc, st);
    c->proj_area.download(g->A_proj.data(), nc, st);
    std::vector<double> ratio((size_t)c->nA, 0.0);
    for (size_t id = 0; id < nc; ++id) {
        const int64_t s = g->A_to_sparse[id];
        const double r = g->A_native[id] / g->A_proj[id];
        IBH_CHECK(std::isfinite(r) && r > 0, "atmosphere cell %ld: native/proj area ratio %g is not positive", (long)s, r);
        ratio[(size_t)s] = r;
    }
    g->A_ratio_s.upload(ratio.data(), ratio.size(), st);
    // the ice cells' centres, from the edges (the arena still holds the copies exgrid_generate_polys made, but not by contract)
    DevBuf<double> xe, ye;
    xe.upload(d->xedges, (size_t)d->nx + 1, st); ye.upload(d->yedges, (size_t)d->ny + 1, st);
    g->I_centroid.alloc(2 * (size_t)nI);
    hipLaunchKernelGGL(k_ll_centroids, dim3(ceil_div(nI, 256)), dim3(256), 0, st, xe.p, ye.p, d->nx, d->ny, d->x_fastest, g->I_centroid.p);
    IBH_HIP(hipGetLastError());
    g->has_centroid = true;
    g->cmin[0] = .5 * (d->xedges[0] + d->xedges[1]); g->cmax[0] = .5 * (d->xedges[d->nx - 1] + d->xedges[d->nx]);
    g->cmin[1] = .5 * (d->yedges[0] + d->yedges[1]); g->cmax[1] = .5 * (d->yedges[d->ny - 1] + d->yedges[d->ny]);
    for (int k = 0; k < 2; ++k) IBH_CHECK(std::isfinite(g->cmin[k]) && std::isfinite(g->cmax[k]), "ice grid: non-finite edges");
    DevBuf<int64_t> dA;
    if (dimA_out) {
        dA.alloc(nc);
        if (nc) IBH_HIP(hipMemcpyAsync(dA.p, c->iA.p, sizeof(int64_t) * nc, hipMemcpyDeviceToDevice, st));
    }
    IBH_HIP(hipStreamSynchronize(st));
    g->ex_indices = std::move(ex.indices);
    g->ex_area = std::move(ex.overlaps);
    if (g->nX == 0) { g->ex_indices.alloc(0); g->ex_area.alloc(0); }
    // nothing below can fail
    if (dimA_out) dimA_out->adopt_device(std::move(dA), c->ncell, c->nA);
    *out = g.release();
}

}  // namespace ibh

using namespace ibh;

extern "C" {

int ibh_parse_sproj(const char *sproj, ibh_stere_params *out) {
    return guarded([&] { parse_sproj(sproj, out); });
}

int ibh_lonlat_project(const ibh_stere_params *proj, int64_t n, const double *lon, const double *lat, double *x, double *y) {
    return guarded([&] {
        IBH_CHECK(n >= 0 && (n == 0 || (lon && lat && x && y)), "null argument");
        const StereProj P = stere_setup(proj);
        if (n == 0) return;
        require_device();
        DevBuf<double> dlon, dlat, dx((size_t)n), dy((size_t)n);
        dlon.upload(lon, (size_t)n); dlat.upload(lat, (size_t)n);
        hipLaunchKernelGGL(k_ll_project, dim3(ceil_div(n, 256)), dim3(256), 0, nullptr, P, n, dlon.p, dlat.p, dx.p, dy.p);
        IBH_HIP(hipGetLastError());
        dx.download(x, (size_t)n); dy.download(y, (size_t)n);
    });
}

int ibh_lonlat_cells_create(const ibh_lonlat_cells_desc *desc, ibh_lonlat_cells **out) {
    return guarded([&] {
        IBH_CHECK(out != nullptr, "null argument");
        *out = nullptr;
        lonlat_cells_create(desc, out);
    });
}
int ibh_lonlat_cells_size(const ibh_lonlat_cells *c, int32_t *ncell, int64_t *nvert, int64_t *nA) {
    return guarded([&] {
        IBH_CHECK(c != nullptr, "null argument");
        if (ncell) *ncell = c->ncell;
        if (nvert) *nvert = c->nvert;
        if (nA) *nA = c->nA;
    });
}
int ibh_lonlat_cells_get(const ibh_lonlat_cells *c, int64_t *iA, int32_t *polyptr, double *vx, double *vy, double *native_area,
                         double *proj_area, double *lon, double *lat) {
    return guarded([&] {
        check_cells_device(c);
        IBH_CHECK((!lon && !lat) || c->has_lonlat, "the handle was created without keep_lonlat");
        const size_t nc = (size_t)c->ncell, nv = (size_t)c->nvert;
        if (iA) c->iA.download(iA, nc);
        if (polyptr) c->polyptr.download(polyptr, nc + 1);
        if (vx) c->vx.download(vx, nv);
        if (vy) c->vy.download(vy, nv);
        if (native_area) c->native_area.download(native_area, nc);
        if (proj_area) c->proj_area.download(proj_area, nc);
        if (lon) c->lon.download(lon, nv);
        if (lat) c->lat.download(lat, nv);
    });
}
int ibh_lonlat_cells_destroy(ibh_lonlat_cells *c) { delete c; return IBH_OK; }

int ibh_exgrid_generate_lonlat(const ibh_lonlat_cells *c, int32_t nx, int32_t ny, const double *xedges, const double *yedges,
                               int32_t x_fastest, ibh_exgrid **out) {
    return guarded([&] {
        IBH_CHECK(out != nullptr, "null argument");
        *out = nullptr;
        check_cells_device(c);
        std::unique_ptr<ibh_exgrid> ex(new ibh_exgrid);
        exgrid_generate_polys(nx, ny, xedges, yedges, x_fastest, c->ncell, c->polyptr.p, c->vx.p, c->vy.p, c->iA.p, ex.get(), nullptr);
        *out = ex.release();
    });
}

int ibh_regridder_create_lonlat(const ibh_lonlat_regridder_desc *desc, ibh_sparse_set *dimA_out, ibh_regridder **out) {
    return guarded([&] {
        if (out) *out = nullptr;
        regridder_create_lonlat(desc, dimA_out, out);
    });
}

}  // extern "C"
