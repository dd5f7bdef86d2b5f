"""A float64 statement, in the kernels' operation order, of what lonlat.hip and gridgen.hip's streamed clip compute: proj.4's
`stere` as lonlat.hip's header spells it, the lon/lat cells of make_grid (gridgen/GridGen_LonLat.cpp:109-232), their native and
projected areas, and the re-entrant Sutherland-Hodgman clip with the shoelace sum relative to the ice cell's corner.  Python
floats are IEEE doubles and every operation below rounds on its own, as the kernels' do (-ffp-contract=off); libm's sin / cos /
tan / atan / pow stand in for the device's, which differ by a few ulp."""
import math

import numpy as np

D2R = math.pi / 180.0
HALFPI, FORTPI = math.pi / 2, math.pi / 4
NORTH, SOUTH, OBLIQUE = 0, 1, 2


def tsfn(phi, e):
    s = math.sin(phi)
    return math.tan(FORTPI - .5 * phi) / math.pow((1 - e * s) / (1 + e * s), .5 * e)


def stere_setup(p):
    """p: icebin_amd.gridgen.parse_sproj's dict -> the constants stere_setup makes on the host."""
    a, b = p["a"], p["b"]
    P = dict(a=a, lon_0=p["lon_0"], x_0=p["x_0"], y_0=p["y_0"], sphere=a == b, sinX1=0., cosX1=0.)
    e = P["e"] = 0.0 if a == b else math.sqrt(1 - (b * b) / (a * a))
    phi0 = p["lat_0"] * D2R
    P["mode"] = (NORTH if p["lat_0"] > 0 else SOUTH) if abs(p["lat_0"]) == 90 else OBLIQUE
    if P["mode"] != OBLIQUE:
        ts = bool(p["has_lat_ts"]) and abs(p["lat_ts"]) != 90
        phits = abs(p["lat_ts"]) * D2R
        if P["sphere"]:
            P["akm1"] = math.cos(phits) / math.tan(FORTPI - .5 * phits) if ts else 2 * p["k_0"]
        elif ts:
            s = math.sin(phits)
            P["akm1"] = math.cos(phits) / tsfn(phits, e) / math.sqrt(1 - (e * e) * (s * s))
        else:
            P["akm1"] = 2 * p["k_0"] / math.sqrt(math.pow(1 + e, 1 + e) * math.pow(1 - e, 1 - e))
    elif P["sphere"]:
        P["akm1"] = 2 * p["k_0"]
        P["sinX1"], P["cosX1"] = math.sin(phi0), math.cos(phi0)
    else:
        s = math.sin(phi0)
        X1 = 2 * math.atan(math.tan(FORTPI + .5 * phi0) * math.pow((1 - e * s) / (1 + e * s), .5 * e)) - HALFPI
        P["akm1"] = 2 * p["k_0"] * math.cos(phi0) / math.sqrt(1 - (e * e) * (s * s))
        P["sinX1"], P["cosX1"] = math.sin(X1), math.cos(X1)
    return P


def stere_forward(P, lon, lat):
    lon, lat = float(lon), float(lat)
    phi, dl = lat * D2R, (lon - P["lon_0"]) * D2R
    a, e, akm1 = P["a"], P["e"], P["akm1"]
    if P["mode"] != OBLIQUE:
        if P["mode"] == SOUTH:
            phi = -phi
        t = math.tan(FORTPI - .5 * phi)
        if not P["sphere"]:
            s = math.sin(phi)
            t = t / math.pow((1 - e * s) / (1 + e * s), .5 * e)
        r = a * (akm1 * t)
        x = r * math.sin(dl) + P["x_0"]
        rc = r * math.cos(dl)
        return x, (-rc if P["mode"] == NORTH else rc) + P["y_0"]
    s1, c1 = P["sinX1"], P["cosX1"]
    if not P["sphere"]:
        s = math.sin(phi)
        X = 2 * math.atan(math.tan(FORTPI + .5 * phi) * math.pow((1 - e * s) / (1 + e * s), .5 * e)) - HALFPI
        sX, cX, cl = math.sin(X), math.cos(X), math.cos(dl)
        A = akm1 / (c1 * (1 + s1 * sX + (c1 * cX) * cl))
        return ((a * A) * cX) * math.sin(dl) + P["x_0"], (a * A) * (c1 * sX - (s1 * cX) * cl) + P["y_0"]
    s, c, cl = math.sin(phi), math.cos(phi), math.cos(dl)
    k = akm1 / (1 + s1 * s + (c1 * c) * cl)
    return ((a * k) * c) * math.sin(dl) + P["x_0"], (a * k) * (c1 * s - (s1 * c) * cl) + P["y_0"]


def project(P, lon, lat):
    xy = [stere_forward(P, lo, la) for lo, la in zip(np.ravel(lon), np.ravel(lat))]
    return np.array([v[0] for v in xy]), np.array([v[1] for v in xy])


# ---- the cells -----------------------------------------------------------------------------------------------------------
def decode(spec, idx):
    """('cell', ilon, ilat) | ('north',) | ('south',) | None for a sparse index (GridGen_LonLat.cpp:136-138,180-182,202)."""
    nlon, nlat, sp = spec.nlon, spec.nlat, int(spec.south_pole)
    if spec.north_pole and idx == nlat * nlon + nlon - 1:
        return ("north",)
    if spec.south_pole and idx == 0:
        return ("south",)
    if idx < 0 or idx >= nlon * nlat:
        return None
    i, j = (idx % nlon, idx // nlon) if spec.indices == (1, 0) else (idx // nlat, idx % nlat)
    ilat = j - sp
    return ("cell", int(i), int(ilat)) if 0 <= ilat < len(spec.latb) - 1 else None


def cell_lonlat(spec, idx):
    """The lon/lat vertices of one cell, in the reference's order."""
    n, lonb, latb = spec.points_in_side, [float(v) for v in spec.lonb], [float(v) for v in spec.latb]
    kind = decode(spec, idx)
    pts = []
    if kind[0] == "cell":
        _, ilon, ilat = kind
        lon0, lon1, lat0, lat1 = lonb[ilon], lonb[ilon + 1], latb[ilat], latb[ilat + 1]
        lons = [lon0 + (lon1 - lon0) * (float(i) / float(n)) for i in range(n + 1)]
        lats = [lat0 + (lat1 - lat0) * (float(i) / float(n)) for i in range(n + 1)]
        pts += [(lons[i], lat0) for i in range(n)]
        pts += [(lon1, lats[i]) for i in range(n)]
        pts += [(lons[i], lat1) for i in range(n, 0, -1)]
        pts += [(lon0, lats[i]) for i in range(n, 0, -1)]
    elif kind[0] == "north":
        for ilon in range(spec.nlon):
            lon0, lon1 = lonb[ilon], lonb[ilon + 1]
            pts += [(lon0 + (lon1 - lon0) * (float(i) / float(n)), latb[-1]) for i in range(n)]
    else:
        for ilon in range(spec.nlon, 0, -1):
            lon0, lon1 = lonb[ilon], lonb[ilon - 1]
            pts += [(lon0 + (lon1 - lon0) * (float(i) / float(n)), latb[0]) for i in range(n)]
    return pts


def loncorrect(lon, lo):
    hi = lo + 360.0
    while lon >= hi:
        lon -= 360.0
    while lon < lo:
        lon += 360.0
    return lon


def native_area(spec, idx):
    kind, R = decode(spec, idx), spec.eq_rad
    lonb, latb = [float(v) for v in spec.lonb], [float(v) for v in spec.latb]
    if kind[0] == "cell":
        _, ilon, ilat = kind
        dlon = loncorrect(lonb[ilon + 1] - lonb[ilon], 0) * D2R
        lat0, lat1 = latb[ilat] * D2R, latb[ilat + 1] * D2R
        return dlon * (R * R) * (math.sin(lat1) - math.sin(lat0))
    theta = ((90.0 - latb[-1]) if kind[0] == "north" else (90.0 + latb[0])) * D2R
    return 2.0 * math.pi * (R * R) * (1.0 - math.cos(theta))


def proj_area(x, y):
    """Cell::proj_area (Grid.cpp:42-71): from the last vertex."""
    ret, x0, y0 = 0.0, float(x[-1]), float(y[-1])
    for x1, y1 in zip(x, y):
        x1, y1 = float(x1), float(y1)
        ret += (x0 * y1) - (x1 * y0)
        x0, y0 = x1, y1
    return ret * .5


def cells(spec, realised, P):
    """dict(polyptr, lon, lat, vx, vy, native_area, proj_area) of the realised cells."""
    polyptr, lon, lat, nat, prj = [0], [], [], [], []
    for idx in realised:
        pts = cell_lonlat(spec, int(idx))
        lon += [p[0] for p in pts]
        lat += [p[1] for p in pts]
        polyptr.append(len(lon))
        nat.append(native_area(spec, int(idx)))
    vx, vy = project(P, lon, lat) if lon else (np.zeros(0), np.zeros(0))
    for c in range(len(realised)):
        prj.append(proj_area(vx[polyptr[c]:polyptr[c + 1]], vy[polyptr[c]:polyptr[c + 1]]))
    return dict(polyptr=np.asarray(polyptr, np.int32), lon=np.asarray(lon), lat=np.asarray(lat), vx=vx, vy=vy,
                native_area=np.asarray(nat), proj_area=np.asarray(prj))


# ---- the streamed clip ---------------------------------------------------------------------------------------------------
class _Clip:
    """k_gg_clip_stream's ClipState: four stages of (first, previous) and the shoelace stage."""

    def __init__(self, w, h):
        self.bound = (0.0, w, 0.0, h)
        self.first, self.prev = [None] * 4, [None] * 4
        self.f = self.s = None
        self.sum, self.n = 0.0, 0

    def _inside(self, k, p):
        c = p[k >> 1]
        return c >= self.bound[k] if k & 1 == 0 else c <= self.bound[k]

    def _cross(self, k, s, p):
        axis, b = k >> 1, self.bound[k]
        t = (b - s[axis]) / (p[axis] - s[axis])
        return (s[0] + t * (p[0] - s[0]), b) if axis else (b, s[1] + t * (p[1] - s[1]))

    def push(self, k, p):
        if k == 4:
            if self.n:
                self.sum += (self.s[0] * p[1]) - (p[0] * self.s[1])
            else:
                self.f = p
            self.s = p
            self.n += 1
            return
        inside = self._inside(k, p)
        if self.first[k] is not None:
            s = self.prev[k]
            if self._inside(k, s) != inside:
                self.push(k + 1, self._cross(k, s, p))
        else:
            self.first[k] = p
        self.prev[k] = p
        if inside:
            self.push(k + 1, p)

    def close(self, k=0):
        if k == 4:
            if self.n:
                self.sum += (self.s[0] * self.f[1]) - (self.f[0] * self.s[1])
            return
        if self.first[k] is not None:
            s, p = self.prev[k], self.first[k]
            if self._inside(k, s) != self._inside(k, p):
                self.push(k + 1, self._cross(k, s, p))
        self.close(k + 1)


def clip_area(px, py, x0, x1, y0, y1):
    """Area of polygon (px, py) inside the ice cell [x0, x1] x [y0, y1], as k_gg_clip_stream takes it."""
    x0, x1, y0, y1 = float(x0), float(x1), float(y0), float(y1)
    st = _Clip(x1 - x0, y1 - y0)
    for x, y in zip(px, py):
        st.push(0, (float(x) - x0, float(y) - y0))
    st.close()
    return st.sum * .5 if st.n >= 3 else 0.0


def cell_range(e, lo, hi):
    """gridgen.hip cell_range: cells whose open interior can meet (lo, hi)."""
    n = len(e) - 1
    k0 = max(int(np.searchsorted(e, lo, side="right")) - 1, 0)
    k1 = min(int(np.searchsorted(e, hi, side="left")), n)
    return k0, max(k1 - k0, 0)


def exchange_grid(xe, ye, polyptr, vx, vy, iA, x_fastest=False):
    """(indices int32[nX, 2], overlaps f64[nX]) as ibh_exgrid_generate gives them through the streamed clip."""
    xe, ye = np.asarray(xe, np.float64), np.asarray(ye, np.float64)
    nx, ny = len(xe) - 1, len(ye) - 1
    idx, area = [], []
    for p in range(len(iA)):
        px, py = vx[polyptr[p]:polyptr[p + 1]], vy[polyptr[p]:polyptr[p + 1]]
        ix0, nxr = cell_range(xe, px.min(), px.max())
        iy0, nyr = cell_range(ye, py.min(), py.max())
        pairs = ([(ix, iy) for iy in range(iy0, iy0 + nyr) for ix in range(ix0, ix0 + nxr)] if x_fastest else
                 [(ix, iy) for ix in range(ix0, ix0 + nxr) for iy in range(iy0, iy0 + nyr)])
        for ix, iy in pairs:
            a = clip_area(px, py, xe[ix], xe[ix + 1], ye[iy], ye[iy + 1])
            if a > 0:
                idx.append((int(iA[p]), iy * nx + ix if x_fastest else ix * ny + iy))
                area.append(a)
    return np.asarray(idx, np.int32).reshape(-1, 2), np.asarray(area, np.float64)
