"""Exchange-grid generation (slib/icebin/gridgen/GridGen_Exchange.cpp:175-284) over the C-ABI: a rectilinear
ice grid in the projected plane under GCM-cell polygons (convex ones of up to 16 vertices through the array
clip, anything else -- more vertices, concave -- through the streamed one).  Inputs only -- the overlap arithmetic
runs in gridgen.hip."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import check, lib, ptr


def make_exchange_grid(xedges, yedges, polys, iA, x_fastest=False):
    """xedges [nx+1], yedges [ny+1]: ice-cell edges (ascending); polys: list of [nv, 2] vertex arrays
    (simple, counter-clockwise, projected XY; concave ones are served, by the streamed clip) of the realised GCM
    cells; iA: their sparse indices (ascending).
    Returns dict(indices=int32[nX, 2] (iA, iI), overlaps=f64[nX]) sorted by (iA, iI)."""
    xe, ye = np.ascontiguousarray(xedges, np.float64), np.ascontiguousarray(yedges, np.float64)
    iA = np.ascontiguousarray(iA, np.int64)
    assert len(polys) == len(iA)
    polyptr = np.zeros(len(polys) + 1, np.int32)
    polyptr[1:] = np.cumsum([len(p) for p in polys])
    v = np.concatenate([np.asarray(p, np.float64).reshape(-1, 2) for p in polys]) if len(polys) else np.zeros((0, 2))
    vx, vy = np.ascontiguousarray(v[:, 0]), np.ascontiguousarray(v[:, 1])
    d = _capi.ExgridDesc(nx=len(xe) - 1, ny=len(ye) - 1, xedges=ptr(xe).value, yedges=ptr(ye).value, x_fastest=int(bool(x_fastest)),
                         npoly=len(polys), polyptr=ptr(polyptr).value, vx=ptr(vx).value if len(vx) else None,
                         vy=ptr(vy).value if len(vy) else None, iA=ptr(iA).value if len(iA) else None)
    h = C.c_void_p()
    check(lib().ibh_exgrid_generate(C.byref(d), C.byref(h)))
    try:
        n = C.c_int64()
        check(lib().ibh_exgrid_size(h, C.byref(n)))
        idx, ov = np.empty((n.value, 2), np.int32), np.empty(n.value, np.float64)
        check(lib().ibh_exgrid_get(h, ptr(idx), ptr(ov)))
    finally:
        lib().ibh_exgrid_destroy(h)
    return dict(indices=idx, overlaps=ov)


# ---- from grid specs: lon/lat GCM cells generated, projected and measured on the device (lonlat.hip) ----------------------
WGS84_A, WGS84_RF = 6378137.0, 298.257223563


class GridSpec_LonLat:
    """GridSpec_LonLat (GridSpec.hpp:180-247): lonb [nlon+1], latb in degrees, indices ((0, 1): index = i*nlat + j; (1, 0):
    index = j*nlon + i), the caps, points_in_side and the radius of the native areas."""

    def __init__(self, lonb, latb, indices=(1, 0), south_pole=False, north_pole=False, points_in_side=1, eq_rad=6371000.):
        self.lonb, self.latb = np.ascontiguousarray(lonb, np.float64), np.ascontiguousarray(latb, np.float64)
        self.indices = tuple(int(k) for k in indices)
        self.south_pole, self.north_pole = bool(south_pole), bool(north_pole)
        self.points_in_side, self.eq_rad = int(points_in_side), float(eq_rad)

    @property
    def nlon(self):
        return len(self.lonb) - 1

    @property
    def nlat(self):
        return len(self.latb) - 1 + int(self.south_pole) + int(self.north_pole)

    @property
    def nA(self):
        """Sparse extent of the cell indices: the north cap's index is nlat*nlon + nlon - 1 (GridGen_LonLat.cpp:180-182), one
        row past ncells_full()."""
        return self.nlon * (self.nlat + int(self.north_pole))

    def cell_index(self, ilon, ilat):
        """Sparse index of ordinary cell (ilon, ilat) of lonb / latb (GridGen_LonLat.cpp:136-138)."""
        j = ilat + int(self.south_pole)
        return j * self.nlon + ilon if self.indices == (1, 0) else ilon * self.nlat + j

    @property
    def south_cap_index(self):
        return 0

    @property
    def north_cap_index(self):
        return self.nlat * self.nlon + self.nlon - 1


def parse_sproj(sproj):
    """The `sproj` string of an XY grid spec as the library's parser reads it (ibh_parse_sproj): proj=stere with lat_0, lon_0,
    lat_ts, k / k_0, x_0, y_0, ellps=WGS84 / datum=WGS84 / a, b / R, units=m, no_defs.  Returns a dict; any other key or value
    raises IcebinHipError(IBH_EINVAL) naming the key."""
    def bad(msg):
        raise _capi.IcebinHipError(_capi.IBH_EINVAL, "sproj: " + msg)
    p = dict(lat_0=0., lon_0=0., lat_ts=0., k_0=1., x_0=0., y_0=0., a=0., b=0., has_lat_ts=0)
    has_proj = has_a = has_b = has_R = wgs84 = False
    for tok in sproj.split():
        tok = tok[1:] if tok.startswith("+") else tok
        key, eq, val = tok.partition("=")

        def num():
            try:
                v = float(val)
            except ValueError:
                v = float("nan")
            if not val or not np.isfinite(v):
                bad("key '%s' has no numeric value ('%s')" % (key, val))
            return v
        if key == "proj":
            if val != "stere":
                bad("key 'proj' is '%s'; only stere is supported" % val)
            has_proj = True
        elif key in ("lat_0", "lon_0", "x_0", "y_0"):
            p[key] = num()
        elif key == "lat_ts":
            p["lat_ts"], p["has_lat_ts"] = num(), 1
        elif key in ("k", "k_0"):
            p["k_0"] = num()
        elif key in ("ellps", "datum"):
            if val != "WGS84":
                bad("key '%s' is '%s'; only WGS84 is supported" % (key, val))
            wgs84 = True
        elif key == "a":
            p["a"], has_a = num(), True
        elif key == "b":
            p["b"], has_b = num(), True
        elif key == "R":
            p["a"] = p["b"] = num()
            has_R = True
        elif key == "units":
            if val != "m":
                bad("key 'units' is '%s'; only m is supported" % val)
        elif key == "no_defs":
            if eq:
                bad("key 'no_defs' takes no value")
        else:
            bad("unknown key '%s'" % key)
    if not has_proj:
        bad("key 'proj' is missing")
    if has_R:
        if has_a or has_b or wgs84:
            bad("key 'R' excludes a, b, ellps and datum")
    elif has_a or has_b:
        if not has_a or wgs84:
            bad("key 'b' needs 'a' (and excludes ellps / datum)")
        if not has_b:
            p["b"] = p["a"]
    else:
        p["a"] = WGS84_A
        p["b"] = p["a"] * (1 - 1 / WGS84_RF)
    return p


def _stere_params(sproj):
    p = parse_sproj(sproj) if isinstance(sproj, str) else sproj
    return _capi.StereParams(**{k: p[k] for k in ("lat_0", "lon_0", "lat_ts", "k_0", "x_0", "y_0", "a", "b", "has_lat_ts")})


def project(sproj, lon, lat):
    """(lon, lat) in degrees -> (x, y) through the device's projection function (ibh_lonlat_project)."""
    lon, lat = np.ascontiguousarray(lon, np.float64), np.ascontiguousarray(lat, np.float64)
    assert lon.shape == lat.shape
    x, y = np.empty_like(lon), np.empty_like(lat)
    sp = _stere_params(sproj)
    check(lib().ibh_lonlat_project(C.byref(sp), lon.size, ptr(lon), ptr(lat), ptr(x), ptr(y)))
    return x, y


class LonLatCells(_capi.Handle):
    """The realised cells of a GridSpec_LonLat in HBM (ibh_lonlat_cells): projected polygons, native and projected areas."""
    _destroy = "ibh_lonlat_cells_destroy"

    def __init__(self, handle, spec):
        self._h, self.spec = handle, spec
        nc, nv, nA = C.c_int32(), C.c_int64(), C.c_int64()
        check(lib().ibh_lonlat_cells_size(handle, C.byref(nc), C.byref(nv), C.byref(nA)))
        self.ncell, self.nvert, self.nA = nc.value, nv.value, nA.value

    def get(self, lonlat=False):
        """Copy-out: dict(iA, polyptr, vx, vy, native_area, proj_area[, lon, lat])."""
        nc, nv = self.ncell, self.nvert
        out = dict(iA=np.empty(nc, np.int64), polyptr=np.empty(nc + 1, np.int32), vx=np.empty(nv), vy=np.empty(nv),
                   native_area=np.empty(nc), proj_area=np.empty(nc))
        if lonlat:
            out.update(lon=np.empty(nv), lat=np.empty(nv))
        check(lib().ibh_lonlat_cells_get(self._h, ptr(out["iA"]), ptr(out["polyptr"]), ptr(out["vx"]), ptr(out["vy"]),
                                         ptr(out["native_area"]), ptr(out["proj_area"]), ptr(out.get("lon")), ptr(out.get("lat"))))
        return out


def lonlat_cells(spec, realised, sproj, keep_lonlat=False):
    """make_grid (gridgen/GridGen_LonLat.cpp:109-232) for the cells whose sparse indices `realised` lists (strictly ascending),
    projected with `sproj` (a string or parse_sproj's dict).  Returns a LonLatCells; nothing but the spec crosses the host."""
    realised = np.ascontiguousarray(realised, np.int64)
    sp = _stere_params(sproj)
    d = _capi.LonLatCellsDesc(nlonb=len(spec.lonb), nlatb=len(spec.latb), lonb=ptr(spec.lonb).value, latb=ptr(spec.latb).value,
                              indices=(C.c_int32 * 2)(*spec.indices), south_pole=int(spec.south_pole), north_pole=int(spec.north_pole),
                              points_in_side=spec.points_in_side, eq_rad=spec.eq_rad, nrealised=len(realised),
                              realised=ptr(realised).value if len(realised) else None, proj=C.pointer(sp), keep_lonlat=int(keep_lonlat))
    h = C.c_void_p()
    check(lib().ibh_lonlat_cells_create(C.byref(d), C.byref(h)))
    return LonLatCells(h, spec)


def make_exchange_grid_lonlat(cells, xedges, yedges, x_fastest=False):
    """make_exchange_grid under the cells of lonlat_cells(): dict(indices=int32[nX, 2] (iA, iI), overlaps=f64[nX])."""
    xe, ye = np.ascontiguousarray(xedges, np.float64), np.ascontiguousarray(yedges, np.float64)
    h = C.c_void_p()
    check(lib().ibh_exgrid_generate_lonlat(cells._h, len(xe) - 1, len(ye) - 1, ptr(xe), ptr(ye), int(bool(x_fastest)), C.byref(h)))
    try:
        n = C.c_int64()
        check(lib().ibh_exgrid_size(h, C.byref(n)))
        idx, ov = np.empty((n.value, 2), np.int32), np.empty(n.value, np.float64)
        check(lib().ibh_exgrid_get(h, ptr(idx), ptr(ov)))
    finally:
        lib().ibh_exgrid_destroy(h)
    return dict(indices=idx, overlaps=ov)


def ice_centroids(xedges, yedges, x_fastest=False):
    """Centres of a rectilinear ice grid's cells, f64[nI, 2] by ice index (what ibh_regridder_create_lonlat uses)."""
    xe, ye = np.asarray(xedges, np.float64), np.asarray(yedges, np.float64)
    cx, cy = .5 * (xe[:-1] + xe[1:]), .5 * (ye[:-1] + ye[1:])
    if x_fastest:
        return np.stack([np.tile(cx, len(cy)), np.repeat(cy, len(cx))], 1)
    return np.stack([np.repeat(cx, len(cy)), np.tile(cy, len(cx))], 1)


def regridder_from_specs(spec_lonlat, realised, xedges, yedges, sproj, hcdefs, x_fastest=False, correctA=True,
                         interp_style="Z_INTERP", sheet_name="ice", hc_strides=None, dimA=None):
    """From a GridSpec_LonLat, the realised cells, an XY ice spec (edges, index order) and its `sproj` to a GCMRegridder with
    one sheet: cells, exchange grid and regridder are built on the device (ibh_regridder_create_lonlat).  dimA: an empty
    SparseSet that receives the realised cells, or None."""
    from .global_ec import _HntrSheet
    from .regrid import _INTERP, GCMRegridder
    if interp_style not in _INTERP:
        raise ValueError("unknown interp_style %r" % (interp_style,))
    cells = lonlat_cells(spec_lonlat, realised, sproj)
    xe, ye = np.ascontiguousarray(xedges, np.float64), np.ascontiguousarray(yedges, np.float64)
    hc = np.ascontiguousarray(hcdefs, np.float64)
    strides = (1, cells.nA) if hc_strides is None else (int(hc_strides[0]), int(hc_strides[1]))
    d = _capi.LonLatRegridderDesc(cells=cells._h.value, nx=len(xe) - 1, ny=len(ye) - 1, xedges=ptr(xe).value, yedges=ptr(ye).value,
                                  x_fastest=int(bool(x_fastest)), nhc=len(hc), hcdefs=ptr(hc).value if len(hc) else None,
                                  hc_stride_A=strides[0], hc_stride_HC=strides[1], interp_style=_INTERP[interp_style])
    h = C.c_void_p()
    check(lib().ibh_regridder_create_lonlat(C.byref(d), dimA._h if dimA is not None else None, C.byref(h)))
    sheet = _HntrSheet(h, (len(xe) - 1) * (len(ye) - 1), interp_style)
    sheet.centroid = ice_centroids(xe, ye, x_fastest).reshape(-1)
    a2s, nat = sheet.agridA()
    mm = GCMRegridder(dict(nA=cells.nA, to_sparse=a2s, native_area=nat), hc, correctA)
    mm._hc_strides = strides
    mm._sheets[sheet_name] = sheet
    return mm


def spherical_clip_lonlat(spec, min_lon, min_lat, max_lon, max_lat):
    """SphericalClip::lonlat (gridgen/clippers.cpp:44-70) over every cell of the spec as make_grid offers them
    (GridGen_LonLat.cpp:141,183,204): the ascending sparse indices of the cells to realise."""
    def in_lon(lo, hi, x):
        while x > hi:
            x -= 360.
        while x < lo:
            x += 360.
        return x <= hi

    def keep(lon0, lat0, lon1, lat1):
        if not (in_lon(lon0, lon1, min_lon) or in_lon(lon0, lon1, max_lon) or in_lon(min_lon, max_lon, lon0) or in_lon(min_lon, max_lon, lon1)):
            return False
        if lat0 < min_lat and lat1 < min_lat:
            return False
        if lat0 > max_lat and lat1 > max_lat:
            return False
        return True
    out = []
    for ilat in range(len(spec.latb) - 1):
        for ilon in range(spec.nlon):
            if keep(spec.lonb[ilon], spec.latb[ilat], spec.lonb[ilon + 1], spec.latb[ilat + 1]):
                out.append(spec.cell_index(ilon, ilat))
    if spec.north_pole and keep(0., spec.latb[-1], 360., 90.):
        out.append(spec.north_cap_index)
    if spec.south_pole and keep(0., -90., 360., spec.latb[0]):
        out.append(spec.south_cap_index)
    return np.asarray(sorted(out), np.int64)
