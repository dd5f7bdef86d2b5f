"""L1 ice grids over the C-ABI: a triangle mesh with piecewise-linear fields (pylib/icebin/element_l1.py) under convex
GCM cells.  Inputs only -- clipping, the basis integrals and the assembly run in l1.hip."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import check, lib, ptr


class Mesh(_capi.Handle):
    """Vertices vx, vy [nvert] and elements tri [ntri, 3] (vertex ids, counter-clockwise), resident in HBM."""
    _destroy = "ibh_l1_mesh_destroy"

    def __init__(self, vx, vy, tri):
        self.vx, self.vy = np.ascontiguousarray(vx, np.float64), np.ascontiguousarray(vy, np.float64)
        self.tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
        if len(self.vx) != len(self.vy):
            raise ValueError("vx has %d entries, vy %d" % (len(self.vx), len(self.vy)))
        h = C.c_void_p()
        check(lib().ibh_l1_mesh_create(len(self.vx), ptr(self.vx), ptr(self.vy), len(self.tri), ptr(self.tri), C.byref(h)))
        self._h = h

    nvert = property(lambda self: len(self.vx))
    ntri = property(lambda self: len(self.tri))


class ExchangeGrid(_capi.Handle):
    """The exchange grid of a mesh in HBM, sorted by (iA, iTri).  indices int32[nX, 2] (iA, iTri), areas f64[nX], and the
    ragged polygons vptr int32[nX+1], qx, qy are copied out on first use."""
    _destroy = "ibh_l1_exgrid_destroy"

    def __init__(self, handle):
        self._h = handle
        self._arrays = None

    def _get(self):
        if self._arrays is None:
            nX, nq = C.c_int64(), C.c_int64()
            check(lib().ibh_l1_exgrid_size(self._h, C.byref(nX), C.byref(nq)))
            idx, areas = np.empty((nX.value, 2), np.int32), np.empty(nX.value, np.float64)
            vptr, qx, qy = np.empty(nX.value + 1, np.int32), np.empty(nq.value, np.float64), np.empty(nq.value, np.float64)
            check(lib().ibh_l1_exgrid_get(self._h, ptr(idx), ptr(areas), ptr(vptr), ptr(qx), ptr(qy)))
            self._arrays = dict(indices=idx, areas=areas, vptr=vptr, qx=qx, qy=qy)
        return self._arrays

    indices = property(lambda self: self._get()["indices"])
    areas = property(lambda self: self._get()["areas"])
    vptr = property(lambda self: self._get()["vptr"])
    qx = property(lambda self: self._get()["qx"])
    qy = property(lambda self: self._get()["qy"])

    def __len__(self):
        return len(self.areas)

    @property
    def polygons(self):
        """The overlap polygons as a list of [nv, 2] arrays."""
        v, q = self.vptr, np.stack([self.qx, self.qy], 1)
        return [q[v[k]:v[k + 1]] for k in range(len(v) - 1)]


def _ragged(polys):
    vptr = np.zeros(len(polys) + 1, np.int32)
    vptr[1:] = np.cumsum([len(p) for p in polys])
    v = np.concatenate([np.asarray(p, np.float64).reshape(-1, 2) for p in polys]) if len(polys) else np.zeros((0, 2))
    return vptr, np.ascontiguousarray(v[:, 0]), np.ascontiguousarray(v[:, 1])


def make_exchange_grid(mesh, polys, iA):
    """make_exchange_grid (slib/icebin/gridgen/GridGen_Exchange.cpp:175-284) for a triangle mesh.  polys: list of [nv, 2]
    vertex arrays (convex, counter-clockwise, projected XY, at most 16 vertices) of the realised GCM cells; iA: their
    sparse indices (ascending).  A polygon that is clockwise, has a reflex vertex (beyond rounding: sides with computed
    collinear points pass) or winds more than once raises IcebinHipError(IBH_EINVAL) naming polygon and vertex.
    Returns an ExchangeGrid: indices, areas and polygons."""
    iA = np.ascontiguousarray(iA, np.int64)
    if len(polys) != len(iA):
        raise ValueError("%d polygons, %d indices" % (len(polys), len(iA)))
    polyptr, px, py = _ragged(polys)
    h = C.c_void_p()
    check(lib().ibh_l1_exgrid_generate(mesh._h, len(polys), ptr(polyptr), ptr(px), ptr(py), ptr(iA), C.byref(h)))
    return ExchangeGrid(h)


def exchange_grid_from_polygons(iA, iTri, polys=None, vptr=None, qx=None, qy=None):
    """An exchange grid as the reference's own exgrid.cells carry it (element_l1.py:118-124): per cell the GCM cell iA,
    the element iTri and the overlap polygon -- a list of [nv, 2] arrays, or the ragged form (vptr, qx, qy).  Any order:
    sorted by (iA, iTri) on the device, ties in input order."""
    iA, iTri = np.ascontiguousarray(iA, np.int32), np.ascontiguousarray(iTri, np.int32)
    if polys is not None:
        vptr, qx, qy = _ragged(polys)
    vptr = np.ascontiguousarray(vptr, np.int32)
    qx, qy = np.ascontiguousarray(qx, np.float64), np.ascontiguousarray(qy, np.float64)
    if not (len(iA) == len(iTri) == len(vptr) - 1 and len(qx) == len(qy) == vptr[-1]):
        raise ValueError("exchange-grid arrays disagree in length")
    h = C.c_void_p()
    check(lib().ibh_l1_exgrid_from_polygons(len(iA), ptr(iA), ptr(iTri), ptr(vptr), ptr(qx), ptr(qy), C.byref(h)))
    return ExchangeGrid(h)


def terms(exgrid, nA, mesh, which="AvI"):
    """The 3*nX triplets (row, col, val) of compute_AvI before any summing, in stream order: exchange cell, then basis
    function."""
    n = 3 * len(exgrid)
    row, col, val = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float64)
    check(lib().ibh_l1_terms(exgrid._h, mesh._h, int(nA), which.encode(), ptr(row), ptr(col), ptr(val)))
    return row, col, val


def compute_AvI(exgrid, nA, mesh, scale=False, which="AvI"):
    """compute_AvI (element_l1.py:96-148) as a linear_Weighted in HBM: rows over nA, columns over the mesh's vertices
    ("IvA": the transpose); wM, Mw the reference's weightsA, weightsI; scale: M = diag(1/wM) M."""
    from .linear import linear_Weighted
    h = C.c_void_p()
    check(lib().ibh_l1_matrix(exgrid._h, mesh._h, int(nA), which.encode(), int(bool(scale)), C.byref(h)))
    return linear_Weighted(h)
