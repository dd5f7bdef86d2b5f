"""GCMRegridder.to_modele (pylib/_icebin.pyx:128-147): the regridder ModelE couples through.  The ice model and the
regridder it wraps live on ModelE's OCEAN grid O; the matrices handed out here are on the atmosphere grid A =
make_hntrA(O), with the two models' ocean masks folded in (modele/GCMRegridder_ModelE.cpp:487-571)."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import check, lib, ptr
from .hntr import HntrSpec
from .linear import linear_Weighted


def make_hntrA(hspecO):
    """modele/hntr.cpp:232-241: the atmosphere grid is exactly twice as coarse as the ocean grid."""
    if hspecO.im % 2 or hspecO.jm % 2:
        raise ValueError("Ocean grid must have even number of gridcells for im and jm (vs. %d %d)" % (hspecO.im, hspecO.jm))
    return HntrSpec(hspecO.im // 2, hspecO.jm // 2, hspecO.offi * 0.5, hspecO.dlat * 2.)


class RegridMatrices_ModelE:
    """The RegridMatrices_Dynamic that GCMRegridder_ModelE::regrid_matrices returns: matrix() / matrix_d() over
    AvI EvI AvX EvX IvA IvE XvA XvE, the aliases EAmvIp AAmvIp IpvEAm IpvAAm and the test matrices AOmvAAm / AAmvAOm."""

    def __init__(self, handle, keep, scale):
        self._h = handle
        self._keep = keep
        self._scale = bool(scale)

    def __del__(self):
        try:
            _capi.destroy("ibh_modele_matrices_destroy", getattr(self, "_h", None))
        except Exception:      # interpreter shutdown
            pass
        self._h = None

    def matrix(self, spec_name):
        """Own dims, the scale the object was made with (_icebin.pyx:56-75)."""
        return self.matrix_d(spec_name, scale=self._scale)

    def matrix_d(self, spec_name, dims=(None, None), scale=True, correctA=False, sigma=(0., 0., 0.)):
        """matrix_d(spec, dims, RegridParams(scale, correctA, sigma)): correctA is ignored, as compute_XAmvGp and
        compute_GpvXAm ignore it; sigma must be zero."""
        if np.any(np.asarray(sigma, np.float64) != 0):
            raise NotImplementedError("smoothing through to_modele is not supported")
        h = C.c_void_p()
        d0 = dims[0]._h if dims[0] is not None else None
        d1 = dims[1]._h if dims[1] is not None else None
        check(lib().ibh_modele_matrices_matrix_d(self._h, spec_name.encode(), d0, d1, int(scale), C.byref(h)))
        return linear_Weighted(h, keep=(self, dims))


class GCMRegridder_ModelE:
    """GCMRegridder_WrapE (modele/GCMRegridder_ModelE.hpp): a GCMRegridder_ModelE over `gcmO` together with the two ocean
    fractions, so that regrid_matrices keeps the signature of GCMRegridder.regrid_matrices."""

    def __init__(self, gcmO, hspecO, eq_rad, focean=None):
        self.gcmO, self.hspecO, self.eq_rad = gcmO, hspecO, float(eq_rad)
        self.hspecA = make_hntrA(hspecO)
        if hspecO.size != gcmO.nA:
            raise ValueError("hspecO has %d cells, the regridder's grid nA=%d" % (hspecO.size, gcmO.nA))
        if focean is None:
            focean = (np.zeros(gcmO.nA), np.zeros(gcmO.nA))
        self.foceanOp = np.ascontiguousarray(np.asarray(focean[0], np.float64).reshape(-1))
        self.foceanOm = np.ascontiguousarray(np.asarray(focean[1], np.float64).reshape(-1))

    @property
    def nA(self):
        return self.hspecA.size

    @property
    def nhc(self):
        return self.gcmO.nhc

    @property
    def nE(self):
        return self.nA * self.nhc

    def agridA(self, sheet_name):
        """make_agridA (GCMRegridder_ModelE.cpp:57-78): the realised atmosphere cells, first-seen (int64)."""
        o = self.hspecO
        n = C.c_int32()
        out = np.empty(self.nA, np.int64)
        check(lib().ibh_modele_agridA(self.gcmO._sheets[sheet_name].h, o.im, o.jm, float(o.offi), float(o.dlat), C.byref(n), ptr(out)))
        return out[:n.value].copy()

    def wA(self, sheet_name, snative, fill=0.):
        raise NotImplementedError("wA on the ModelE regridder is not supported")

    def regrid_matrices(self, sheet_name, elevmaskI, scale=True, correctA=True, sigma=(0, 0, 0), conserve=True):
        """_icebin.pyx:164-175 on the ModelE regridder."""
        if np.any(np.asarray(sigma, np.float64) != 0):
            raise NotImplementedError("smoothing through to_modele is not supported")
        rmO = self.gcmO.regrid_matrices(sheet_name, elevmaskI, scale=scale, correctA=correctA, sigma=sigma, conserve=conserve)
        o = self.hspecO
        h = C.c_void_p()
        check(lib().ibh_modele_matrices_create(rmO._h, o.im, o.jm, float(o.offi), float(o.dlat), self.eq_rad, ptr(self.foceanOp),
                                              ptr(self.foceanOm), len(self.foceanOp), C.byref(h)))
        return RegridMatrices_ModelE(h, keep=(rmO, self), scale=scale)


def to_modele(gcmO, focean=None, hspecO=None, eq_rad=None):
    """GCMRegridder.to_modele(focean=None).  The ocean grid's HntrSpec and the earth's radius come from the regridder when
    it was built from a spec (HntrGCMRegridder.hspecA / .eq_rad) or from the keywords."""
    hspecO = hspecO if hspecO is not None else getattr(gcmO, "hspecA", None)
    eq_rad = eq_rad if eq_rad is not None else getattr(gcmO, "eq_rad", None)
    if hspecO is None or eq_rad is None:
        raise RuntimeError("make_gridA() requires specO have a Hntr source")       # GCMRegridder_ModelE.cpp:40-41
    return GCMRegridder_ModelE(gcmO, hspecO, eq_rad, focean)
