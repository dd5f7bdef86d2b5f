"""GCMRegridder.to_modele (pylib/_icebin.pyx:128-147): the regridder ModelE couples through.  The ice model and the
regridder it wraps live on ModelE's OCEAN grid O; the matrices handed out here are on the atmosphere grid A =
make_hntrA(O), with the two models' ocean masks folded in (modele/GCMRegridder_ModelE.cpp:487-571)."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import check, lib, ptr
from .hntr import HntrSpec
from .linear import SparseSet, linear_Weighted

UI_LOCALICE, UI_GLOBALICE = 1, 2            # modele/grids.hpp:44-46


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


class EOpvAOpResult:
    """EOpvAOpResult (modele/merge_topo.hpp): the merged (and perhaps squashed) EOpvAOp over {dimEOp, dimAOp}, unscaled, with
    the elevation classes it stacks: hcdefs, underice_hc (UI_LOCALICE / UI_GLOBALICE per class), offsetE (the first row key of
    the base ice) and indexingHC as (stride_A, stride_HC) with the extents (nO, nhc)."""

    def __init__(self, dimEOp, dimAOp, EOpvAOp, offsetE, hcdefs, underice_hc, indexingHC, nO):
        self.dimEOp, self.dimAOp, self.EOpvAOp, self.offsetE = dimEOp, dimAOp, EOpvAOp, offsetE
        self.hcdefs, self.underice_hc, self.indexingHC, self.nO = hcdefs, underice_hc, indexingHC, nO

    @property
    def nhc(self):
        return len(self.hcdefs)


def compute_EOpvAOp_merged(rmOs, base=None, use_global_ice=True, use_local_ice=True, squash_ecs=False, dimAOp=None, nO=None,
                           indexingHC_base=None):
    """compute_EOpvAOp_merged and, with squash_ecs, squash_ECs (modele/merge_topo.cpp:375-527).  rmOs: the O-grid
    RegridMatrices of the ice sheets, in sheet order (their masks are the emI_ice; EvA is built unscaled whatever they were made
    with).  base = (hcdefs_base, (iE, iO, val), shape): the base (global) ice EOpvAOp, unscaled, in sparse indices, entries in
    the order of the arrays; None: there is no global ice.  dimAOp: a SparseSet to append to (None: a fresh one).  nO: the cells
    of the ocean grid (default: the base's shape[1], else the sheets').  indexingHC_base: (stride_A, stride_HC), default (1, nO)."""
    rmOs = list(rmOs)
    use_global_ice = bool(use_global_ice) and base is not None
    if base is not None:
        hc_b, (iE, iO, val), shape = base
        hc_b = np.ascontiguousarray(hc_b, np.float64)
        iE, iO = np.ascontiguousarray(iE, np.int64).reshape(-1), np.ascontiguousarray(iO, np.int64).reshape(-1)
        val = np.ascontiguousarray(val, np.float64).reshape(-1)
        if not len(iE) == len(iO) == len(val):
            raise ValueError("the base matrix's arrays have %d, %d and %d entries" % (len(iE), len(iO), len(val)))
        shape = (int(shape[0]), int(shape[1]))
    else:
        hc_b, iE, iO, val, shape = np.zeros(0), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), (0, 0)
    if nO is None:
        nO = shape[1] if base is not None else (rmOs[0]._keep[0].nA if rmOs else None)
    if nO is None:
        raise ValueError("nO is needed without sheets and without a base")
    sA, sHC = indexingHC_base if indexingHC_base is not None else (1, int(nO))
    dimAOp = dimAOp if dimAOp is not None else SparseSet()
    dimEOp = SparseSet()
    handles = (C.c_void_p * max(len(rmOs), 1))(*[rm._h for rm in rmOs])
    nhc_max = sum(rm._keep[0].nhc for rm in rmOs[:1]) + len(hc_b)
    hcdefs, underice = np.zeros(nhc_max), np.zeros(nhc_max, np.int16)
    h, offsetE, nhc = C.c_void_p(), C.c_int64(), C.c_int32()
    sA_out, sHC_out = C.c_int64(), C.c_int64()
    check(lib().ibh_modele_merge_EOpvAOp(handles, len(rmOs), int(nO), shape[0], shape[1], len(val), ptr(iE), ptr(iO), ptr(val), ptr(hc_b),
                                        len(hc_b), int(sA), int(sHC), int(use_global_ice), int(bool(use_local_ice)), int(bool(squash_ecs)),
                                        dimAOp._h, dimEOp._h, C.byref(h), C.byref(offsetE), C.byref(nhc), ptr(hcdefs), ptr(underice),
                                        C.byref(sA_out), C.byref(sHC_out)))
    w = linear_Weighted(h, keep=(dimEOp, dimAOp))
    return EOpvAOpResult(dimEOp, dimAOp, w, offsetE.value, hcdefs[:nhc.value].copy(), underice[:nhc.value].copy(),
                         (sA_out.value, sHC_out.value), int(nO))


def compute_AAmvEAm(EOpvAOp_result, hspecO, eq_rad, foceanAOp, foceanAOm, scale=True, nhc=None, dims=(None, None), indexingHCO=None,
                    indexingHCA=None):
    """_compute_AAmvEAm_EIGEN / _compute_AAmvEAm (modele/topo.cpp:242-374): AAmvEAm of a merged EOpvAOp on the atmosphere grid
    make_hntrA(hspecO); to_coo() and get_weights() of the result are the reference's to_tuple form.  nhc and the two indexings
    (stride_A, stride_HC) default to what the offline tools pass (make_topoa.cpp:131-135): every merged class, the result's own
    indexing on O and the same order on A.  dims: (dimAAm, dimEAm) to append to."""
    r = EOpvAOp_result
    hspecA = make_hntrA(hspecO)
    nhc = r.nhc if nhc is None else int(nhc)
    sO = r.indexingHC if indexingHCO is None else indexingHCO
    sA = ((1, hspecA.size) if sO[1] >= sO[0] else (nhc, 1)) if indexingHCA is None else indexingHCA
    fp = np.ascontiguousarray(np.asarray(foceanAOp, np.float64).reshape(-1))
    fm = np.ascontiguousarray(np.asarray(foceanAOm, np.float64).reshape(-1))
    if not len(fp) == len(fm) == hspecO.size:
        raise ValueError("focean arrays have %d and %d elements, the ocean grid %d cells" % (len(fp), len(fm), hspecO.size))
    d0 = dims[0]._h if dims[0] is not None else None
    d1 = dims[1]._h if dims[1] is not None else None
    h = C.c_void_p()
    check(lib().ibh_modele_AAmvEAm(r.EOpvAOp._h, r.dimEOp._h, r.dimAOp._h, hspecO.im, hspecO.jm, float(hspecO.offi), float(hspecO.dlat),
                                  float(eq_rad), nhc, int(sO[0]), int(sO[1]), int(sA[0]), int(sA[1]), ptr(fp), ptr(fm), len(fp), int(bool(scale)),
                                  d0, d1, C.byref(h)))
    return linear_Weighted(h, keep=(dims,))


class GCMRegridder_ModelE:
    """GCMRegridder_WrapE (modele/GCMRegridder_ModelE.hpp): a GCMRegridder_ModelE over `gcmO` together with the two ocean
    fractions, so that regrid_matrices keeps the signature of GCMRegridder.regrid_matrices.  global_ec = (hcdefs_base, (iE, iO,
    val), shape): the base (global) ice EOpvAOp of the global_ecO file (GCMRegridder_ModelE.hpp:111-114), for global_AvE."""

    def __init__(self, gcmO, hspecO, eq_rad, focean=None, global_ec=None):
        self.global_ec = global_ec
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

    @property
    def hcdefs(self):
        """hcdefs() (GCMRegridder_ModelE.cpp:468-471): the local classes, then the base ice's."""
        base = np.zeros(0) if self.global_ec is None else np.asarray(self.global_ec[0], np.float64)
        return np.concatenate([np.asarray(self.gcmO._hcdefs, np.float64), base])

    def underice(self, ihc):
        """underice(ihc) (GCMRegridder_ModelE.hpp:157)."""
        if not 0 <= ihc < len(self.hcdefs):
            raise IndexError(ihc)
        return UI_LOCALICE if ihc < self.gcmO.nhc else UI_GLOBALICE

    def global_AvE(self, emI_lands, emI_ices, foceanAOp, foceanAOm, scale=True):
        """global_AvE (GCMRegridder_ModelE.cpp:579-628) -> (linear_Weighted AAmvEAm, offsetE), composed the way the offline
        tools compose the library functions: the merge with the BASE hcdefs, then _compute_AAmvEAm over every merged class
        (DESIGN.md 16).  emI_ices: one elevmask per sheet, in the order the sheets were added; emI_lands is accepted and, as
        in the reference, not used."""
        names = list(self.gcmO._sheets)
        if len(emI_ices) != len(names):
            raise ValueError("%d ice masks for %d sheets" % (len(emI_ices), len(names)))
        rmOs = [self.gcmO.regrid_matrices(n, em, scale=False, correctA=False) for n, em in zip(names, emI_ices)]
        merged = compute_EOpvAOp_merged(rmOs, self.global_ec, use_global_ice=True, use_local_ice=True, squash_ecs=False,
                                        nO=self.gcmO.nA, indexingHC_base=self.gcmO._hc_strides)
        return compute_AAmvEAm(merged, self.hspecO, self.eq_rad, foceanAOp, foceanAOm, scale=scale), merged.offsetE

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


def to_modele(gcmO, focean=None, hspecO=None, eq_rad=None, global_ec=None):
    """GCMRegridder.to_modele(focean=None).  The ocean grid's HntrSpec and the earth's radius come from the regridder when
    it was built from a spec (HntrGCMRegridder.hspecA / .eq_rad) or from the keywords.  global_ec: the base ice that
    global_AvE merges in (GCMRegridder_ModelE)."""
    hspecO = hspecO if hspecO is not None else getattr(gcmO, "hspecA", None)
    eq_rad = eq_rad if eq_rad is not None else getattr(gcmO, "eq_rad", None)
    if hspecO is None or eq_rad is None:
        raise RuntimeError("make_gridA() requires specO have a Hntr source")       # GCMRegridder_ModelE.cpp:40-41
    return GCMRegridder_ModelE(gcmO, hspecO, eq_rad, focean, global_ec)
