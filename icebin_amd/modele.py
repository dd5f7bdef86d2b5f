"""GCMRegridder.to_modele (pylib/_icebin.pyx:128-147): the regridder ModelE couples through.  The ice model and the
regridder it wraps live on ModelE's OCEAN grid O; the matrices handed out here are on the atmosphere grid A =
make_hntrA(O), with the two models' ocean masks folded in (modele/GCMRegridder_ModelE.cpp:487-571)."""
import ctypes as C

import numpy as np

from . import _capi
from ._arrays import dptr, is_cuda, stream_arg, to_device
from ._capi import check, lib, ptr
from .hntr import HntrSpec
from .linear import SparseSet, linear_Weighted

UI_UNUSED, UI_LOCALICE, UI_GLOBALICE, UI_VGHOST, UI_HGHOST, UI_SEALAND = 0, 1, 2, 3, 4, 5      # modele/grids.hpp:44-49

# topoo_bundle's names (modele/topo.cpp:384-474) in the order of merge_topoO's planes (merge_topo.cpp:89-101), the labels its
# sanity checks print (:159-167), make_topoA's ocean planes (topo.cpp:584-592) and TopoABundles' names (:482-483)
TOPOO_MERGE = ("FOCEANF", "FGICEF", "ZATMOF", "FOCEAN", "FLAKE", "FGRND", "FGICE", "ZATMO", "ZICETOP", "ZLAND_MIN", "ZLAND_MAX")
MERGE_LABELS = ("foceanOp2", "fgiceOp2", "zatmoOp2", "foceanOm2", "flakeOm2", "fgrndOm2", "fgiceOm2", "zatmoOm2", "zicetopO2")
TOPOO_MAKEA = ("FOCEAN", "FLAKE", "FGRND", "FGICE", "ZATMO", "ZLAKE", "ZICETOP", "ZLAND_MIN", "ZLAND_MAX")
TOPOA_NAMES = ("focean", "flake", "fgrnd", "fgice", "zatmo", "hlake", "zicetop", "zland_min", "zland_max")


def make_hntrA(hspecO):
    """modele/hntr.cpp:232-241: the atmosphere grid is exactly twice as coarse as the ocean grid."""
    if hspecO.im % 2 or hspecO.jm % 2:
        raise ValueError("Ocean grid must have even number of gridcells for im and jm (vs. %d %d)" % (hspecO.im, hspecO.jm))
    return HntrSpec(hspecO.im // 2, hspecO.jm // 2, hspecO.offi * 0.5, hspecO.dlat * 2.)


class RegridMatrices_ModelE(_capi.Handle):
    """The RegridMatrices_Dynamic that GCMRegridder_ModelE::regrid_matrices returns: matrix() / matrix_d() over
    AvI EvI AvX EvX IvA IvE XvA XvE, the aliases EAmvIp AAmvIp IpvEAm IpvAAm and the test matrices AOmvAAm / AAmvAOm."""
    _destroy = "ibh_modele_matrices_destroy"

    def __init__(self, handle, keep, scale, sigma=(0., 0., 0.)):
        self._h = handle
        self._keep = keep
        self._scale = bool(scale)
        self._sigma = tuple(float(s) for s in sigma)

    def matrix(self, spec_name):
        """Own dims, the scale and the sigma the object was made with (_icebin.pyx:56-75; RegridMatrices_Dynamic.cpp:425-437)."""
        return self.matrix_d(spec_name, scale=self._scale, sigma=self._sigma)

    def matrix_d(self, spec_name, dims=(None, None), scale=True, correctA=False, sigma=(0., 0., 0.)):
        """matrix_d(spec, dims, RegridParams(scale, correctA, sigma)): correctA is ignored, as compute_XAmvGp and
        compute_GpvXAm ignore it.  sigma smooths IvA / IvE (IpvAAm / IpvEAm) -- it goes to the O-grid build of IpvXOp alone, as
        in compute_GpvXAm --, is ignored by AvI EvI AvX EvX and the test matrices, and is refused for XvA / XvE
        (ibh_modele_matrices_matrix_d_sigma)."""
        sg = np.ascontiguousarray(sigma, np.float64).reshape(-1)
        if len(sg) != 3:
            raise ValueError("sigma has %d values, not 3" % len(sg))
        h = C.c_void_p()
        d0 = dims[0]._h if dims[0] is not None else None
        d1 = dims[1]._h if dims[1] is not None else None
        check(lib().ibh_modele_matrices_matrix_d_sigma(self._h, spec_name.encode(), d0, d1, int(scale), ptr(sg), C.byref(h)))
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


def _planes(arrays, n, what):
    """The planes of one call as flat float64 arrays of n cells, all on the host (numpy or CPU torch, used in place when they
    can be) or all in HBM (torch CUDA tensors, always in place) -> (planes, on_device)."""
    dev = [is_cuda(a) for a in arrays if a is not None]
    if any(dev) and not all(dev):
        raise ValueError("%s: host and device planes are mixed" % what)
    on_device = bool(dev) and dev[0]
    out = []
    for a in arrays:
        if a is None:
            out.append(None)
        elif on_device:
            if not (str(a.dtype) == "torch.float64" and a.is_contiguous() and a.numel() == n):
                raise ValueError("%s: a device plane must be a contiguous float64 CUDA tensor of %d cells" % (what, n))
            out.append(a)
        else:
            b = np.ascontiguousarray(a, np.float64)
            if b.size != n:
                raise ValueError("%s: a plane has %d cells, the grid %d" % (what, b.size, n))
            out.append(b)
    return out, on_device


def _pointer_list(planes):
    return (C.c_void_p * len(planes))(*[p.data_ptr() if is_cuda(p) else p.ctypes.data for p in planes])


def _host(a):
    return a.cpu().numpy() if is_cuda(a) else np.asarray(a)


def land_fraction_errors(bad, focean, flake, fgrnd, fgice, im):
    """sanity_check_land_fractions' strings (modele/topo.cpp:873-888) for the flat cells `bad` (ascending: j, then i)."""
    out = []
    for c in bad:
        fo, fl, fr, fi = float(focean[c]), float(flake[c]), float(fgrnd[c]), float(fgice[c])
        out.append("(%d, %d): FOCEAN(%g) + FGRND(%g) + FLAKE(%g) + FGICE(%g)  = %g" % (c % im + 1, c // im + 1, fo, fr, fl, fi, fo + fr + fl + fi))
    return out


def merge_topoO(topoo, gcmO, emI_lands, emI_ices, hspecO, eq_rad=0.):
    """merge_topoO (modele/merge_topo.cpp:84-360) -> (mergemaskOm, errors).  topoo: a dict of planes under topoo_bundle's
    names; FOCEANF FGICEF ZATMOF FOCEAN FLAKE FGRND FGICE ZATMO ZICETOP are merged into (in place where the plane is a
    contiguous float64 array; the dict holds the results either way, shaped (jmO, imO)), ZLAND_MIN / ZLAND_MAX are made.  Numpy
    planes go through the host entry; torch CUDA planes (and masks) stay in HBM, on torch's current stream.  gcmO: the
    GCMRegridder on the ocean grid, whose sheets (in the order they were added) emI_lands / emI_ices belong to.  errors: the
    reference's sanity-check strings, check by check, then j, then i; the call itself succeeds when there are some."""
    names = list(gcmO._sheets)
    if len(emI_lands) != len(names) or len(emI_ices) != len(names):
        raise ValueError("%d land masks and %d ice masks for %d sheets" % (len(emI_lands), len(emI_ices), len(names)))
    lands = [gcmO.regrid_matrices(n, em, scale=False, correctA=True) for n, em in zip(names, emI_lands)]
    ices = [gcmO.regrid_matrices(n, em, scale=False, correctA=True) for n, em in zip(names, emI_ices)]
    return merge_topoO_rm(topoo, lands, ices, hspecO, eq_rad)


def merge_topoO_rm(topoo, lands, ices, hspecO, eq_rad=0.):
    """merge_topoO on the RegridMatrices of the masks (ibh_modele_merge_topoO[_device])."""
    nO, im = hspecO.size, hspecO.im
    planes, on_device = _planes([topoo[k] for k in TOPOO_MERGE[:9]], nO, "merge_topoO")
    hl = (C.c_void_p * max(len(lands), 1))(*[rm._h for rm in lands])
    hi = (C.c_void_p * max(len(ices), 1))(*[rm._h for rm in ices])
    nerr = C.c_int64()
    if on_device:
        import torch
        dev = planes[0].device
        planes += [torch.empty(nO, dtype=torch.float64, device=dev) for _ in range(2)]
        mask = torch.empty(nO, dtype=torch.int16, device=dev)
        flags = torch.empty(nO, dtype=torch.int32, device=dev)
        check(lib().ibh_modele_merge_topoO_device(hl, len(lands), hi, len(ices), hspecO.im, hspecO.jm, float(eq_rad), _pointer_list(planes),
                                                 dptr(mask), dptr(flags), C.byref(nerr), stream_arg(mask)))
    else:
        planes += [np.empty(nO), np.empty(nO)]
        mask, flags = np.zeros(nO, np.int16), np.zeros(nO, np.uint32)
        check(lib().ibh_modele_merge_topoO(hl, len(lands), hi, len(ices), hspecO.im, hspecO.jm, float(eq_rad), _pointer_list(planes), ptr(mask),
                                          ptr(flags), C.byref(nerr)))
    for k, p in zip(TOPOO_MERGE, planes):
        topoo[k] = p.reshape(hspecO.jm, hspecO.im)
    errors = []
    if nerr.value:
        f = _host(flags).astype(np.int64) & 0xFFFFFFFF
        for bit in range(18):
            label = MERGE_LABELS[bit % 9] + ("-0" if bit < 9 else "")
            errors += ["(%d, %d): %s is NaN" % (c % im + 1, c // im + 1, label) for c in np.flatnonzero(f >> bit & 1)]
        bad = np.flatnonzero(f >> 18 & 1)
        if len(bad):
            errors += land_fraction_errors(bad, _host(planes[3]), _host(planes[4]), _host(planes[5]), _host(planes[6]), im)
        assert len(errors) == nerr.value
    return mask.reshape(hspecO.jm, hspecO.im), errors


def make_topoA(topoo, mergemaskOm, hspecO, hspecA, indexingHCA, hcdefs, underice_hc, AAmvEAm):
    """make_topoA (modele/topo.cpp:581-855) -> (topoa, errors).  topoo: the planes FOCEAN FLAKE FGRND FGICE ZATMO ZLAKE ZICETOP
    ZLAND_MIN ZLAND_MAX (numpy, or torch CUDA tensors with a torch int16 mergemaskOm: then everything stays in HBM);
    indexingHCA: (stride_A, stride_HC); AAmvEAm: a linear_Weighted.  topoa: a dict of the planes under TopoABundles' names
    (jmA, imA), mergemask (int16) and fhc, elevE (float64), underice (int16) of shape (nhc + 1, jmA, imA).  errors: the
    strings of sanity_check_land_fractions, then sanity_check_fhc."""
    nO, nA, im = hspecO.size, hspecA.size, hspecA.im
    hc = np.ascontiguousarray(hcdefs, np.float64).reshape(-1)
    ui = np.ascontiguousarray(underice_hc, np.int16).reshape(-1)
    if len(hc) != len(ui):
        raise ValueError("%d hcdefs for %d underice_hc" % (len(hc), len(ui)))
    nhc = len(hc)
    planesO, on_device = _planes([topoo[k] for k in TOPOO_MAKEA], nO, "make_topoA")
    nerr = C.c_int64()
    args = (hspecO.im, hspecO.jm, float(hspecO.offi), float(hspecO.dlat), hspecA.im, hspecA.jm, float(hspecA.offi), float(hspecA.dlat),
            int(indexingHCA[0]), int(indexingHCA[1]), ptr(hc), ptr(ui), nhc, AAmvEAm._h)
    if on_device:
        import torch
        dev = planesO[0].device
        if not (is_cuda(mergemaskOm) and mergemaskOm.dtype == torch.int16 and mergemaskOm.is_contiguous() and mergemaskOm.numel() == nO):
            raise ValueError("make_topoA: mergemaskOm must be a contiguous int16 CUDA tensor of %d cells" % nO)
        planesA = [torch.empty(nA, dtype=torch.float64, device=dev) for _ in range(9)]
        maskA = torch.empty(nA, dtype=torch.int16, device=dev)
        fhc, elevE = (torch.empty((nhc + 1) * nA, dtype=torch.float64, device=dev) for _ in range(2))
        underice = torch.empty((nhc + 1) * nA, dtype=torch.int16, device=dev)
        flags = torch.empty(nA, dtype=torch.int32, device=dev)
        check(lib().ibh_modele_make_topoA_device(_pointer_list(planesO), dptr(mergemaskOm), *args, _pointer_list(planesA),
                                                *[dptr(t) for t in (maskA, fhc, elevE, underice, flags)], C.byref(nerr), stream_arg(maskA)))
    else:
        mO = np.ascontiguousarray(mergemaskOm, np.int16).reshape(-1)
        if mO.size != nO:
            raise ValueError("make_topoA: mergemaskOm has %d cells, the ocean grid %d" % (mO.size, nO))
        planesA = [np.empty(nA) for _ in range(9)]
        maskA, flags = np.zeros(nA, np.int16), np.zeros(nA, np.uint32)
        fhc, elevE, underice = np.empty((nhc + 1) * nA), np.empty((nhc + 1) * nA), np.zeros((nhc + 1) * nA, np.int16)
        check(lib().ibh_modele_make_topoA(_pointer_list(planesO), ptr(mO), *args, _pointer_list(planesA), ptr(maskA), ptr(fhc), ptr(elevE),
                                         ptr(underice), ptr(flags), C.byref(nerr)))
    shape2, shape3 = (hspecA.jm, hspecA.im), (nhc + 1, hspecA.jm, hspecA.im)
    topoa = {k: p.reshape(shape2) for k, p in zip(TOPOA_NAMES, planesA)}
    topoa.update(mergemask=maskA.reshape(shape2), fhc=fhc.reshape(shape3), elevE=elevE.reshape(shape3), underice=underice.reshape(shape3))
    errors = []
    if nerr.value:
        f = _host(flags).astype(np.int64)
        bad = np.flatnonzero(f & 1)
        if len(bad):
            errors += land_fraction_errors(bad, *[_host(planesA[k]) for k in (0, 1, 2, 3)], im)
        bad = np.flatnonzero(f >> 1 & 1)
        if len(bad):
            fh = _host(fhc).reshape(nhc + 1, nA)
            for c in bad:
                all_fhc = 0.
                for ihc in range(nhc + 1):
                    all_fhc += float(fh[ihc, c])
                all_fhc += 1.0
                errors.append("(%d, %d): sum(FHC) = %g" % (c % im + 1, c // im + 1, all_fhc - 1.0))
        assert len(errors) == nerr.value
    return topoa, errors


TOPOE_NAMES = ("fhc", "elevE", "underice_d")       # topoa.a3's arrays once underice_d is added (GCMCoupler_ModelE.cpp:1090-1097)


class TopoPacker:
    """The end of GCMCoupler_ModelE::update_topo (modele/GCMCoupler_ModelE.cpp:1090-1167) and couple()'s unit conversion
    (:1216-1228): the TOPOA planes packed into the two VectorMultivecs ModelE scatters, gcm_ivalss_s[ATOPO] and [ETOPO].

    varsA: the contract's ATOPO variables, names of TopoABundles' 2-D planes; varsE: the ETOPO variables, names out of fhc,
    elevE, underice_d; an unknown name raises KeyError (the reference's .at(name), :1114, :1147).  index_strides_E: indexingE
    as (stride of the cell j * im + i, stride of the class).  mm / bb: the contract's scale and offset per variable; without
    either no conversion runs.  The object owns mergemaskA0, the previous step's mask (:1017, :1167): on the device when the
    planes are, else numpy."""

    def __init__(self, varsA, varsE, index_strides_E, mmA=None, bbA=None, mmE=None, bbE=None):
        self.varsA, self.varsE = tuple(varsA), tuple(varsE)
        for name in self.varsA:
            if name not in TOPOA_NAMES:
                raise KeyError(name)
        for name in self.varsE:
            if name not in TOPOE_NAMES:
                raise KeyError(name)
        self.index_strides_E = (int(index_strides_E[0]), int(index_strides_E[1]))
        self.affineA = self._affine(mmA, bbA, len(self.varsA))
        self.affineE = self._affine(mmE, bbE, len(self.varsE))
        self.mergemaskA0 = None

    @staticmethod
    def _affine(mm, bb, nvar):
        if mm is None and bb is None:
            return None
        mm = np.ones(nvar) if mm is None else np.asarray(mm, np.float64).reshape(-1)
        bb = np.zeros(nvar) if bb is None else np.asarray(bb, np.float64).reshape(-1)
        if len(mm) != nvar or len(bb) != nvar:
            raise ValueError("%d mm and %d bb for %d variables" % (len(mm), len(bb), nvar))
        return mm, bb

    def pack(self, topoa, nhc, run_ice, outA=None, outE=None):
        """topoa: make_topoA's / update_topo's dict; nhc: the classes to pack (fhc, elevE and underice carry nhc + 1: the
        sea-land class is not packed, as in the reference).  run_ice = False (initialisation): the previous mask is this
        step's (:1017).  Afterwards this step's mask is kept -- the array itself, as the reference keeps a reference (:1167).
        outA / outE: vectors to append to (default: fresh ones).  The conversion runs over ALL entries of each vector, as
        :1216-1228 does: append what else belongs in them first.  -> (gcm_ivalsA, gcm_ivalsE)."""
        from .multivec import VectorMultivec, append_planes_many
        mask = topoa["mergemask"]
        on_device = is_cuda(mask)
        ncell = mask.numel() if on_device else np.asarray(mask).size
        if not run_ice:
            mask0 = mask
        else:
            mask0 = self.mergemaskA0
            if mask0 is None:
                raise RuntimeError("TopoPacker.pack: run_ice without a mask of an earlier step (initialise with run_ice=False)")
            if is_cuda(mask0) != on_device:      # the planes moved between the host and the device since the last step
                mask0 = to_device(np.ascontiguousarray(mask0), mask.device) if on_device else mask0.cpu().numpy()
        source = {"fhc": "fhc", "elevE": "elevE", "underice_d": "underice"}
        outA = VectorMultivec(len(self.varsA)) if outA is None else outA
        outE = VectorMultivec(len(self.varsE)) if outE is None else outE
        append_planes_many([dict(vec=outA, planes=[topoa[k] for k in self.varsA], nclass=1, index_strides=(1, ncell)),
                            dict(vec=outE, planes=[topoa[source[k]] for k in self.varsE], nclass=int(nhc), plane_class_stride=ncell,
                                 index_strides=self.index_strides_E)], mask, mask0)
        self.mergemaskA0 = mask
        for vec, aff in ((outA, self.affineA), (outE, self.affineE)):
            if aff is not None:
                vec.affine(*aff)
        return outA, outE


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

    def update_topo(self, topoo, emI_lands, emI_ices, run_ice=True, packer=None):
        """GCMCoupler_ModelE::update_topo's body (modele/GCMCoupler_ModelE.cpp:1026-1167): merge_topoO with RegridParams(false,
        true, 0), global_AvE(scale = true), wEAm_base, make_topoA and, with a TopoPacker, the packing.  topoo: a dict of the twelve planes under topoo_bundle's
        names (ZLAND_MIN / ZLAND_MAX need not be there); it holds the merged planes afterwards.  Numpy planes and masks go
        through the host entries; torch CUDA planes and masks stay in HBM between the calls (global_AvE alone reads the two
        ocean fractions on the host).  Raises RuntimeError with the sanity-check strings when a check fails.  Returns a dict:
        the TOPOA planes under TopoABundles' names, mergemask, fhc, elevE, underice, wEAm_base = (iE, weight) of the entries of
        AAmvEAm's Mw whose sparse index is >= offsetE, and offsetE.  packer: a TopoPacker, which holds mergemaskA0 from step
        to step; the dict then also has gcm_ivalsA and gcm_ivalsE, the VectorMultivecs of :1099-1164 after couple()'s unit
        conversion (:1216-1228), packed on the device without a host copy of any plane.  Not done here: reading the TOPOO file."""
        mergemaskOm, errors = merge_topoO(topoo, self.gcmO, emI_lands, emI_ices, self.hspecO, self.eq_rad)
        self.foceanOp = np.ascontiguousarray(_host(topoo["FOCEANF"]), np.float64).reshape(-1).copy()
        if not run_ice:
            self.foceanOm = np.ascontiguousarray(_host(topoo["FOCEAN"]), np.float64).reshape(-1).copy()
        if errors:
            raise RuntimeError("Errors in TOPO merging or regridding; halting!\n" + "\n".join("ERROR: " + e for e in errors))
        foceanOm = np.ascontiguousarray(_host(topoo["FOCEAN"]), np.float64).reshape(-1)
        AAmvEAm, offsetE = self.global_AvE(emI_lands, emI_ices, self.foceanOp, foceanOm, scale=True)
        iE, Mw = AAmvEAm.dim(1), AAmvEAm.Mw
        keep = iE >= offsetE
        nhc = len(self.hcdefs)
        sO = self.gcmO._hc_strides
        indexingHCA = (1, self.hspecA.size) if sO[1] >= sO[0] else (nhc, 1)
        topoa, errors2 = make_topoA(topoo, mergemaskOm, self.hspecO, self.hspecA, indexingHCA, self.hcdefs,
                                    [self.underice(k) for k in range(nhc)], AAmvEAm)
        if errors2:
            raise RuntimeError("Errors in TOPO merging or regridding; halting!\n" + "\n".join("ERROR: " + e for e in errors2))
        topoa.update(wEAm_base=(iE[keep].copy(), Mw[keep].copy()), offsetE=offsetE)
        if packer is not None:
            topoa["gcm_ivalsA"], topoa["gcm_ivalsE"] = packer.pack(topoa, nhc, run_ice)
        return topoa

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
        """_icebin.pyx:164-175 on the ModelE regridder.  The O-grid matrices are made with a zero sigma; the caller's is kept,
        and matrix() passes it per call, as the reference's matrix(name) uses the params the object was made with
        (RegridMatrices_Dynamic.cpp:425-437)."""
        rmO = self.gcmO.regrid_matrices(sheet_name, elevmaskI, scale=scale, correctA=correctA, sigma=(0, 0, 0), conserve=conserve)
        o = self.hspecO
        h = C.c_void_p()
        check(lib().ibh_modele_matrices_create(rmO._h, o.im, o.jm, float(o.offi), float(o.dlat), self.eq_rad, ptr(self.foceanOp),
                                              ptr(self.foceanOm), len(self.foceanOp), C.byref(h)))
        return RegridMatrices_ModelE(h, keep=(rmO, self), scale=scale, sigma=sigma)


def to_modele(gcmO, focean=None, hspecO=None, eq_rad=None, global_ec=None):
    """GCMRegridder.to_modele(focean=None).  The ocean grid's HntrSpec and the earth's radius come from the regridder when
    it was built from a spec (HntrGCMRegridder.hspecA / .eq_rad) or from the keywords.  global_ec: the base ice that
    global_AvE merges in (GCMRegridder_ModelE)."""
    hspecO = hspecO if hspecO is not None else getattr(gcmO, "hspecA", None)
    eq_rad = eq_rad if eq_rad is not None else getattr(gcmO, "eq_rad", None)
    if hspecO is None or eq_rad is None:
        raise RuntimeError("make_gridA() requires specO have a Hntr source")       # GCMRegridder_ModelE.cpp:40-41
    return GCMRegridder_ModelE(gcmO, hspecO, eq_rad, focean, global_ec)
