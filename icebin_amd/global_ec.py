"""global_ec (modele/global_ec.cpp): elevation-class matrices for a global lat-lon ice grid, built from grid specs and an
ice mask.  new_gcmA_standard's exchange grid (Hntr's overlap under the mask, ExchAccum) and regridder are built in place on
the device (ibh_regridder_create_hntr); make_I2vX maps IvE / IvA onto a coarser plottable grid (ibh_weighted_make_I2vX)."""
import ctypes as C
import math

import numpy as np

from . import _capi
from ._capi import check, lib, ptr
from .hntr import Hntr
from .linear import SparseSet, linear_Weighted
from .regrid import _INTERP, GCMRegridder

D2R = math.pi / 180.0           # gridgen/GridGen_LonLat.cpp:38
MATRIX_NAMES = ("AvI", "EvI", "IvE", "IvA", "AvE", "EvA")


def hcdefs(ec_lo, ec_hi, ec_skip):
    """The elevation classes of new_gcmA_standard (global_ec.cpp:403-407): `for (elev = lo; elev <= hi; elev += skip)`, the
    sum accumulated (so 0.1-steps carry their rounding along, as the reference's do)."""
    out = []
    elev = float(ec_lo)
    while elev <= ec_hi:
        out.append(elev)
        elev += float(ec_skip)
    return np.asarray(out, np.float64)


def make_grid_spec(hspec):
    """make_grid_spec(hspec, pole_caps=false) (GridSpec.cpp:80-122): (lonb [im+1], latb [2*(jm/2)+1]) in degrees.  The
    reference refuses an odd im; the boundaries are well defined for one, and it is accepted, as the library does."""
    deg_by_im = 360. / float(hspec.im)
    lonb = [-180. + (hspec.offi + float(i)) * deg_by_im for i in range(hspec.im)]
    lonb.append(lonb[0] + 360.)
    latb = [0.]
    dlat_d = hspec.dlat / 60.
    for j in range(1, hspec.jm // 2):
        lat = j * dlat_d
        latb += [lat, -lat]
    lat = hspec.jm // 2 * dlat_d
    if abs(lat - 90.) < 1.e-10:
        lat = 90.
    latb += [lat, -lat]
    return np.asarray(lonb), np.asarray(sorted(latb))


def native_area(hspec, to_sparse, eq_rad):
    """make_abbr_grid's native_area (GridGen_LonLat.cpp:254-265) for the cells to_sparse of the grid hspec, i-fastest:
    (sin(latb[j+1]) - sin(latb[j])) * (lonb[i+1] - lonb[i]) * (D2R*eq_rad*eq_rad), with the reference's latitudes in DEGREES
    passed to sin (libm, as the library computes it)."""
    lonb, latb = make_grid_spec(hspec)
    dxyp = [math.sin(latb[j + 1]) - math.sin(latb[j]) for j in range(len(latb) - 1)]
    d2r_r2 = D2R * eq_rad * eq_rad
    s = np.asarray(to_sparse, np.int64)
    return np.asarray([dxyp[int(k) // hspec.im] * (lonb[int(k) % hspec.im + 1] - lonb[int(k) % hspec.im]) * d2r_r2 for k in s],
                      np.float64)


def _mask_arg(elevmaskI):
    """(pointer, n, on_device, stream, keep-alive) of a host array or a torch.float64 CUDA tensor."""
    if hasattr(elevmaskI, "is_cuda") and elevmaskI.is_cuda:
        import torch
        em = elevmaskI.reshape(-1).contiguous()
        assert em.dtype == torch.float64
        return em.data_ptr(), em.numel(), 1, torch.cuda.current_stream(em.device).cuda_stream, em
    em = np.ascontiguousarray(np.asarray(elevmaskI, np.float64).reshape(-1))
    return ptr(em).value, len(em), 0, None, em


def _desc(hntr, elevmaskI, hcdefs_, eq_rad, interp_style):
    p, n, dev, st, keep = _mask_arg(elevmaskI)
    hc = np.ascontiguousarray(hcdefs_, np.float64)
    d = _capi.HntrRegridderDesc(hntr=hntr._h.value, eq_rad=float(eq_rad), elevmaskI=p, nmask=n, mask_on_device=dev, stream=st,
                                nhc=len(hc), hcdefs=ptr(hc).value if len(hc) else None, hc_stride_A=1,
                                hc_stride_HC=hntr.Bgrid.size, interp_style=_INTERP[interp_style])
    return d, (keep, hc)


def exgrid_count(hspecA, hspecI, elevmaskI, eq_rad):
    """The number of exchange cells new_gcmA_standard would build (64 bits, counted on the device, nothing built)."""
    hntr = Hntr(17.17, hspecA, hspecI)
    d, keep = _desc(hntr, elevmaskI, np.zeros(0), eq_rad, "Z_INTERP")
    n = C.c_int64()
    check(lib().ibh_hntr_exgrid_count(C.byref(d), C.byref(n)))
    return n.value


class _HntrSheet:
    """A sheet whose arrays live on the device; ncio_write's host copies are fetched on first use."""

    def __init__(self, handle, nI, interp_style):
        self.h, self.nI, self.interp_style, self.centroid = handle, nI, interp_style, None
        self._arrays = self._agridA = None

    @property
    def arrays(self):
        """(exchange-grid indices int32[2*nX], overlaps f64[nX], gridA_proj_area f64[nA_dense]), read back once."""
        if self._arrays is None:
            n = C.c_int64()
            check(lib().ibh_regridder_exgrid(self.h, C.byref(n), None, None))
            idx, area = np.zeros(2 * n.value, np.int32), np.zeros(n.value)
            check(lib().ibh_regridder_exgrid(self.h, C.byref(n), ptr(idx), ptr(area)))
            nA = C.c_int32()
            check(lib().ibh_regridder_agridA(self.h, C.byref(nA), None, None, None))
            proj = np.zeros(nA.value)
            check(lib().ibh_regridder_agridA(self.h, C.byref(nA), None, None, ptr(proj)))
            self._arrays = (idx, area, proj)
        return self._arrays

    def agridA(self):
        """(to_sparse int64[nA_dense], native_area f64[nA_dense]), read back once (without the exchange grid)."""
        if self._agridA is None:
            nA = C.c_int32()
            check(lib().ibh_regridder_agridA(self.h, C.byref(nA), None, None, None))
            a2s, nat = np.zeros(nA.value, np.int64), np.zeros(nA.value)
            check(lib().ibh_regridder_agridA(self.h, C.byref(nA), ptr(a2s), ptr(nat), None))
            self._agridA = (a2s, nat)
        return self._agridA


class HntrGCMRegridder(GCMRegridder):
    """GCMRegridder_Standard of new_gcmA_standard: one sheet "globalI" built on the device.  regrid_matrices, wA and
    ncio_write work as for any GCMRegridder; agridA's host arrays are read back when first needed."""

    def __init__(self, hspecA, hspecI, handle, nI, hcdefs_, correctA, eq_rad, interp_style, dimA, dimI):
        self._nA = hspecA.size
        self._hcdefs = np.ascontiguousarray(hcdefs_, np.float64)
        self.correctA = bool(correctA)
        self._hc_strides = (1, self._nA)
        self.hspecA, self.hspecI, self.eq_rad = hspecA, hspecI, float(eq_rad)
        self.dimA, self.dimI = dimA, dimI
        self._sheets = {"globalI": _HntrSheet(handle, nI, interp_style)}

    @property
    def _A_to_sparse(self):
        return self._sheets["globalI"].agridA()[0]

    @property
    def _A_native(self):
        return self._sheets["globalI"].agridA()[1]

    def exgrid(self):
        """(indices int32[nX, 2] (iA, iI), overlaps f64[nX]) of the sheet, read back from the device."""
        idx, area, _ = self._sheets["globalI"].arrays
        return idx.reshape(-1, 2), area


def gcm_from_hntr(hspecA, hspecI, elevmaskI, hcdefs, correctA=True, eq_rad=6371000., interp_style="Z_INTERP"):
    """new_gcmA_standard(hspecA, grid_name, args, elevmaskI) (global_ec.cpp:384-432) with hspecA the GCM grid (the reference's
    `ocean` option) and hspecI the ice grid; elevmaskI [hspecI.size] on the host or a torch.float64 CUDA tensor (NaN: no ice).
    The result's dimA / dimI hold the reference's _dimA (GCM cells with ice, ascending) and _dimI (ice cells, first-seen)."""
    hntr = Hntr(17.17, hspecA, hspecI)
    d, keep = _desc(hntr, elevmaskI, hcdefs, eq_rad, interp_style)
    dimA, dimI = SparseSet(), SparseSet()
    h = C.c_void_p()
    check(lib().ibh_regridder_create_hntr(C.byref(d), dimA._h, dimI._h, C.byref(h)))
    del keep
    return HntrGCMRegridder(hspecA, hspecI, h, hspecI.size, hcdefs, correctA, eq_rad, interp_style, dimA, dimI)


def make_I2vX(IvX, hspecI, hspecI2, elevmaskI, dimI2=None, eq_rad=6371000.):
    """make_I2vX (global_ec.cpp:345-376): IvX (IvE or IvA from matrix_d, dims {dimI, dimX}) on the plottable grid hspecI2,
    through I2vI = Hntr(17.17, hspecI, hspecI2).overlap(eq_rad, ElevMaskClip(elevmaskI)).  dimI2: SparseSet (appended to) or
    None.  Returns a linear_Weighted with dims {dimI2, dimX}."""
    hntr = Hntr(17.17, hspecI, hspecI2)
    em = np.asarray(elevmaskI.cpu() if hasattr(elevmaskI, "cpu") else elevmaskI, np.float64).reshape(-1)
    incl = np.ascontiguousarray(~np.isnan(em), np.uint8)
    h = C.c_void_p()
    check(lib().ibh_weighted_make_I2vX(IvX._h, hntr._h, float(eq_rad), ptr(incl), len(incl), dimI2._h if dimI2 is not None else None,
                                       C.byref(h)))
    return linear_Weighted(h, keep=(IvX, dimI2))


def check_negative(mat, name):
    """check_negative (global_ec.cpp:440-463): prints every negative weight and entry, then raises RuntimeError."""
    neg = False
    for j, wt in enumerate((mat.wM, mat.Mw)):
        for i in np.nonzero(np.asarray(wt) < 0)[0]:
            print("wt[%d](%d) = %g" % (j, i, wt[i]))
            neg = True
    row, col, val = mat.coo_dense()
    for k in np.nonzero(val < 0)[0]:
        print("%s(%d,%d)=%g" % (name, row[k], col[k], val[k]))
        neg = True
    if neg:
        raise RuntimeError("Negative values found in matrix or weights for %s" % name)


def write_matrices(gcm, elevmaskI, hspecI2, fname, names=MATRIX_NAMES, correctA=True, sigma=(0., 0., 0.), Achar="A"):
    """global_ec_section (global_ec.cpp:509-655) without chunking: RegridParams(scale=false, correctA, sigma), the dims
    dimA / dimE / dimI / dimI2 shared by every matrix, each matrix checked by check_negative, IvE and IvA followed by
    I2vE / I2vA, written in the Eigen format through the NetCDF-classic writer under the reference's names (AvI, EvI, IvE,
    I2vE, IvA, I2vA, AvE, EvA; A -> Achar).  Returns {variable name in the file: linear_Weighted}."""
    from . import ncio
    rm = gcm.regrid_matrices("globalI", elevmaskI, scale=False, correctA=correctA, sigma=sigma)
    dimA, dimI, dimE, dimI2 = SparseSet(), SparseSet(), SparseSet(), SparseSet(hspecI2.size)
    dims = {"A": dimA, "E": dimE, "I": dimI}
    built = []          # (reference name, matrix, dim names), A not yet replaced by Achar
    for name in MATRIX_NAMES:
        if name not in names:
            continue
        mat = rm.matrix_d(name, (dims[name[0]], dims[name[2]]), scale=False, correctA=correctA, sigma=sigma)
        check_negative(mat, name)
        built.append((name, mat, ("dim" + name[0], "dim" + name[2])))
        if name in ("IvE", "IvA"):
            mat2 = make_I2vX(mat, gcm.hspecI, hspecI2, elevmaskI, dimI2, gcm.eq_rad)
            built.append(("I2v" + name[2], mat2, ("dimI2", "dim" + name[2])))
    ds = ncio.Dataset()
    out = {}
    for name, mat, dn in built:
        vname = name.replace("A", Achar)
        mat.ncio(ds, vname, tuple(n.replace("A", Achar) for n in dn))
        out[vname] = mat
    shapes = {"dimA": [gcm.hspecA.jm, gcm.hspecA.im], "dimE": [gcm.nhc, gcm.hspecA.jm, gcm.hspecA.im],
              "dimI": [gcm.hspecI.jm, gcm.hspecI.im], "dimI2": [hspecI2.jm, hspecI2.im]}
    desc = {"dimA": "GCM ('Atmosphere' or 'Ocean') Grid", "dimE": "Elevation Grid", "dimI": "Fine-scale ('Ice') Grid",
            "dimI2": "Recuction of Fine-scale Grid, for easy plotting"}
    for k, s in (("dimA", dimA), ("dimE", dimE), ("dimI", dimI), ("dimI2", dimI2)):
        vn = k.replace("A", Achar)
        ncio.put_sparse_set(ds, vn, s.to_sparse(), s.sparse_extent())
        ds.variables[vn].attrs["shape"] = np.asarray(shapes[k], np.int32)
        ds.variables[vn].attrs["description"] = desc[k]
    ds.write(fname)
    return out
