"""global_ec (modele/global_ec.cpp): elevation-class matrices for a global lat-lon ice grid, built from grid specs and an
ice mask.  new_gcmA_standard's exchange grid (Hntr's overlap under the mask, ExchAccum) and regridder are built in place on
the device (ibh_regridder_create_hntr); make_I2vX maps IvE / IvA onto a coarser plottable grid (ibh_weighted_make_I2vX)."""
import ctypes as C
import math

import numpy as np

from . import _capi
from ._arrays import dptr, einval, is_cuda, named_planes, stream_arg
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
    if is_cuda(elevmaskI):
        em = elevmaskI.reshape(-1).contiguous()
        assert str(em.dtype) == "torch.float64"
        return em.data_ptr(), em.numel(), 1, stream_arg(em).value or 0, em
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


# ---- global_ec in chunks: main() below "Check that I grid fits neatly into O grid" (global_ec.cpp:752-893) and
# combine_global_ec.cpp's combine_chunks (:94-262) ----------------------------------------------------------------------------
CHUNK_SIZE = 12000000           # global_ec.cpp:100


def chunk_plan(imO, jmO, mult_i, mult_j, counts, chunk_size=CHUNK_SIZE):
    """The chunk walk of global_ec.cpp:863-893 over host counts c[k] = fgiceO[k] != 0 ? nice[k] : 0, k = jO*imO + iO (no GPU
    needed): [((chunkno, jO0, iO0, jO1, iO1), nice), ...].  See IceScan.chunks."""
    c = np.ascontiguousarray(np.asarray(counts).reshape(-1), np.int32)
    if len(c) != int(imO) * int(jmO):
        raise einval("counts: %d cells, the ocean grid has %d" % (len(c), int(imO) * int(jmO)))
    n = C.c_int32()
    args = (int(imO), int(jmO), int(mult_i), int(mult_j), ptr(c), int(chunk_size))
    check(lib().ibh_global_ec_chunk_plan_counts(*args, 0, None, None, C.byref(n)))
    ch, nice = np.zeros((n.value, 5), np.int32), np.zeros(n.value, np.int64)
    check(lib().ibh_global_ec_chunk_plan_counts(*args, n.value, ptr(ch), ptr(nice), C.byref(n)))
    return [(tuple(int(x) for x in ch[i]), int(nice[i])) for i in range(n.value)]


class IceScan(_capi.Handle):
    """The global ice of global_ec's main() (global_ec.cpp:752-816) on the device: fgiceI / elevI are the int16 planes
    [jmI, imI] (FGICE1m / ZICETOP1m), host numpy arrays (uploaded once in their own width and kept) or torch.int16 CUDA
    tensors (kept as they are).  hspecI must nest in hspecO.  One pass over both planes gives .nice and .elevI_range;
    .fgiceO is Hntr(17.17, hspecO, hspecI).regrid(1.0, fgiceI).  fgiceO and nice are torch CUDA tensors [jmO, imO]."""
    _destroy = "ibh_global_ec_scan_destroy"

    def __init__(self, hspecO, hspecI, fgiceI, elevI):
        self.hspecO, self.hspecI = hspecO, hspecI
        planes, dev = named_planes((("fgiceI", fgiceI, "int16", hspecI.size), ("elevI", elevI, "int16", hspecI.size)),
                                   "fgiceI / elevI: one plane is on the host and one on the device", mix_detail=False,
                                   dtype_is="the ice planes are %s", cells_of="hspecI has %d", null=None)
        pp = [dptr(p) if dev else ptr(p) for p in planes]
        h = C.c_void_p()
        from .hntr import I16
        check(lib().ibh_global_ec_scan_create(hspecO.im, hspecO.jm, hspecO.offi, hspecO.dlat, hspecI.im, hspecI.jm, hspecI.offi, hspecI.dlat,
                                              pp[0], pp[1], hspecI.size, I16, int(dev), stream_arg(planes[0]) if dev else None, C.byref(h)))
        self._h = h
        self._planes = planes if dev else None       # device planes are read in place: they live as long as the scan
        self.mult_i, self.mult_j = hspecI.im // hspecO.im, hspecI.jm // hspecO.jm
        r = np.zeros(2, np.int16)
        check(lib().ibh_global_ec_scan_get(h, None, None, ptr(r), None, None))
        self.elevI_range = (int(r[0]), int(r[1]))
        self._fgiceO = self._nice = None

    def _copies(self):
        """fgiceO and nice as torch tensors: device-to-device copies of the scan's arrays, made once."""
        if self._fgiceO is None:
            import torch
            shape = (self.hspecO.jm, self.hspecO.im)
            f = torch.empty(shape, dtype=torch.float64, device="cuda")
            n = torch.empty(shape, dtype=torch.int32, device="cuda")
            check(lib().ibh_global_ec_scan_copy_device(self._h, dptr(f), dptr(n), stream_arg(f)))
            self._fgiceO, self._nice = f, n
        return self._fgiceO, self._nice

    @property
    def fgiceO(self):
        """[jmO, imO] float64 on the device: Hntr(17.17, hspecO, hspecI).regrid(1.0, fgiceI)."""
        return self._copies()[0]

    @property
    def nice(self):
        """[jmO, imO] int32 on the device: the ice cells (fgiceI != 0) of every ocean cell's tile."""
        return self._copies()[1]

    def ec_range(self, ec_skip):
        """(ec_skip*floor(min/ec_skip), ec_skip*ceil(max/ec_skip)) (global_ec.cpp:815-816): global, so every chunk gets the
        same classes hcdefs(lo, hi, ec_skip)."""
        r, out = np.asarray(self.elevI_range, np.int16), np.zeros(2)
        check(lib().ibh_global_ec_ec_range(ptr(r), float(ec_skip), ptr(out)))
        return float(out[0]), float(out[1])

    def chunks(self, chunk_size=CHUNK_SIZE):
        """The chunk plan (global_ec.cpp:863-893): [((chunkno, jO0, iO0, jO1, iO1), nice), ...], the last bound (jmO, 0).
        A chunk ends, exclusive, at the first ocean cell at which its running ice count reaches chunk_size; that cell is the
        next chunk's first, and its ice is in the reported nice of both.  chunk_size must exceed mult_i*mult_j."""
        n = C.c_int32()
        check(lib().ibh_global_ec_chunk_plan(self._h, int(chunk_size), 0, None, None, C.byref(n)))
        ch, nice = np.zeros((n.value, 5), np.int32), np.zeros(n.value, np.int64)
        check(lib().ibh_global_ec_chunk_plan(self._h, int(chunk_size), n.value, ptr(ch), ptr(nice), C.byref(n)))
        return [(tuple(int(x) for x in ch[i]), int(nice[i])) for i in range(n.value)]

    def chunk_mask(self, chunk, out=None):
        """elevmaskI of one chunk (global_ec.cpp:818-855) as a torch.float64 CUDA tensor [nI]: elevI where the cell has ice and
        its ocean cell lies in the chunk and has fgiceO != 0, else NaN.  chunk: (chunkno, jO0, iO0, jO1, iO1), or a pair
        (chunk, nice) as .chunks() returns them."""
        import torch
        if len(chunk) == 2:
            chunk = chunk[0]
        if len(chunk) != 5:
            raise einval("chunk: expected (chunkno, jO0, iO0, jO1, iO1)")
        if out is None:
            out = torch.empty(self.hspecI.size, dtype=torch.float64, device="cuda")
        if not (is_cuda(out) and out.dtype == torch.float64 and out.is_contiguous()):
            raise einval("out: the mask is written to a contiguous torch.float64 CUDA tensor of %d cells" % self.hspecI.size)
        check(lib().ibh_global_ec_chunk_mask(self._h, *[int(x) for x in chunk[1:]], dptr(out), out.numel(), stream_arg(out)))
        return out


def run_chunk(scan, chunk, hspecA, hspecI2, ec_skip, ofname=None, names=MATRIX_NAMES, correctA=True, sigma=(0., 0., 0.), Achar=None,
              eq_rad=6371000.):
    """One chunk of global_ec (--runchunk, global_ec.cpp:818-861): the chunk's mask, new_gcmA_standard on hspecA with the
    classes of the WHOLE globe's ice (scan.ec_range), and global_ec_section through write_matrices into "%s-%02d" % (ofname,
    chunkno) (:529; ofname None: nothing is kept).  Achar defaults to "O" when hspecA is the scan's ocean grid (the `ocean`
    option), else "A".  Returns write_matrices' {variable name: linear_Weighted}."""
    import os
    if len(chunk) == 2:
        chunk = chunk[0]
    mask = scan.chunk_mask(chunk)
    lo, hi = scan.ec_range(ec_skip)
    gcm = gcm_from_hntr(hspecA, scan.hspecI, mask, hcdefs(lo, hi, ec_skip), correctA, eq_rad)
    if Achar is None:
        O = scan.hspecO
        Achar = "O" if (hspecA.im, hspecA.jm, hspecA.offi, hspecA.dlat) == (O.im, O.jm, O.offi, O.dlat) else "A"
    # write_matrices always writes its file (it is global_ec_section); without a name the image goes to the null device
    fname = os.devnull if ofname is None else "%s-%02d" % (ofname, int(chunk[0]))
    return write_matrices(gcm, mask, hspecI2, fname, names, correctA, sigma, Achar)


class CombinedWeighted(linear_Weighted):
    """What combine_chunks returns: the combined matrix over {dimB_out, dimA_out} with the weights wM_out / Mw_out, and the
    triplet stream it was summed from."""

    def coo_sparse(self):
        """(iB, iA, val): the reference's stream (combine_global_ec.cpp:217-227) in sparse indices, chunks in order, each chunk's
        entries in stored row-major order; duplicates across chunks are NOT summed.  With shape, the base of
        compute_EOpvAOp_merged."""
        return self._stream


def _combine(mats, scale, host=None):
    """mats: the chunks' matrices in order; host: None (the handles' own sets) or [(dimB, dimA, extB, extA), ...]."""
    n = len(mats)
    if n == 0:
        raise einval("chunk_results: combine_chunks needs at least one chunk")
    hs = (C.c_void_p * n)(*[m._h.value for m in mats])
    nnz = sum(m.nnz for m in mats)
    iB, iA, val = np.zeros(nnz, np.int64), np.zeros(nnz, np.int64), np.zeros(nnz)
    dp = ext = keep = None
    if host is not None:
        keep = [np.ascontiguousarray(d, np.int64) for h_ in host for d in h_[:2]]
        dp = (C.c_void_p * (2 * n))(*[ptr(d).value if len(d) else None for d in keep])
        ext = np.asarray([e for h_ in host for e in h_[2:]], np.int64)
    h = C.c_void_p()
    check(lib().ibh_global_ec_combine_chunks(n, hs, dp, ptr(ext), int(bool(scale)), ptr(iB), ptr(iA), ptr(val), C.byref(h)))
    w = CombinedWeighted(h)
    w._stream = (iB, iA, val)
    return w


def _chunk_matrix(result, c, name):
    for vn in (name, name.replace("A", "O")):
        if vn in result:
            return result[vn]
    raise einval("name: chunk %d holds no matrix %r (it has %s)" % (c, name, ", ".join(sorted(result))))


def combine_chunks(chunk_results, name, scale=False):
    """combine_chunks (combine_global_ec.cpp:94-262) for the matrix `name` ("EvA", ...; found under A -> O in the results of an
    ocean run, :124-127).  chunk_results: run_chunk's results in chunk order.  The chunks' matrices, sets and weights are read
    where they are, in HBM.  Returns a CombinedWeighted: dims = the first-seen numbering of the chunks' sets, wM / Mw = the
    chunks' weights summed in chunk order, M = setFromTriplets of the stream (scale: values times 1/wM of their row), and
    .coo_sparse() the stream itself."""
    chunk_results = list(chunk_results)
    return _combine([_chunk_matrix(r, c, name) for c, r in enumerate(chunk_results)], scale)


def combine_chunk_files(ifnames, ofname, names=MATRIX_NAMES, scale=False):
    """combine_global_ec's main loop: every matrix of `names` read from the chunk files `ifnames` (ncio), combined, and
    written in the Eigen format under BvA, with A -> O when the files are an ocean run's (:124-127).  Returns {variable
    name: CombinedWeighted}."""
    from . import ncio
    dss = [ncio.Dataset.read(f) for f in ifnames]
    if not dss:
        raise einval("ifnames: combine_chunk_files needs at least one chunk file")
    out, ds, written = {}, ncio.Dataset(), {}

    def dim_name(letter, vname, to_sparse):
        """dimB, shared by the matrices whose combined set is the same table; a matrix whose numbering differs gets its own."""
        base = "dim" + letter
        if not np.array_equal(written.setdefault(base, to_sparse), to_sparse):
            base += "_" + vname
            written[base] = to_sparse
        return base

    for name in names:
        vname = name if name + ".info" in dss[0].variables else name.replace("A", "O")
        mats, host = [], []
        for c, d in enumerate(dss):
            if vname + ".info" not in d.variables:
                raise einval("names: chunk file %s holds no matrix %r" % (ifnames[c], name))
            w = linear_Weighted.nc_read(d, vname)
            mats.append(w)
            host.append((w._dims[0], w._dims[1], w._sparse_extents[0], w._sparse_extents[1]))
        w = _combine(mats, scale, host)
        w.ncio(ds, vname, (dim_name(vname[0], vname, w.dim(0)), dim_name(vname[2], vname, w.dim(1))))
        out[vname] = w
    ds.write(ofname)
    return out
