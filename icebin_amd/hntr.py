"""Hntr: GISS's HNTR4 conservative regridder between two lat-lon grids (icebin::modele::Hntr,
slib/icebin/modele/hntr.{hpp,cpp}), over the C-ABI of libicebin_hip.so (ibh_hntr_*).

Fields are stored i-fastest (flat index IJ = IA + im*(JA-1)): numpy shape (jm, im) in C order, or a flat
(im*jm,) vector; several fields stack as (nvar, im*jm) or (nvar, jm, im)."""
import ctypes as C

import numpy as np

from . import _capi
from ._arrays import dptr, leading_dim, padded_planes, stream_arg
from ._capi import check, lib, ptr

# kinds of Hntr matrix (ibh_hntr_matrix_d) and the to-dense transforms of MakeDenseEigenT
OVERLAP, SCALED = 0, 1
ADD_DENSE, TO_DENSE, TO_DENSE_IGNORE_MISSING = 0, 1, 2


class HntrSpec:
    """HntrSpec(im, jm, offi, dlat) (GridSpec.hpp:143-160): offi = cells from the date line to the western edge
    of cell 1, dlat = minutes of latitude of a non-polar cell."""

    def __init__(self, im, jm, offi, dlat):
        self.im, self.jm = int(im), int(jm)
        self.offi, self.dlat = float(offi), float(dlat)

    @property
    def size(self):
        return self.im * self.jm

    def __repr__(self):
        return "HntrSpec(%d, %d, %r, %r)" % (self.im, self.jm, self.offi, self.dlat)


def partition(Bspec, Aspec):
    """The constructor's partition (hntr.cpp:63-168), computed on the host by ibh_hntr_partition (no GPU needed):
    dict of SINA[jmA+1], SINB[jmB+1], IMIN, IMAX, FMIN, FMAX [imB], JMIN, JMAX, GMIN, GMAX [jmB] (1-based indices,
    IMAX(imB) already += imA)."""
    out = dict(SINA=np.zeros(Aspec.jm + 1), SINB=np.zeros(Bspec.jm + 1),
               IMIN=np.zeros(Bspec.im, np.int32), IMAX=np.zeros(Bspec.im, np.int32),
               FMIN=np.zeros(Bspec.im), FMAX=np.zeros(Bspec.im),
               JMIN=np.zeros(Bspec.jm, np.int32), JMAX=np.zeros(Bspec.jm, np.int32),
               GMIN=np.zeros(Bspec.jm), GMAX=np.zeros(Bspec.jm))
    check(lib().ibh_hntr_partition(Aspec.im, Aspec.jm, Aspec.offi, Aspec.dlat, Bspec.im, Bspec.jm, Bspec.offi, Bspec.dlat,
                                   *[ptr(out[k]) for k in ("SINA", "SINB", "IMIN", "IMAX", "FMIN", "FMAX", "JMIN", "JMAX", "GMIN",
                                                           "GMAX")]))
    return out


def make_dxyp(spec):
    """make_dxyp(spec) (hntr.cpp:33-52): the areas of grid rows on a unit sphere, [jm], host only (ibh_hntr_dxyp).  Index j-1
    holds the reference's dxyp(j)."""
    out = np.zeros(spec.jm)
    check(lib().ibh_hntr_dxyp(spec.im, spec.jm, ptr(out)))
    return out


# element codes of the typed regrid (IBH_HNTR_F64 / _I16 / _F32); 0 and 1 are ibh_multivec_append_planes_*'s plane types
F64, I16, F32 = 0, 1, 2
_CODES = {"float64": F64, "int16": I16, "float32": F32}


def _code(dtype):
    """The element code of a numpy or torch dtype; KeyError for any other (a numpy dtype that is not in native byte order
    included: the library reads the memory as it is)."""
    name = str(dtype).replace("torch.", "")
    if name not in _CODES:
        try:
            d = np.dtype(dtype)
        except TypeError:       # a torch dtype without a numpy counterpart
            raise KeyError(name) from None
        name = d.name if d.isnative else str(d)
    return _CODES[name]


def _is_scalar(x):
    return isinstance(x, (int, float, np.integer, np.floating)) or (isinstance(x, np.ndarray) and x.ndim == 0)


def _kind(kind):
    k = {"overlap": OVERLAP, "scaled": SCALED}.get(kind, kind)
    return int(k)


class Hntr(_capi.Handle):
    """Hntr(yp17, Bspec, Aspec, DATMIS=0) (hntr.hpp:114, hntr.cpp:63-79): yp17 is ignored, as in the reference.
    Creating one uploads the partition to the current HIP device (IBH_ENODEVICE without one)."""
    _destroy = "ibh_hntr_destroy"

    def __init__(self, yp17, Bgrid, Agrid, DATMIS=0.):
        self.Bgrid, self.Agrid, self.DATMIS = Bgrid, Agrid, float(DATMIS)
        h = C.c_void_p()
        check(lib().ibh_hntr_create(C.byref(h), Agrid.im, Agrid.jm, Agrid.offi, Agrid.dlat, Bgrid.im, Bgrid.jm, Bgrid.offi,
                                    Bgrid.dlat, self.DATMIS))
        self._h = h

    def _planes(self, X, what):
        X = np.asarray(X)
        # int16, float32 and float64 planes in native byte order travel as they are; anything else (a byte-swapped array from
        # a netCDF-3 or Fortran file included) becomes native float64, as np.asarray(X, np.float64) always did
        if not (X.dtype.isnative and X.dtype.name in _CODES):
            X = X.astype(np.float64)
        nA = self.Agrid.size
        if X.ndim == 1 or (X.ndim == 2 and X.shape == (self.Agrid.jm, self.Agrid.im)):
            if X.size != nA:
                raise ValueError("%s has %d cells, grid A has %d" % (what, X.size, nA))
            return np.ascontiguousarray(X.reshape(1, nA)), True
        X2 = X.reshape(X.shape[0], -1)
        if X2.shape[1] != nA:
            raise ValueError("%s: shape %s does not hold planes of %d cells" % (what, X.shape, nA))
        return np.ascontiguousarray(X2), False

    def regrid(self, WTA, A, mean_polar=False, wtm=1., wtb=0.):
        """Hntr::regrid(WTA, A, B, mean_polar, wtm, wtb) (hntr.hpp:341-435): returns B.  A is one field ((size,) or
        (jm, im)) or several ((nvar, size) or (nvar, jm, im)); WTA is one weight plane for all of them or one per
        field, or a scalar: the constant weight (the reference's const_array(shape, c)).  int16, float32 and float64 arrays
        are copied to the device in their own dtype (regrid<WeightT, SrcT, double>, hntr.hpp:385-391) and may differ between
        WTA and A; any other dtype is converted to float64 first.  One field comes back shaped like A on grid B, several as
        (nvar, Bgrid.size); B is float64."""
        A2, single = self._planes(A, "A")
        nvar = A2.shape[0]
        const = _is_scalar(WTA)
        if const:
            W2, wcode, wta_ld, wconst = None, F64, 0, float(WTA)
        else:
            W2, _ = self._planes(WTA, "WTA")
            if W2.shape[0] not in (1, nvar):
                raise ValueError("WTA has %d planes for %d fields" % (W2.shape[0], nvar))
            wcode, wta_ld, wconst = _code(W2.dtype), 0 if W2.shape[0] == 1 else W2.shape[1], 0.
        nB = self.Bgrid.size
        B = np.empty((nvar, nB))
        if nvar:
            check(lib().ibh_hntr_regrid_typed_host(self._h, None if const else ptr(W2), wcode, wta_ld, wconst, ptr(A2), _code(A2.dtype),
                                                   nvar, A2.shape[1], ptr(B), nB, int(bool(mean_polar)), float(wtm), float(wtb)))
        if single:
            return B[0].reshape(self.Bgrid.jm, self.Bgrid.im) if np.ndim(A) == 2 else B[0]
        return B

    def _mask(self, includeB):
        if includeB is None:
            return None
        m = np.ascontiguousarray(np.asarray(includeB).reshape(-1), np.uint8)
        if m.size != self.Bgrid.size:
            raise ValueError("includeB has %d entries, grid B has %d cells" % (m.size, self.Bgrid.size))
        return m

    def triplets(self, kind, eq_rad=1., includeB=None):
        """The entries of Hntr::matrix in stream order (ibh_hntr_triplets): (iB, iA, val), 0-based sparse indices."""
        m = self._mask(includeB)
        n = C.c_int64()
        mp = ptr(m) if m is not None else None
        check(lib().ibh_hntr_triplets(self._h, _kind(kind), float(eq_rad), mp, C.byref(n), None, None, None))
        iB, iA, val = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32), np.zeros(n.value)
        if n.value:
            check(lib().ibh_hntr_triplets(self._h, _kind(kind), float(eq_rad), mp, C.byref(n), ptr(iB), ptr(iA), ptr(val)))
        return iB, iA, val

    def overlap(self, eq_rad, includeB=None):
        """Hntr::overlap(accum, eq_rad, includeB) (hntr.hpp:284-291): what the accumulator receives, in order, as
        (iB, iA, val); includeB is a boolean mask over grid B (the functor or DimClip evaluated), None for every cell."""
        return self.triplets(OVERLAP, eq_rad, includeB)

    def scaled_regrid_matrix(self, includeB=None):
        """Hntr::scaled_regrid_matrix(accum, includeB) (hntr.hpp:327-336) as stream-order (iB, iA, val)."""
        return self.triplets(SCALED, 1., includeB)

    def matrix_d(self, kind, eq_rad=1., includeB=None, dims=(None, None), transforms=(ADD_DENSE, ADD_DENSE), transpose=False):
        """MakeDenseEigenT(overlap | scaled_regrid_matrix, transforms, dims, 'T' if transpose else '.') as a linear_Weighted in
        HBM (ibh_hntr_matrix_d).  kind: OVERLAP / SCALED or "overlap" / "scaled".  dims = (dimB, dimA): SparseSet (IN/OUT) or
        None for a fresh identity set; transforms: per generator index (B, then A) ADD_DENSE, TO_DENSE or
        TO_DENSE_IGNORE_MISSING; transpose swaps only the output (rows A, columns B)."""
        from .linear import linear_Weighted
        m = self._mask(includeB)
        h = C.c_void_p()
        dB = dims[0]._h if dims[0] is not None else None
        dA = dims[1]._h if dims[1] is not None else None
        check(lib().ibh_hntr_matrix_d(self._h, _kind(kind), float(eq_rad), ptr(m) if m is not None else None, dB, int(transforms[0]),
                                      dA, int(transforms[1]), int(bool(transpose)), C.byref(h)))
        return linear_Weighted(h, keep=(self, dims))

    def regrid_device(self, WTA, A, out=None, mean_polar=False, wtm=1., wtb=0., stream=None):
        """The same on fields resident in HBM: torch.float64, float32 or int16 CUDA tensors (A and WTA may differ), A [nvar,
        Agrid.size] (row stride >= size), WTA [Agrid.size] or [1, size] (shared) or [nvar, size], or a scalar: the constant
        weight; only enqueues work on `stream` (default: torch's current stream).  Returns out [nvar, Bgrid.size], float64."""
        import torch
        nA, nB = self.Agrid.size, self.Bgrid.size
        types = (torch.float64, torch.float32, torch.int16)
        assert A.is_cuda and A.dtype in types and A.dim() == 2 and A.stride(1) == 1 and A.shape[1] == nA
        nvar = A.shape[0]
        const = _is_scalar(WTA)
        if not const:
            W = WTA if WTA.dim() == 2 else WTA.reshape(1, -1)
            assert W.is_cuda and W.dtype in types and W.dim() == 2 and W.stride(1) == 1 and W.shape[1] == nA
            assert W.shape[0] in (1, nvar)
        if out is None:
            out = padded_planes(nvar, nB, A.device)
        assert out.is_cuda and out.dtype == torch.float64 and out.dim() == 2 and out.shape == (nvar, nB) and out.stride(1) == 1
        wta_ld, lda, ldb = device_strides(nvar, nA, nB, 1 if const else W.shape[0], 0 if const else W.stride(0), A.stride(0),
                                          out.stride(0))
        check(lib().ibh_hntr_regrid_typed_device(self._h, None if const else dptr(W), F64 if const else _code(W.dtype),
                                                 wta_ld, float(WTA) if const else 0., dptr(A), _code(A.dtype), nvar,
                                                 lda, dptr(out), ldb, int(bool(mean_polar)), float(wtm), float(wtb), stream_arg(A, stream)))
        return out

    def regrid_shape(self, nvar, WTA_dtype, A_dtype, per_field=False):
        """What regrid of nvar fields would launch (ibh_hntr_regrid_shape; launches nothing): dict(NV, L, K, lds_bytes) = fields
        per group, chain lanes per wave, columns per chunk, LDS bytes per workgroup.  WTA_dtype None: the constant weight;
        per_field: one weight plane per field."""
        NV, L, K, lds = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        const = WTA_dtype is None
        check(lib().ibh_hntr_regrid_shape(self._h, int(nvar), int(const), F64 if const else _code(WTA_dtype),
                                          1 if per_field and not const else 0, _code(A_dtype), C.byref(NV), C.byref(L), C.byref(K),
                                          C.byref(lds)))
        return dict(NV=NV.value, L=L.value, K=K.value, lds_bytes=lds.value)


def device_strides(nvar, nA, nB, wta_planes, wta_stride, a_stride, out_stride):
    """(wta_ld, lda, ldb) for ibh_hntr_regrid_device from the plane strides of torch tensors.  A single plane's stride is
    never read.  One weight plane, or planes broadcast with stride 0 (`w.expand(nvar, -1)`), is the shared weight
    (wta_ld = 0).  Otherwise every stride must hold a whole plane (leading_dim: refused before anything is launched)."""
    wta_ld = 0 if wta_planes == 1 or wta_stride == 0 else leading_dim(wta_planes, wta_stride, nA, "WTA")
    return wta_ld, leading_dim(nvar, a_stride, nA, "A"), leading_dim(nvar, out_stride, nB, "out")
