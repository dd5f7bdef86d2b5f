"""VectorMultivec: the Python face of icebin::VectorMultivec (slib/icebin/multivec.hpp), the parallel sparse vectors the
coupler exchanges with the GCM, resident in HBM (ibh_multivec, include/icebin_hip.h).

Array arguments are torch.float64 CUDA tensors (used in place, on torch's current stream) or numpy arrays (copied to the
device and back), the way linear_Weighted.apply_transformed takes them."""
import ctypes as C

import numpy as np

from . import _capi
from ._arrays import dptr, is_cuda, plane_stride, stream_arg, to_device
from ._capi import check, lib, ptr


def _to_device(a, ndim):
    """(tensor, came from the host): a float64 CUDA tensor with unit inner stride."""
    if is_cuda(a):
        assert str(a.dtype) == "torch.float64" and a.dim() == ndim and a.stride(-1) == 1
        return a, False
    h = np.ascontiguousarray(a, np.float64)
    assert h.ndim == ndim
    return to_device(h), True


def _back(t, host):
    if not host:
        return t
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


class VectorMultivec(_capi.Handle):
    """VectorMultivec(nvar): index int64[n], weights float64[n], vals float64[n, nvar] (multivec.hpp:25-31)."""
    _destroy = "ibh_multivec_destroy"

    def __init__(self, nvar, _handle=None):
        h = C.c_void_p()
        if _handle is not None:
            h = _handle
        else:
            check(lib().ibh_multivec_create(int(nvar), C.byref(h)))
        self._h = h

    def _size(self):
        n, nvar = C.c_int64(), C.c_int32()
        check(lib().ibh_multivec_size(self._h, C.byref(n), C.byref(nvar)))
        return n.value, nvar.value

    @property
    def nvar(self):
        return self._size()[1]

    def size(self):
        return self._size()[0]

    __len__ = size

    def clear(self):
        check(lib().ibh_multivec_clear(self._h))

    def reserve(self, n):
        """Room for n entries in all: appends up to there allocate nothing (ibh_multivec_reserve)."""
        check(lib().ibh_multivec_reserve(self._h, int(n)))

    def add(self, ix, val, weight):
        """add(ix, val, weight) (multivec.cpp:8-13); arrays add many entries at once: ix[k], val[k, nvar], weight[k]."""
        index = np.ascontiguousarray(np.atleast_1d(ix), np.int64)
        weights = np.ascontiguousarray(np.atleast_1d(weight), np.float64)
        vals = np.ascontiguousarray(val, np.float64).reshape(len(index), -1)
        if vals.shape[1] != self.nvar or len(weights) != len(index):
            raise ValueError("add: %d indices, %d weights, values of shape %s for nvar=%d" % (len(index), len(weights), vals.shape, self.nvar))
        check(lib().ibh_multivec_add_host(self._h, len(index), ptr(index), ptr(weights), ptr(vals)))

    def _get(self, which):
        n, nvar = self._size()
        out = np.empty((n, nvar) if which == 2 else n, np.int64 if which == 0 else np.float64)
        args = [None, None, None]
        args[which] = ptr(out)
        check(lib().ibh_multivec_get(self._h, *args))
        return out

    @property
    def index(self):
        return self._get(0)

    @property
    def weights(self):
        return self._get(1)

    @property
    def vals(self):
        """float64[n, nvar]: val(ivar, ix) of the reference is vals[ix, ivar]."""
        return self._get(2)

    def device_view(self):
        """(n, nvar, index, weights, vals) with the three as device addresses, valid until the next append."""
        v = _capi.MultivecDeviceView()
        check(lib().ibh_multivec_device_view_get(self._h, C.byref(v)))
        return v.n, v.nvar, v.index, v.weights, v.vals

    def append_weighted(self, w, B):
        """One entry per dense row of the linear_Weighted w from its field-major product B[nvar, nrow_d]
        (IceCoupler.cpp:447-458): index = dims[0] to_sparse, weight = wM, values = B[:, row]."""
        dB, _ = _to_device(B, 2)
        assert dB.shape[1] == w.nrow_d
        check(lib().ibh_multivec_append_weighted_device(self._h, w._h, dptr(dB), dB.shape[0], plane_stride(dB, w.nrow_d, "B"),
                                                       stream_arg(dB)))

    def append(self, other):
        check(lib().ibh_multivec_append(self._h, other._h))

    def append_planes(self, planes, mask, mask0=None, nclass=1, plane_class_stride=None, index_strides=None, types=None):
        """update_topo's packing (modele/GCMCoupler_ModelE.cpp:1099-1164): for ihc < nclass (outer) and every cell c ascending
        with mask[c] != 0 or mask0[c] != 0, one entry (c * index_strides[0] + ihc * index_strides[1], planes[k][ihc *
        plane_class_stride + c] for every k, weight 1.0) -> the number of kept cells.  planes: nvar float64 or int16 arrays
        (types: 0 / 1 per plane, default: by dtype); mask, mask0: int16, ncell = mask's size.  All numpy arrays, or all torch
        CUDA tensors (used in place, on torch's current stream).  Defaults: plane_class_stride = ncell, index_strides = (1, ncell)."""
        return append_planes_many([dict(vec=self, planes=planes, nclass=nclass, plane_class_stride=plane_class_stride,
                                        index_strides=index_strides, types=types)], mask, mask0)

    def affine(self, mm, bb):
        """couple()'s unit conversion (modele/GCMCoupler_ModelE.cpp:1216-1228): vals[:, k] = vals[:, k] * mm[k] + bb[k] over every
        entry, one product then one add.  Enqueued on torch's current stream; the grouping of the merge calls stays valid."""
        mm, bb = np.ascontiguousarray(mm, np.float64).reshape(-1), np.ascontiguousarray(bb, np.float64).reshape(-1)
        if len(mm) != self.nvar or len(bb) != self.nvar:
            raise ValueError("affine: %d mm and %d bb for nvar=%d" % (len(mm), len(bb), self.nvar))
        check(lib().ibh_multivec_affine_device(self._h, ptr(mm), ptr(bb), stream_arg()))

    def to_dense_scale(self, nE, out=None):
        """1 / (sum of weights per cell) over [0, nE), +inf where no entry falls (multivec.cpp:35-50).  Returns a CUDA tensor
        (or fills `out`)."""
        import torch
        if out is None:
            out = torch.empty(int(nE), dtype=torch.float64, device="cuda")
        assert is_cuda(out) and out.dtype == torch.float64 and out.shape == (int(nE),) and out.is_contiguous()
        check(lib().ibh_multivec_to_dense_scale(self._h, int(nE), dptr(out), stream_arg(out)))
        return out

    def to_dense(self, scale, fill):
        """All variables of to_dense (multivec.cpp:55-81) at once: [nvar, nE] with nE = len(scale); same kind of array as `scale`."""
        import torch
        ds, host = _to_device(scale, 1)
        nE = ds.shape[0]
        out = torch.empty((self.nvar, nE), dtype=torch.float64, device=ds.device)
        check(lib().ibh_multivec_to_dense(self._h, dptr(ds), float(fill), dptr(out), nE, nE, stream_arg(ds)))
        return _back(out, host)

    def update_dense(self, scale, out):
        """The in-place merge into the GCM's arrays (GCMCoupler_ModelE.cpp:864-892): out[nvar, nE]; cells no entry names keep
        their contents.  A CUDA tensor is updated in place; a numpy array is updated through a device copy.  Returns out."""
        ds, _ = _to_device(scale, 1)
        do, host = _to_device(out, 2)
        nE = ds.shape[0]
        assert do.shape == (self.nvar, nE)
        check(lib().ibh_multivec_update_dense(self._h, dptr(ds), dptr(do), plane_stride(do, nE, "out"), nE, stream_arg(do)))
        if host:
            out[...] = _back(do, True)
        return out

    def densify(self, sparse_set, out=None):
        """gcm_ovalsE of IceCoupler.cpp:306-314: a CUDA tensor [nvar, dense_extent], zero plus the values of every entry added at
        to_dense(index) in entry order.  An index the set lacks raises."""
        import torch
        nd = sparse_set.dense_extent()
        if out is None:
            out = torch.empty((self.nvar, nd), dtype=torch.float64, device="cuda")
        assert is_cuda(out) and out.dtype == torch.float64 and out.shape == (self.nvar, nd) and out.stride(1) == 1
        check(lib().ibh_multivec_densify_device(self._h, sparse_set._h, dptr(out), plane_stride(out, nd, "out"), stream_arg(out)))
        return out


def append_planes_many(packs, mask, mask0=None):
    """VectorMultivec.append_planes for several vectors from ONE pass over the masks (ibh_multivec_append_planes_many_*): packs
    is a list of dict(vec, planes, nclass=1, plane_class_stride=None, index_strides=None, types=None) -> the number of kept
    cells.  The masks and every plane are numpy arrays, or all are torch CUDA tensors."""
    arrays = [mask] + ([] if mask0 is None else [mask0]) + [p for k in packs for p in k["planes"]]
    dev = [is_cuda(a) for a in arrays]
    if any(dev) and not all(dev):
        raise ValueError("append_planes: host and device arrays are mixed")
    on_device = dev[0]
    if on_device:
        import torch

    def flat(a, int16_only=False):
        if on_device:
            if a.dtype not in ((torch.int16,) if int16_only else (torch.int16, torch.float64)) or not a.is_contiguous():
                raise ValueError("append_planes: a device array must be a contiguous %s CUDA tensor" % ("int16" if int16_only else "float64 or int16"))
            return a.reshape(-1)
        a = np.asarray(a)
        return np.ascontiguousarray(a, np.int16 if int16_only or a.dtype == np.int16 else np.float64).reshape(-1)

    def address(a):
        return None if a is None else a.data_ptr() if on_device else a.ctypes.data

    def size(a):
        return a.numel() if on_device else a.size

    m = flat(mask, True)
    m0 = None if mask0 is None else flat(mask0, True)
    ncell = size(m)
    if m0 is not None and size(m0) != ncell:
        raise ValueError("append_planes: mask0 has %d cells, mask %d" % (size(m0), ncell))
    keep, structs = [m, m0], (_capi.PlanePack * len(packs))()
    for s, k in zip(structs, packs):
        vec, nclass = k["vec"], int(k.get("nclass", 1))
        stride = k.get("plane_class_stride")
        stride = ncell if stride is None else int(stride)
        strides = k.get("index_strides") or (1, ncell)
        planes = [flat(p) for p in k["planes"]]
        by_dtype = [int(p.dtype == (torch.int16 if on_device else np.int16)) for p in planes]
        types = np.ascontiguousarray(by_dtype if k.get("types") is None else k["types"], np.int32).reshape(-1)
        if len(types) != len(planes) or any(t in (0, 1) and t != d for t, d in zip(types, by_dtype)):
            raise ValueError("append_planes: types %s for planes of types %s" % (types.tolist(), by_dtype))
        need = (max(nclass, 1) - 1) * stride + ncell
        for p in planes:
            if nclass > 0 and size(p) < need:
                raise ValueError("append_planes: a plane has %d elements, %d classes of stride %d over %d cells need %d"
                                 % (size(p), nclass, stride, ncell, need))
        table = (C.c_void_p * max(len(planes), 1))(*[address(p) for p in planes])
        keep += [planes, types, table]
        s.mv, s.planes, s.plane_type = vec._h.value, C.cast(table, C.c_void_p).value, types.ctypes.data
        s.nvar, s.nclass, s.plane_class_stride = len(planes), nclass, stride
        s.index_stride_cell, s.index_stride_class = int(strides[0]), int(strides[1])
    nkept = C.c_int64()
    args = (C.cast(structs, C.c_void_p), len(packs), ncell, address(m), address(m0), C.byref(nkept))
    if on_device:
        check(lib().ibh_multivec_append_planes_many_device(*args, stream_arg(m)))
    else:
        check(lib().ibh_multivec_append_planes_many_host(*args))
    return nkept.value


def concatenate(vecs):
    """icebin::concatenate (multivec.cpp:15-33)."""
    vecs = list(vecs)
    arr = (C.c_void_p * max(len(vecs), 1))(*[v._h.value for v in vecs])
    h = C.c_void_p()
    check(lib().ibh_multivec_concatenate(len(vecs), arr, C.byref(h)))
    return VectorMultivec(0, _handle=h)

