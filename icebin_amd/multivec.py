"""VectorMultivec: the Python face of icebin::VectorMultivec (slib/icebin/multivec.hpp), the parallel sparse vectors the
coupler exchanges with the GCM, resident in HBM (ibh_multivec, include/icebin_hip.h).

Array arguments are torch.float64 CUDA tensors (used in place, on torch's current stream) or numpy arrays (copied to the
device and back), the way linear_Weighted.apply_transformed takes them."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import check, lib, ptr


def _is_cuda(a):
    return hasattr(a, "is_cuda") and a.is_cuda


def _stream(t):
    import torch
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _to_device(a, ndim):
    """(tensor, came from the host): a float64 CUDA tensor with unit inner stride."""
    import torch
    if _is_cuda(a):
        assert a.dtype == torch.float64 and a.dim() == ndim and a.stride(-1) == 1
        return a, False
    h = np.ascontiguousarray(a, np.float64)
    assert h.ndim == ndim
    return torch.from_numpy(h).cuda(), True


def _back(t, host):
    if not host:
        return t
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


class VectorMultivec:
    """VectorMultivec(nvar): index int64[n], weights float64[n], vals float64[n, nvar] (multivec.hpp:25-31)."""

    def __init__(self, nvar, _handle=None):
        h = C.c_void_p()
        if _handle is not None:
            h = _handle
        else:
            check(lib().ibh_multivec_create(int(nvar), C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            _capi.destroy("ibh_multivec_destroy", getattr(self, "_h", None))
        except Exception:      # interpreter shutdown
            pass
        self._h = None

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
        check(lib().ibh_multivec_append_weighted_device(self._h, w._h, C.c_void_p(dB.data_ptr()), dB.shape[0],
                                                       max(dB.stride(0), w.nrow_d), _stream(dB)))

    def append(self, other):
        check(lib().ibh_multivec_append(self._h, other._h))

    def to_dense_scale(self, nE, out=None):
        """1 / (sum of weights per cell) over [0, nE), +inf where no entry falls (multivec.cpp:35-50).  Returns a CUDA tensor
        (or fills `out`)."""
        import torch
        if out is None:
            out = torch.empty(int(nE), dtype=torch.float64, device="cuda")
        assert _is_cuda(out) and out.dtype == torch.float64 and out.shape == (int(nE),) and out.is_contiguous()
        check(lib().ibh_multivec_to_dense_scale(self._h, int(nE), C.c_void_p(out.data_ptr()), _stream(out)))
        return out

    def to_dense(self, scale, fill):
        """All variables of to_dense (multivec.cpp:55-81) at once: [nvar, nE] with nE = len(scale); same kind of array as `scale`."""
        import torch
        ds, host = _to_device(scale, 1)
        nE = ds.shape[0]
        out = torch.empty((self.nvar, nE), dtype=torch.float64, device=ds.device)
        check(lib().ibh_multivec_to_dense(self._h, C.c_void_p(ds.data_ptr()), float(fill), C.c_void_p(out.data_ptr()), nE, nE, _stream(ds)))
        return _back(out, host)

    def update_dense(self, scale, out):
        """The in-place merge into the GCM's arrays (GCMCoupler_ModelE.cpp:864-892): out[nvar, nE]; cells no entry names keep
        their contents.  A CUDA tensor is updated in place; a numpy array is updated through a device copy.  Returns out."""
        ds, _ = _to_device(scale, 1)
        do, host = _to_device(out, 2)
        nE = ds.shape[0]
        assert do.shape == (self.nvar, nE)
        check(lib().ibh_multivec_update_dense(self._h, C.c_void_p(ds.data_ptr()), C.c_void_p(do.data_ptr()), max(do.stride(0), nE), nE,
                                             _stream(do)))
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
        assert _is_cuda(out) and out.dtype == torch.float64 and out.shape == (self.nvar, nd) and out.stride(1) == 1
        check(lib().ibh_multivec_densify_device(self._h, sparse_set._h, C.c_void_p(out.data_ptr()), max(out.stride(0), nd), _stream(out)))
        return out


def concatenate(vecs):
    """icebin::concatenate (multivec.cpp:15-33)."""
    vecs = list(vecs)
    arr = (C.c_void_p * max(len(vecs), 1))(*[v._h.value for v in vecs])
    h = C.c_void_p()
    check(lib().ibh_multivec_concatenate(len(vecs), arr, C.byref(h)))
    return VectorMultivec(0, _handle=h)

