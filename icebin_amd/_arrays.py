"""How an array argument becomes a pointer, a stream and a stride for the C-ABI: the one place that tells host arrays (numpy)
from device arrays (torch CUDA tensors).  torch is imported where it is needed, so the package imports without it."""
import ctypes as C

import numpy as np

from ._capi import IBH_EINVAL, IcebinHipError


def einval(msg):
    return IcebinHipError(IBH_EINVAL, msg)


def is_cuda(x):
    """True only for a tensor in HBM: a numpy array, a list, None and a CPU torch tensor are host arrays."""
    return bool(getattr(x, "is_cuda", False))


_current_stream = None        # torch.cuda.current_stream, looked up once: stream_arg runs in front of every apply


def stream_arg(t=None, stream=None):
    """The caller's raw stream handle, else torch's current stream on t's device (t None: on the current device)."""
    if stream is None:
        global _current_stream
        if _current_stream is None:
            import torch
            _current_stream = torch.cuda.current_stream
        stream = _current_stream(None if t is None else t.device).cuda_stream
    return C.c_void_p(stream)


def dptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def to_device(a, device=None):
    """A numpy array as a tensor on `device` (default: the current one).  torch takes no read-only array: that one is copied."""
    import torch
    t = torch.from_numpy(a if a.flags.writeable else a.copy())
    return t.cuda() if device is None else t.to(device)


def padded_planes(nvar, n, device, zero=False):
    """[nvar, n] float64 view whose rows (field planes) start on 512-byte boundaries: whole-line
    wave stores measure 6.0 instead of 4.0 TB/s on MI355X (shortrow)."""
    import torch
    return (torch.zeros if zero else torch.empty)((nvar, (n + 63) // 64 * 64), dtype=torch.float64, device=device)[:, :n]


def leading_dim(nplanes, stride, n, what):
    """The leading dimension of nplanes planes of n cells that lie `stride` apart.  No address is computed from a single plane's
    stride (nor from that of no plane at all), so any value is taken; one that holds the plane is passed on, since the apply picks
    its whole-line stores by the alignment of the leading dimension.  Otherwise the stride must hold a whole plane: a smaller one
    (a broadcast `x.expand(nvar, -1)`, an overlapping as_strided view) would make a kernel read or write past the tensor, so it is
    refused before anything is launched."""
    if nplanes <= 1:
        return max(stride, n)
    if stride < n:
        raise ValueError("%s planes overlap: stride %d < %d cells" % (what, stride, n))
    return stride


def plane_stride(t, n, what):
    """leading_dim of a [nvar, n] tensor."""
    return leading_dim(t.shape[0], t.stride(0), n, what)


def named_planes(named, what, mix_detail=True, dtype_is="the plane is %s", cells_of="its grid has %d", null="each"):
    """The planes of one call, named = [(name, array, dtype name, cells), ...], as flat contiguous arrays that are all numpy or
    all torch CUDA tensors: (arrays, on_device).  Needs no device.  `what` is the refusal of a mix of the two, followed with
    mix_detail by who is where; dtype_is and cells_of end the refusals of a dtype and of a cell count.  null: "first" refuses a
    None plane before anything else, "each" when its turn comes, None leaves it to the dtype check."""
    if null == "first":
        for name, p, _, _ in named:
            if p is None:
                raise einval("%s: null plane" % name)
    dev = [is_cuda(p) for _, p, _, _ in named]
    if any(dev) != all(dev):
        where = " (%s)" % ", ".join("%s: %s" % (n[0], "device" if d else "host") for n, d in zip(named, dev))
        raise einval(what + (where if mix_detail else ""))
    out = []
    for name, p, dtype, cells in named:
        if p is None and null == "each":
            raise einval("%s: null plane" % name)
        if dev[0]:
            ok = str(p.dtype) == "torch." + dtype
        else:
            p = np.asarray(p)
            ok = p.dtype == np.dtype(dtype)
        if not ok:
            raise einval("%s: dtype %s, %s" % (name, p.dtype, dtype_is % dtype))
        p = p.reshape(-1).contiguous() if dev[0] else np.ascontiguousarray(p.reshape(-1))
        n = p.numel() if dev[0] else p.size
        if n != cells:
            raise einval("%s: the plane holds %d cells, %s" % (name, n, cells_of % cells))
        out.append(p)
    return out, dev[0]
