"""The Python layer's shared plumbing, without a device: _arrays.named_planes through its three callers (the refusals are the
texts those callers raised before they shared one intake, recorded from that code and written out here), is_cuda, modele._planes
on CPU torch tensors, the one leading-dimension rule plane_stride, and _capi.Handle's lifetime."""
import ctypes as C
import gc

import numpy as np
import pytest

from icebin_amd import _arrays, _capi, etopo1, global_ec, modele, topoo
from icebin_amd.hntr import HntrSpec, device_strides

I, O = HntrSpec(4, 2, 0., 5400.), HntrSpec(2, 2, 0., 5400.)       # 8 fine cells in 4 coarse ones


class OnDevice:
    """What the intake looks at in a torch CUDA tensor, without a device."""
    is_cuda = True

    def __init__(self, dtype, n):
        self.dtype, self.n = "torch." + dtype, n

    def reshape(self, *shape):
        return self

    def contiguous(self):
        return self

    def numel(self):
        return self.n


def host(dtype, n):
    a = np.zeros(n, dtype)
    a.flags.writeable = False           # every host plane of these tests is read-only: the intake only reads
    return a


CALLERS = {
    "etopo1": (lambda *p: etopo1.etopo1_ice(I, O, *p), ("int16", "int16", "int16", "float64"), (8, 8, 8, 4)),
    "topoo": (lambda *p: topoo.make_topoO(I, O, *p[:4], O, p[4]), ("int16", "int16", "int16", "int16", "float64"), (8, 8, 8, 8, 4)),
    "scan": (lambda *p: global_ec.IceScan(O, I, *p), ("int16", "int16"), (8, 8)),
}
MIX = "some planes are on the host and some on the device"
# (caller, what is wrong with the second plane) -> the refusal
REFUSALS = {
    ("etopo1", "null"): "zictop: null plane",
    ("etopo1", "mix"): "focean / zictop / zsolid / fgiceC: " + MIX + " (focean: host, zictop: device, zsolid: host, fgiceC: host)",
    ("etopo1", "dtype host"): "zictop: dtype float32, the plane is int16",
    ("etopo1", "dtype device"): "zictop: dtype torch.float32, the plane is int16",
    ("etopo1", "short host"): "zictop: the plane holds 7 cells, its grid has 8",
    ("etopo1", "short device"): "zictop: the plane holds 7 cells, its grid has 8",
    ("topoo", "null"): "ZICETOP1m: null plane",
    ("topoo", "mix"): "FGICE1m / ZICETOP1m / ZSOLG1m / FOCEAN1m / FLAKES: " + MIX
                      + " (FGICE1m: host, ZICETOP1m: device, ZSOLG1m: host, FOCEAN1m: host, FLAKES: host)",
    ("topoo", "dtype host"): "ZICETOP1m: dtype float32, the plane is int16",
    ("topoo", "dtype device"): "ZICETOP1m: dtype torch.float32, the plane is int16",
    ("topoo", "short host"): "ZICETOP1m: the plane holds 7 cells, its grid has 8",
    ("topoo", "short device"): "ZICETOP1m: the plane holds 7 cells, its grid has 8",
    ("scan", "null"): "elevI: dtype object, the ice planes are int16",
    ("scan", "mix"): "fgiceI / elevI: one plane is on the host and one on the device",
    ("scan", "dtype host"): "elevI: dtype float32, the ice planes are int16",
    ("scan", "dtype device"): "elevI: dtype torch.float32, the ice planes are int16",
    ("scan", "short host"): "elevI: the plane holds 7 cells, hspecI has 8",
    ("scan", "short device"): "elevI: the plane holds 7 cells, hspecI has 8",
}


@pytest.mark.parametrize("caller,wrong", list(REFUSALS), ids=lambda v: v.replace(" ", "_"))
def test_named_planes_refusals_keep_their_text(caller, wrong):
    call, dtypes, cells = CALLERS[caller]
    make = OnDevice if wrong.endswith("device") else host
    planes = [make(d, n) for d, n in zip(dtypes, cells)]
    planes[1] = {"null": None, "mix": OnDevice("int16", 8), "dtype host": host("float32", 8), "dtype device": OnDevice("float32", 8),
                 "short host": host("int16", 7), "short device": OnDevice("int16", 7)}[wrong]
    with pytest.raises(_capi.IcebinHipError) as ei:
        call(*planes)
    assert str(ei.value) == REFUSALS[caller, wrong] and ei.value.code == _capi.IBH_EINVAL


def test_the_order_of_the_checks_is_each_caller_s_own():
    et, tp = CALLERS["etopo1"][0], CALLERS["topoo"][0]
    # a null plane and a mix: topoo names the null plane first, etopo1 the mix
    with pytest.raises(_capi.IcebinHipError) as ei:
        tp(OnDevice("int16", 8), host("int16", 8), host("int16", 8), host("int16", 8), None)
    assert str(ei.value) == "FLAKES: null plane"
    with pytest.raises(_capi.IcebinHipError) as ei:
        et(OnDevice("int16", 8), host("int16", 8), host("int16", 8), None)
    assert str(ei.value) == "focean / zictop / zsolid / fgiceC: " + MIX + " (focean: device, zictop: host, zsolid: host, fgiceC: host)"
    # a null plane after a plane of the wrong dtype: etopo1 takes the planes in turn
    with pytest.raises(_capi.IcebinHipError) as ei:
        et(host("float32", 8), host("int16", 8), host("int16", 8), None)
    assert str(ei.value) == "focean: dtype float32, the plane is int16"
    with pytest.raises(_capi.IcebinHipError) as ei:
        tp(host("float32", 8), host("int16", 8), host("int16", 8), host("int16", 8), None)
    assert str(ei.value) == "FLAKES: null plane"


def test_named_planes_takes_read_only_and_shaped_planes_as_they_are():
    a, b = host("int16", 8).reshape(2, 4), host("float64", 4)
    (fa, fb), on_device = _arrays.named_planes((("a", a, "int16", 8), ("b", b, "float64", 4)), "a / b: mixed")
    assert on_device is False and fa.shape == (8,) and fb.shape == (4,)
    assert np.shares_memory(fa, a) and np.shares_memory(fb, b) and not fa.flags.writeable
    d = [OnDevice("int16", 8), OnDevice("float64", 4)]
    out, on_device = _arrays.named_planes((("a", d[0], "int16", 8), ("b", d[1], "float64", 4)), "a / b: mixed")
    assert on_device is True and out[0] is d[0] and out[1] is d[1]


def test_is_cuda_is_true_only_for_a_tensor_on_a_device():
    import torch
    for x in (np.zeros(3), [1., 2.], None, torch.zeros(3), 1.5):
        assert _arrays.is_cuda(x) is False
    assert _arrays.is_cuda(OnDevice("float64", 3)) is True
    assert _arrays.dptr(None) is None and _arrays.stream_arg(None, 5).value == 5


def test_modele_planes_take_cpu_torch_tensors_as_host_arrays():
    import torch
    t = [torch.arange(6, dtype=torch.float64), torch.ones(6, dtype=torch.float64)]
    planes, on_device = modele._planes(t + [None], 6, "merge_topoO")
    assert on_device is False and planes[2] is None
    for p, x in zip(planes, t):
        assert isinstance(p, np.ndarray) and p.dtype == np.float64 and np.shares_memory(p, x.numpy())
    planes[0][2] = -5.
    assert float(t[0][2]) == -5.
    assert np.array_equal(modele._host(t[1]), np.ones(6))
    with pytest.raises(ValueError, match="merge_topoO: host and device planes are mixed"):
        modele._planes([t[0], OnDevice("float64", 6)], 6, "merge_topoO")
    with pytest.raises(ValueError, match="make_topoA: a plane has 6 cells, the grid 7"):
        modele._planes(t, 7, "make_topoA")


def test_plane_stride_is_the_one_leading_dimension_rule():
    import torch
    n = 11
    buf = torch.zeros(3, n + 5, dtype=torch.float64)
    assert _arrays.plane_stride(torch.zeros(1, n), n, "A") == n
    assert _arrays.plane_stride(torch.zeros(n).expand(1, -1), n, "A") == n         # one plane: no stride is refused,
    assert _arrays.plane_stride(torch.as_strided(torch.zeros(n), (1, n), (4, 1)), n, "A") == n
    assert _arrays.plane_stride(buf[:1, :n], n, "A") == n + 5                      # and one that holds the plane is passed on
    assert _arrays.plane_stride(torch.zeros(3, n), n, "A") == n
    assert _arrays.plane_stride(buf[:, :n], n, "A") == n + 5
    with pytest.raises(ValueError, match="^A planes overlap: stride 0 < 11 cells$"):
        _arrays.plane_stride(torch.zeros(n).expand(3, -1), n, "A")
    with pytest.raises(ValueError, match="^out planes overlap: stride 4 < 11 cells$"):
        _arrays.plane_stride(torch.as_strided(torch.zeros(3 * n), (3, n), (4, 1)), n, "out")
    # hntr.device_strides is the same rule over three tensors' strides
    assert device_strides(3, n, 7, 3, 0, n + 5, 7) == (0, n + 5, 7) and device_strides(1, n, 7, 1, 0, 0, 0) == (0, n, 7)
    assert device_strides(3, n, 7, 3, n + 2, n, 8) == (n + 2, n, 8)
    for strides, what in (((0, 0, 7), "A"), ((0, n, 6), "out"), ((4, n, 7), "WTA")):
        with pytest.raises(ValueError, match="^%s planes overlap: stride" % what):
            device_strides(3, n, 7, 3, *strides)


class FakeLib:
    def __init__(self):
        self.destroyed = []

    def ibh_sparse_set_destroy(self, h):
        self.destroyed.append(h.value)
        return 0


class H(_capi.Handle):
    _destroy = "ibh_sparse_set_destroy"

    def __init__(self, value=None, fail=False):
        if fail:
            raise RuntimeError("before the handle is set")
        if value is not None:
            self._h = C.c_void_p(value)


@pytest.fixture
def fake_lib(monkeypatch):
    L = FakeLib()
    monkeypatch.setattr(_capi, "_lib", L)
    return L


def test_handle_is_destroyed_exactly_once(fake_lib):
    h = H(41)
    del h
    gc.collect()
    assert fake_lib.destroyed == [41]
    h = H(42)
    h.close()
    assert fake_lib.destroyed == [41, 42] and h._h is None
    h.close()
    del h
    gc.collect()
    assert fake_lib.destroyed == [41, 42]


def test_handle_without_a_handle_destroys_nothing(fake_lib):
    h = H()
    assert h._h is None
    h.close()
    del h
    with pytest.raises(RuntimeError):
        H(fail=True)                    # the half-constructed object goes without a word
    h = H(0)                            # a null handle
    del h
    gc.collect()
    assert fake_lib.destroyed == []


def test_handle_goes_quietly_when_the_library_is_gone(monkeypatch):
    monkeypatch.setattr(_capi, "_lib", None)        # what interpreter shutdown leaves
    h = H(43)
    h.close()
    assert h._h is None
    h = H(44)
    h.__del__()
    assert h._h is None
