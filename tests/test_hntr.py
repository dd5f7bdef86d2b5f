"""Hntr (icebin::modele::Hntr, slib/icebin/modele/hntr.{hpp,cpp}) without a GPU: the host-side partition is bitwise an
independent restatement of the reference's constructor, bad specs are refused, the Cython module has the reference's
Hntr surface, and creating a regridder without a GPU fails loudly."""
import math
import os
import sys

import numpy as np
import pytest

from icebin_amd import _capi
from icebin_amd.build import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def partition_restated(Bspec, Aspec):
    """hntr.cpp:84-168 in plain Python, libm sin through math.sin (np.sin's SIMD path may differ by an ulp)."""
    imA, jmA, offiA, dlatA = Aspec
    imB, jmB, offiB, dlatB = Bspec
    IMIN, IMAX, FMIN, FMAX = [0] * imB, [0] * imB, [0.] * imB, [0.] * imB
    DIA = float(imB)
    IA = 1
    RIA = (IA + offiA - imA) * imB
    IB = imB
    for IBp1 in range(1, imB + 1):
        RIB = (IBp1 - 1 + offiB) * imA
        while RIA < RIB:
            IA += 1
            RIA += DIA
        if RIA == RIB:
            IMAX[IB - 1], FMAX[IB - 1] = IA, 0.
            IA += 1
            RIA += DIA
            IMIN[IBp1 - 1], FMIN[IBp1 - 1] = IA, 0.
        else:
            IMAX[IB - 1], FMAX[IB - 1] = IA, (RIA - RIB) / DIA
            IMIN[IBp1 - 1], FMIN[IBp1 - 1] = IA, 1 - FMAX[IB - 1]
        IB = IBp1
    IMAX[imB - 1] += imA

    MIN_TO_RAD = (2. * math.pi) / (360 * 60)
    SINA = [0.] * (jmA + 1)
    SINB = [0.] * (jmB + 1)
    FJEQA = .5 * (1 + jmA)
    for JA in range(1, jmA):
        SINA[JA] = math.sin(((JA + .5 - FJEQA) * dlatA) * MIN_TO_RAD)
    SINA[0], SINA[jmA] = -1., 1.
    FJEQB = .5 * (1 + jmB)
    for JB in range(1, jmB):
        SINB[JB] = math.sin(((JB + .5 - FJEQB) * dlatB) * MIN_TO_RAD)
    SINB[0], SINB[jmB] = -1., 1.
    JMIN, JMAX, GMIN, GMAX = [0] * jmB, [0] * jmB, [0.] * jmB, [0.] * jmB
    JMIN[0], GMIN[0] = 1, 0.
    JA = 1
    for JB in range(1, jmB):
        while SINA[JA] < SINB[JB]:
            JA += 1
        if SINA[JA] == SINB[JB]:
            JMAX[JB - 1], GMAX[JB - 1] = JA, 0.
            JA += 1
            JMIN[JB], GMIN[JB] = JA, 0.
        else:
            JMAX[JB - 1], GMAX[JB - 1] = JA, SINA[JA] - SINB[JB]
            JMIN[JB], GMIN[JB] = JA, SINB[JB] - SINA[JA - 1]
    JMAX[jmB - 1], GMAX[jmB - 1] = jmA, 0.
    return dict(SINA=SINA, SINB=SINB, IMIN=IMIN, IMAX=IMAX, FMIN=FMIN, FMAX=FMAX, JMIN=JMIN, JMAX=JMAX, GMIN=GMIN, GMAX=GMAX)


# (im, jm, offi, dlat) pairs; each is checked in both directions
GRIDS = {
    "4x2": (4, 2, 0., 5400.), "8x4": (8, 4, 0., 2700.), "16x8": (16, 8, 0., 1350.),      # tests/test_hntr.cpp:174-482
    "144x90": (144, 90, 0., 120.), "288x180": (288, 180, 0., 60.),
    "72x46": (72, 46, 0., 240.), "360x180": (360, 180, 0., 60.),                         # half-height polar cells
    "72x46_east": (72, 46, 0.5, 240.), "144x90_east": (144, 90, 0.25, 120.),            # windows across the date line
    "91x45": (91, 45, 0.3, 240.), "100x50": (100, 50, 0.0, 216.),                        # edges that never coincide
}
PAIRS = [("4x2", "8x4"), ("4x2", "16x8"), ("8x4", "16x8"), ("144x90", "288x180"), ("72x46", "360x180"),
         ("72x46_east", "360x180"), ("144x90_east", "288x180"), ("72x46_east", "144x90_east"), ("91x45", "360x180"),
         ("100x50", "144x90"), ("91x45", "100x50")]


@pytest.fixture(scope="module")
def lib():
    build_library()
    return _capi.lib()


# the 2-minute grid of tests/test_gpu_hntr.py's large cases, whose steps take several column chunks
GRIDS.update({"10800x5400": (10800, 5400, 0., 2.), "720x360": (720, 360, 0., 30.)})
PARTITION_PAIRS = PAIRS + [("720x360", "10800x5400"), ("360x180", "10800x5400")]


@pytest.mark.parametrize("b,a", PARTITION_PAIRS + [(a, b) for b, a in PARTITION_PAIRS], ids=lambda x: x)
def test_partition_is_bitwise_the_restatement(lib, b, a):
    from icebin_amd import HntrSpec
    from icebin_amd.hntr import partition
    got = partition(HntrSpec(*GRIDS[b]), HntrSpec(*GRIDS[a]))
    ref = partition_restated(GRIDS[b], GRIDS[a])
    for k, v in ref.items():
        g = got[k]
        if k.startswith(("I", "J")):
            assert g.dtype == np.int32 and g.tolist() == v, k
        else:
            assert np.array_equal(g.view(np.uint64), np.asarray(v, np.float64).view(np.uint64)), k
    # the pairs include coincident and non-coincident edges
    if (b, a) in (("4x2", "8x4"), ("144x90", "288x180")):
        assert np.all(got["FMIN"] == 0) and np.all(got["GMAX"] == 0)
    if (b, a) == ("91x45", "360x180"):
        assert np.any(got["FMIN"] != 0)
    if (b, a) == ("100x50", "144x90"):
        assert np.any(got["GMIN"] != 0) and np.any(got["GMAX"][:-1] != 0)


def test_partition_wraps_the_date_line(lib):
    from icebin_amd import HntrSpec
    from icebin_amd.hntr import partition
    p = partition(HntrSpec(*GRIDS["72x46_east"]), HntrSpec(*GRIDS["360x180"]))
    assert p["IMIN"][0] > 360 and p["IMAX"][-1] > 720      # the reference's IA = 1 + (IAREV-1) % imA wraps both
    p = partition(HntrSpec(*GRIDS["360x180"]), HntrSpec(*GRIDS["144x90_east"]))
    assert p["IMIN"][0] == 144 and p["IMAX"][0] == 145       # B cell 1 straddles A cells 144 and 1


BAD_SPECS = [((0, 4, 0., 2700.), "im=0"), ((8, 0, 0., 2700.), "jm=0"), ((8, 4, 0., 0.), "dlat=0"), ((8, 4, 0., -60.), "dlat=-60"),
             ((8, 4, float("nan"), 60.), "offi=nan"), ((8, 4, 0., float("inf")), "dlat=inf")]


@pytest.mark.parametrize("spec,msg", BAD_SPECS, ids=[m for _, m in BAD_SPECS])
def test_out_of_range_specs_are_einval(lib, spec, msg):
    from icebin_amd import Hntr, HntrSpec
    from icebin_amd.hntr import partition
    good = HntrSpec(4, 2, 0., 5400.)
    for B, A in ((HntrSpec(*spec), good), (good, HntrSpec(*spec))):
        with pytest.raises(_capi.IcebinHipError, match=msg) as ei:
            partition(B, A)
        assert ei.value.code == _capi.IBH_EINVAL
        with pytest.raises(_capi.IcebinHipError, match=msg) as ei:    # refused before any device is touched
            Hntr(17.17, B, A, 0.)
        assert ei.value.code == _capi.IBH_EINVAL


def test_partitions_leaving_the_grid_are_einval(lib):
    from icebin_amd import HntrSpec
    from icebin_amd.hntr import partition
    # an interior B edge at the north pole: the reference steps JA past jmA and reads SINA(jmA+1)
    with pytest.raises(_capi.IcebinHipError, match="north-south partition") as ei:
        partition(HntrSpec(4, 4, 0., 5400.), HntrSpec(8, 4, 0., 2700.))
    assert ei.value.code == _capi.IBH_EINVAL
    # an offset of many turns: the reference walks IA for as long as it takes
    with pytest.raises(_capi.IcebinHipError, match="east-west partition") as ei:
        partition(HntrSpec(4, 2, 100., 5400.), HntrSpec(8, 4, 0., 2700.))
    assert ei.value.code == _capi.IBH_EINVAL


def test_device_strides_refuse_overlapping_planes():
    # Hntr.regrid_device's stride rule, checked before any launch: a broadcast (stride-0) weight is the shared weight,
    # a broadcast or overlapping A / out is refused, a single plane's stride is never read
    from icebin_amd.hntr import device_strides
    nA, nB = 64800, 3312
    assert device_strides(3, nA, nB, 1, 0, nA, nB) == (0, nA, nB)
    assert device_strides(3, nA, nB, 3, 0, nA + 8, nB + 16) == (0, nA + 8, nB + 16)
    assert device_strides(3, nA, nB, 3, nA + 4, nA, nB) == (nA + 4, nA, nB)
    assert device_strides(1, nA, nB, 1, 0, 0, 0) == (0, nA, nB)
    with pytest.raises(ValueError, match="A planes overlap"):
        device_strides(3, nA, nB, 1, 0, 0, nB)
    with pytest.raises(ValueError, match="A planes overlap"):
        device_strides(3, nA, nB, 1, 0, nA - 1, nB)
    with pytest.raises(ValueError, match="out planes overlap"):
        device_strides(3, nA, nB, 1, 0, nA, 0)
    with pytest.raises(ValueError, match="WTA planes overlap"):
        device_strides(3, nA, nB, 3, 17, nA, nB)


def test_regrid_rejects_bad_arguments_without_a_handle(lib):
    x = np.zeros(8)
    rc = lib.ibh_hntr_regrid_host(None, x.ctypes.data, 0, x.ctypes.data, 1, 8, x.ctypes.data, 8, 0, 1.0, 0.0)
    assert rc == _capi.IBH_EINVAL and b"null Hntr handle" in lib.ibh_last_error()
    rc = lib.ibh_hntr_partition(8, 4, 0., 2700., 4, 2, 0., 5400., *([None] * 10))
    assert rc == _capi.IBH_EINVAL and b"null output" in lib.ibh_last_error()
    assert lib.ibh_hntr_create(None, 8, 4, 0., 2700., 4, 2, 0., 5400., 0.) == _capi.IBH_EINVAL


@pytest.mark.skipif(_capi.device_count() > 0, reason="checks the no-GPU failure mode")
def test_no_gpu_hntr_fails_loudly(lib):
    from icebin_amd import Hntr, HntrSpec
    with pytest.raises(_capi.IcebinHipError, match="no CPU fallback") as ei:
        Hntr(17.17, HntrSpec(4, 2, 0., 5400.), HntrSpec(8, 4, 0., 2700.), 0.)
    assert ei.value.code == _capi.IBH_ENODEVICE


def test_cython_hntr_surface():
    # _icebin.pyx:180-227: HntrSpec(im, jm, offi, dlat) with im / jm / size / offi / dlat, Hntr(yp17, Bgrid, Agrid, DATMIS)
    # with regrid(WTA, A, mean_polar); the constructors take C float, so offi / dlat / DATMIS are rounded through float32
    from icebin_amd.cython.build_ext import build
    build()
    sys.path.insert(0, os.path.join(ROOT, "icebin_amd", "cython"))
    import icebin
    s = icebin.HntrSpec(144, 90, 0.1, 120.3)
    assert (s.im, s.jm, s.size) == (144, 90, 144 * 90)
    assert s.offi == float(np.float32(0.1)) and s.offi != 0.1
    assert s.dlat == float(np.float32(120.3)) and s.dlat != 120.3
    assert hasattr(icebin.Hntr, "regrid")
    with pytest.raises(TypeError):
        icebin.Hntr(17.17, s, s)                    # DATMIS has no default in the reference either
    if _capi.device_count() == 0:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            icebin.Hntr(17.17, icebin.HntrSpec(4, 2, 0., 5400.), icebin.HntrSpec(8, 4, 0., 2700.), 0.)
    with pytest.raises(RuntimeError, match="dlat"):
        icebin.Hntr(17.17, icebin.HntrSpec(4, 2, 0., 0.), icebin.HntrSpec(8, 4, 0., 2700.), 0.)
