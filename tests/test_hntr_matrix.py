"""Hntr's matrix forms without a GPU: make_dxyp (hntr.cpp:33-52) is bitwise an independent math.sin restatement, bad
arguments are refused with IBH_EINVAL, and building a matrix without a device fails loudly."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from icebin_amd import _capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hntr import GRIDS  # noqa: E402


def dxyp_restated(im, jm):
    """make_dxyp: dLON*(sin(dLAT*(j-jm/2)) - sin(dLAT*(j-jm/2-1))), jm/2 in C integer division; offi and dlat unused."""
    dLON = (2. * math.pi) / im
    dLAT = math.pi / jm
    return np.array([dLON * (math.sin(dLAT * (j - jm // 2)) - math.sin(dLAT * (j - jm // 2 - 1))) for j in range(1, jm + 1)])


@pytest.mark.parametrize("name", sorted(GRIDS) + ["odd_jm_7", "odd_jm_1"])
def test_dxyp_bitwise(name):
    from icebin_amd import HntrSpec
    from icebin_amd.hntr import make_dxyp
    spec = HntrSpec(*GRIDS[name]) if name in GRIDS else HntrSpec(12, int(name.split("_")[-1]), 0., 60.)
    got, ref = make_dxyp(spec), dxyp_restated(spec.im, spec.jm)
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))


def test_odd_jm_is_pinned():
    # jm = 45: jm/2 = 22 (not 22.5), so the rows are NOT symmetric about the equator
    d = dxyp_restated(91, 45)
    assert d[0] != d[-1]
    from icebin_amd import HntrSpec
    from icebin_amd.hntr import make_dxyp
    assert np.array_equal(make_dxyp(HntrSpec(91, 45, 0.3, 240.)), d)


def test_bad_arguments_are_einval():
    L = _capi.lib()
    out = C.c_void_p()
    n = C.c_int64()
    # kind, transforms and the output pointer are checked before the handle
    assert L.ibh_hntr_matrix_d(None, 2, 1., None, None, 0, None, 0, 0, C.byref(out)) == -1
    assert L.ibh_hntr_matrix_d(None, 0, 1., None, None, 3, None, 0, 0, C.byref(out)) == -1
    assert L.ibh_hntr_matrix_d(None, 0, 1., None, None, 0, None, -1, 0, C.byref(out)) == -1
    assert L.ibh_hntr_matrix_d(None, 0, 1., None, None, 0, None, 0, 0, None) == -1
    assert L.ibh_hntr_triplets(None, 5, 1., None, C.byref(n), None, None, None) == -1
    assert L.ibh_hntr_dxyp(0, 4, None) == -1
    assert L.ibh_hntr_dxyp(4, 0, (C.c_double * 1)()) == -1


def test_matrix_without_device_fails_loudly():
    """Without a device no Hntr handle exists (ibh_hntr_create fails with IBH_ENODEVICE), so the matrix entry points are never
    reached here: this pins that the Python path to matrix_d ends in that loud error, not in a CPU fallback.  The builds
    themselves are tested in test_gpu_hntr_matrix.py."""
    if _capi.device_count() > 0:
        pytest.skip("GPU present: the build is covered by tests/test_gpu_hntr_matrix.py")
    from icebin_amd import Hntr, HntrSpec, IcebinHipError
    with pytest.raises(IcebinHipError) as e:
        Hntr(17.17, HntrSpec(*GRIDS["8x4"]), HntrSpec(*GRIDS["16x8"])).matrix_d("overlap")
    assert e.value.code == -2 and "no CPU fallback" in str(e.value)
