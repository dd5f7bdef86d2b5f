"""global_ec's host-side pieces (no GPU): the hcdefs loop, make_grid_spec's boundaries and make_abbr_grid's area with the
reference's degree quirk, against independent restatements."""
import math

import numpy as np
import pytest

from icebin_amd import HntrSpec, global_ec


def test_hcdefs_accumulates_like_the_reference():
    got = global_ec.hcdefs(-100., 100., 0.1)
    ref, e = [], -100.
    while e <= 100.:
        ref.append(e)
        e = e + 0.1
    assert got.tolist() == ref
    assert got[-1] != 100.0 or len(got) == 2001          # the accumulated sum, not lo + k*skip
    assert global_ec.hcdefs(0., 3000., 500.).tolist() == [0., 500., 1000., 1500., 2000., 2500., 3000.]
    assert global_ec.hcdefs(1., 0., 1.).tolist() == []


@pytest.mark.parametrize("im,jm,offi,dlat", [(72, 46, 0., 240.), (144, 90, 0.5, 120.), (360, 180, 0., 60.), (4, 2, 0.25, 5400.)])
def test_grid_spec_boundaries(im, jm, offi, dlat):
    lonb, latb = global_ec.make_grid_spec(HntrSpec(im, jm, offi, dlat))
    assert len(lonb) == im + 1 and len(latb) == 2 * (jm // 2) + 1
    for i in range(im):
        assert lonb[i] == -180. + (offi + i) * (360. / im)
    assert lonb[im] == lonb[0] + 360.
    top = (jm // 2) * (dlat / 60.)
    top = 90. if abs(top - 90.) < 1e-10 else top
    assert latb[0] == -top and latb[-1] == top and latb[jm // 2] == 0.
    assert np.all(np.diff(latb) > 0)


def test_native_area_degree_quirk():
    spec = HntrSpec(72, 46, 0., 240.)
    cells = np.arange(spec.size)
    got = global_ec.native_area(spec, cells, 6371000.)
    lonb, latb = global_ec.make_grid_spec(spec)
    for s in (0, 71, 72 * 23 + 5, spec.size - 1):
        i, j = s % 72, s // 72
        ref = (math.sin(latb[j + 1]) - math.sin(latb[j])) * (lonb[i + 1] - lonb[i]) * (math.pi / 180.0 * 6371000. * 6371000.)
        assert got[s] == ref
    assert (got < 0).any() and (got > 0).any()          # degrees into sin: some areas come out negative


def test_check_negative_messages(capsys):
    class W:
        wM = np.array([1., -1.])
        Mw = np.array([2.])

        def coo_dense(self):
            return np.array([0]), np.array([0]), np.array([-3.])
    with pytest.raises(RuntimeError, match="Negative values found in matrix or weights for X"):
        global_ec.check_negative(W(), "X")
    out = capsys.readouterr().out
    assert "wt[0](1) = -1" in out and "X(0,0)=-3" in out
