"""CPU checks of make_topoO: the restatement (tests/make_topoo_restatement.py) against answers walked by hand through
modele/topo_base.cpp:20-221 and :578-711, and every refusal of the library that needs no device."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from icebin_amd import HntrSpec, _capi
from icebin_amd import topoo

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_topoo_restatement as mr  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def test_std_round_is_half_away_from_zero():
    for x, want in ((.5, 1.), (1.5, 2.), (2.5, 3.), (-.5, -1.), (0.49999999999999994, 0.), (-2.5, -3.), (3.49, 3.), (-0.2, -0.)):
        got = mr.std_round(x)
        assert got == want and np.signbit(got) == np.signbit(want), (x, got)
    # numpy's and Python's own rounding go to the even neighbour at 0.5 and 2.5, and floor(x + .5) is wrong just below .5
    assert np.round(.5) == 0. and round(2.5) == 2 and np.floor(0.49999999999999994 + .5) == 1.


def land(rows):
    return [[0] * len(r) for r in rows]


def test_sort_ties_keep_traversal_order_across_rows_of_different_area():
    """Depth first; at equal depth the earlier row (areas differ, so the order shows in the walk); at equal depth in one row the
    earlier column (equal areas: either order gives the same sums).  Rows of area 1 and 2, depths 10 5 / 5 10: sorted (1, 5) (2, 5)
    (1, 10) (2, 10).  FLAKE = .25: SAREA = 6, the lake ends where ANSUM = 1, 3 first exceeds 1.5: NLAKE = 1, VNSUM = 15,
    ZLBOT = (15 - 1.5 * 5) / 1.5 = 5, dZLAKE = max(0, 1) = 1; AZATMO = 3 * 5 + 10 + 20 = 45; ANSUM = 3 - 2 = 1, then 3, 4 > 3:
    NGRND = 2.  With the tie the other way round the lake would end at NLAKE = 0."""
    zt = [[10, 5], [5, 10]]
    o = mr.callZ_cell(land(zt), land(zt), zt, [1., 2.], False, .25, .25)
    assert o["_walk"] == (1, 2, 4)
    assert (o["ZSGLO"], o["ZLAKE"], o["dZLAKE"], o["ZATMO"], o["ZGRND"], o["ZSGHI"]) == (5., 5., 1., 7.5, 10., 10.)
    assert o["ZSOLDG"] == o["ZATMOF"] == (10 + 5 + 10 + 20) / 6. and o["ZICETOP"] == 0.
    # the same depths in one row: the column order cannot show
    o = mr.callZ_cell(land([[5, 5, 7]]), land([[5, 5, 7]]), [[5, 5, 7]], [1.], False, .5, 0.)
    assert o["_walk"] == (1, 1, 3) and o["ZLAKE"] == 5.


def test_lake_walk_clamp_not_taken_and_ground_walk_to_the_end():
    """One row of area 1, depths 0 10 20 30, FLAKE = .5: ANSUM = 1, 2, 3 > 2: NLAKE = 2, VNSUM = 30, ZLBOT = (30 - 20) / 2 = 5,
    dZLAKE = 15 (above the clamp); AZATMO = 60 + 30.  FGRND = .5: ANSUM = 2, then 3, 4, never > 4: NGRND runs to the end."""
    zt = [[30, 0, 20, 10]]
    o = mr.callZ_cell(land(zt), land(zt), zt, [1.], False, .5, .5)
    assert o["_walk"] == (2, 3, 4) and o["ZLAKE"] == 20. and o["dZLAKE"] == 15. and o["ZATMO"] == 22.5 and o["ZGRND"] == 30.


def test_lake_walk_ends_and_flake_zero():
    zt = [[30, 0, 20, 10]]
    # FLAKE = 1: ANSUM never exceeds SAREA * FLAKE, the walk ends by --NLAKE (:165-168) on the last cell
    o = mr.callZ_cell(land(zt), land(zt), zt, [1.], False, 1., 0.)
    assert o["_walk"] == (3, 3, 4) and o["ZLAKE"] == 30. and o["dZLAKE"] == 30. - (60. - 0. * 30.) / 4. and o["ZATMO"] == 30.
    # FLAKE = 0: the first cell already exceeds 0; dZLAKE = 0 (:180-181)
    o = mr.callZ_cell(land(zt), land(zt), zt, [1.], False, 0., .5)
    assert o["_walk"] == (0, 2, 4) and o["ZLAKE"] == 0. and o["dZLAKE"] == 0. and o["ZATMO"] == 15. and o["ZGRND"] == 20.
    # a lake of one low cell among equal ones: ZLBOT equals the surface, the clamp gives 1 m
    o = mr.callZ_cell(land([[7, 7]]), land([[7, 7]]), [[7, 7]], [1.], False, .25, 0.)
    assert o["dZLAKE"] == 1.


def test_ocean_cell_and_the_two_fatal_cells():
    zt, fo, fg = [[-50, 20], [-200, 40]], [[1, 0], [1, 0]], [[0, 1], [0, 0]]
    o = mr.callZ_cell(fg, fo, zt, [1., 2.], True, 0., 0.)
    assert o["ZSGLO"] == -200. and o["ZICETOP"] == 20. and o["ZATMOF"] == (20. + 80.) / 6. and o["ZATMO"] == 0. and "ZSOLDG" not in o
    with pytest.raises(ValueError, match="ocean"):
        mr.callZ_cell(fg, land(zt), zt, [1., 2.], True, 0., 0.)
    with pytest.raises(ValueError, match="continental"):
        mr.callZ_cell(fg, [[1, 1], [1, 1]], zt, [1., 2.], False, 0., 0.)


def small(FOCEANF=0., FGICEF=.25, FLAKE=.5, ocean_cells=(), **kw):
    """ocean 12 x 12 over a fine grid of the same size, every regridded plane constant"""
    n = 12
    z = np.zeros((n, n), np.int16)
    full = lambda v: np.full((n, n), float(v))  # noqa: E731
    fo = np.full((n, n), 1 if FOCEANF >= .5 else 0, np.int16)
    fo[0, 0] = 0
    for i, j in ocean_cells:
        fo[j - 1, i - 1] = 1
    return mr.make_topoO(n, n, n, n, z, z, z, fo, full(FOCEANF), full(FGICEF), full(FLAKE), full(0.), full(0.), full(0.), **kw)


def test_bands_wedge_and_the_mean_ice_thickness():
    planes, counts, pow_cells = small()
    zero = {(I, J) for J in range(1, 13) for I in range(1, 13) if planes["FLAKE"][J - 1, I - 1] == 0}
    want = {(I, J) for J in (1, 2, 12) for I in range(1, 13)} | {(I, 11) for I in range(1, 7)} | {(5, 10), (5, 11), (6, 11)}
    assert zero == want and (planes["FLAKE"][2:9] == .5).all()
    assert [mr.wedge_imax(12, 12, J) for J in (10, 11)] == [5, 6] and mr.wedge_imax(288, 180, 150) == 115       # .5 + 216 * 96 / 180 = 115.7
    assert (planes["FGICE"][0] == 1).all() and (planes["FGICE"][1:] == .25).all() and (planes["FOCEAN"] == 0).all()
    assert pow_cells.all()          # zictop == zsolg everywhere: every cell is filled at :708
    d = np.asarray(mr.make_dxyp(12, 12))[:, None]
    mean = (d * planes["FGICE"] * planes["dZGICE"]).sum() / (d * planes["FGICE"]).sum()
    assert abs(mean - 264.7) < 1e-10                                # what CONSTK is chosen for (:666-670)
    assert counts == dict.fromkeys(mr.COUNTS, 0)
    ld = small(real=np.longdouble, only_dzgice=True)[0]["dZGICE"]
    assert ld.dtype == np.longdouble and np.abs(ld.astype(np.float64) - planes["dZGICE"]).max() < 1e-12


def test_set_to_resets_counts_and_the_block_pass():
    planes, counts, _ = small(FOCEANF=.25, FLAKE=.75, FGICEF=.5, set_to_land=[(3, 4)], set_to_ocean=[(3, 4), (8, 6)], ocean_cells=[(3, 4), (8, 6)],
                              resets=[(-30., [(5, 5), (5, 5)])])
    assert planes["FOCEAN"][3, 2] == 1 and planes["FOCEAN"][5, 7] == 1 and planes["FOCEAN"].sum() == 2    # the later SET_TO wins
    # FLAKE = round(.75 / .75 * 256) / 256 = 1 on land, FGICE = .5 / .75: the sum exceeds 1 on every land cell above J = 2 that
    # has a lake: 120 cells less the 2 ocean cells and the 19 of the bands and the wedge (12 + 6 + 1)
    assert counts["FLAKE_reduced"] == 120 - 2 - 19 and counts["FGICE_high"] == 0
    assert planes["ZLAKE"][4, 4] == -30. and planes["ZATMO"][4, 4] == -30.
    for (i, j) in ((3, 3), (4, 3), (4, 4), (7, 5), (7, 6), (8, 5)):      # the blocks of the two ocean cells lost their lakes
        assert planes["FLAKE"][j - 1, i - 1] == 0 and planes["dZLAKE"][j - 1, i - 1] == 0
    assert planes["FLAKE"][6, 6] > 0
    with pytest.raises(mr.Fatal) as ei:
        small(set_to_ocean=[(5, 5)])
    assert (ei.value.kind, ei.value.I, ei.value.J) == ("ocean", 5, 5)


def test_the_settings_fixture_holds_the_reference_lists():
    d = json.load(open(os.path.join(HERE, "golden", "make_topoo_g1qx1_cells.json")))
    assert (d["im"], d["jm"]) == (288, 180) and len(d["set_to_land"]) == 30 and len(d["set_to_ocean"]) == 46
    assert d["set_to_land"][0] == [84, 18] and d["set_to_ocean"][-1] == [225, 169]
    assert [r["elev"] for r in d["resets"]] == [-30., 53., 75.] and [len(r["cells"]) for r in d["resets"]] == [13, 1, 1]
    for i, j in d["set_to_land"] + d["set_to_ocean"] + [c for r in d["resets"] for c in r["cells"]]:
        assert 1 <= i <= 288 and 1 <= j <= 180


# ---- the refusals that need no device -----------------------------------------------------------------------------------------
def planes(I, S):
    z = np.zeros((I.jm, I.im), np.int16)
    return z, z, z, z, np.zeros((S.jm, S.im))


def call(I, O, S, p=None, **kw):
    p = p or planes(I, S)
    return topoo.make_topoO(I, O, p[0], p[1], p[2], p[3], S, p[4], **kw)


GOOD = (HntrSpec(36, 36, 0., 300.), HntrSpec(12, 12, 0., 900.), HntrSpec(18, 9, 0., 1200.))


@pytest.mark.parametrize("I, O, what", [
    (HntrSpec(38, 36, 0., 300.), GOOD[1], r"\(38x36\).*\(12x12\)"),         # does not nest in i
    (HntrSpec(36, 30, 0., 360.), GOOD[1], r"\(36x30\).*\(12x12\)"),         # nor in j
    (HntrSpec(33, 36, 0., 300.), HntrSpec(11, 12, 0., 900.), r"\(11x12\).*even"),
    (HntrSpec(36, 33, 0., 300.), HntrSpec(12, 11, 0., 900.), r"\(12x11\).*even"),
    (HntrSpec(65536, 32768, 0., .33), HntrSpec(2, 2, 0., 5400.), "overflow int32"),
])
def test_grids_are_refused_before_a_device_is_looked_for(I, O, what):
    with pytest.raises(_capi.IcebinHipError, match=what) as ei:
        z = np.zeros(1, np.int16)
        fake = np.lib.stride_tricks.as_strided(z, (I.jm, I.im), (0, 0))     # the shape alone is looked at before the grids are
        topoo.make_topoO(I, O, fake, fake, fake, fake, GOOD[2], np.zeros((9, 18)))
    assert ei.value.code == _capi.IBH_EINVAL


@pytest.mark.parametrize("kw, what", [
    (dict(set_to_land=[(13, 1)]), r"set_to_land: entry 0 is \(13, 1\)"),
    (dict(set_to_ocean=[(1, 1), (0, 5)]), r"set_to_ocean: entry 1 is \(0, 5\)"),
    (dict(resets=[(-30., [(1, 1)]), (53., [(2, 13)])]), r"resets: entry 1 is \(2, 13\)"),
    (dict(set_to_land=[(2 ** 31, 1)]), "overflows int32"),
])
def test_cell_lists_are_refused_before_a_device_is_looked_for(kw, what):
    with pytest.raises(_capi.IcebinHipError, match=what) as ei:
        call(*GOOD, **kw)
    assert ei.value.code == _capi.IBH_EINVAL


def test_planes_are_refused_before_a_device_is_looked_for():
    I, O, S = GOOD
    p = planes(I, S)
    for k in range(5):
        bad = list(p)
        bad[k] = None
        with pytest.raises(_capi.IcebinHipError, match="null plane"):
            call(I, O, S, bad)
        bad[k] = p[k].astype(np.float32)
        with pytest.raises(_capi.IcebinHipError, match="dtype float32"):
            call(I, O, S, bad)
        bad[k] = p[k][1:]
        with pytest.raises(_capi.IcebinHipError, match="cells, its grid has"):
            call(I, O, S, bad)

    class OnDevice:                 # stands for a torch CUDA tensor: the mix is refused before anything is touched
        is_cuda = True
    with pytest.raises(_capi.IcebinHipError, match="some planes are on the host and some on the device"):
        call(I, O, S, (p[0], OnDevice(), p[2], p[3], p[4]))


def test_c_entries_refuse_null_and_bad_sizes():
    L = _capi.lib()
    h = C.c_void_p()

    def create(imI=36, jmI=36, imO=12, jmO=12, imS=18, jmS=9, out=C.byref(h), nland=0, land=None):
        return L.ibh_make_topoo_create(out, imI, jmI, 0., 300., imO, jmO, 0., 900., imS, jmS, 0., 1200., nland, land, 0, None, 0, None, None)
    for kw in (dict(out=None), dict(imI=0), dict(jmO=0), dict(imS=-1), dict(imO=10), dict(jmO=24), dict(nland=-1), dict(nland=2)):
        assert create(**kw) == _capi.IBH_EINVAL, kw
        assert h.value is None
    assert create(imO=10) == _capi.IBH_EINVAL and b"(36x36)" in L.ibh_last_error() and b"(10x12)" in L.ibh_last_error()
    assert L.ibh_make_topoo_device(None, *[None] * 6, 0, None) == _capi.IBH_EINVAL and b"null handle" in L.ibh_last_error()
    assert L.ibh_make_topoo_host(None, *[None] * 6, 0, None) == _capi.IBH_EINVAL
    assert L.ibh_make_topoo_status(None, None, None) == _capi.IBH_EINVAL
    assert L.ibh_selftest_pow03(None, 4, None, None) == _capi.IBH_EINVAL
    assert L.ibh_make_topoo_destroy(None) == _capi.IBH_OK


def test_fatal_messages_are_the_references():
    I, O = HntrSpec(21600, 10800, 0., 1.), HntrSpec(288, 180, 0., 60.)
    assert topoo.fatal_message("ocean", I, O, 90, 100) == \
        "Ocean cell FOCEAN(100,90)=1 has no ocean area on 2-minute grid; I11,I1M,J11,J1M = 7426,7500,5341,5400"
    assert topoo.fatal_message("continental", I, O, 1, 1) == "Continental cell (1,1) has no continental area on 2-minute grid. (1-21600, 1-60)"
    assert topoo.PLANES == mr.PLANES and topoo.COUNTS == mr.COUNTS and len(topoo.PLANES) == 20
