"""CPU checks of etopo1_ice: the restatement (tests/etopo1_ice_restatement.py) against answers walked by hand through
modele/etopo1_ice.cpp:166-224, the closed form of :212-224 the library computes against the reference's sequential loop, and every
refusal that needs no device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from icebin_amd import HntrSpec, _capi
from icebin_amd import etopo1

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import etopo1_ice_restatement as er  # noqa: E402


# ---- the walk of :190-207, areas of 1.0 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("remain,taken", [
    (2.5, "abc"),               # two cells and the rounded third
    (2.25, "ab"),               # two cells, the third not rounded up
    (2.0, "ab"),                # exactly two: `area <= remain` holds at equality, then 0 >= .5 fails
    (float("nan"), ""),         # every comparison with NaN is false
    (-1.0, ""),
    (0.5, "a"),                 # the first cell by rounding alone
    (0.4999, ""),
    (5.0, "abcde"),             # enough for all: the loop ends without a break
    (1e9, "abcde"),
])
def test_fill_by_hand(remain, taken):
    keys = list("abcde")
    assert er.fill(keys, [1.0] * 5, remain) == list(taken)


def test_fill_subtracts_in_order():
    # the chain subtracts cell by cell: 2 - 1 = 1, the two cells of 1e-17 each leave 1 as it is (1 - 1e-17 rounds to 1), and the last
    # cell still fits by `<=`.  With a large cell first, 1e16 + 2 - 1e16 = 2 exactly
    # and both small cells fit; with it last, 1e16 + 2 - 1 - 1 = 1e16 and it fits by the equality
    assert er.fill("abcd", [1.0, 1e-17, 1e-17, 1.0], 2.0) == list("abcd")
    assert er.fill("abc", [1e16, 1.0, 1.0], 1e16 + 2) == list("abc")
    assert er.fill("abc", [1.0, 1.0, 1e16], 1e16 + 2) == list("abc")        # 1e16 + 2 - 1 - 1 = 1e16: the equality again


def test_fill_uses_each_cells_own_area():
    assert er.fill("abc", [1.0, 4.0, 1.0], 3.5) == list("ab")       # b: 4 > 2.5, 2.5 >= 2.0 rounds it in, and c is never seen
    assert er.fill("abc", [1.0, 6.0, 1.0], 3.5) == list("a")        # b: 2.5 < 3.0, not rounded; stop


# ---- the order of a tile (:176-184) ----------------------------------------------------------------------------------------------
def test_tile_order_three_tie_levels():
    fo = np.zeros((4, 4), np.int16)
    zt = np.asarray([[5, 5, 9, 5], [7, 5, 5, 9], [0, 0, 0, 0], [0, 0, 0, 0]], np.int16)
    cells = er.tile_cells(fo, zt, 0, 0, 2, 4, False)
    # highest first; equal elevations by row, then by column
    assert [(j, i) for _, j, i in cells] == [(0, 2), (1, 3), (1, 0), (0, 0), (0, 1), (0, 3), (1, 1), (1, 2)]
    assert [c[0] for c in cells] == [-9, -9, -7, -5, -5, -5, -5, -5]


def test_tile_order_lowest_int16_sorts_last():
    fo = np.zeros((1, 4), np.int16)
    zt = np.asarray([[-32768, 32767, -32767, 0]], np.int16)
    cells = er.tile_cells(fo, zt, 0, 0, 1, 4, False)
    assert [i for _, _, i in cells] == [1, 3, 2, 0]
    assert cells[-1][0] == 32768            # negated in int: no int16 holds it


def test_tile_candidates_are_land_only_whatever_the_flag():
    fo = np.asarray([[0, 1, 2, 3]], np.int16)
    zt = np.zeros((1, 4), np.int16)
    for incl in (False, True):              # the Greenland clause of :179 compares a bool with 2
        assert [i for _, _, i in er.tile_cells(fo, zt, 0, 0, 1, 4, incl)] == [0]


# ---- :212-224: the closed form against the sequential loop ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 4), (6, 6), (8, 5), (5, 8), (6, 13), (13, 6), (2, 2), (3, 7), (1, 3)])
@pytest.mark.parametrize("incl", [False, True])
def test_closed_form_of_the_transposed_check(shape, incl):
    rng = np.random.default_rng(shape[0] * 100 + shape[1] + int(incl) * 7)
    for trial in range(40):
        fo = rng.integers(0, 4, shape).astype(np.int16)
        if trial % 3 == 0:
            fo[rng.random(shape) < 0.5] = 2             # dense Greenland: many pairs (j, i), (i, j) in both orders
        fg = rng.integers(0, 2, shape).astype(np.int16)
        fo_seq, fg_seq = fo.copy(), fg.copy()
        er.remove_greenland(fo_seq, fg_seq, incl)
        fg_cf = fg.copy()
        fo_cf = er.remove_greenland_closed_form(fo, fg_cf, incl)
        assert np.array_equal(fo_cf, fo_seq), (shape, incl, trial)
        assert np.array_equal(fg_cf, fg_seq), (shape, incl, trial)


def test_transposed_check_by_hand():
    # 4x4, north half = rows 2, 3.  Greenland at (2, 3), (3, 2) and (3, 3); the check of (j, i) looks at (i, j)
    fo = np.asarray([[0, 0, 0, 0], [0, 0, 0, 1], [1, 0, 0, 2], [0, 1, 2, 2]], np.int16)
    fg = np.ones((4, 4), np.int16)
    f2, g2 = fo.copy(), fg.copy()
    er.remove_greenland(f2, g2, False)
    # (2, 3): becomes 1; reads (3, 2), still 2 -> nothing.  (3, 2): becomes 1; reads (2, 3), already 1 -> fgice(2, 3) = 0.
    # (3, 3): becomes 1; reads itself, 1 -> fgice(3, 3) = 0.
    assert f2.tolist() == [[0, 0, 0, 0], [0, 0, 0, 1], [1, 0, 0, 1], [0, 1, 1, 1]]
    assert np.argwhere(g2 == 0).tolist() == [[2, 3], [3, 3]]
    f3, g3 = fo.copy(), fg.copy()
    er.remove_greenland(f3, g3, True)       # the new value is 0: no Greenland cell reads 1 from a Greenland cell
    assert np.argwhere(g3 == 0).tolist() == []
    fo[2, 3] = 1                            # an ocean cell at the transposed place of (3, 2), in either mode
    for incl in (False, True):
        f4, g4 = fo.copy(), fg.copy()
        er.remove_greenland(f4, g4, incl)
        assert [2, 3] in np.argwhere(g4 == 0).tolist()


# ---- the whole restatement on a grid small enough to check by eye ------------------------------------------------------------
def test_restatement_small_case():
    I, Cg = HntrSpec(4, 4, 0., 2700.), HntrSpec(2, 2, 0., 5400.)
    fo = np.asarray([[0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 2, 1], [0, 0, 0, 2]], np.int16)
    zt = np.asarray([[100, 100, 10, 60], [49, 50, 99, 0], [5, 7, 500, 0], [9, 9, 9, 400]], np.int16)
    zs = np.zeros((4, 4), np.int16)
    fC = np.zeros((2, 2))
    fC[1, 0] = 0.5          # the north-west tile: rows 2-3, columns 0-1, all land
    out = er.etopo1_ice(I, Cg, fo, zt, zs, fC, False)
    # south (rows 0, 1): land with thickness >= 50.  78N band: rows >= 4*14//15 = 3, land.  Tile (1, 0): its two rows differ in
    # area (row 3 is polar-most and smaller); the order is (3, 0), (3, 1), (2, 1), (2, 0); half the tile's area takes row 3
    # and then whatever of row 2 the rest reaches -- checked against the restatement's own walk below
    assert out["FGICE1m"][0].tolist() == [1, 0, 0, 1] and out["FGICE1m"][1].tolist() == [0, 1, 0, 0]
    assert out["FGICE1m"][3].tolist() == [1, 1, 1, 0]
    assert out["ZICETOP1m"][2, 2] == -300 and out["ZSOLG1m"][3, 3] == -300 and out["ZICETOP1m"][2, 3] == 0
    assert out["FOCEAN1m"].tolist() == [[0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 1, 1], [0, 0, 0, 1]]
    dI, dC = er.make_dxyp(I), er.make_dxyp(Cg)
    cells = er.tile_cells(fo, zt, 1, 0, 2, 2, False)
    assert [(j, i) for _, j, i in cells] == [(3, 0), (3, 1), (2, 1), (2, 0)]
    taken = er.fill(cells, [dI[c[1]] for c in cells], 0.5 * dC[1])
    assert [tuple(c[1:]) for c in taken if c[1] == 2] == [(j, i) for j, i in ((2, 1), (2, 0)) if out["FGICE1m"][j, i] == 1]
    with_g = er.etopo1_ice(I, Cg, fo, zt, zs, fC, True)
    assert with_g["FGICE1m"][2, 2] == 1 and with_g["FGICE1m"][3, 3] == 1 and with_g["ZICETOP1m"][2, 2] == 500
    assert with_g["FOCEAN1m"][2, 2] == 0 and with_g["FOCEAN1m"][3, 3] == 0


# ---- refusals that need no device ------------------------------------------------------------------------------------------------
def planes(I, Cg):
    return (np.zeros((I.jm, I.im), np.int16), np.zeros((I.jm, I.im), np.int16), np.zeros((I.jm, I.im), np.int16), np.zeros((Cg.jm, Cg.im)))


@pytest.mark.parametrize("I,Cg,words", [
    (HntrSpec(25, 12, 0., 900.), HntrSpec(8, 4, 0., 2700.), ("25x12", "8x4")),          # imI % imC
    (HntrSpec(24, 13, 0., 900.), HntrSpec(8, 4, 0., 2700.), ("24x13", "8x4")),          # jmI % jmC
    (HntrSpec(8, 4, 0., 2700.), HntrSpec(24, 12, 0., 900.), ("8x4", "24x12")),          # the coarse grid is the finer one
])
def test_grids_that_do_not_nest_are_refused(I, Cg, words):
    with pytest.raises(_capi.IcebinHipError) as ei:
        etopo1.etopo1_ice(I, Cg, *planes(I, Cg))
    assert ei.value.code == _capi.IBH_EINVAL
    assert all(w in str(ei.value) for w in words), str(ei.value)


def test_a_tile_above_the_limit_is_refused_by_name():
    # 2731 x 3 = 8193 fine cells in a coarse cell, one above the limit
    I, Cg = HntrSpec(2731, 6, 0., 1800.), HntrSpec(1, 2, 0., 5400.)
    assert (I.im // Cg.im) * (I.jm // Cg.jm) == etopo1.MAX_TILE + 1
    with pytest.raises(_capi.IcebinHipError, match=str(etopo1.MAX_TILE)) as ei:
        etopo1.etopo1_ice(I, Cg, *planes(I, Cg))
    assert ei.value.code == _capi.IBH_EINVAL and "8193" in str(ei.value)


def test_create_rejects_bad_shapes_before_a_device():
    L = _capi.lib()
    h = C.c_void_p()

    def create(imI=24, jmI=12, imC=8, jmC=4, imH=0, jmH=0, dlatH=0., out=C.byref(h)):
        return L.ibh_etopo1_ice_create(out, imI, jmI, 0., 900., imC, jmC, imH, jmH, 0., dlatH)

    for bad in (dict(imI=0), dict(jmI=-1), dict(imC=0), dict(jmC=0), dict(imI=25), dict(jmI=14), dict(out=None), dict(imH=4), dict(jmH=4),
                dict(imH=4, jmH=1, dlatH=10800.), dict(imH=4, jmH=2, dlatH=0.), dict(imI=65536, jmI=65536, imC=65536, jmC=65536)):
        assert create(**bad) == _capi.IBH_EINVAL, bad
        assert not h.value
    # a NULL handle is refused by every entry
    assert L.ibh_etopo1_ice_device(None, *[None] * 4, 0, *[None] * 4, None, 0, None) == _capi.IBH_EINVAL
    assert L.ibh_etopo1_ice_host(None, *[None] * 4, 0, *[None] * 4, None, 0) == _capi.IBH_EINVAL
    assert L.ibh_etopo1_ice_destroy(None) == _capi.IBH_OK


def test_bad_planes_are_refused():
    I, Cg = HntrSpec(24, 12, 0., 900.), HntrSpec(8, 4, 0., 2700.)
    fo, zt, zs, fC = planes(I, Cg)
    cases = [((fo.astype(np.int32), zt, zs, fC), "focean"), ((fo, zt.astype(np.float64), zs, fC), "zictop"), ((fo, zt, zs[:-1], fC), "zsolid"),
             ((fo, zt, zs, fC.astype(np.float32)), "fgiceC"), ((fo, zt, zs, fC[:, :-1]), "fgiceC"), ((fo, None, zs, fC), "zictop"),
             ((fo.astype(">i2"), zt, zs, fC), "focean")]
    for args, word in cases:
        with pytest.raises(_capi.IcebinHipError, match=word) as ei:
            etopo1.etopo1_ice(I, Cg, *args)
        assert ei.value.code == _capi.IBH_EINVAL


def test_mixing_host_and_device_planes_is_refused():
    class OnDevice:             # what the check looks at, without a device
        is_cuda = True
        dtype = "torch.int16"

    I, Cg = HntrSpec(24, 12, 0., 900.), HntrSpec(8, 4, 0., 2700.)
    fo, zt, zs, fC = planes(I, Cg)
    for args in ((OnDevice(), zt, zs, fC), (fo, zt, OnDevice(), fC), (fo, zt, zs, OnDevice())):
        with pytest.raises(_capi.IcebinHipError, match="host and some on the device") as ei:
            etopo1.etopo1_ice(I, Cg, *args)
        assert ei.value.code == _capi.IBH_EINVAL


@pytest.mark.skipif(_capi.device_count() > 0, reason="checks the no-GPU failure mode")
def test_no_gpu_fails_loudly():
    I, Cg = HntrSpec(24, 12, 0., 900.), HntrSpec(8, 4, 0., 2700.)
    with pytest.raises(_capi.IcebinHipError, match="no CPU fallback") as ei:
        etopo1.etopo1_ice(I, Cg, *planes(I, Cg))
    assert ei.value.code == _capi.IBH_ENODEVICE
    with pytest.raises(_capi.IcebinHipError, match="no CPU fallback"):
        etopo1.etopo1_ice(I, Cg, *planes(I, Cg), hspecH=HntrSpec(12, 6, 0., 1800.))
