"""CPU checks of the chunked global_ec: the restatement (tests/global_ec_chunks_restatement.py) against answers walked by hand
through modele/global_ec.cpp:805-893 and combine_global_ec.cpp:145-249, the library's host-only chunk walk against both, and
every argument error that needs no device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from icebin_amd import HntrSpec, _capi, global_ec

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_ec_chunks_restatement as gr  # noqa: E402

KNOWN_COUNTS = [0, 5, 0, 4, 9, 0, 0, 1]
KNOWN_CHUNKS = [((0, 0, 0, 1, 0), 18), ((1, 1, 0, 1, 3), 10), ((2, 1, 3, 2, 0), 1)]      # walked by hand through :868-893


def test_plan_known_answer():
    assert gr.chunk_plan_counts(KNOWN_COUNTS, 4, 2, 10) == KNOWN_CHUNKS
    assert global_ec.chunk_plan(4, 2, 3, 3, KNOWN_COUNTS, 10) == KNOWN_CHUNKS


def test_plan_without_ice_is_one_chunk():
    assert gr.chunk_plan_counts([0] * 8, 4, 2, 10) == [((0, 0, 0, 2, 0), 0)]
    assert global_ec.chunk_plan(4, 2, 3, 3, [0] * 8, 10) == [((0, 0, 0, 2, 0), 0)]


def test_plan_rejects_a_chunk_size_one_cell_can_reach():
    for size in (9, 1, 0, -5):
        with pytest.raises(_capi.IcebinHipError, match="chunk_size") as ei:
            global_ec.chunk_plan(4, 2, 3, 3, KNOWN_COUNTS, size)
        assert ei.value.code == _capi.IBH_EINVAL
    assert global_ec.chunk_plan(4, 2, 3, 3, KNOWN_COUNTS, 10) == KNOWN_CHUNKS
    with pytest.raises(_capi.IcebinHipError, match="counts"):
        global_ec.chunk_plan(4, 2, 3, 3, [0, 10, 0, 0, 0, 0, 0, 0], 20)           # more ice than a tile holds
    with pytest.raises(_capi.IcebinHipError, match="counts"):
        global_ec.chunk_plan(4, 2, 3, 3, KNOWN_COUNTS[:7], 20)


@pytest.mark.parametrize("seed", range(4))
def test_plan_walk_matches_the_restatement(seed):
    rng = np.random.default_rng(seed)
    imO, jmO, mult = 7, 5, 3
    c = rng.integers(0, mult * mult + 1, imO * jmO) * (rng.random(imO * jmO) < 0.6)
    for size in (10, 11, 17, 40, 10 ** 6):
        want = gr.chunk_plan_counts(c, imO, jmO, size)
        assert global_ec.chunk_plan(imO, jmO, mult, mult, c, size) == want
        ks = [(ch[1] * imO + ch[2], ch[3] * imO + ch[4]) for ch, _ in want]
        assert ks[0][0] == 0 and ks[-1][1] == imO * jmO and all(a[1] == b[0] for a, b in zip(ks, ks[1:]))
        assert all(c[k0:k1].sum() < size for k0, k1 in ks)


def test_range_and_counts_by_hand():
    fg = np.zeros((4, 6), np.int16)
    el = np.arange(24, dtype=np.int16).reshape(4, 6) * 100 - 700
    assert gr.elev_range(fg, el) == (10000, -10000)
    fg[0, 5], fg[3, 0], fg[1, 1] = 1, -3, 2
    assert gr.elev_range(fg, el) == (-200, 1100)
    assert gr.ec_range((-200, 1100), 500.) == (-500., 1500.)
    assert gr.ec_range((-1000, 1000), 500.) == (-1000., 1000.)
    assert gr.tile_counts(fg, 3, 2).tolist() == [[1, 0, 1], [1, 0, 0]]
    out = np.zeros(2)
    r = np.asarray([-200, 1100], np.int16)
    assert _capi.lib().ibh_global_ec_ec_range(r.ctypes.data, 500., out.ctypes.data) == 0 and out.tolist() == [-500., 1500.]
    assert _capi.lib().ibh_global_ec_ec_range(r.ctypes.data, 0., out.ctypes.data) == _capi.IBH_EINVAL


def test_mask_by_hand():
    fg = np.ones((2, 4), np.int16)
    fg[0, 0] = 0
    el = np.arange(8, dtype=np.int16).reshape(2, 4)
    fgO = np.asarray([[1., 0., 0.5, 1.]])              # O is 4 x 1, mult = (1, 2): cell 1 has no ice on the ocean grid
    em = gr.chunk_mask(fg, el, fgO, (0, 0, 0, 0, 3))
    want = np.asarray([[np.nan, np.nan, 2., np.nan], [4., np.nan, 6., np.nan]])
    assert np.array_equal(em, want, equal_nan=True)
    assert np.array_equal(gr.chunk_mask(fg, el, fgO, (1, 0, 3, 1, 0)), np.asarray([[np.nan] * 3 + [3.], [np.nan] * 3 + [7.]]), equal_nan=True)


def test_combine_by_hand():
    a = dict(dimB=[5, 2], dimA=[7, 1], wM=[1., 2.], Mw=[4., 8.], row=[0, 0, 1], col=[0, 1, 1], val=[.5, .25, 3.], extents=(6, 8))
    b = dict(dimB=[2, 0], dimA=[1, 3], wM=[6., 1.], Mw=[2., 5.], row=[0, 1], col=[0, 1], val=[10., 7.], extents=(6, 8))
    r = gr.combine([a, b], False)
    assert r["dimB"].tolist() == [5, 2, 0] and r["dimA"].tolist() == [7, 1, 3]
    assert r["wM"].tolist() == [1., 8., 1.] and r["Mw"].tolist() == [4., 10., 5.]
    assert (r["iB"].tolist(), r["iA"].tolist(), r["val"].tolist()) == ([5, 5, 2, 2, 0], [7, 1, 1, 1, 3], [.5, .25, 3., 10., 7.])
    row, col, val = gr.set_from_triplets(r["dimB"], r["dimA"], r["iB"], r["iA"], r["val"])
    assert (row.tolist(), col.tolist(), val.tolist()) == ([0, 0, 1, 2], [0, 1, 1, 2], [.5, .25, 13., 7.])
    s = gr.combine([a, b], True)
    assert s["val"].tolist() == [.5, .25, 3. * (1. / 8.), 10. * (1. / 8.), 7.]
    one = gr.combine([a], False)                        # a single chunk is the identity
    assert one["dimB"].tolist() == a["dimB"] and one["wM"].tolist() == a["wM"] and one["val"].tolist() == a["val"]


# ---- errors that need no device: every one is IBH_EINVAL with a message that names the argument --------------------------------
O, I = HntrSpec(8, 4, 0., 2700.), HntrSpec(32, 16, 0., 675.)


def planes(spec, dtype=np.int16):
    return np.ones((spec.jm, spec.im), dtype), np.zeros((spec.jm, spec.im), dtype)


def einval(match):
    return pytest.raises(_capi.IcebinHipError, match=match)


def test_scan_rejects_grids_that_do_not_nest():
    for bad in (HntrSpec(36, 16, 0., 675.), HntrSpec(32, 18, 0., 600.)):
        with einval(r"hspecI: Hntr grid \(%dx%d\) must be an even multiple of \(8x4\)" % (bad.im, bad.jm)) as ei:
            global_ec.IceScan(O, bad, *planes(bad))
        assert ei.value.code == _capi.IBH_EINVAL


def test_scan_rejects_wrong_planes():
    fg, el = planes(I)
    with einval("elevI: the plane holds 480 cells, hspecI has 512"):
        global_ec.IceScan(O, I, fg, el[:15])
    with einval("fgiceI: the plane holds 256 cells"):
        global_ec.IceScan(O, I, fg[:8], el)
    with einval("fgiceI: dtype float64"):
        global_ec.IceScan(O, I, fg.astype(np.float64), el)
    with einval("elevI: dtype int32"):
        global_ec.IceScan(O, I, fg, el.astype(np.int32))
    # the C entry on its own: the plane type, the size, null planes and a null result, before any device is touched
    h = C.c_void_p()
    call = lambda **k: _capi.lib().ibh_global_ec_scan_create(       # noqa: E731
        8, 4, 0., 2700., 32, 16, 0., 675., k.get("fg", fg.ctypes.data), k.get("el", el.ctypes.data), k.get("n", 512), k.get("t", 1), 0, None,
        k.get("out", C.byref(h)))
    for bad, msg in ((dict(t=0), "plane type 0"), (dict(t=2), "plane type 2"), (dict(n=511), "hold 511 cells"), (dict(fg=None), "null plane"),
                     (dict(el=None), "null plane"), (dict(out=None), "out: null")):
        assert call(**bad) == _capi.IBH_EINVAL and msg in _capi.lib().ibh_last_error().decode(), bad
        assert not h.value


def test_combine_rejects_bad_arguments_without_a_device():
    L = _capi.lib()
    h = C.c_void_p()
    assert L.ibh_global_ec_combine_chunks(0, None, None, None, 0, None, None, None, C.byref(h)) == _capi.IBH_EINVAL
    assert "mats" in L.ibh_last_error().decode()
    one = (C.c_void_p * 1)(None)
    assert L.ibh_global_ec_combine_chunks(1, one, None, None, 0, None, None, None, C.byref(h)) == _capi.IBH_EINVAL
    assert "mats: chunk 0 is null" in L.ibh_last_error().decode()
    assert L.ibh_global_ec_combine_chunks(1, one, None, None, 0, None, None, None, None) == _capi.IBH_EINVAL
    with einval("chunk_results"):
        global_ec.combine_chunks([], "EvA")
    with einval("name: chunk 0 holds no matrix 'XvY'"):
        global_ec.combine_chunks([{"EvO": None, "OvE": None}], "XvY")
    with einval("ifnames"):
        global_ec.combine_chunk_files([], "nowhere")


def test_plan_and_mask_reject_a_null_scan():
    L = _capi.lib()
    n = C.c_int32()
    assert L.ibh_global_ec_chunk_plan(None, 100, 0, None, None, C.byref(n)) == _capi.IBH_EINVAL and "scan" in L.ibh_last_error().decode()
    assert L.ibh_global_ec_chunk_mask(None, 0, 0, 1, 0, None, 0, None) == _capi.IBH_EINVAL and "scan" in L.ibh_last_error().decode()
    assert L.ibh_global_ec_scan_get(None, None, None, None, None, None) == _capi.IBH_EINVAL
