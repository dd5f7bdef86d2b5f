"""make_topoO on the GPU (icebin_amd.topoo) against the plain-loop restatement of modele/topo_base.cpp:20-221, :263-809
(tests/make_topoo_restatement.py), which is fed Hntr.regrid_device of the same inputs.  Every plane is compared bit for bit; the one
exception is the set of dZGICE cells filled through pow (:708), which the test names (the restatement's pow_cells) and compares
with the restatement evaluated in numpy.longdouble under (2 * U + imO + jmO + 8) * 2^-53: U bounds the device pow's error in ulp
(profiles/make_topoo_pow_ulp.txt), imO + jmO + 8 the two positive-term chains and the final operations."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_topoo_restatement as mr  # noqa: E402

POW_ULP = 2.5752    # U: twice the largest error measured (1.2876 ulp) over 2^20 log-uniform points of [1e-6, 1] (profiles/make_topoo_pow_ulp.txt)


def spec(im, jm, offi=0.):
    from icebin_amd import HntrSpec
    return HntrSpec(im, jm, offi, 180. * 60. / jm)


# name -> (ocean, fine, lakes (im, jm, offi)).  Ocean 12 x 12: JM/6 = 2, the wedge is J = 10..11, every band is non-empty.
# m3 / m4 / m5: the multiples; m3s: FLAKES on the ocean grid itself, so that the 1/512 boundaries reach std::round as they are;
# r24x30: mult_i != mult_j; real: the production tile 75 x 60 (pole tiles of 54000 cells: the long path); limit: a tile of exactly
# MAX_TILE (128 x 64); over: one cell above it (2731 x 3), the long path on every interior cell.  Lakes: grids that do not nest in
# the ocean grid, one of them with offi != 0.
GRIDS = {"m3": ((12, 12), (36, 36), (18, 9, 0.)), "m4": ((12, 12), (48, 48), (30, 18, .5)), "m5": ((12, 12), (60, 60), (20, 10, 0.)),
         "m3s": ((12, 12), (36, 36), (12, 12, 0.)), "r24x30": ((24, 30), (72, 60), (36, 20, 0.)),
         "real": ((12, 12), (900, 720), (72, 36, 0.)), "limit": ((12, 12), (1536, 768), (18, 9, 0.)),
         "over": ((12, 12), (32772, 36), (18, 9, 0.))}
SMALL = ("m3", "m4", "m5", "m3s", "r24x30")


def grids(name):
    o, f, s = GRIDS[name]
    return spec(*f), spec(*o), spec(*s)


def tile(a, I, O, J, Ic):
    """the fine cells of ocean cell (Ic, J), 1-based, as a view"""
    mi, mj = I.im // O.im, I.jm // O.jm
    return a[(J - 1) * mj:J * mj, (Ic - 1) * mi:Ic * mi]


# the special tiles, as ocean cells (I, J) 1-based on a 12-wide grid; all lie in J = 3..9, outside FLAKE's zero bands
ALL_OCEAN, ALL_LAND, ONE_LAND, ONE_OCEAN, LEFT_HALF = (2, 3), (4, 3), (6, 3), (8, 3), (10, 3)
LAND_OVER_OCEAN, OCEAN_OVER_LAND, RESET, ICE_AND_LAKE = (2, 5), (4, 5), (6, 5), (8, 5)
BLOCK = (9, 7)          # the 2 x 2 block (9..10, 7..8): one ocean cell, three land cells with lakes


@functools.lru_cache(maxsize=None)
def make_planes(name):
    """FOCEAN1m in {0, 1} at random, FGICE1m in {0, 1}, depths with many ties and both int16 extremes, ZSOLG1m below ZICETOP1m on
    the western half only (so that the eastern cells take :688-691 and the pow fill), FLAKES half on multiples of 1/512.  Then the
    special tiles.  Returns (FGICE1m, ZICETOP1m, ZSOLG1m, FOCEAN1m, FLAKES, set_to_land, set_to_ocean, resets)."""
    I, O, S = grids(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    shape = (I.jm, I.im)
    fo = (rng.random(shape) < .5).astype(np.int16)
    fg = (rng.random(shape) < .4).astype(np.int16)
    zt = (rng.integers(-3, 4, shape) * 100).astype(np.int16)
    zt[rng.random(shape) < 0.03] = -32768
    zt[rng.random(shape) < 0.03] = 32767
    zs = zt.copy()
    west = np.zeros(shape, bool)
    west[:, :I.im // 2] = rng.random((I.jm, I.im // 2)) < .3
    zs[west] = np.clip(zt[west].astype(np.int64) - rng.integers(1, 100, int(west.sum())), -32768, 32767).astype(np.int16)
    fl = np.where(rng.random((S.jm, S.im)) < .5, rng.integers(0, 513, (S.jm, S.im)) / 512., rng.random((S.jm, S.im)))
    fl[rng.random(fl.shape) < .2] = 0.
    fo[0, 0] = 0                                    # land in the south polar tile (:498-502 makes row 1 continental)
    fo[-1, 0], fo[-1, 1] = 0, 1                     # and both kinds in the north polar one
    land, ocean, resets = [], [], []
    if O.im == 12:
        t = lambda a, c: tile(a, I, O, c[1], c[0])  # noqa: E731
        t(fo, ALL_OCEAN)[:] = 1
        for c in ((3, 3), (3, 4), (4, 4), (5, 5), (5, 6), (6, 6)):         # the 2 x 2 blocks of ALL_LAND and RESET hold no ocean: their
            t(fo, c)[:] = 0                                                # lakes survive :774-795
        t(fo, ALL_LAND)[:] = 0
        t(fo, ONE_LAND)[:] = 1
        t(fo, ONE_LAND)[-1, 0] = 0
        t(fo, ONE_OCEAN)[:] = 0
        t(fo, ONE_OCEAN)[0, -1] = 1
        t(fo, LEFT_HALF)[:] = 0
        t(fo, LEFT_HALF)[:, :t(fo, LEFT_HALF).shape[1] // 2] = 1
        t(fo, LAND_OVER_OCEAN)[:] = 1
        t(fo, LAND_OVER_OCEAN)[0, :2] = 0
        land.append(LAND_OVER_OCEAN)
        t(fo, OCEAN_OVER_LAND)[:] = 0
        t(fo, OCEAN_OVER_LAND)[-1, -2:] = 1
        ocean.append(OCEAN_OVER_LAND)
        t(fo, RESET)[:] = 0
        resets = [(-30., [RESET, (7, 5)]), (53., [RESET])]          # a cell listed twice
        t(fo, ICE_AND_LAKE)[:] = 0                  # FGICE = 1 and a lake: FGICE + FLAKE + FOCEAN > 1
        t(fg, ICE_AND_LAKE)[:] = 1
        bi, bj = BLOCK
        for c in ((bi, bj), (bi + 1, bj), (bi, bj + 1), (bi + 1, bj + 1)):
            t(fo, c)[:] = 1 if c == (bi, bj) else 0
            t(fg, c)[:] = 0
        if name == "m3s":                           # lakes on exact 1/512 boundaries over all-land tiles, and a large one on the ice
            fl[ALL_LAND[1] - 1, ALL_LAND[0] - 1] = 257 / 512.
            fl[RESET[1] - 1, RESET[0] - 1] = 3 / 512.
            fl[ONE_OCEAN[1] - 1, ONE_OCEAN[0] - 1] = 1 / 512.
            fl[ICE_AND_LAKE[1] - 1, ICE_AND_LAKE[0] - 1] = .75
            for c in ((bi + 1, bj), (bi, bj + 1), (bi + 1, bj + 1)):
                fl[c[1] - 1, c[0] - 1] = .25
    for a in (fg, zt, zs, fo, fl):
        a.setflags(write=False)
    return fg, zt, zs, fo, fl, tuple(land), tuple(ocean), tuple(resets)


def regrids(name, planes=None):
    """the six planes of step 1 through Hntr.regrid_device, as numpy [jmO, imO]"""
    import torch
    from icebin_amd import Hntr
    I, O, S = grids(name)
    fg, zt, zs, fo, fl = [torch.from_numpy(np.array(p)).cuda().reshape(1, -1) for p in (planes or make_planes(name))[:5]]
    hI, hS = Hntr(17.17, O, I), Hntr(17.17, O, S)
    r = [hI.regrid_device(1., fo, mean_polar=True), hI.regrid_device(1., fg, mean_polar=True), hS.regrid_device(1., fl, mean_polar=True),
         hI.regrid_device(fo, zs, mean_polar=True), hI.regrid_device(fg, zt, mean_polar=True), hI.regrid_device(fg, zs, mean_polar=True)]
    return [x.cpu().numpy().reshape(O.jm, O.im) for x in r]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(planes, counts, pow_cells, dZGICE in long double, the six regrids): computed once per grid and never written"""
    I, O, S = grids(name)
    p = make_planes(name)
    six = regrids(name)
    args = (I.im, I.jm, O.im, O.jm, p[0], p[1], p[2], p[3], *six)
    kw = dict(set_to_land=p[5], set_to_ocean=p[6], resets=p[7])
    planes, counts, pow_cells = mr.make_topoO(*args, **kw)
    ld = mr.make_topoO(*args, real=np.longdouble, only_dzgice=True, **kw)[0]["dZGICE"]
    for a in list(planes.values()) + [pow_cells, ld] + six:
        a.setflags(write=False)
    return planes, counts, pow_cells, ld, six


def run(name, planes=None, **kw):
    from icebin_amd import topoo
    I, O, S = grids(name)
    p = planes or make_planes(name)
    kw.setdefault("set_to_land", p[5]); kw.setdefault("set_to_ocean", p[6]); kw.setdefault("resets", p[7])
    return topoo.make_topoO(I, O, p[0], p[1], p[2], p[3], S, p[4], **kw)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def check(name, res):
    planes, counts, pow_cells, ld, six = reference(name)
    I, O, S = grids(name)
    for n in mr.PLANES:
        got = getattr(res, n).cpu().numpy()
        assert got.shape == (O.jm, O.im) and got.dtype == np.float64
        if n == "dZGICE":
            exact = ~pow_cells
            bad = np.argwhere(bits(got)[exact] != bits(planes[n])[exact])
            assert bad.size == 0, (name, n, len(bad))
            if pow_cells.any():
                g, want = got[pow_cells].astype(np.longdouble), ld[pow_cells]
                rel = np.abs(g - want) / np.abs(want)
                bound = (2 * POW_ULP + O.im + O.jm + 8) * 2. ** -53
                print("%s: %d cells through pow, largest relative error %.3g, bound %.3g" % (name, int(pow_cells.sum()), float(rel.max()), bound))
                assert (rel <= bound).all(), (name, float(rel.max()), bound)
            continue
        bad = np.argwhere(bits(got) != bits(planes[n]))
        assert bad.size == 0, (name, n, len(bad), bad[:4].tolist(), got[tuple(bad[0])], planes[n][tuple(bad[0])])
    assert dict(res.counts) == counts, name


@pytest.mark.parametrize("name", list(GRIDS))
def test_planes_equal_the_restatement(name):
    check(name, run(name))


@pytest.mark.parametrize("name", ["m4", "m3s"])
def test_step1_is_bitwise_the_regrids_and_unwritten_planes_are_zero(name):
    res = run(name)
    six = reference(name)[4]
    assert np.array_equal(bits(res.FOCEANF.cpu().numpy()), bits(six[0]))
    assert np.array_equal(bits(res.FGICEF.cpu().numpy())[1:], bits(six[1])[1:]) and (res.FGICEF[0] == 1).all()       # :501
    for n in ("ZLAND_MIN", "ZLAND_MAX", "FGICE_greenland"):
        assert not getattr(res, n).any()
    assert not res.ZATMOF[0, 1:].any() and not res.ZATMOF[-1, 1:].any()


def test_the_cases_are_there():
    """the inputs reach what they are meant to reach (read from the restatement, so the GPU result is not what decides)"""
    planes, counts, pow_cells, _, six = reference("m3s")
    at = lambda n, c: planes[n][c[1] - 1, c[0] - 1]  # noqa: E731
    assert at("FOCEAN", ALL_OCEAN) == 1 and at("FOCEAN", ONE_LAND) == 1 and at("FOCEAN", ALL_LAND) == 0 and at("FOCEAN", ONE_OCEAN) == 0
    half = reference("m4")[4][0][LEFT_HALF[1] - 1, LEFT_HALF[0] - 1]          # two of four columns: at or beside .5
    assert abs(half - .5) < 1e-15
    assert at("FOCEAN", LAND_OVER_OCEAN) == 0 and six[0][LAND_OVER_OCEAN[1] - 1, LAND_OVER_OCEAN[0] - 1] > .5
    assert at("FOCEAN", OCEAN_OVER_LAND) == 1 and six[0][OCEAN_OVER_LAND[1] - 1, OCEAN_OVER_LAND[0] - 1] < .5
    assert at("ZLAKE", RESET) == 53. and at("ZATMO", RESET) == 53.
    # lakes at or beside a 1/512 boundary (the regrid of one cell is w * a / w, which may round): 128.5 and 1.5 go to either
    # neighbour, by what the regrid gave and std::round's half away from zero (pinned on the CPU)
    for c, k in ((ALL_LAND, 128), (RESET, 1)):
        v = six[2][c[1] - 1, c[0] - 1] * 256.
        assert abs(v - (k + .5)) < 1e-12 and at("FLAKE", c) == (k + 1 if v >= k + .5 else k) / 256.
    assert counts["FLAKE_reduced"] >= 1 and at("FGICE", ICE_AND_LAKE) == 1 and at("FLAKE", ICE_AND_LAKE) == 0
    bi, bj = BLOCK
    for c in ((bi + 1, bj), (bi, bj + 1), (bi + 1, bj + 1)):        # the lakes of the block went to the ground
        assert at("FLAKE", c) == 0 and at("dZLAKE", c) == 0 and at("FGRND", c) == 1
    assert pow_cells.any() and not pow_cells.all()
    for name in ("real", "limit", "over"):
        assert reference(name)[2].any()


def test_long_path_is_taken_where_the_tiles_say():
    from icebin_amd import topoo
    for name, interior, poles in (("m5", False, False), ("real", False, True), ("limit", False, True), ("over", True, True)):
        I, O, S = grids(name)
        mi, mj = I.im // O.im, I.jm // O.jm
        assert (mi * mj > topoo.MAX_TILE) == interior and (I.im * mj > topoo.MAX_TILE) == poles
    I, O, S = grids("limit")
    assert (I.im // O.im) * (I.jm // O.jm) == topoo.MAX_TILE
    I, O, S = grids("over")
    assert (I.im // O.im) * (I.jm // O.jm) == topoo.MAX_TILE + 1


def test_device_planes_in_place_and_at_odd_offsets_inputs_unchanged():
    import torch
    from icebin_amd import topoo
    name = "m5"
    I, O, S = grids(name)
    p = make_planes(name)
    dev = [torch.from_numpy(np.array(a)).cuda() for a in p[:5]]
    before = [d.clone() for d in dev]
    res = topoo.make_topoO(I, O, dev[0], dev[1], dev[2], dev[3], S, dev[4], set_to_land=p[5], set_to_ocean=p[6], resets=p[7])
    check(name, res)
    assert all(torch.equal(a, b) for a, b in zip(dev, before))
    assert res._keep[0].data_ptr() == dev[0].data_ptr()             # read in place
    # every int16 plane at its own odd element offset (2, 6, 10, 14 bytes past a 16-byte boundary)
    odd = []
    for k, d in enumerate(dev[:4]):
        buf = torch.zeros(d.numel() + 16, dtype=torch.int16, device="cuda")
        off = 2 * k + 1
        buf[off:off + d.numel()] = d.reshape(-1)
        odd.append(buf[off:off + d.numel()])
        assert odd[-1].data_ptr() % 16 == 2 * off
    res2 = topoo.make_topoO(I, O, odd[0], odd[1], odd[2], odd[3], S, dev[4], set_to_land=p[5], set_to_ocean=p[6], resets=p[7])
    check(name, res2)
    with pytest.raises(Exception, match="host and some on the device"):
        topoo.make_topoO(I, O, dev[0], p[1], dev[2], dev[3], S, dev[4])


def test_real_tile_rows_at_every_alignment():
    """mult_i = 75: a tile row is 150 bytes, so the rows of one tile start at every even offset from a 16-byte boundary"""
    import torch
    from icebin_amd import topoo
    name = "real"
    I, O, S = grids(name)
    p = make_planes(name)
    d = torch.from_numpy(np.array(p[3])).cuda()
    buf = torch.zeros(d.numel() + 16, dtype=torch.int16, device="cuda")
    buf[3:3 + d.numel()] = d.reshape(-1)
    others = [torch.from_numpy(np.array(a)).cuda() for a in (p[0], p[1], p[2], p[4])]
    res = topoo.make_topoO(I, O, others[0], others[1], others[2], buf[3:3 + d.numel()], S, others[3], set_to_land=p[5], set_to_ocean=p[6],
                           resets=p[7])
    check(name, res)


def test_fatal_cells_status_message_and_first_cell():
    from icebin_amd import topoo
    name = "m4"
    I, O, S = grids(name)
    p = make_planes(name)
    # an ocean cell without an ocean fine cell: SET_TO ocean over the all-land tile; a later one is not the one reported
    with pytest.raises(ValueError) as ei:
        run(name, set_to_ocean=p[6] + (ALL_LAND, RESET))
    assert str(ei.value) == topoo.fatal_message("ocean", I, O, ALL_LAND[1], ALL_LAND[0])
    assert str(ei.value) == "Ocean cell FOCEAN(4,3)=1 has no ocean area on 2-minute grid; I11,I1M,J11,J1M = 13,16,9,12"
    # a continental cell without land: SET_TO land over the all-ocean tile
    with pytest.raises(ValueError) as ei:
        run(name, set_to_land=p[5] + (ALL_OCEAN,))
    assert str(ei.value) == "Continental cell (2,3) has no continental area on 2-minute grid. (5-8, 9-12)"
    # both kinds: the first cell in the reference's order (J outer, I inner) is the one reported, and the restatement agrees
    with pytest.raises(ValueError) as ei:
        run(name, set_to_land=p[5] + (ALL_OCEAN,), set_to_ocean=p[6] + (ALL_LAND,))
    assert str(ei.value).startswith("Continental cell (2,3)")
    six = reference(name)[4]
    with pytest.raises(mr.Fatal) as fi:
        mr.make_topoO(I.im, I.jm, O.im, O.jm, p[0], p[1], p[2], p[3], *six, set_to_land=p[5] + (ALL_OCEAN,), set_to_ocean=p[6] + (ALL_LAND,))
    assert (fi.value.kind, fi.value.I, fi.value.J) == ("continental", 2, 3)
    # the south pole is always continental: without land there, (1, 1) with the whole row as its tile
    fo = np.array(p[3])
    fo[:I.jm // O.jm] = 1
    with pytest.raises(ValueError) as ei:
        run(name, planes=(p[0], p[1], p[2], fo) + p[4:])
    assert str(ei.value) == "Continental cell (1,1) has no continental area on 2-minute grid. (1-48, 1-4)"


def test_etopo1_ice_make_topoO_equals_the_call_on_copies():
    from icebin_amd import etopo1, topoo
    name = "m4"
    I, O, S = grids(name)
    rng = np.random.default_rng(5)
    Cg = spec(6, 6)
    fo = rng.integers(0, 3, (I.jm, I.im)).astype(np.int16)
    zt = (rng.integers(-3, 4, fo.shape) * 100).astype(np.int16)
    zs = (zt - rng.integers(0, 100, fo.shape)).astype(np.int16)
    fo[0, 0] = 0
    e = etopo1.etopo1_ice(I, Cg, fo, zt, zs, rng.random((Cg.jm, Cg.im)), include_greenland=True)
    fl = make_planes(name)[4]
    a = e.make_topoO(O, S, fl)
    b = topoo.make_topoO(I, O, e.FGICE1m.cpu().numpy(), e.ZICETOP1m.cpu().numpy(), e.ZSOLG1m.cpu().numpy(), e.FOCEAN1m.cpu().numpy(), S, fl)
    for n in topoo.PLANES:
        assert np.array_equal(bits(getattr(a, n).cpu().numpy()), bits(getattr(b, n).cpu().numpy())), n
    assert a.counts == b.counts and a._keep[0].data_ptr() == e.FGICE1m.data_ptr()


def test_topoo_dict_is_accepted_by_merge_topoO():
    import torch
    from icebin_amd import GCMRegridder, HntrSpec, global_ec, merge_topoO, topoo
    res = run("m3")
    t = res.topoo()
    assert list(t) == list(topoo.PLANES) and all(torch.is_tensor(v) and v.is_cuda for v in t.values())
    I, O, S = grids("m3")
    R, Is, hc = 6371000., HntrSpec(72, 72, 0.5, 150.), [0., 1500., 3000.]
    i0 = np.arange(Is.size)
    land = np.where((i0 * 7) % 5 == 0, np.nan, (i0 % 3000) - 100.)
    with np.errstate(invalid="ignore"):
        ice = np.where((i0 % 3 == 0) | ~((land >= 0.) & (land <= 3000.)), np.nan, land)
    gcm = GCMRegridder(dict(nA=O.size, to_sparse=np.arange(O.size), native_area=np.full(O.size, 1.e13)), hc, True)
    idx, area = global_ec.gcm_from_hntr(O, Is, land, hc, True, R).exgrid()
    gcm.add_sheet("sheet0", dict(nI=Is.size), dict(indices=idx.copy(), overlaps=area.copy()))
    untouched = res.ZLAKE.clone()
    mask, errors = merge_topoO(t, gcm, [land], [ice], O, R)
    assert tuple(mask.shape) == (O.jm, O.im) and isinstance(errors, list)
    assert all(torch.is_tensor(t[k]) and t[k].is_cuda and tuple(t[k].shape) == (O.jm, O.im) for k in t)     # merged in HBM
    assert torch.equal(t["ZLAKE"], untouched) and torch.isfinite(t["FOCEAN"]).all()


def test_write_reads_back(tmp_path):
    from icebin_amd import ncio, topoo
    res = run("m3")
    I, O, S = grids("m3")
    f = res.write(str(tmp_path / "topoo.nc"))
    assert open(f, "rb").read(4) == b"CDF\x05"
    ds = ncio.Dataset.read(f)
    assert dict(ds.dims) == {"jm": O.jm, "im": O.im}
    assert list(ds.variables)[:2] == ["lon", "lat"] and list(ds.variables)[2:] == list(topoo.PLANES)
    assert np.array_equal(ds.variables["lon"].data, -180. + (np.arange(O.im) + .5) * (360. / O.im))
    assert np.allclose(ds.variables["lat"].data, -90. + (np.arange(O.jm) + .5) * (180. / O.jm), rtol=0, atol=1e-12)
    for n in topoo.PLANES:
        v = ds.variables[n]
        assert np.array_equal(bits(v.data), bits(getattr(res, n).cpu().numpy())) and dict(v.attrs) == dict(topoo.ATTRS[n]), n
    assert ds.variables["FOCEAN"].attrs["source"] == "GISS 1Qx1" and ds.variables["dZGICE"].attrs["sources"] == "Ekholm,Bamber"


def test_c_host_entry_and_device_refusals():
    import torch
    from icebin_amd import _capi, topoo
    name = "m3"
    I, O, S = grids(name)
    p = make_planes(name)
    res = run(name)
    L = _capi.lib()
    ptr = _capi.ptr
    host = [np.ascontiguousarray(a) for a in p[:5]]
    ld = O.size + 3
    out = np.full(19 * ld + O.size, -7.)
    st = np.zeros(10, np.int64)
    _capi.check(L.ibh_make_topoo_host(res._h, *[ptr(a) for a in host], ptr(out), ld, ptr(st)))
    for k, n in enumerate(topoo.PLANES):
        assert np.array_equal(bits(out[k * ld:k * ld + O.size]), bits(getattr(res, n).cpu().numpy().reshape(-1))), n
        if k < 19:
            assert (out[k * ld + O.size:(k + 1) * ld] == -7.).all()         # the gaps are left alone
    assert st[1] == -1 and st[3] == -1 and dict(zip(topoo.COUNTS, st[4:].tolist())) == dict(res.counts)
    dev = [torch.from_numpy(np.array(a)).cuda() for a in p[:5]]
    o = torch.zeros(20 * O.size + 8, dtype=torch.float64, device="cuda")

    def call(ptrs, ld=O.size, h=res._h):
        return L.ibh_make_topoo_device(h, *[C.c_void_p(x) for x in ptrs], ld, None)
    good = [d.data_ptr() for d in dev] + [o.data_ptr()]
    for k in range(6):                              # a NULL plane, then a misaligned one
        bad = list(good); bad[k] = 0
        assert call(bad) == _capi.IBH_EINVAL and b"null" in L.ibh_last_error()
        bad = list(good); bad[k] = good[k] + 1
        assert call(bad) == _capi.IBH_EINVAL and b"aligned" in L.ibh_last_error()
    assert call(good, ld=O.size - 1) == _capi.IBH_EINVAL and b"ld=" in L.ibh_last_error()
    big = torch.zeros(20 * O.size + I.size, dtype=torch.float64, device="cuda")
    inside = big.data_ptr() + 8 * (19 * O.size)     # an input inside the outputs' last plane
    assert call([inside] + good[1:4] + [good[4], big.data_ptr()]) == _capi.IBH_EINVAL and b"overlap" in L.ibh_last_error()
    assert call(good[:4] + [big.data_ptr() + 8, big.data_ptr()]) == _capi.IBH_EINVAL and b"overlap" in L.ibh_last_error()
    assert call(good, h=None) == _capi.IBH_EINVAL
    torch.cuda.synchronize()
    assert call(good) == _capi.IBH_OK               # and the good call goes through
    torch.cuda.synchronize()
    assert np.array_equal(bits(o[:O.size].cpu().numpy()), bits(res.FOCEAN.cpu().numpy().reshape(-1)))
