"""The sorted-tile walks of etopo1_ice (k_et_tiles) and make_topoO (k_to_tiles<false>, k_to_tiles<true>) on the case tiles of
tests/tile_walk_cases.py, against the plain-loop restatements: every plane equal bit for bit, nothing takes a tolerance.  What each
tile reaches (land count, padded sort size, the index and the manner of every stop) is shown on the CPU by
tests/test_tile_walk_cases.py; here a mismatch is reported with the name of the case tile it lies in."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import etopo1_ice_restatement as er  # noqa: E402
import make_topoo_restatement as mr  # noqa: E402
import tile_walk_cases as tw  # noqa: E402

ET_PLANES = ("FOCEAN1m", "FGICE1m", "ZICETOP1m", "ZSOLG1m")


def spec(g):
    from icebin_amd import HntrSpec
    return HntrSpec(g.im, g.jm, 0., 180. * 60. / g.jm)


# ---- etopo1_ice --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def et_reference(name, incl):
    I, Cg = tw.et_grids(name)
    out = er.etopo1_ice(spec(I), spec(Cg), *tw.et_cases(name)[0], incl)
    for a in out.values():
        a.setflags(write=False)
    return out


def et_assert(name, incl, res, what):
    ref = et_reference(name, incl)
    for n in ET_PLANES:
        got = getattr(res, n)
        assert str(got.dtype) == "torch.int16" and got.is_cuda and tuple(got.shape) == ref[n].shape, (what, n)
        got = got.cpu().numpy()
        bad = np.argwhere(got != ref[n])
        if len(bad):
            cases = []
            for j, i in bad.tolist():
                c = tw.et_case_at(name, j, i)
                label = c.name if c else "no case tile"
                if label not in cases:
                    cases.append(label)
            j, i = bad[0]
            raise AssertionError("%s: %s differs in %d cells; first (j, i) = (%d, %d): got %d, want %d; case tiles:\n  %s"
                                 % (what, n, len(bad), j, i, got[j, i], ref[n][j, i], "\n  ".join(cases[:12])))


@pytest.mark.parametrize("incl", [False, True], ids=["no_greenland", "greenland"])
@pytest.mark.parametrize("name", list(tw.ET_GEOM))
def test_etopo1_case_tiles_match_the_restatement(name, incl):
    from icebin_amd import etopo1
    I, Cg = tw.et_grids(name)
    planes = tw.et_cases(name)[0]
    res = etopo1.etopo1_ice(spec(I), spec(Cg), *planes, include_greenland=incl)
    et_assert(name, incl, res, (name, incl, "host"))
    ref = et_reference(name, incl)["FGICE1m"]
    assert ref.any() and (ref == 0).any()


@pytest.mark.parametrize("name", list(tw.ET_GEOM))
def test_etopo1_case_tiles_from_device_planes_at_odd_offsets(name):
    import torch
    from icebin_amd import etopo1
    I, Cg = tw.et_grids(name)
    planes = tw.et_cases(name)[0]
    # FOCEAN and ZICTOP 2 bytes past a 16-byte boundary, ZSOLID 6 bytes past one: a tile's rows then start at other alignments
    mis = []
    for p, off in zip(planes[:3], (1, 1, 3)):
        buf = torch.full((p.size + 8,), -7, dtype=torch.int16, device="cuda")
        buf[off:off + p.size] = torch.from_numpy(p.reshape(-1).copy())
        assert buf.data_ptr() % 16 == 0
        mis.append((buf, buf[off:off + p.size]))
    snap = [b.clone() for b, _ in mis]
    fC = torch.from_numpy(planes[3].copy()).cuda()
    res = etopo1.etopo1_ice(spec(I), spec(Cg), *[v for _, v in mis], fC, include_greenland=True)
    et_assert(name, True, res, (name, "device, odd offsets"))
    assert all(torch.equal(b, s) for (b, _), s in zip(mis, snap))


# ---- make_topoO --------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def to_regrids(name):
    """the six planes of step 1 through Hntr.regrid_device, as numpy [jmO, imO] (the regrid is Hntr's and is tested there)"""
    import torch
    from icebin_amd import Hntr
    I, O = tw.to_grids(name)
    fg, zt, zs, fo, fl = [torch.from_numpy(np.array(p)).cuda().reshape(1, -1) for p in tw.to_cases(name)[0]]
    hI, hS = Hntr(17.17, spec(O), spec(I)), Hntr(17.17, spec(O), spec(O))
    r = [hI.regrid_device(1., fo, mean_polar=True), hI.regrid_device(1., fg, mean_polar=True), hS.regrid_device(1., fl, mean_polar=True),
         hI.regrid_device(fo, zs, mean_polar=True), hI.regrid_device(fg, zt, mean_polar=True), hI.regrid_device(fg, zs, mean_polar=True)]
    return [x.cpu().numpy().reshape(O.jm, O.im) for x in r]


@functools.lru_cache(maxsize=None)
def to_reference(name):
    """(planes, counts): the restatement fed the regrids, once per geometry and never written.  The walks the restatement takes
    with these regrids are the ones the case table names, and no cell is filled through pow: every plane is exact."""
    walks, planes, counts, pow_cells = tw.to_walks(name, to_regrids(name))
    assert not pow_cells.any()
    for c in tw.to_cases(name)[2]:
        walk = walks[(c.I, c.J)][0]
        assert walk[2] == c.n and (c.walk is None or walk[:2] == c.walk), (c.name, walk)
    for a in planes.values():
        a.setflags(write=False)
    return planes, counts


def to_run(name, planes=None):
    from icebin_amd import topoo
    I, O = tw.to_grids(name)
    p, land = tw.to_cases(name)[:2]
    p = planes or p
    return topoo.make_topoO(spec(I), spec(O), p[0], p[1], p[2], p[3], spec(O), p[4], set_to_land=land)


def to_check(name, res, what):
    planes, counts = to_reference(name)
    I, O = tw.to_grids(name)
    for n in mr.PLANES:
        got = getattr(res, n).cpu().numpy()
        assert got.shape == (O.jm, O.im) and got.dtype == np.float64
        bad = np.argwhere(bits(got) != bits(planes[n]))
        if len(bad):
            cases = []
            for j, i in bad.tolist():
                c = tw.to_case_at(name, i + 1, j + 1)
                label = c.name if c else "no case tile (%d, %d)" % (i + 1, j + 1)
                if label not in cases:
                    cases.append(label)
            j, i = bad[0]
            raise AssertionError("%s: %s differs in %d cells; first (I, J) = (%d, %d): got %r, want %r; case tiles:\n  %s"
                                 % (what, n, len(bad), i + 1, j + 1, float(got[j, i]), float(planes[n][j, i]), "\n  ".join(cases[:12])))
    assert dict(res.counts) == counts, what


@pytest.mark.parametrize("name", list(tw.TO_GEOM))
def test_make_topoo_case_tiles_match_the_restatement(name):
    to_check(name, to_run(name), (name, "host"))


@pytest.mark.parametrize("name", list(tw.TO_GEOM))
def test_make_topoo_case_tiles_from_int16_planes_at_odd_offsets(name):
    """every int16 plane at its own odd element offset (2, 6, 10, 14 bytes past a 16-byte boundary)"""
    import torch
    p = tw.to_cases(name)[0]
    odd = []
    for k, a in enumerate(p[:4]):
        buf = torch.zeros(a.size + 16, dtype=torch.int16, device="cuda")
        off = 2 * k + 1
        buf[off:off + a.size] = torch.from_numpy(np.array(a)).reshape(-1)
        odd.append(buf[off:off + a.size])
        assert odd[-1].data_ptr() % 16 == 2 * off
    fl = torch.from_numpy(np.array(p[4])).cuda()
    to_check(name, to_run(name, planes=odd + [fl]), (name, "device, odd offsets"))


def test_each_geometry_takes_the_path_it_is_meant_to():
    from icebin_amd import etopo1, topoo
    for name, interior, poles in (("short", False, False), ("long", True, True)):
        I, O = tw.to_grids(name)
        mi, mj = I.im // O.im, I.jm // O.jm
        assert (mi * mj > topoo.MAX_TILE) == interior and (I.im * mj > topoo.MAX_TILE) == poles
    I, O = tw.to_grids("long")
    assert (I.im // O.im) * (I.jm // O.jm) == topoo.MAX_TILE + 1 == tw.TO_MAX_TILE + 1
    # etopo1_ice has one path; its walk has two branches, the unrolled 64-cell step and the partial one: the walk geometry's tiles
    # reach six full steps and a partial one, the limit geometry's exactly 128 full steps
    I, Cg = tw.et_grids("walk")
    assert (I.im // Cg.im) * (I.jm // Cg.jm) == 400 == 6 * 64 + 16
    I, Cg = tw.et_grids("limit")
    assert (I.im // Cg.im) * (I.jm // Cg.jm) == etopo1.MAX_TILE == 128 * 64
