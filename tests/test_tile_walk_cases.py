"""The case tiles of tests/tile_walk_cases.py reach what their names say.  Everything here is read from the restatements
(etopo1_ice_restatement.py, make_topoo_restatement.py) on the CPU: the GPU result never decides whether a case counts, and the
tables are walked in full, so no case can drop out unseen."""
import functools
import os
import sys

import numpy as np
import pytest

from icebin_amd import HntrSpec, etopo1, topoo

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import etopo1_ice_restatement as er  # noqa: E402
import make_topoo_restatement as mr  # noqa: E402
import tile_walk_cases as tw  # noqa: E402


def spec(g):
    return HntrSpec(g.im, g.jm, 0., 180. * 60. / g.jm)


# ---- A. etopo1_ice -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def et_reference(name):
    I, Cg = tw.et_grids(name)
    out = er.etopo1_ice(spec(I), spec(Cg), *tw.et_cases(name)[0], False)
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("name", list(tw.ET_GEOM))
def test_etopo1_cases_do_what_their_names_say(name):
    I, Cg = tw.et_grids(name)
    (fo, zt, zs, fC), table = tw.et_cases(name)
    mi, mj = I.im // Cg.im, I.jm // Cg.jm
    dI, dC = er.make_dxyp(spec(I)), er.make_dxyp(spec(Cg))
    # the builders' areas are the library's, bit for bit
    assert dI.tolist() == mr.make_dxyp(I.im, I.jm) and dC.tolist() == mr.make_dxyp(Cg.im, Cg.jm)
    jband = I.jm * 14 // 15
    assert not (fo[I.jm // 2:] == er.GREENLAND_VAL).any() and (fo[:I.jm // 2] == er.GREENLAND_VAL).any()
    fgice = et_reference(name)["FGICE1m"]
    seen, extremes = 0, 0
    assert len({(c.j1, c.i1) for c in table}) == len(table)
    for c in table:
        assert Cg.jm // 2 <= c.j1 and (c.j1 + 1) * mj <= jband, c.name             # north half, wholly south of the 78N band
        cells = er.tile_cells(fo, zt, c.j1, c.i1, mj, mi, False)
        assert len(cells) == c.n and tw.pow2(c.n) == c.n2 and c.n2 // 2 < max(c.n, 1) <= c.n2, c.name
        elev = [-e for e, _, _ in cells]
        if c.name.startswith("ties: one"):
            assert len(set(elev)) == 1
        elif c.name.startswith("ties: two"):
            t = zt[c.j1 * mj:(c.j1 + 1) * mj, c.i1 * mi:(c.i1 + 1) * mi].reshape(-1)
            assert len(set(elev)) == 2 and (t[::2] == t[0]).all() and (t[1::2] == t[1]).all() and t[0] != t[1]
        elif c.name.startswith("ties: stop between"):
            (e0, j0, _), (e1, j1, _) = cells[c.k - 1], cells[c.k]
            assert e0 == e1 and j0 < j1 and dI[j0] != dI[j1] and len(set(elev)) == c.n - 1
        else:
            assert len(set(elev)) == c.n, c.name                                    # distinct: the order shows in the output
            extremes += c.n >= 2 and elev[0] == 32767 and elev[-1] == -32768
        areas = [float(dI[j]) for _, j, _ in cells]
        remain = float(fC[c.j1, c.i1]) * float(dC[c.j1])
        taken = er.fill(cells, areas, remain)
        ntake, stop, rounded = tw.et_trace(areas, remain)
        assert len(taken) == ntake == c.taken, c.name
        if c.outcome is None:                                                       # never stops
            assert fC[c.j1, c.i1] == 1.5 and stop is None and ntake == c.n, c.name
        elif c.outcome == "quarter":
            assert (stop, rounded, ntake) == (c.k, False, c.k), c.name
        elif c.outcome == "three_quarters":
            assert (stop, rounded, ntake) == (c.k, True, c.k + 1), c.name
        else:                                                                       # `<=` holds at cell k, the next cell fails
            assert ntake == c.k + 1 and rounded is False and stop == (c.k + 1 if c.k + 1 < c.n else None), c.name
        # observable: FGICE1m inside the tile is the walk's prefix and nothing else
        t = fgice[c.j1 * mj:(c.j1 + 1) * mj, c.i1 * mi:(c.i1 + 1) * mi]
        want = np.zeros_like(t)
        for _, j, i in cells[:ntake]:
            want[j - c.j1 * mj, i - c.i1 * mi] = 1
        assert np.array_equal(t, want), c.name
        seen += 1
    assert seen == len(table) and extremes >= (3 if name == "walk" else 1)            # none left out
    if name == "walk":
        assert len(table) == 22 + 3 * (14 + 8 + 9) + 2 + 3
        assert sorted(c.n for c in table if c.name.startswith("sort")) == list(tw.ET_SORT_N)
        assert all(c.k == c.n // 2 and c.outcome == "quarter" for c in table if c.name.startswith("sort"))
        assert {c.n2 for c in table} >= {1, 2, 4, 8, 16, 32, 64, 128, 256, 512}      # every shape of the network up to the tile
        for n in (400, 128, 129):
            stops = {k for k in tw.ET_STOPS if k < n} | {n - 2, n - 1}
            got = {(c.k, c.outcome) for c in table if c.name.startswith("stop n=%d " % n)}
            assert got == {(k, oc) for k in stops for oc in tw.ET_OUTCOMES}, n
        # a stop and a rounding-in on lane 63 and on lane 0 of a later 64-cell step, and in the partial last step of n = 400
        k_oc = {(c.k % 64, c.k // 64, c.outcome) for c in table if c.name.startswith("stop")}
        assert {(63, 1, "quarter"), (63, 1, "three_quarters"), (0, 2, "quarter"), (0, 3, "three_quarters"), (15, 6, "exact")} <= k_oc
        assert sorted(c.n for c in table if c.outcome is None) == [64, 128]
    else:
        assert mi * mj == etopo1.MAX_TILE and sorted(c.n for c in table) == list(tw.ET_LIMIT_N)
        assert all(c.taken == c.n // 2 for c in table)


# ---- B, C. make_topoO ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def to_reference(name):
    I, O = tw.to_grids(name)
    return tw.to_walks(name, tw.to_six(I, O, tw.to_cases(name)[0]))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.mark.parametrize("name", list(tw.TO_GEOM))
def test_make_topoo_cases_do_what_their_names_say(name):
    I, O = tw.to_grids(name)
    (fg, zt, zs, fo, fl), land, table, oceans = tw.to_cases(name)
    walks, planes, counts, pow_cells = to_reference(name)
    assert not pow_cells.any()                      # so every plane is compared bit for bit
    mi, mj = I.im // O.im, I.jm // O.jm
    d = mr.make_dxyp(I.im, I.jm)
    assert len({(c.I, c.J) for c in table + oceans}) == len(table) + len(oceans)
    seen = 0
    for c in table:
        sl = tw.to_tile_slices(I, O, c.I, c.J)
        walk, o, FLAKE, FGRND = walks[(c.I, c.J)]
        assert planes["FOCEAN"][c.J - 1, c.I - 1] == 0 and walk[2] == c.n == int((fo[sl] == 0).sum()), c.name
        if "pole" not in c.tags:
            # outside FLAKE's zero bands, a 2 x 2 block without ocean: the lake survives and the planes are what callZ was given
            jb, ib = (c.J - 1) // 2 * 2, (c.I - 1) // 2 * 2
            assert 3 <= c.J <= 8 and not planes["FOCEAN"][jb:jb + 2, ib:ib + 2].any(), c.name
        # FLAKE is a multiple of 1 / 256 (the requested one on an all-land tile) unless :621 cut it to 1 - FGICE, leaving no ground
        reduced = FLAKE * 256 != int(FLAKE * 256)
        assert (FGRND == 0 and FLAKE < c.p / 256.) if reduced else (c.n < mi * mj or FLAKE == c.p / 256.), c.name
        for n in ("ZLAKE", "ZGRND", "ZATMO", "dZLAKE", "ZSGLO", "ZSGHI", "ZICETOP", "ZSOLDG", "ZATMOF"):
            assert bits(planes[n][c.J - 1, c.I - 1]) == bits(o[n]), (c.name, n)
        if c.walk is not None:
            assert walk[:2] == c.walk, (c.name, walk)
        # the regrid that feeds the GPU test need not round as regrid_nested does: the walks have room for that
        for eps in (-1e-9, 1e-9):
            o2 = mr.callZ_cell(fg[sl].tolist(), fo[sl].tolist(), zt[sl].tolist(), d[sl[0]], False, FLAKE + (eps if reduced else 0.),
                               FGRND if reduced else max(FGRND + eps, 0.))
            assert o2["_walk"] == walk, (c.name, eps)
        landmask = fo[sl].reshape(-1) == 0
        depth = zt[sl].reshape(-1)[landmask].astype(np.float64)
        area = np.repeat(np.asarray(d[sl[0]]), fo[sl].shape[1])[landmask]
        a, b, clamped, exceeded = tw.to_walk_detail(depth.tolist(), area.tolist(), FLAKE, FGRND)
        assert (a, b) == walk[:2], c.name
        if "clamp" in c.tags:
            assert clamped and FLAKE == 1 and walk[:2] == (c.n - 1, c.n - 1)
        else:
            assert not clamped, c.name
        if "ground_last_exceeded" in c.tags:
            assert exceeded and b == c.n - 1 and a < b
        if "ground_never" in c.tags:
            assert not exceeded and b == c.n - 1 and a < b
        if "ties" not in c.tags and "every_chunk" not in c.tags:
            assert len(set(depth.tolist())) == c.n, c.name
        seen += 1
    assert seen == len(table)                       # none left out
    W = [walks[(c.I, c.J)][0] for c in table]
    if name == "short":
        assert mi * mj == 256 and I.im * mj == 3072 <= topoo.MAX_TILE
        assert {w[0] for w in W} >= {0, 62, 63, 64, 65, 127, 128, 255}
        assert {w[1] for w in W} >= {63, 64, 65, 127, 128, 129, 191, 192, 193, 255}
        assert any(w[1] == w[0] for w in W) and any(w[1] == w[0] + 1 for w in W)
        assert {w[2] for w in W} >= {1, 2, 63, 64, 65, 128, 129, 255, 256}
        assert {t for c in table for t in c.tags} >= {"clamp", "ground_last_exceeded", "ground_never", "ties", "n", "steered"}
        assert sum(1 for c in table if -32768 in zt[tw.to_tile_slices(I, O, c.I, c.J)] and 32767 in zt[tw.to_tile_slices(I, O, c.I, c.J)]) >= 5
        one = [c for c in table if c.name == "all one depth"][0]
        two = [c for c in table if c.name == "two depths alternating"][0]
        assert len(np.unique(zt[tw.to_tile_slices(I, O, one.I, one.J)])) == 1 and len(np.unique(zt[tw.to_tile_slices(I, O, two.I, two.J)])) == 2
        # the ocean cells: the lowest ocean fine cell is alone, where the name says, and land lies below it
        assert sorted(c.lowest_at for c in oceans) == [0, 63, 64, 255, 3071]
        for c in oceans:
            sl = tw.to_tile_slices(I, O, c.I, c.J)
            f, z = fo[sl].reshape(-1), zt[sl].reshape(-1).astype(np.int64)
            assert planes["FOCEAN"][c.J - 1, c.I - 1] == 1 and f.size == c.ncell
            zo = np.where(f == 1, z, 1 << 20)
            assert int(zo.argmin()) == c.lowest_at and (zo == zo.min()).sum() == 1 and z[f == 0].min() < zo.min()
            assert planes["ZSGLO"][c.J - 1, c.I - 1] == zo.min() == -30000
    else:
        assert mi * mj == topoo.MAX_TILE + 1 and I.im * mj > topoo.MAX_TILE and O.im == 2
        assert {w[0] % 64 for w in W if w[0] > 64} >= {63, 0, 1} and {w[1] % 64 for w in W if w[1] > 64} >= {63, 0, 1}
        by = {t: c for c in table for t in c.tags}
        assert set(by) >= {"full", "one", "two", "last_chunk", "every_chunk", "n", "pole"}
        tile = lambda c: zt[tw.to_tile_slices(I, O, c.I, c.J)].reshape(-1).astype(np.int64)  # noqa: E731
        for c in table:
            if "full" in c.tags:            # every thread's 256 bins hold a cell, both extremes included
                z = tile(c) + 32768
                assert len(set((z // 256).tolist())) == 256 and z.min() == 0 and z.max() == 65535
        assert len(set(tile(by["one"]).tolist())) == 1
        z = tile(by["two"])
        assert all(sorted(np.unique(z[c0:c0 + 256], return_counts=True)[1].tolist()) == [128, 128] for c0 in range(0, 8192, 256))
        z = tile(by["last_chunk"])
        assert np.flatnonzero(z == z.min()).tolist() == [8192]
        z = tile(by["every_chunk"])
        assert [int((z[c0:c0 + 256] == 4242).sum()) for c0 in range(0, 8193, 256)] == [1] * 33
        assert len({int(np.flatnonzero(z[c0:c0 + 256] == 4242)[0]) for c0 in range(0, 8193, 256)}) > 8
        assert sorted(c.n for c in table if "n" in c.tags) == [257, 8000] and by["pole"].n == I.im * mj == 16386
