"""The fixtures tests/test_topo_restatement.py (CPU) and tests/test_gpu_topo.py share: T1, the two sheets of
tests/global_ave_cases.py on the 8 x 6 ocean with land masks that are supersets of the ice masks, and T2, one regional
sheet on a 16 x 12 ocean arranged so that cells cross foceanOp < 0.5, an interior single-cell ocean appears and an edge
candidate is skipped.  Everything here is made on the host: the exchange grids are the restated Hntr overlaps
(tests/modele_restatement.py: hntr_grids), and every sheet of a fixture lives on ONE ocean grid whose cells are all realised."""
import numpy as np

import global_ave_cases as gc
import modele_restatement as mr

R = gc.R
HC = gc.HC


def one_grid(O, I, em_land):
    """The oracle-layout arrays of one sheet whose exchange grid holds every cell of the LAND mask, on the full ocean grid."""
    from test_hntr_matrix import dxyp_restated
    g = mr.hntr_grids(O, I, em_land, HC, R)
    allO = np.arange(O.size, dtype=np.int64)
    nat = np.repeat(R * R * np.asarray(dxyp_restated(O.im, O.jm), np.float64), O.im)     # the areas Hntr's overlaps add up to
    g.update(A_to_sparse=allO, A_native_area=nat, A_proj_area=nat)
    return g


def planes(O, seed, ocean_cells=None):
    """The nine TOPOO planes merge_topoO reads, plus ZLAKE: ModelE ocean (foceanOm = 1: no land fractions) on ocean_cells (default:
    a random third), land elsewhere with fgice + flake + fgrnd = 1; foceanOp follows foceanOm except on a few coastal cells."""
    rng = np.random.default_rng(seed)
    n = O.size
    om = np.zeros(n)
    om[rng.random(n) < 0.35 if ocean_cells is None else ocean_cells] = 1.
    fgice = np.where(om == 1., 0., np.round(rng.uniform(0., 0.5, n), 3))
    flake = np.where(om == 1., 0., 0.125)
    fgrnd = np.where(om == 1., 0., 1.0 - fgice - flake)
    op = om.copy()
    coast = rng.random(n) < 0.3
    op[coast & (om == 1.)] = 0.75
    op[coast & (om == 0.)] = 0.25
    zatmo = np.where(om == 1., 0., rng.uniform(10., 900., n))
    return dict(foceanOp=op, fgiceOp=fgice * (1. - op), zatmoOp=zatmo * (1. - op), foceanOm=om, flakeOm=flake, fgrndOm=fgrnd, fgiceOm=fgice,
                zatmoOm=zatmo, zicetopO=np.where(fgice > 0, zatmo + 50., 0.), zlakeOm=np.where(flake > 0, 5., 0.))


def t1():
    """-> dict(O, Is, lands, ices, grids, planes)"""
    O, Is = gc.specs()
    ices = gc.masks()
    lands = []
    for seed, em in zip((31, 32), ices):
        rng = np.random.default_rng(seed)
        land = em.copy()
        bare = np.isnan(em) & (rng.random(len(em)) < 0.5)
        land[bare] = rng.uniform(-300., 3400., int(bare.sum()))
        I = Is[len(lands)]
        land.reshape(I.jm, I.im)[I.jm - I.jm // O.jm:, :] = np.nan      # no land either under the northernmost row of O cells
        lands.append(land)
    return dict(O=O, Is=Is, lands=lands, ices=ices, grids=[one_grid(O, I, em) for I, em in zip(Is, lands)], planes=planes(O, 41))


# T2: the 16 x 12 ocean, cells (i, j); the sheet covers i in 3..12, j in 3..9.  Of the 36 ice cells under an O cell the land
# mask keeps `cover`: FULL cells turn to land (foceanOp falls below 0.5), SOME cells stay ocean with foceanOp != 1.
T2_SINGLE = (6, 5)          # an interior ModelE ocean cell, lightly covered, whose four neighbours all become land
T2_EDGE = (0, 6)            # the same pattern on the western edge: the reference skips it
T2_PAIR = ((9, 7), (10, 7))  # two adjacent lightly covered ocean cells: neither qualifies


def t2():
    from icebin_amd import HntrSpec
    O, I = HntrSpec(16, 12, 0., 900.), HntrSpec(96, 72, 0., 150.)
    rng = np.random.default_rng(51)
    land = np.full(I.size, np.nan).reshape(I.jm, I.im)
    ocean_cells = np.zeros(O.size, bool)
    light = {T2_SINGLE, T2_EDGE} | set(T2_PAIR)
    for j in range(O.jm):
        for i in range(O.im):
            inside = 3 <= i <= 12 and 3 <= j <= 9
            blk = land[6 * j:6 * j + 6, 6 * i:6 * i + 6]
            if (i, j) in light:
                blk[0, :4] = rng.uniform(5., 400., 4)               # 4 of 36 ice cells: foceanOp = 1 - 1/9
                ocean_cells[j * O.im + i] = True
            elif inside or (i, j) in ((0, 5), (0, 7), (1, 6)):
                # FULL; the southern half below the second class (no ice in the third: a vertical ghost there)
                blk[:, :] = rng.uniform(100., 1400., (6, 6)) if j <= 5 else rng.uniform(-100., 2950., (6, 6))
                ocean_cells[j * O.im + i] = (i + j) % 2 == 0        # half of them ModelE ocean before the merge
            else:
                ocean_cells[j * O.im + i] = (i * 7 + j * 3) % 5 < 2
    # around T2_EDGE the neighbours are FULL ((0, 5), (0, 7), (1, 6)); make them ModelE ocean so that they convert
    for i, j in ((0, 5), (0, 7), (1, 6), (5, 5), (7, 5), (6, 4), (6, 6)):
        ocean_cells[j * O.im + i] = True
    for i, j in ((14, 4), (15, 4), (14, 5), (15, 5)):                 # an atmosphere cell over pure ocean, away from the sheet
        ocean_cells[j * O.im + i] = True
    land = land.reshape(-1)
    ice = land.copy()
    ice[(rng.random(I.size) < 0.4) | (land < 600.)] = np.nan         # ice on the higher land only: a subset of the land mask
    return dict(O=O, Is=(I,), lands=[land], ices=[ice], grids=[one_grid(O, I, land)], planes=planes(O, 52, ocean_cells))


def base(case, ice):
    """The base (global) ice EOpvAOp a fixture is merged with, (hcdefs_base, (iE, iO, val), shape): T1 takes F2 of
    tests/global_ave_cases.py, which also puts ice on the southernmost row; T2 keeps the base ice off both polar rows (classes
    1500 / 4000 on a few cells under the sheet and two outside it), so that no pole row holds a part of its cells' ice."""
    O = case["O"]
    ice = np.asarray(ice, np.int64)
    if len(case["Is"]) == 2:
        return gc.base(ice, gc.ocean("zero", ice, O)[2], O)
    nO = O.size
    cells = [int(c) for c in ice[::7][:8]] + [8 * O.im + 14, 9 * O.im + 1]
    iO = np.asarray([c for c in cells for _ in (0, 1)], np.int64)
    ihc = np.asarray([h for _ in cells for h in (0, 1)], np.int64)
    rng = np.random.default_rng(61)
    val = rng.uniform(1e9, 5e10, len(iO))
    p = rng.permutation(len(iO))
    iO, ihc, val = iO[p], ihc[p], val[p]
    return np.asarray([1500., 4000.]), (iO + nO * ihc, iO, val), (nO * 2, nO)


def native_area(case):
    return np.asarray(case["grids"][0]["A_native_area"], np.float64).tolist()


def oracle_sheets(orc, case, lands=None, ices=None):
    lands = case["lands"] if lands is None else lands
    ices = case["ices"] if ices is None else ices
    return [(orc.Regridder(g), el, ei) for g, el, ei in zip(case["grids"], lands, ices)]
