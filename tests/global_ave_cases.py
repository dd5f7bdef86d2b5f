"""The fixtures tests/test_global_ave_restatement.py (CPU) and tests/test_gpu_global_ave.py share: F1, two ice sheets on one
8 x 6 ocean grid under a 4 x 3 atmosphere, and F2, base (global) ice matrices on that ocean."""
import numpy as np

R = 6371000.
HC = [0., 1500., 3000.]
PATTERNS = ("zero", "om1", "om2", "om4", "frac", "op1")


def specs():
    from icebin_amd import HntrSpec
    return HntrSpec(8, 6, 0., 1800.), (HntrSpec(48, 36, 0.5, 300.), HntrSpec(24, 18, 0.25, 600.))


def masks():
    """Elevations of the two sheets: default_rng(11) / (12), 40 % NaN, and no ice at all under the northernmost row of O
    cells (so that the ocean has cells outside every sheet)."""
    O, Is = specs()
    out = []
    for seed, I in zip((11, 12), Is):
        rng = np.random.default_rng(seed)
        em = rng.uniform(0., 3000., I.size)
        em[rng.random(I.size) < 0.4] = np.nan
        em.reshape(I.jm, I.im)[I.jm - I.jm // O.jm:, :] = np.nan
        out.append(em)
    return out


def ice_cells(sheet_grids):
    """Per sheet, the O cells that carry unmasked ice (ascending)."""
    return [np.unique(np.asarray(g["ex_indices"]).reshape(-1, 2)[:, 0]).astype(np.int64) for g in sheet_grids]


def ocean(pattern, ice, O):
    """(foceanAOp, foceanAOm) of one pattern of tests/test_gpu_modele.py, on a parent whose four children all carry ice."""
    fp, fm = np.zeros(O.size), np.zeros(O.size)
    has = np.zeros(O.size, bool)
    has[ice] = True
    kids = None
    for ja in range(O.jm // 2):
        for ia in range(O.im // 2):
            k = [(2 * ja + dj) * O.im + 2 * ia + di for dj in (0, 1) for di in (0, 1)]
            if kids is None and all(has[k]):
                kids = k
    assert kids is not None
    rng = np.random.default_rng(5)
    if pattern in ("om1", "om2", "om4"):
        n = int(pattern[2])
        fm[kids[:n]] = 1.
        fp[kids[:n]] = 1.
    elif pattern == "frac":
        fp[ice] = rng.uniform(0.05, 0.95, len(ice))
    elif pattern == "op1":
        fp[kids[1]] = 1.
        fp[ice[::3]] = 1.
    return fp, fm, kids


def base(ice_all, kids, O, nhc_base=2):
    """F2: (hcdefs_base, (iE, iO, val), shape) with hcdefs_base = [1500, 4000] (1500 is also a local class) and, for nhc_base =
    72, seventy more distinct classes that one O cell carries all of.  About 20 entries in shuffled order: cells also under
    local ice (kids[0] among them, which the om* patterns make ModelE ocean), cells outside every sheet, one (iE, iO) pair
    twice.  Row keys are class-slowest: iE = iO + nO * ihc."""
    nO = O.size
    hc = [1500., 4000.] + [5000. + 10. * k for k in range(nhc_base - 2)]
    rng = np.random.default_rng(21)
    outside = np.setdiff1d(np.arange(nO), ice_all)
    assert len(outside) >= 4 and len(ice_all) >= 8
    cells = [int(kids[0]), int(kids[3])] + [int(c) for c in ice_all[::5][:6]] + [int(c) for c in outside[:4]]
    iO, ihc = [], []
    for c in cells:
        for h in ((0, 1) if c % 3 else (1,)):
            iO.append(c); ihc.append(h)
    iO.append(iO[2]); ihc.append(ihc[2])                # the duplicated pair
    if nhc_base > 2:
        for h in range(2, nhc_base):
            iO.append(int(kids[3])); ihc.append(h)
    iO, ihc = np.asarray(iO, np.int64), np.asarray(ihc, np.int64)
    val = rng.uniform(1e9, 5e10, len(iO))
    p = rng.permutation(len(iO))
    iO, ihc, val = iO[p], ihc[p], val[p]
    return np.asarray(hc), (iO + nO * ihc, iO, val), (nO * len(hc), nO)
