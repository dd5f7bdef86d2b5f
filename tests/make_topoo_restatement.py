"""Plain-loop restatement of _make_topoO (slib/icebin/modele/topo_base.cpp:263-809) and callZ (:20-221), with the grids as arguments
and the six regridded planes handed in (the regrid itself is Hntr's and is tested there).  Indices are the reference's, 1-based;
planes are numpy [jm, im], so the reference's A(I, J) is a[J - 1][I - 1].  Python floats are IEEE doubles and every operation below
is written once, in the reference's order, so the results are the reference's bits for one admissible order of its std::sort: ties
in depth keep traversal order here (the reference's comparator looks at the depth alone, :117-118)."""
import math

import numpy as np

PLANES = ("FOCEAN", "FLAKE", "FGRND", "FGICE", "FGICE_greenland", "ZATMO", "dZOCEN", "dZLAKE", "dZGICE", "ZSOLDG", "ZICETOP", "ZLAND_MIN",
          "ZLAND_MAX", "ZSGLO", "ZLAKE", "ZGRND", "ZSGHI", "FOCEANF", "FGICEF", "ZATMOF")
COUNTS = ("FGICE_low", "FGICE_high", "FLAKE_reduced", "FGRND_range", "dZOCEN_nonpositive", "FLAKE_one")


class Fatal(Exception):
    """icebin_error(-1, ...) of :85 / :146: kind 'ocean' or 'continental', the cell (I, J) 1-based."""

    def __init__(self, kind, I, J):
        super().__init__("%s (%d, %d)" % (kind, I, J))
        self.kind, self.I, self.J = kind, I, J


def make_dxyp(im, jm):
    """make_dxyp (hntr.cpp:33-52); index j - 1 holds dxyp(j)."""
    dLON, dLAT = 2. * math.pi / im, math.pi / jm
    return [dLON * (math.sin(dLAT * (j - jm // 2)) - math.sin(dLAT * (j - jm // 2 - 1))) for j in range(1, jm + 1)]


def std_round(x):
    """std::round: to the nearest integer, halves away from zero (numpy and Python round halves to even)."""
    frac, whole = math.modf(x)          # both carry x's sign; x - whole is exact
    if abs(frac) >= .5:
        whole += math.copysign(1., x)
    return whole


def _div(a, b):
    """a / b as C does it: inf and NaN instead of an exception"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def wedge_imax(IM, JM, J):
    """the upper I of the Greenland wedge (:584), (int)(.5 + .75*IM*(J-JM*.3)/JM)"""
    return int(.5 + .75 * IM * (J - JM * .3) / JM)


def callZ_cell(fgice, focean, zicetop, area_rows, is_ocean, FLAKE, FGRND):
    """One (I, J) of :69-206.  fgice / focean / zicetop: the tile's fine cells as lists of rows; area_rows[r]: dxyp(J1m) of tile
    row r.  Returns the dict of the planes the cell gets (ZSOLDG only for a continental cell), or raises Fatal's kind as a str."""
    o = {}
    if is_ocean:
        o.update(ZATMO=0., dZLAKE=0., ZLAKE=0., ZGRND=0., ZSGHI=0., ZICETOP=0.)
        ZSGLO = 999999.
        for r in range(len(zicetop)):               # :78-83
            for c in range(len(zicetop[r])):
                if ZSGLO > zicetop[r][c] and focean[r][c] == 1:
                    ZSGLO = float(zicetop[r][c])
        if ZSGLO == 999999.:
            raise ValueError("ocean")
        o["ZSGLO"] = ZSGLO
        SAREA = SAZSG = SAREA_li = SAZSG_li = 0.
        for r in range(len(zicetop)):               # :96-108
            area = area_rows[r]
            for c in range(len(zicetop[r])):
                SAREA += area
                if focean[r][c] == 1:
                    continue
                SAZSG += area * zicetop[r][c]
                if fgice[r][c] != 0:
                    SAREA_li += area
                    SAZSG_li += area * zicetop[r][c]
        o["ZICETOP"] = SAZSG_li / SAREA_li if SAREA_li > 0 else 0.
        o["ZATMOF"] = SAZSG / SAREA
        return o
    cells2 = []                                     # (area, depth), :123-142
    SAREA = SAZSG = SAREA_li = SAZSG_li = 0.
    for r in range(len(zicetop)):
        area = area_rows[r]
        for c in range(len(zicetop[r])):
            if focean[r][c] == 1:
                continue
            cells2.append((area, float(zicetop[r][c])))
            SAREA += area
            SAZSG += area * zicetop[r][c]
            if fgice[r][c] != 0:
                SAREA_li += area
                SAZSG_li += area * zicetop[r][c]
    if SAREA == 0:
        raise ValueError("continental")
    o["ZATMOF"] = SAZSG / SAREA
    cells2.sort(key=lambda ad: ad[1])               # :144; Python's sort is stable: ties keep traversal order
    o["ZSOLDG"] = SAZSG / SAREA
    o["ZICETOP"] = SAZSG_li / SAREA_li if SAREA_li > 0 else 0.
    o["ZSGLO"] = cells2[0][1]
    ANSUM = VNSUM = 0.
    NLAKE = 0
    while True:                                     # :164-172
        if NLAKE == len(cells2):
            NLAKE -= 1
            break
        ANSUM += cells2[NLAKE][0]
        VNSUM += cells2[NLAKE][0] * cells2[NLAKE][1]
        if ANSUM > SAREA * FLAKE:
            break
        NLAKE += 1
    o["ZLAKE"] = cells2[NLAKE][1]
    if FLAKE > 0:                                   # :176-182
        ZLBOT = (VNSUM - (ANSUM - SAREA * FLAKE) * cells2[NLAKE][1]) / (SAREA * FLAKE)
        o["dZLAKE"] = max(cells2[NLAKE][1] - ZLBOT, 1.0)
    else:
        o["dZLAKE"] = 0.
    AZATMO = ANSUM * o["ZLAKE"]                     # :185-189
    for N in range(NLAKE + 1, len(cells2)):
        AZATMO += cells2[N][0] * cells2[N][1]
    o["ZATMO"] = AZATMO / SAREA
    ANSUM -= cells2[NLAKE][0]                       # :192-203
    NGRND = NLAKE
    while True:
        if NGRND == len(cells2):
            NGRND -= 1
            break
        ANSUM += cells2[NGRND][0]
        if ANSUM > SAREA * (FLAKE + FGRND):
            break
        NGRND += 1
    o["ZGRND"] = cells2[NGRND][1]
    o["ZSGHI"] = cells2[-1][1]
    o["_walk"] = (NLAKE, NGRND, len(cells2))        # for the tests that pin where the walks end
    return o


def make_topoO(imI, jmI, imO, jmO, FGICE1m, ZICETOP1m, ZSOLG1m, FOCEAN1m, FOCEANF, FGICEF, FLAKE_regrid, dZOCEN_regrid, zictop, zsolg,
               set_to_land=(), set_to_ocean=(), resets=(), real=float, only_dzgice=False):
    """_make_topoO from its six regridded planes ([jmO, imO] float64: :392, :399, :575, :646, :661, :663).  set_to_land /
    set_to_ocean: 1-based (i, j); resets: (elev, [(i, j), ...]).  real: the type step 4's pow and chains are evaluated in (float:
    the reference's doubles; numpy.longdouble: the yardstick for the cells filled through pow).  Returns (planes, counts,
    pow_cells): dict name -> float64 [jmO, imO] (dZGICE of dtype `real`), dict of COUNTS, bool [jmO, imO] of the cells filled at
    :708.  only_dzgice: stop after :711 (dZGICE and the planes before it are final, the rest 0).  Raises Fatal for the first
    cell of :85 / :146."""
    IM, JM = imO, jmO
    assert imI % IM == 0 and jmI % JM == 0 and IM % 2 == 0 and JM % 2 == 0
    out = {n: [[0.] * IM for _ in range(JM)] for n in PLANES}
    cnt = dict.fromkeys(COUNTS, 0)
    FOCEAN, FLAKE, FGRND, FGICE, dZOCEN = out["FOCEAN"], out["FLAKE"], out["FGRND"], out["FGICE"], out["dZOCEN"]
    out["FOCEANF"] = np.asarray(FOCEANF, np.float64).reshape(JM, IM).tolist()
    out["FGICEF"] = np.asarray(FGICEF, np.float64).reshape(JM, IM).tolist()
    FOCEANF, FGICEF = out["FOCEANF"], out["FGICEF"]
    out["FLAKE"] = FLAKE = np.asarray(FLAKE_regrid, np.float64).reshape(JM, IM).tolist()
    out["dZOCEN"] = dZOCEN = np.asarray(dZOCEN_regrid, np.float64).reshape(JM, IM).tolist()
    zictop = np.asarray(zictop, np.float64).reshape(JM, IM).tolist()
    zsolg = np.asarray(zsolg, np.float64).reshape(JM, IM).tolist()
    TO_OCEAN, TO_LAND = 1, 2
    SET_TO = [[0] * IM for _ in range(JM)]
    for i, j in set_to_land:                        # :416-446
        SET_TO[j - 1][i - 1] = TO_LAND
    for i, j in set_to_ocean:                       # :449-494
        SET_TO[j - 1][i - 1] = TO_OCEAN
    for i in range(1, IM + 1):                      # :498-502
        FOCEAN[0][i - 1] = 0.
        FGICE[0][i - 1] = 1.
        FGICEF[0][i - 1] = 1.
    for j in range(2, JM + 1):                      # :506-531
        for i in range(1, IM + 1):
            foceanf = FOCEANF[j - 1][i - 1]
            s = SET_TO[j - 1][i - 1]
            to_ocean = True if s == TO_OCEAN else False if s == TO_LAND else foceanf >= .5
            if to_ocean:
                FOCEAN[j - 1][i - 1] = 1.
                FGICE[j - 1][i - 1] = 0.
            else:
                fact = _div(1., 1. - foceanf)
                FOCEAN[j - 1][i - 1] = 0.
                FGICE[j - 1][i - 1] = FGICEF[j - 1][i - 1] * fact
    for J in range(1, JM + 1):                      # :578-580
        for I in range(1, IM + 1):
            if J <= JM // 6 or J >= JM * 14 // 15 + 1 or (I <= IM // 2 and J >= JM * 41 // 45 + 1):
                FLAKE[J - 1][I - 1] = 0.
    for J in range((JM * 5) // 6, (JM * 11) // 12 + 1):     # :583-586
        for I in range(IM // 3 + 1, wedge_imax(IM, JM, J) + 1):
            FLAKE[J - 1][I - 1] = 0.
    for j in range(1, JM + 1):                      # :589-600
        for i in range(1, IM + 1):
            fcont = 1. - FOCEAN[j - 1][i - 1]
            fcontf = 1. - FOCEANF[j - 1][i - 1]
            if fcontf != 0.:
                v = FLAKE[j - 1][i - 1] * fcont / (fcontf + 1e-20)
                FLAKE[j - 1][i - 1] = std_round(v * 256.) / 256.
    for J in range(JM // 6 + 1, JM + 1):            # :608-623
        for I in range(1, IM + 1):
            if FGICE[J - 1][I - 1] < 0:
                cnt["FGICE_low"] += 1
                FGICE[J - 1][I - 1] = 0.
            if FGICE[J - 1][I - 1] > 1:
                cnt["FGICE_high"] += 1
                FGICE[J - 1][I - 1] = 1.
            if FLAKE[J - 1][I - 1] + FGICE[J - 1][I - 1] + FOCEAN[J - 1][I - 1] > 1:
                cnt["FLAKE_reduced"] += 1
                FLAKE[J - 1][I - 1] = 1. - FGICE[J - 1][I - 1] - FOCEAN[J - 1][I - 1]
    for j in range(1, JM + 1):                      # :633-641
        for i in range(1, IM + 1):
            v = 1.0 - FOCEAN[j - 1][i - 1] - FLAKE[j - 1][i - 1] - FGICE[j - 1][i - 1]
            if abs(v) < 1.e-14:
                v = 0.
            if v < 0 or v > 1:
                cnt["FGRND_range"] += 1
            FGRND[j - 1][i - 1] = v
    for j in range(1, JM + 1):                      # :647-655
        for i in range(1, IM + 1):
            dZOCEN[j - 1][i - 1] = -dZOCEN[j - 1][i - 1] * FOCEAN[j - 1][i - 1]
            if FOCEAN[j - 1][i - 1] == 1 and dZOCEN[j - 1][i - 1] <= 0:
                cnt["dZOCEN_nonpositive"] += 1
    # :671-711
    dxypO = make_dxyp(IM, JM)
    R = real
    dZGICE = [[R(0.)] * IM for _ in range(JM)]
    RGICE = [[None] * IM for _ in range(JM)]
    pow_cells = np.zeros((JM, IM), bool)
    SUMDFR = SUMDF = R(0.)
    for J in range(1, JM + 1):
        sum_dfr = sum_df = R(0.)
        for I in range(1, IM + 1):
            dzgice = zictop[J - 1][I - 1] - zsolg[J - 1][I - 1]
            if dzgice != 0:
                dZGICE[J - 1][I - 1] = R(dzgice)
            else:
                fcont = 1. - FOCEAN[J - 1][I - 1]
                RGICE[J - 1][I - 1] = FGICE[J - 1][I - 1] / (fcont + 1e-20)
                sum_dfr += R(FGICE[J - 1][I - 1]) * _pow(R, RGICE[J - 1][I - 1])
                sum_df += R(FGICE[J - 1][I - 1])
        SUMDFR += R(dxypO[J - 1]) * sum_dfr
        SUMDF += R(dxypO[J - 1]) * sum_df
    with np.errstate(all="ignore"):
        CONSTK = R(264.7) * SUMDF / SUMDFR if R is not float else _div(264.7 * SUMDF, SUMDFR)
    for J in range(1, JM + 1):
        for I in range(1, IM + 1):
            if FGICE[J - 1][I - 1] == 0:
                dZGICE[J - 1][I - 1] = R(0.)
            elif dZGICE[J - 1][I - 1] == 0:
                dZGICE[J - 1][I - 1] = CONSTK * _pow(R, RGICE[J - 1][I - 1])
                pow_cells[J - 1, I - 1] = True
    out["dZGICE"] = dZGICE
    if only_dzgice:
        return {n: np.asarray(out[n], np.float64 if n != "dZGICE" or R is float else R) for n in PLANES}, cnt, pow_cells
    # :723-728
    ZSOLDG = out["ZSOLDG"]
    for j in range(JM):
        for i in range(IM):
            ZSOLDG[j][i] = -dZOCEN[j][i]
    dxypI = make_dxyp(imI, jmI)
    fg1, fo1, zt1 = (np.asarray(a).reshape(jmI, imI) for a in (FGICE1m, FOCEAN1m, ZICETOP1m))
    Z8 = ("ZATMO", "dZLAKE", "ZSOLDG", "ZICETOP", "ZSGLO", "ZLAKE", "ZGRND", "ZSGHI")
    for J in range(1, JM + 1):                      # :61-220
        J11, J1M = (J - 1) * jmI // JM + 1, J * jmI // JM
        IMAX = 1 if J == 1 or J == JM else IM
        for I in range(1, IMAX + 1):
            I11 = (I - 1) * imI // IM + 1
            I1M = imI if IMAX == 1 else I * imI // IM
            sl = (slice(J11 - 1, J1M), slice(I11 - 1, I1M))
            try:
                o = callZ_cell(fg1[sl].tolist(), fo1[sl].tolist(), zt1[sl].tolist(), dxypI[J11 - 1:J1M], FOCEAN[J - 1][I - 1] != 0,
                               FLAKE[J - 1][I - 1], FGRND[J - 1][I - 1])
            except ValueError as e:
                raise Fatal(str(e), I, J) from None
            for n, v in o.items():
                if n != "_walk":
                    out[n][J - 1][I - 1] = v
        if J == 1 or J == JM:                       # :210-219
            for n in Z8:
                for i in range(2, IM + 1):
                    out[n][J - 1][i - 1] = out[n][J - 1][0]
    for elev, ijs in resets:                        # :747-758
        for i, j in ijs:
            out["dZLAKE"][j - 1][i - 1] += (elev - out["ZLAKE"][j - 1][i - 1])
            out["ZATMO"][j - 1][i - 1] = float(elev)
            out["ZLAKE"][j - 1][i - 1] = float(elev)
    for J in range(1, JM + 1):                      # :761-767
        for I in range(1, IM + 1):
            if FLAKE[J - 1][I - 1] == 1:
                cnt["FLAKE_one"] += 1
    for jb in range(JM // 2):                       # :774-795
        for ib in range(IM // 2):
            foceanb = 0.
            for j in range(jb * 2, jb * 2 + 2):
                for i in range(ib * 2, ib * 2 + 2):
                    foceanb += FOCEAN[j][i]
            if foceanb > 0:
                for j in range(jb * 2, jb * 2 + 2):
                    for i in range(ib * 2, ib * 2 + 2):
                        if FLAKE[j][i] > 0:
                            FGRND[j][i] += FLAKE[j][i]
                            FLAKE[j][i] = 0.
                            out["dZLAKE"][j][i] = 0.
    planes = {n: np.asarray(out[n], np.float64 if n != "dZGICE" or R is float else R) for n in PLANES}
    return planes, cnt, pow_cells


def _pow(R, x):
    """std::pow(x, .3) in R; .3 is the double nearest to 0.3, as in the source"""
    if R is float:
        return math.pow(x, .3)
    with np.errstate(all="ignore"):
        return np.power(R(x), R(.3))
