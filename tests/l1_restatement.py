"""The L1 path of icebin_amd/csrc/l1.hip restated in numpy, operation for operation: the polygon area, the basis integrals
of an exchange cell (k_l1_integrals) and the order the assembly sums in.  numpy rounds every + - * / on its own, like the
library's kernels (compiled without contraction), so the results agree in every bit.  Beside it: the same terms in exact
rational arithmetic from the same float inputs, a plain Sutherland-Hodgman that makes the fixtures' exchange polygons, and
the cases of tests/golden/l1_reference.npz (tests/golden/make_l1_reference.py writes it)."""
import os
from fractions import Fraction

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "l1_reference.npz")
CASES = ("four_tri_a1", "four_tri_a2", "jit9", "jit9_far", "jit24", "edges")


# ---- restatement -----------------------------------------------------------------------------------------------------------
def sort_cells(iA, iTri):
    """The permutation into (iA, iTri) order, ties in input order."""
    return np.lexsort((np.arange(len(iA)), iTri, iA))


def poly_areas(vptr, qx, qy):
    """l1_area: Cell::proj_area with the polygon's vertex 0 as the origin, summed from the edge (last, first) on."""
    out = np.zeros(len(vptr) - 1)
    for c in range(len(vptr) - 1):
        x, y = qx[vptr[c]:vptr[c + 1]] - qx[vptr[c]], qy[vptr[c]:vptr[c + 1]] - qy[vptr[c]]
        ret, x0, y0 = np.float64(0), x[-1], y[-1]
        for k in range(len(x)):
            ret = ret + ((x0 * y[k]) - (x[k] * y0))
            x0, y0 = x[k], y[k]
        out[c] = ret * .5
    return out


def _bary(ux, uy, e1x, e1y, e2x, e2y, det):
    l1 = (ux * e2y - uy * e2x) / det
    l2 = (e1x * uy - e1y * ux) / det
    return (1.0 - l1) - l2, l1, l2


def cell_terms(vx, vy, tri, iTri, vptr, qx, qy):
    """k_l1_integrals: [nX, 3] integrals of the element's three basis functions over each cell's polygon."""
    vx, vy, qx, qy = (np.asarray(a, np.float64) for a in (vx, vy, qx, qy))
    tri, vptr = np.asarray(tri).reshape(-1, 3), np.asarray(vptr)
    nX = len(iTri)
    t = tri[np.asarray(iTri)]
    x0, y0 = vx[t[:, 0]], vy[t[:, 0]]
    e1x, e1y, e2x, e2y = vx[t[:, 1]] - x0, vy[t[:, 1]] - y0, vx[t[:, 2]] - x0, vy[t[:, 2]] - y0
    det = e1x * e2y - e1y * e2x
    b, n = vptr[:-1], np.diff(vptr)
    ax, ay = qx[b] - x0, qy[b] - y0
    la = _bary(ax, ay, e1x, e1y, e2x, e2y, det)
    bx, by = qx[b + 1] - x0, qy[b + 1] - y0
    lb = _bary(bx, by, e1x, e1y, e2x, e2y, det)
    s = np.zeros((nX, 3))
    for i in range(2, int(n.max()) if nX else 0):
        m = n > i
        j = np.where(m, b + i, b)
        cx, cy = qx[j] - x0, qy[j] - y0
        lc = _bary(cx, cy, e1x, e1y, e2x, e2y, det)
        fa = 0.5 * ((bx - ax) * (cy - ay) - (by - ay) * (cx - ax))
        for k in range(3):
            term = fa * (((la[k] + lb[k]) + lc[k]) / 3.0)
            s[:, k] = np.where(m, term if i == 2 else s[:, k] + term, s[:, k])
        bx, by = np.where(m, cx, bx), np.where(m, cy, by)
        lb = tuple(np.where(m, lc[k], lb[k]) for k in range(3))
    return s


def triplets(tri, iA, iTri, terms, which="AvI"):
    """The stream the assembly receives: cell by cell, basis function by basis function."""
    tri = np.asarray(tri).reshape(-1, 3)
    a, v = np.repeat(np.asarray(iA, np.int64), 3), tri[np.asarray(iTri)].reshape(-1).astype(np.int64)
    return (a, v, terms.reshape(-1)) if which == "AvI" else (v, a, terms.reshape(-1))


def assemble(row, col, val, nrow, ncol):
    """setFromTriplets + the canonical weights: entries in (row, col) order, duplicates summed in stream order with the first
    term assigned; wM = row sums over ascending column, Mw = column sums over ascending row.  Returns rowptr, col, val, wM, Mw."""
    order = np.lexsort((np.arange(len(row)), col, row))
    r, c, v = row[order], col[order], val[order]
    orow, ocol, oval = [], [], []
    for k in range(len(r)):
        if orow and orow[-1] == r[k] and ocol[-1] == c[k]:
            oval[-1] = oval[-1] + v[k]
        else:
            orow.append(r[k]); ocol.append(c[k]); oval.append(v[k])
    orow, ocol, oval = np.asarray(orow, np.int64), np.asarray(ocol, np.int32), np.asarray(oval, np.float64)
    rowptr = np.zeros(nrow + 1, np.int32)
    np.add.at(rowptr, orow + 1, 1)
    rowptr = np.cumsum(rowptr).astype(np.int32)
    wM, Mw = np.zeros(nrow), np.zeros(ncol)
    seen_r, seen_c = np.zeros(nrow, bool), np.zeros(ncol, bool)
    for k in range(len(oval)):          # (row, col) order: ascending column inside a row, ascending row inside a column
        wM[orow[k]] = wM[orow[k]] + oval[k] if seen_r[orow[k]] else oval[k]
        Mw[ocol[k]] = Mw[ocol[k]] + oval[k] if seen_c[ocol[k]] else oval[k]
        seen_r[orow[k]] = seen_c[ocol[k]] = True
    return rowptr, ocol, oval, wM, Mw


def scale_rows(rowptr, val, wM):
    """M = diag(1/wM) M as scale_rows_recip (csrops.hip) does it: one reciprocal per row, one product per entry."""
    out = val.copy()
    for r in range(len(rowptr) - 1):
        if rowptr[r + 1] > rowptr[r]:
            out[rowptr[r]:rowptr[r + 1]] = val[rowptr[r]:rowptr[r + 1]] * (1. / wM[r])
    return out


# ---- exact arithmetic ----------------------------------------------------------------------------------------------------------
def exact_terms(vx, vy, tri, iTri, vptr, qx, qy):
    """The same integrals, the polygon areas and the element areas as Fractions of the float inputs."""
    tri = np.asarray(tri).reshape(-1, 3)
    F = Fraction
    terms, areas, elem = [], [], []
    for c in range(len(iTri)):
        p = [(F(float(vx[v])), F(float(vy[v]))) for v in tri[iTri[c]]]
        q = [(F(float(qx[k])), F(float(qy[k]))) for k in range(vptr[c], vptr[c + 1])]
        det = (p[1][0] - p[0][0]) * (p[2][1] - p[0][1]) - (p[1][1] - p[0][1]) * (p[2][0] - p[0][0])

        def lam(pt):
            ux, uy = pt[0] - p[0][0], pt[1] - p[0][1]
            l1 = (ux * (p[2][1] - p[0][1]) - uy * (p[2][0] - p[0][0])) / det
            l2 = ((p[1][0] - p[0][0]) * uy - (p[1][1] - p[0][1]) * ux) / det
            return (1 - l1 - l2, l1, l2)
        s, area = [F(0)] * 3, F(0)
        for i in range(2, len(q)):
            fa = ((q[i - 1][0] - q[0][0]) * (q[i][1] - q[0][1]) - (q[i - 1][1] - q[0][1]) * (q[i][0] - q[0][0])) / 2
            ls = [lam(q[0]), lam(q[i - 1]), lam(q[i])]
            for k in range(3):
                s[k] += fa * (ls[0][k] + ls[1][k] + ls[2][k]) / 3
            area += fa
        terms.append(s); areas.append(area); elem.append(det / 2)
    return terms, areas, elem


def max_err_over(values, exact, scale):
    """max over cells and basis functions of |value - exact| / scale[cell], in exact arithmetic, as a float."""
    worst = Fraction(0)
    for c in range(len(exact)):
        for k in range(3):
            worst = max(worst, abs(Fraction(float(values[c][k])) - exact[c][k]) / scale[c])
    return float(worst)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
def clip_triangle(p, poly):
    """Sutherland-Hodgman: triangle p ([3, 2]) against the half-planes of the convex counter-clockwise polygon."""
    s = [tuple(map(float, v)) for v in p]
    for e in range(len(poly)):
        a, b = poly[e], poly[(e + 1) % len(poly)]
        d = [(b[0] - a[0]) * (v[1] - a[1]) - (b[1] - a[1]) * (v[0] - a[0]) for v in s]
        out = []
        for k in range(len(s)):
            kn = (k + 1) % len(s)
            if d[k] >= 0:
                out.append(s[k])
            if (d[k] >= 0) != (d[kn] >= 0):
                t = d[k] / (d[k] - d[kn])
                out.append((s[k][0] + t * (s[kn][0] - s[k][0]), s[k][1] + t * (s[kn][1] - s[k][1])))
        s = out
        if not s:
            break
    return s


def make_exgrid(vx, vy, tri, polys, iA):
    """Exchange cells of positive area, triangle by triangle (so NOT in (iA, iTri) order): iA, iTri, vptr, qx, qy."""
    oA, oT, vptr, q = [], [], [0], []
    for t, el in enumerate(np.asarray(tri).reshape(-1, 3)):
        p = [(vx[v], vy[v]) for v in el]
        for n, poly in enumerate(polys):
            s = clip_triangle(p, poly)
            if len(s) < 3:
                continue
            area = sum((s[k][0] - s[0][0]) * (s[(k + 1) % len(s)][1] - s[0][1]) - (s[(k + 1) % len(s)][0] - s[0][0]) * (s[k][1] - s[0][1])
                       for k in range(len(s))) / 2
            if area > 0:
                oA.append(iA[n]); oT.append(t); q += s; vptr.append(len(q))
    q = np.asarray(q, np.float64).reshape(-1, 2)
    return (np.asarray(oA, np.int32), np.asarray(oT, np.int32), np.asarray(vptr, np.int32), np.ascontiguousarray(q[:, 0]),
            np.ascontiguousarray(q[:, 1]))


def square_cells(xe, ye):
    """Cells of a rectilinear grid as counter-clockwise squares, iA = iy * nx + ix."""
    polys = []
    for iy in range(len(ye) - 1):
        for ix in range(len(xe) - 1):
            polys.append(np.array([(xe[ix], ye[iy]), (xe[ix + 1], ye[iy]), (xe[ix + 1], ye[iy + 1]), (xe[ix], ye[iy + 1])], float))
    return polys


def jittered_mesh(n, lo, hi, seed):
    """n x n vertices on linspace(lo, hi, n)^2, each moved by U(-0.3, 0.3) h; two counter-clockwise triangles per quad."""
    g = np.linspace(lo, hi, n)
    h = g[1] - g[0]
    j = np.random.default_rng(seed).uniform(-0.3, 0.3, (n, n, 2)) * h
    x, y = np.meshgrid(g, g)            # [iy, ix]
    vx, vy = (x + j[..., 0]).reshape(-1), (y + j[..., 1]).reshape(-1)
    tri = []
    for iy in range(n - 1):
        for ix in range(n - 1):
            v00, v10, v01, v11 = iy * n + ix, iy * n + ix + 1, (iy + 1) * n + ix, (iy + 1) * n + ix + 1
            tri += [(v00, v10, v11), (v00, v11, v01)]
    return vx, vy, np.asarray(tri, np.int32)


def build_cases():
    """name -> dict(vx, vy, tri, polyptr, px, py, iA_poly, nA): the meshes and the GCM cells of the fixture."""
    cases = {}

    def add(name, vx, vy, tri, polys, iA, nA):
        polyptr = np.zeros(len(polys) + 1, np.int32)
        polyptr[1:] = np.cumsum([len(p) for p in polys])
        v = np.concatenate([np.asarray(p, float) for p in polys])
        cases[name] = dict(vx=np.asarray(vx, float), vy=np.asarray(vy, float), tri=np.asarray(tri, np.int32).reshape(-1, 3),
                           polyptr=polyptr, px=np.ascontiguousarray(v[:, 0]), py=np.ascontiguousarray(v[:, 1]),
                           iA_poly=np.asarray(iA, np.int64), nA=np.int64(nA))
    # the reference's own test mesh (pylib/icebin/tests/test_regrid_l1.py): one cell over everything, then two cells
    fx, fy = [-1., 1., 1., -1., 0.], [-1., -1., 1., 1., 0.]
    ft = [(0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 0, 4)]
    add("four_tri_a1", fx, fy, ft, square_cells([-2., 2.], [-2., 2.]), [0], 1)
    add("four_tri_a2", fx, fy, ft, square_cells([-2., 0., 2.], [-2., 2.]), [0, 1], 2)
    vx, vy, tri = jittered_mesh(9, -8., 8., 20240501)
    cells = square_cells(np.linspace(-10, 10, 5), np.linspace(-10, 10, 5))
    add("jit9", vx, vy, tri, cells, np.arange(16), 16)
    add("jit9_far", vx * 1000 - 6e5, vy * 1000 - 2e6, tri, [c * 1000 + np.array([-6e5, -2e6]) for c in cells], np.arange(16), 16)
    vx, vy, tri = jittered_mesh(24, -8., 8., 20240502)
    add("jit24", vx, vy, tri, square_cells(np.linspace(-10, 10, 6), np.linspace(-10, 10, 6)), np.arange(25), 25)
    # edges: 2 x 2 cells on [0, 4]^2 (iA 0..3) and a cell no triangle touches (iA 5; 4 is not realised).  Elements: inside
    # cell 0; over the four-cell corner (2, 2); a vertex exactly on the edge x = 2; an edge along y = 2; outside every cell
    ex = [.5, 1.5, 1., 1.5, 2.75, 1.75, 2., 3., 3., 2.5, 3.5, 3., 6., 7., 6.]
    ey = [.5, .5, 1.5, 1.5, 1.75, 2.75, .5, .25, 1., 2., 2., 3., 6., 6., 7.]
    cells = square_cells([0., 2., 4.], [0., 2., 4.]) + [np.array([(10., 0.), (12., 0.), (12., 2.), (10., 2.)])]
    add("edges", ex, ey, np.arange(15).reshape(5, 3), cells, [0, 1, 2, 3, 5], 7)
    return cases


def load_case(name):
    """One case of the golden file as a dict (keys without the case prefix)."""
    d = np.load(GOLDEN)
    pre = name + "/"
    return {k[len(pre):]: d[k] for k in d.files if k.startswith(pre)}


def polys_of(c):
    return [np.stack([c["px"][c["polyptr"][k]:c["polyptr"][k + 1]], c["py"][c["polyptr"][k]:c["polyptr"][k + 1]]], 1)
            for k in range(len(c["polyptr"]) - 1)]
