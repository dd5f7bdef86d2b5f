"""Cases that walk the two Sutherland-Hodgman clippers (icebin_amd/csrc/gridgen.hip: k_gg_clip, k_gg_clip_stream;
icebin_amd/csrc/l1.hip: k_l1_clip) to their vertex-count, bin and lane limits, with an exact reference and a vertex counter.
No tests and no GPU here: tests/test_clipper_cases.py checks on the CPU that the cases reach what they claim, and
tests/test_gpu_clippers.py runs them on the device.

  * the exact clipper: Sutherland-Hodgman in Fractions of the float inputs.  The subject may be concave, the clip region is
    convex; used both ways round -- an ice cell's rectangle clips a GCM polygon, and a triangle's three edges clip a GCM polygon.
  * the counter: clip_axis and l1_clip_edge restated in plain floats (each operation rounds on its own, as the kernels' do),
    returning the vertex count after every half-plane -- without the kernels' array limits, so it says what a case NEEDS.
  * l1_bins / l1_bin_range: the uniform-bin candidate search of l1.hip restated, and l1_turns: the refusal bound of
    l1_exgrid_generate restated.
"""
import functools
import math
from fractions import Fraction as F

import numpy as np

GG_MAXV, GG_CLIPV = 16, 20
L1_MAXV, L1_CLIPV, L1_LANES = 16, 19, 64
EPS = 2.0 ** -52
L1_TURN_FACTOR = 16.0


# ---- the exact clipper -----------------------------------------------------------------------------------------------------
def _frac(poly):
    return [(F(float(x)), F(float(y))) for x, y in np.asarray(poly, np.float64).reshape(-1, 2).tolist()]


def _clip_half(poly, d):
    """The part of poly (list of Fraction pairs) where the linear function is >= 0; d: its values at the vertices."""
    out, n = [], len(poly)
    for k in range(n):
        kn = (k + 1) % n
        if d[k] >= 0:
            out.append(poly[k])
        if (d[k] >= 0) != (d[kn] >= 0):
            t = d[k] / (d[k] - d[kn])
            a, b = poly[k], poly[kn]
            out.append((a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1])))
    return out


def _area(poly):
    return sum(poly[k - 1][0] * poly[k][1] - poly[k][0] * poly[k - 1][1] for k in range(len(poly))) / 2 if len(poly) >= 3 else F(0)


def _distinct(poly):
    """Vertices that differ from their predecessor round the cycle."""
    return [p for k, p in enumerate(poly) if p != poly[k - 1]] if len(poly) > 1 else list(poly)


def exact_clip_rect(poly, x0, x1, y0, y1):
    """Subject polygon (Fractions) inside [x0, x1] x [y0, y1]: the clipped polygon."""
    for axis, bound, lower in ((0, F(float(x0)), True), (0, F(float(x1)), False), (1, F(float(y0)), True), (1, F(float(y1)), False)):
        poly = _clip_half(poly, [(p[axis] - bound) if lower else (bound - p[axis]) for p in poly])
        if not poly:
            break
    return poly


def exact_clip_triangle(poly, tri):
    """Subject polygon (Fractions) inside the counter-clockwise triangle tri (three Fraction pairs)."""
    for e in range(3):
        a, b = tri[e], tri[(e + 1) % 3]
        poly = _clip_half(poly, [(b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0]) for p in poly])
        if not poly:
            break
    return poly


def cell_range(e, lo, hi):
    """gridgen.hip's cell_range: the cells of edges e whose open interior can meet (lo, hi) -> (first, count)."""
    n = len(e) - 1
    k0 = max(int(np.searchsorted(e, lo, side="right")) - 1, 0)
    k1 = min(int(np.searchsorted(e, hi, side="left")), n)
    return k0, max(k1 - k0, 0)


def exact_gridgen_poly(xe, ye, poly):
    """[(ix, iy, exact area as a float)] of one GCM polygon over the ice grid, areas > 0 only.  Bounding-box reject: only the
    cells the polygon's box reaches are clipped (every other overlap is empty)."""
    P = np.asarray(poly, np.float64).reshape(-1, 2)
    fp = _frac(P)
    ix0, nxr = cell_range(xe, P[:, 0].min(), P[:, 0].max())
    iy0, nyr = cell_range(ye, P[:, 1].min(), P[:, 1].max())
    out = []
    for ix in range(ix0, ix0 + nxr):
        for iy in range(iy0, iy0 + nyr):
            a = _area(exact_clip_rect(fp, xe[ix], xe[ix + 1], ye[iy], ye[iy + 1]))
            if a > 0:
                out.append((ix, iy, float(a)))
    return out


def assemble_gridgen(xe, ye, per_poly, iA, x_fastest):
    """(keys [(iA, iI)], areas) in (iA, iI) order from exact_gridgen_poly's lists."""
    nx, ny = len(xe) - 1, len(ye) - 1
    rec = sorted((int(a), iy * nx + ix if x_fastest else ix * ny + iy, area) for a, cells in zip(iA, per_poly) for ix, iy, area in cells)
    return [(r[0], r[1]) for r in rec], np.array([r[2] for r in rec], np.float64)


def exact_gridgen(xe, ye, polys, iA, x_fastest=False):
    xe, ye = np.asarray(xe, np.float64), np.asarray(ye, np.float64)
    return assemble_gridgen(xe, ye, [exact_gridgen_poly(xe, ye, p) for p in polys], iA, x_fastest)


def exact_l1(vx, vy, tri, polys, iA):
    """{(iA, iTri): (exact area as a float, distinct vertices of the piece, its perimeter)} for a mesh under GCM polygons,
    areas > 0 only: the polygon is the subject and the element's three edges clip it.  Bounding-box reject first."""
    vx, vy = np.asarray(vx, np.float64), np.asarray(vy, np.float64)
    P = [np.asarray(p, np.float64).reshape(-1, 2) for p in polys]
    box = np.array([(p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max()) for p in P])
    fp = [None] * len(P)
    out = {}
    for t, el in enumerate(np.asarray(tri).reshape(-1, 3)):
        tx, ty = vx[el], vy[el]
        near = np.nonzero((box[:, 2] >= tx.min()) & (box[:, 0] <= tx.max()) & (box[:, 3] >= ty.min()) & (box[:, 1] <= ty.max()))[0]
        T = [(F(float(tx[k])), F(float(ty[k]))) for k in range(3)]
        for n in near:
            if fp[n] is None:
                fp[n] = _frac(P[n])
            s = exact_clip_triangle(fp[n], T)
            a = _area(s)
            if a > 0:
                s = _distinct(s)
                per = sum(math.hypot(float(s[k][0] - s[k - 1][0]), float(s[k][1] - s[k - 1][1])) for k in range(len(s)))
                out[(int(iA[n]), t)] = (float(a), len(s), per)
    return out


# ---- the counter -----------------------------------------------------------------------------------------------------------
def gg_clip_axis(pts, axis, bound, lower):
    """gridgen.hip's clip_axis in floats, without the arrays."""
    out, n = [], len(pts)
    for k in range(n):
        a, b = pts[k], pts[(k + 1) % n]
        ca, cb = a[axis], b[axis]
        ina, inb = (ca >= bound, cb >= bound) if lower else (ca <= bound, cb <= bound)
        if ina:
            out.append(a)
        if ina != inb:
            t = (bound - ca) / (cb - ca)
            out.append((a[0] + t * (b[0] - a[0]), bound) if axis else (bound, a[1] + t * (b[1] - a[1])))
    return out


def gg_counts(poly, x0, x1, y0, y1):
    """([n, after x >= x0, after x <= x1, after y >= y0, after y <= y1], area as k_gg_clip sums it)."""
    pts = [(float(x), float(y)) for x, y in np.asarray(poly, np.float64).reshape(-1, 2).tolist()]
    counts = [len(pts)]
    for axis, bound, lower in ((0, float(x0), True), (0, float(x1), False), (1, float(y0), True), (1, float(y1), False)):
        pts = gg_clip_axis(pts, axis, bound, lower)
        counts.append(len(pts))
    ret = 0.0
    if len(pts) >= 3:
        px, py = pts[-1]
        for qx, qy in pts:
            ret += (px * qy) - (qx * py)
            px, py = qx, qy
        ret *= .5
    return counts, ret


def gg_worst_counts(xe, ye, poly):
    """Per half-plane, the largest vertex count over the candidate ice cells of a polygon."""
    P = np.asarray(poly, np.float64).reshape(-1, 2)
    ix0, nxr = cell_range(xe, P[:, 0].min(), P[:, 0].max())
    iy0, nyr = cell_range(ye, P[:, 1].min(), P[:, 1].max())
    worst = [len(P)] * 5
    for ix in range(ix0, ix0 + nxr):
        for iy in range(iy0, iy0 + nyr):
            worst = [max(a, b) for a, b in zip(worst, gg_counts(P, xe[ix], xe[ix + 1], ye[iy], ye[iy + 1])[0])]
    return worst


def l1_counts(tri, poly):
    """k_l1_clip's loop over the polygon's edges in floats, in the frame of the triangle's vertex 0, without the array limit:
    [3, after edge 0, after edge 1, ...] (it stops, as the kernel does, when nothing is left)."""
    return l1_clip(tri, poly)[0]


def l1_clip(tri, poly):
    """(l1_counts' list, the piece's area as l1_area sums it from the vertices moved back to the mesh's frame)."""
    (x0, y0), (x1, y1), (x2, y2) = [(float(a), float(b)) for a, b in tri]
    s = [(0.0, 0.0), (x1 - x0, y1 - y0), (x2 - x0, y2 - y0)]
    P = np.asarray(poly, np.float64).reshape(-1, 2).tolist()
    counts = [3]
    for e in range(len(P)):
        if not s:
            break
        ax, ay = P[e][0] - x0, P[e][1] - y0
        bx, by = P[(e + 1) % len(P)][0] - x0, P[(e + 1) % len(P)][1] - y0
        ex, ey = bx - ax, by - ay
        out = []
        for k in range(len(s)):
            (sx, sy), (tx, ty) = s[k], s[(k + 1) % len(s)]
            ds, dt = ex * (sy - ay) - ey * (sx - ax), ex * (ty - ay) - ey * (tx - ax)
            if ds >= 0:
                out.append((sx, sy))
            if (ds >= 0) != (dt >= 0):
                t = ds / (ds - dt)
                out.append((sx + t * (tx - sx), sy + t * (ty - sy)))
        s = out
        counts.append(len(s))
    if len(s) < 3:
        return counts, 0.0
    q = [(sx + x0, sy + y0) for sx, sy in s]
    ox, oy = q[0]
    ret, px, py = 0.0, q[-1][0] - ox, q[-1][1] - oy
    for qx, qy in q:
        qx, qy = qx - ox, qy - oy
        ret += (px * qy) - (qx * py)
        px, py = qx, qy
    return counts, ret * .5


# ---- l1.hip's candidate search and refusal bound, restated ---------------------------------------------------------------------
def l1_bins(polys):
    """(x0, y0, x1, y1, sx, sy, nb) as l1_exgrid_generate sets them."""
    v = np.concatenate([np.asarray(p, np.float64).reshape(-1, 2) for p in polys])
    x0, y0, x1, y1 = float(v[:, 0].min()), float(v[:, 1].min()), float(v[:, 0].max()), float(v[:, 1].max())
    nb = 1
    while nb * nb < len(polys) and nb < 1024:
        nb += 1
    return x0, y0, x1, y1, (nb / (x1 - x0) if x1 > x0 else 0.0), (nb / (y1 - y0) if y1 > y0 else 0.0), nb


def l1_bin(v, lo, scale, nb):
    f = (v - lo) * scale
    return (int(f) if f < float(nb) else nb - 1) if f > 0 else 0


def l1_bin_range(g, pts):
    """(bx0, bx1, by0, by1) of the bounding box of pts ([n, 2])."""
    P = np.asarray(pts, np.float64).reshape(-1, 2)
    return (l1_bin(float(P[:, 0].min()), g[0], g[4], g[6]), l1_bin(float(P[:, 0].max()), g[0], g[4], g[6]),
            l1_bin(float(P[:, 1].min()), g[1], g[5], g[6]), l1_bin(float(P[:, 1].max()), g[1], g[5], g[6]))


def l1_turns(poly):
    """Per vertex k+1 the pair (cross(e_k, e_{k+1}), tol): l1_exgrid_generate refuses the polygon when a cross product is below
    -tol, tol = 16 eps M (|e_k|_1 + |e_{k+1}|_1 + eps M) with M the polygon's largest |coordinate| -- derived in l1.hip from
    moving each vertex by one ulp of M plus the rounding of the cross product itself; derived, not measured."""
    P = np.asarray(poly, np.float64).reshape(-1, 2)
    n, eM = len(P), EPS * float(np.abs(P).max())
    out = []
    for k in range(n):
        e, f = P[(k + 1) % n] - P[k], P[(k + 2) % n] - P[(k + 1) % n]
        c = e[0] * f[1] - e[1] * f[0]
        S = (abs(e[0]) + abs(e[1])) + (abs(f[0]) + abs(f[1]))
        out.append((float(c), float(L1_TURN_FACTOR * eM * (S + eM))))
    return out


# ---- shapes ------------------------------------------------------------------------------------------------------------------
def gon16():
    """The regular 16-gon of radius 1, vertices at k * 22.5 degrees."""
    t = np.arange(16) * (math.pi / 8)
    return np.stack([np.cos(t), np.sin(t)], 1)


def star16(cx=0.0, cy=0.0, r=1.0):
    """The {16/7} star: counter-clockwise, every turn a left turn, winding seven times."""
    t = 7 * np.arange(16) * (math.pi / 8)
    return np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], 1)


def ring(n, cx, cy, r, ph=0.1):
    t = ph + np.linspace(0, 2 * np.pi, n, endpoint=False)
    return np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], 1)


ZIGZAG = np.array([(3., -1.), (3., 14.)] + [(-1. if k % 2 == 0 else 1., float(k)) for k in range(13, -1, -1)])
U_SHAPE = np.array([[-5., -4.], [4., -4.], [4., 5.], [0.5, 5.], [0.5, -1.], [-0.5, -1.], [-0.5, 5.], [-5., 5.]])


# ---- G20: gridgen at the array limit ----------------------------------------------------------------------------------------------
def g20():
    """The 16-gon against the single cell [-0.96, 0.96]^2 (each half-plane cuts one tip off: 16, 17, 18, 19, 20 = GG_CLIPV), and on
    a 3 x 3 grid whose centre cell is that square, so that the four tips are cells of their own."""
    one = np.array([-0.96, 0.96])
    three = np.array([-1.5, -0.96, 0.96, 2.25])
    return dict(poly=gon16(), one=(one, one), three=(three, three), iA=[5])


# ---- GNC: gridgen on non-convex input -------------------------------------------------------------------------------------------
def gnc():
    """name -> (xe, ye, polygon).  The zigzag needs 23 vertices after x >= 0; the U is test_gpu_lonlat.py's, alone; the star
    turns left everywhere."""
    return {"zigzag": (np.array([-1.5, 0., 2.5, 3.5]), np.array([-1.5, 4.25, 9., 14.5]), ZIGZAG),
            "u": (-7. + 2. * np.arange(8), -6. + 3. * np.arange(6), U_SHAPE),
            "star": (np.array([-2., 0.5, 3., 4.25, 6., 8.5, 10.]), np.array([-2., 1., 2.75, 5., 7.5, 10.]), star16(4., 4., 5.))}


# ---- GR: candidate ranges and search ties ------------------------------------------------------------------------------------------
# laid out on [1, 12] x [1, 9.5] and then moved to sit round the origin (the array kernel's shoelace runs on absolute coordinates,
# so its rounding grows with their products); every coordinate that has to hit an ice edge exactly is a multiple of 1/4
GR_SHIFT = np.array([-6.5, -5.25])
_XE0 = np.array([1., 2.25, 3., 4.5, 5.5, 7., 7.75, 9.25, 10.5, 12.])      # 9 uneven cells
_YE0 = np.array([1., 2., 3.5, 4.25, 5.75, 7., 8.5, 9.5])                  # 7
GR_XE, GR_YE = _XE0 + GR_SHIFT[0], _YE0 + GR_SHIFT[1]
GR_NSPECIAL = 15
GR_ZERO_CANDIDATES = (0, 7, 8, 11, 13, 256)     # positions in gr()'s list: the last special goes last of all
GR_NPOLY = (255, 256, 257)


def _gr_specials():
    out = ring(4, 20., 20., 1.)                                                       # 0: outside -- no candidates, first
    on_edge = np.array([(4.5, 3.), (6.5, 2.), (7., 4.25)])     # 1: leftmost vertex on the ice edge x = 4.5, lowest on y = 2, third on a corner
    on_corner = np.array([(7., 5.75), (8.5, 6.25), (8.25, 7.75), (6.5, 7.25)])       # 2: its lowest vertex on the ice corner (7, 5.75)
    whole = np.array([(1., 5.5), (5.5, 1.), (12., 5.5), (7.5, 9.5)])                 # 3: bounding box = the grid's extent
    left, right = ring(5, 1.25, 6., 1.), ring(6, 11.7, 3.15, 1.2)                     # 4, 5: out of the left and right sides
    bottom = ring(7, 6.6, 0.95, 1.1)                                                # 6: out of the bottom
    far1, far2 = ring(3, -9., 4., 2.), ring(5, 6., 25., 3.)                          # 7, 8: two without candidates in a row
    top = ring(3, 8.3, 9.05, 1.4, 0.7)                                              # 9: out of the top
    corner = ring(8, 11.6, 9.2, 1.)                                                  # 10: over the grid's corner
    touch = np.array([(12., 3.), (13.5, 3.), (13.5, 6.), (12., 6.)])                 # 11: shares the boundary x = 12 only: no candidates
    # 12: its box reaches into the corner cell, the polygon touches the grid in the corner (12, 9.5) alone: one candidate, no cell
    point = np.array([(11., 10.5), (13., 8.5), (13., 10.5)])
    below = np.array([(3., -1.), (8., -1.), (8., 1.), (3., 1.)])                      # 13: shares the boundary y = 1 only... from below
    last = ring(6, 30., -4., 2.)                                                     # 14: outside -- no candidates, last
    return [out, on_edge, on_corner, whole, left, right, bottom, far1, far2, top, corner, touch, point, below, last]


def _gr_tiles(n):
    """Small rotated quads: over an interior ice corner (four candidates), astride an ice edge (two), inside one cell (one)."""
    tiles, k = [], 0
    nx, ny = len(_XE0) - 1, len(_YE0) - 1
    dx, dy = np.diff(_XE0), np.diff(_YE0)
    while len(tiles) < n:
        ix, iy = k % (nx - 1), (k // (nx - 1)) % (ny - 1)
        kind, ph = k % 3, 0.15 + 0.1 * (k % 7)
        if kind == 0:
            c, r = (_XE0[ix + 1], _YE0[iy + 1]), 0.42 * min(dx[ix], dx[ix + 1], dy[iy], dy[iy + 1])
        elif kind == 1:
            c, r = (_XE0[ix + 1], _YE0[iy] + 0.5 * dy[iy]), 0.4 * min(dx[ix], dx[ix + 1], dy[iy])
        else:
            c, r = (_XE0[ix] + 0.5 * dx[ix], _YE0[iy] + 0.5 * dy[iy]), 0.45 * min(dx[ix], dy[iy])
        tiles.append(ring(4, c[0], c[1], r, ph))
        k += 1
    return tiles


@functools.lru_cache(maxsize=None)
def gr():
    """dict(xe, ye, polys, per_poly): the 257 polygons (specials, tiles, the last special) and the exact cells of each."""
    sp = _gr_specials()
    polys = [p + GR_SHIFT for p in sp[:-1] + _gr_tiles(max(GR_NPOLY) - GR_NSPECIAL) + sp[-1:]]
    return dict(xe=GR_XE, ye=GR_YE, polys=polys, per_poly=[exact_gridgen_poly(GR_XE, GR_YE, p) for p in polys])


def gr_variant(npoly):
    """(polygons, iA, positions in gr()'s list) of the variant with npoly polygons: tiles dropped from the end, the last special
    kept last."""
    full = gr()["polys"]
    pos = list(range(npoly - 1)) + [len(full) - 1]
    return [full[k] for k in pos], 3 * np.asarray(pos, np.int64) + 2, pos


# ---- L19: L1 at the piece limit -----------------------------------------------------------------------------------------------------
def l19():
    """The 16-gon under the counter-clockwise triangle bounded by the lines n . x = 0.96 with normals at 90, 202.5 and 337.5
    degrees -- each cuts one vertex of the 16-gon off, so the overlap has 16 - 3 + 6 = 19 = L1_CLIPV vertices, and the triangle as
    k_l1_clip's subject gains one vertex at each of the 16 edges.  Element 0 is that triangle; 1..3 share its edges and pick up the
    three tips; 4 lies outside the 16-gon; a second GCM cell (a square) meets elements 2 and 4."""
    ang = [math.radians(a) for a in (90., 202.5, 337.5)]

    def meet(a, b):
        det = math.cos(a) * math.sin(b) - math.sin(a) * math.cos(b)
        return (0.96 * (math.sin(b) - math.sin(a)) / det, 0.96 * (math.cos(a) - math.cos(b)) / det)
    A, B, C = meet(ang[0], ang[1]), meet(ang[1], ang[2]), meet(ang[2], ang[0])
    vx = [A[0], B[0], C[0], 0.3, -2.9, 2.7, 3.5]
    vy = [A[1], B[1], C[1], 2.6, -1.7, -2.1, 1.5]
    tri = [(0, 1, 2), (2, 3, 0), (1, 0, 4), (2, 1, 5), (5, 6, 2)]
    polys = [gon16(), np.array([(1.5, -2.5), (4., -2.5), (4., 0.5), (1.5, 0.5)])]
    return dict(vx=np.array(vx), vy=np.array(vy), tri=np.array(tri, np.int32), polys=polys, iA=np.array([3, 8], np.int64))


# ---- LB: L1's candidate search --------------------------------------------------------------------------------------------------------
LB_NTRI = (1, 63, 64, 65, 129)
LB_SEED = 20241022


@functools.lru_cache(maxsize=None)
def lb():
    """16 x 16 unit cells and one cell [16, 24] x [0, 16] (257 polygons, 17 bins a side, the big cell over many bins and its corner
    (24, 16) on the box's maximum), under a mesh over [-1, 25] x [-1, 17] of jittered rectangles cut in two, some smaller than a bin
    (24/17 x 16/17) and some several bins wide; the elements come in a shuffled order so that every leading sub-mesh is spread out.
    dict(vx, vy, tri, polys, iA, exact)."""
    polys, iA = lb_polys()
    vx, vy, tri = lb_mesh(LB_SEED)
    return dict(vx=vx, vy=vy, tri=tri, polys=polys, iA=iA, exact=exact_l1(vx, vy, tri, polys, iA))


def lb_polys():
    polys = [np.array([(i, j), (i + 1., j), (i + 1., j + 1.), (i, j + 1.)], float) for j in range(16) for i in range(16)]
    polys.append(np.array([(16., 0.), (24., 0.), (24., 16.), (16., 16.)]))
    return polys, np.arange(257, dtype=np.int64) * 2 + 1


def lb_mesh(seed):
    xs = np.array([-1., -0.4, 0.3, 0.9, 1.3, 2.0, 5.5, 6.1, 6.6, 10.5, 11., 15.7, 16.4, 19., 23.6, 24.3, 25.])
    ys = np.array([-1., -0.3, 0.4, 0.9, 4.2, 4.8, 8.9, 9.4, 12.5, 15.6, 16.3, 17.])
    rng = np.random.default_rng(seed)
    X, Y = np.meshgrid(xs, ys)                       # [iy, ix]
    jx, jy = rng.uniform(-0.12, 0.12, X.shape), rng.uniform(-0.12, 0.12, Y.shape)
    jx[:, [0, -1]] = 0; jx[[0, -1], :] = 0; jy[:, [0, -1]] = 0; jy[[0, -1], :] = 0      # the outline stays a rectangle
    vx, vy = (X + jx).reshape(-1), (Y + jy).reshape(-1)
    n, tri = len(xs), []
    for iy in range(len(ys) - 1):
        for ix in range(n - 1):
            v00, v10, v01, v11 = iy * n + ix, iy * n + ix + 1, (iy + 1) * n + ix, (iy + 1) * n + ix + 1
            tri += [(v00, v10, v11), (v00, v11, v01)] if (ix + iy) % 2 else [(v00, v10, v01), (v10, v11, v01)]
    tri = np.asarray(tri, np.int32)[rng.permutation(len(tri))]
    return vx, vy, tri


# ---- LNC: L1's refusals and near-refusals -------------------------------------------------------------------------------------------------
def lnc():
    """reflex: one clearly reflex vertex (3); clockwise: a square walked the wrong way; star: the {16/7} star; far: a rotated quad at
    2e6 with two computed points on each side (12 vertices, straight to rounding) and a small mesh under it -- to be accepted."""
    c, th = np.array([-6.0e5, -2.0e6]), 0.3
    R = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
    corners = [c + R @ np.array(v) for v in ((-1.0e4, -0.8e4), (1.1e4, -0.7e4), (0.9e4, 0.8e4), (-1.2e4, 0.9e4))]
    far = []
    for k in range(4):
        a, b = corners[k], corners[(k + 1) % 4]
        far += [a, a + (1.0 / 3.0) * (b - a), a + (2.0 / 3.0) * (b - a)]
    out = [c + np.array(v) for v in ((-1.7e4, -1.5e4), (1.6e4, -1.8e4), (1.9e4, 1.4e4), (-1.5e4, 1.7e4))]
    mesh = dict(vx=np.array([c[0] + 1.0e3] + [p[0] for p in out]), vy=np.array([c[1] - 2.0e3] + [p[1] for p in out]),
                tri=np.array([(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 1)], np.int32))
    return dict(reflex=np.array([(0., 0.), (4., 0.), (4., 4.), (2., 1.5), (0., 4.)]),
                clockwise=np.array([(0., 0.), (0., 1.), (1., 1.), (1., 0.)]),
                star=star16(4., 4., 5.), far=np.array(far), far_mesh=mesh)
