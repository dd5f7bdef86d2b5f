"""The L1 path on the GPU (icebin_amd/csrc/l1.hip): exchange-grid generation for a triangle mesh, the basis integrals and the
AvI / IvA matrices.  Inputs and expected values come from tests/golden/l1_reference.npz and the numpy restatement in
tests/l1_restatement.py; nothing here reads the reference."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import l1_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def l1():
    from icebin_amd import l1 as mod
    return mod


@pytest.fixture(scope="module")
def built(l1):
    """Per case, made once: the fixture arrays, the mesh, the exchange grid from the fixture's polygons, the generated one,
    and the restatement's terms in (iA, iTri) order."""
    cache = {}

    def get(name):
        if name not in cache:
            c = R.load_case(name)
            c["mesh"] = l1.Mesh(c["vx"], c["vy"], c["tri"])
            c["given"] = l1.exchange_grid_from_polygons(c["ex_iA"], c["ex_iTri"], vptr=c["ex_vptr"], qx=c["ex_qx"], qy=c["ex_qy"])
            c["generated"] = l1.make_exchange_grid(c["mesh"], R.polys_of(c), c["iA_poly"])
            c["perm"] = R.sort_cells(c["ex_iA"], c["ex_iTri"])
            c["restated"] = R.cell_terms(c["vx"], c["vy"], c["tri"], c["ex_iTri"], c["ex_vptr"], c["ex_qx"], c["ex_qy"])[c["perm"]]
            cache[name] = c
        return cache[name]
    return get


def csr_of(w):
    rowptr, col, val = w.csr_dense()
    return rowptr, col, val, w.wM, w.Mw


def assert_same_matrix(got, want, what):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what + ": structure"
    for g, x, part in zip(got[2:], want[2:], ("values", "wM", "Mw")):
        assert np.array_equal(bits(g), bits(x)), "%s: %s differ in bits" % (what, part)


# ---- integral and assembly, given the fixture's polygons -------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASES)
def test_integrals_and_assembly_match_the_restatement_in_bits(l1, built, name):
    c = built(name)
    ex, p = c["given"], c["perm"]
    nA, nI = int(c["nA"]), len(c["vx"])
    # the cells as given, sorted by (iA, iTri), ties in input order
    assert np.array_equal(ex.indices[:, 0], c["ex_iA"][p]) and np.array_equal(ex.indices[:, 1], c["ex_iTri"][p])
    given = [np.stack([c["ex_qx"][c["ex_vptr"][k]:c["ex_vptr"][k + 1]], c["ex_qy"][c["ex_vptr"][k]:c["ex_vptr"][k + 1]]], 1) for k in p]
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(ex.polygons, given))
    assert np.array_equal(bits(ex.areas), bits(R.poly_areas(ex.vptr, ex.qx, ex.qy)))
    # per-cell terms
    row, col, val = l1.terms(ex, nA, c["mesh"])
    want = R.triplets(c["tri"], c["ex_iA"][p], c["ex_iTri"][p], c["restated"], "AvI")
    assert np.array_equal(row, want[0]) and np.array_equal(col, want[1])
    assert np.array_equal(bits(val), bits(want[2])), "terms differ in bits"
    # the matrix and its weights
    avi = csr_of(l1.compute_AvI(ex, nA, c["mesh"]))
    want_avi = R.assemble(*want, nA, nI)
    assert_same_matrix(avi, want_avi, "AvI")
    assert len(avi[2]) == int(c["nnz"])
    # IvA: the roles swapped, the same bits
    iva = csr_of(l1.compute_AvI(ex, nA, c["mesh"], which="IvA"))
    assert_same_matrix(iva, R.assemble(*R.triplets(c["tri"], c["ex_iA"][p], c["ex_iTri"][p], c["restated"], "IvA"), nI, nA), "IvA")
    assert np.array_equal(bits(iva[3]), bits(avi[4])) and np.array_equal(bits(iva[4]), bits(avi[3]))
    rows_a, rows_t = np.repeat(np.arange(nA), np.diff(avi[0])), np.repeat(np.arange(nI), np.diff(iva[0]))
    o = np.lexsort((rows_t, iva[1]))
    assert np.array_equal(iva[1][o], rows_a) and np.array_equal(rows_t[o], avi[1]) and np.array_equal(bits(iva[2][o]), bits(avi[2]))
    # scaled: M = diag(1/wM) M elementwise, the weights unchanged
    for which, plain in (("AvI", avi), ("IvA", iva)):
        w = l1.compute_AvI(ex, nA, c["mesh"], scale=True, which=which)
        assert w.scaled and w.conservative
        s = csr_of(w)
        assert_same_matrix(s, (plain[0], plain[1], R.scale_rows(plain[0], plain[2], plain[3]), plain[3], plain[4]), which + " scaled")


# ---- generation ----------------------------------------------------------------------------------------------------------------
def numpy_exchange_cells(c):
    """An independent Sutherland-Hodgman, the other way round from the library's: the GCM cell is the subject and the
    element's three edges clip it, in rational arithmetic on the float inputs, so the areas are exact.  Returns
    {(iA, iTri): (area, perimeter)}."""
    from fractions import Fraction as F
    out = {}
    polys = R.polys_of(c)
    boxes = [(p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max()) for p in polys]
    for t, el in enumerate(c["tri"]):
        T = [(F(float(c["vx"][v])), F(float(c["vy"][v]))) for v in el]
        tb = (min(v[0] for v in T), min(v[1] for v in T), max(v[0] for v in T), max(v[1] for v in T))
        for n, poly in enumerate(polys):
            if boxes[n][2] < tb[0] or boxes[n][0] > tb[2] or boxes[n][3] < tb[1] or boxes[n][1] > tb[3]:
                continue
            s = [(F(v[0]), F(v[1])) for v in poly.tolist()]
            for e in range(3):
                a, b = T[e], T[(e + 1) % 3]
                side = [(b[0] - a[0]) * (v[1] - a[1]) - (b[1] - a[1]) * (v[0] - a[0]) for v in s]
                nxt = []
                for k in range(len(s)):
                    kn = (k + 1) % len(s)
                    if side[k] >= 0:
                        nxt.append(s[k])
                    if (side[k] > 0 and side[kn] < 0) or (side[k] < 0 and side[kn] > 0):
                        u = side[k] / (side[k] - side[kn])
                        nxt.append((s[k][0] + u * (s[kn][0] - s[k][0]), s[k][1] + u * (s[kn][1] - s[k][1])))
                s = nxt
                if len(s) < 3:
                    break
            if len(s) < 3:
                continue
            area = sum(s[k][0] * s[(k + 1) % len(s)][1] - s[(k + 1) % len(s)][0] * s[k][1] for k in range(len(s))) / 2
            if area > 0:
                per = sum(math.hypot(float(s[(k + 1) % len(s)][0] - s[k][0]), float(s[(k + 1) % len(s)][1] - s[k][1])) for k in range(len(s)))
                out[(int(c["iA_poly"][n]), t)] = (float(area), per)
    return out


@pytest.mark.parametrize("name", R.CASES)
def test_generation_matches_an_independent_clipper(l1, built, name):
    c = built(name)
    ex = c["generated"]
    want = numpy_exchange_cells(c)
    keys = sorted(want)
    assert [tuple(k) for k in ex.indices.tolist()] == keys                 # identical, and sorted by (iA, iTri)
    assert len(ex) == len(c["ex_iA"])                                      # the fixture's own clipper found as many
    ref, per = np.array([want[k][0] for k in keys]), np.array([want[k][1] for k in keys])
    err = np.abs(ex.areas - ref)
    print("%s: %d exchange cells, areas within %.2e relative of the exact ones" % (name, len(ex), np.max(err / ref)))
    # 1e-12 relative: the bar of test_exchange_grid_generation.  Only jit9_far gets a second term: its polygons are stored in
    # doubles at 2e6 m, where a coordinate is rounded by up to half an ulp (1.2e-10 m) -- whoever computes them; moving every
    # vertex of a piece by d changes its area by at most perimeter x d, which for a sliver 2e-5 of an element exceeds 1e-12 of
    # its own area (measured 1.6e-11).  d = one ulp of the largest coordinate covers both coordinates moving.
    slack = per * np.spacing(max(np.abs(c["vx"]).max(), np.abs(c["vy"]).max())) if name == "jit9_far" else 0.0
    assert np.all(err <= 1e-12 * ref + slack), np.max(err / ref)
    nv = np.diff(ex.vptr)
    assert ex.vptr[0] == 0 and nv.min() >= 3 and nv.max() <= 19 and np.all(ex.areas > 0)
    # two runs: identical bytes
    again = l1.make_exchange_grid(c["mesh"], R.polys_of(c), c["iA_poly"])
    for k in ("indices", "areas", "vptr", "qx", "qy"):
        assert getattr(ex, k).tobytes() == getattr(again, k).tobytes(), k


def test_generation_edges(l1, built):
    c = built("edges")
    ex = c["generated"]
    pairs = [tuple(k) for k in ex.indices.tolist()]
    # element 0 inside cell 0 unclipped; 1 over the corner of all four; 2 touches cell 0 with a vertex, 3 cell 1 with an edge:
    # no zero-area record; 4 lies outside every cell
    assert pairs == [(0, 0), (0, 1), (1, 1), (1, 2), (2, 1), (3, 1), (3, 3)]
    assert np.all(ex.areas > 0) and 4 not in ex.indices[:, 1]
    assert np.array_equal(bits(ex.polygons[0]), bits(np.stack([c["vx"][:3], c["vy"][:3]], 1)))
    nA = int(c["nA"])
    w = l1.compute_AvI(ex, nA, c["mesh"], scale=True)
    assert np.all(w.wM[[4, 5, 6]] == 0) and np.all(w.wM[:4] > 0)          # 5: realised, no triangle touches it; 4, 6: not realised
    f = 1.0 + np.arange(len(c["vx"]), dtype=float)
    y = w.apply_M(f, fill=-777.0, force_conservation=False)
    assert np.all(y[[4, 5, 6]] == -777.0) and np.all(y[:4] != -777.0)


# ---- invariants, end to end from generation --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASES)
def test_invariants_from_generation(l1, built, name):
    c = built(name)
    ex, nA = c["generated"], int(c["nA"])
    _, _, val = l1.terms(ex, nA, c["mesh"])
    t = c["tri"][ex.indices[:, 1]]
    e1x, e1y = c["vx"][t[:, 1]] - c["vx"][t[:, 0]], c["vy"][t[:, 1]] - c["vy"][t[:, 0]]
    e2x, e2y = c["vx"][t[:, 2]] - c["vx"][t[:, 0]], c["vy"][t[:, 2]] - c["vy"][t[:, 0]]
    elem = 0.5 * (e1x * e2y - e1y * e2x)
    sums = np.array([math.fsum(v) for v in val.reshape(-1, 3)])
    err = np.max(np.abs(sums - ex.areas) / elem)
    print("%s: per cell, |sum of the three terms - area| <= %.2e x element area" % (name, err))
    assert err <= 1e-15
    w = l1.compute_AvI(ex, nA, c["mesh"])
    a, b, s = math.fsum(w.wM), math.fsum(w.Mw), math.fsum(ex.areas)
    print("%s: fsum(wM) %.17g fsum(Mw) %.17g fsum(areas) %.17g" % (name, a, b, s))
    assert abs(a - s) < 1e-13 * s and abs(b - s) < 1e-13 * s and abs(a - b) < 1e-13 * s


# ---- linear fields are exact -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["jit9", "jit9_far"])
@pytest.mark.parametrize("nvar", [1, 5])
def test_linear_fields_are_reproduced(l1, built, name, nvar):
    # f = a + b x + c y at the vertices through scaled AvI: the area-weighted mean of f over each cell's overlap, which is f at
    # the overlap's centroid -- from the exchange polygons, with fsum, in the frame of each polygon's vertex 0
    c = built(name)
    ex, nA = c["generated"], int(c["nA"])
    w = l1.compute_AvI(ex, nA, c["mesh"], scale=True)
    coef = np.array([[3.0, 0.25, -0.5], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [-2.0, -0.125, 0.75]])[:nvar]
    f = coef[:, :1] + coef[:, 1:2] * c["vx"][None, :] + coef[:, 2:3] * c["vy"][None, :]
    y = w.apply_M(f if nvar > 1 else f[0], fill=np.nan, force_conservation=False).reshape(nvar, -1)
    mom = {}            # per GCM cell: lists of area, area * centroid x, area * centroid y of the fan triangles
    for x, poly in enumerate(ex.polygons):
        iA = int(ex.indices[x, 0])
        m = mom.setdefault(iA, ([], [], []))
        o = poly[0]
        for i in range(2, len(poly)):
            u, v = poly[i - 1] - o, poly[i] - o
            fa = 0.5 * (u[0] * v[1] - u[1] * v[0])
            m[0].append(fa)
            m[1].extend([fa * o[0], fa * (u[0] + v[0]) / 3.0])
            m[2].extend([fa * o[1], fa * (u[1] + v[1]) / 3.0])
    assert sorted(mom) == list(range(nA))
    want = np.zeros((nvar, nA))
    for iA, m in mom.items():
        area = math.fsum(m[0])
        cx, cy = math.fsum(m[1]) / area, math.fsum(m[2]) / area
        want[:, iA] = coef[:, 0] + coef[:, 1] * cx + coef[:, 2] * cy
    worst = np.max(np.max(np.abs(y - want), 1) / np.max(np.abs(want), 1))       # per field, relative to its largest value
    print("%s, %d fields: worst relative error %.2e" % (name, nvar, worst))
    assert worst <= 1e-12


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(l1):
    from icebin_amd._capi import IBH_EINVAL, IcebinHipError
    vx, vy = [0., 1., 1., 0.], [0., 0., 1., 1.]
    for tri, words in (([(0, 1, 2), (0, 3, 2)], "element 1 .*not counter-clockwise"),       # clockwise
                       ([(0, 1, 2), (0, 2, 3), (1, 1, 3)], "element 2 .*positive area"),     # zero area
                       ([(0, 1, 2), (0, 2, 4)], "element 1 names vertex 4"),                 # id out of range
                       ([(0, -1, 2)], "element 0 names vertex -1")):
        with pytest.raises(IcebinHipError, match=words) as ei:
            l1.Mesh(vx, vy, tri)
        assert ei.value.code == IBH_EINVAL
    mesh = l1.Mesh(vx, vy, [(0, 1, 2), (0, 2, 3)])
    ang = 2 * np.pi * np.arange(17) / 17
    with pytest.raises(IcebinHipError, match="17 vertices") as ei:
        l1.make_exchange_grid(mesh, [np.stack([np.cos(ang), np.sin(ang)], 1)], [0])
    assert ei.value.code == IBH_EINVAL
    ok = l1.make_exchange_grid(mesh, [np.stack([np.cos(ang[:16]), np.sin(ang[:16])], 1) * 2], [0])       # 16 are served
    assert len(ok) == 2 and abs(ok.areas.sum() - 1.0) <= 1e-15
    with pytest.raises(IcebinHipError, match="ascending iA"):
        l1.make_exchange_grid(mesh, [np.array([(0., 0.), (1., 0.), (1., 1.)])] * 2, [1, 1])
    ex = l1.exchange_grid_from_polygons([0], [5], polys=[[(0., 0.), (1., 0.), (1., 1.)]])
    with pytest.raises(IcebinHipError, match="names element 5") as ei:
        l1.compute_AvI(ex, 1, mesh)
    assert ei.value.code == IBH_EINVAL
    with pytest.raises(IcebinHipError, match="AvI"):
        l1.compute_AvI(ok, 1, mesh, which="EvI")
    # the library still works after every refusal
    assert l1.compute_AvI(ok, 1, mesh).nnz == 4


# ---- the reference's entry point ---------------------------------------------------------------------------------------------------
def test_reference_entry_point_on_duck_typed_grids(built):
    from types import SimpleNamespace as NS
    from icebin_amd.cython.build_ext import build
    build()
    sys.path.insert(0, os.path.join(ROOT, "icebin_amd", "cython"))
    from icebin import element_l1
    import scipy.sparse
    c = built("four_tri_a1")
    verts = [NS(index=k, x=float(c["vx"][k]), y=float(c["vy"][k])) for k in range(5)]
    gridI = NS(cells={t: NS(vertices=[verts[v] for v in el]) for t, el in enumerate(c["tri"])}, indexing=NS(base=[0]), vertices_nfull=5)
    exgrid = NS(cells={x: NS(i=0, j=x, vertices=[verts[v] for v in c["tri"][x]]) for x in range(4)})
    AvI, weightsA, weightsI = element_l1.compute_AvI(exgrid, 1, gridI)
    assert scipy.sparse.isspmatrix_coo(AvI) and AvI.shape == (1, 5)
    assert np.max(np.abs(weightsI - np.array([2 / 3, 2 / 3, 2 / 3, 2 / 3, 4 / 3]))) <= 1e-15
    assert weightsA.shape == (1,) and abs(weightsA[0] - 4.0) <= 1e-15
    assert np.max(np.abs(np.asarray(AvI.todense())[0] - weightsI)) <= 1e-15
