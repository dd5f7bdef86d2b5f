"""The smoother's three device forms (smooth.hip: the triplet pipeline, the wave-per-row direct form, the spatial tiles) at their bin,
wave and table edges, each against the oracle and, where the scene is small, against the long-double definition within the derived
entry bound (tests/smoothing_cases.py; tests/test_smoothing_cases.py asserts on the CPU that every scene lies where its leg needs it).
Every leg first asserts its input's side of the limits, then which form built the matrix, then the matrix."""
import functools
import os
import sys

import numpy as np
import pytest

import icebin_amd
from icebin_amd import _capi
from icebin_amd.linear import set_tuning
from oracle import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import smoothing_cases as smc
finally:
    sys.path.pop(0)

pytestmark = pytest.mark.gpu

FORM_KNOBS = {smc.TILE: (0, 1), smc.DIRECT: (1, 0), smc.TRIPLET: (0, 0)}      # the knobs that ask for a form alone
ALL_KNOBS = smc.KNOBS + ((1, 1),)
KNOB_FORM = {knobs: form for form, knobs in FORM_KNOBS.items()}               # the form each leg that asks for one is written for


def smoothed_build(mm, em, name, sigma, knobs):
    set_tuning("smooth_direct", knobs[0])
    set_tuning("smooth_tile", knobs[1])
    try:
        return mm.regrid_matrices("greenland", em, scale=True, correctA=True, sigma=sigma).matrix(name)
    finally:
        set_tuning("smooth_direct", -1)
        set_tuning("smooth_tile", -1)


def same_bits(a, b):
    if (a.nrow_d, a.ncol_d, a.nnz, a.conservative) != (b.nrow_d, b.ncol_d, b.nnz, b.conservative):
        return False
    return all(np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y)
               for x, y in zip(a.csr_dense() + (a.wM, a.Mw), b.csr_dense() + (b.wM, b.Mw)))


@functools.lru_cache(maxsize=None)
def model(kind, *args):
    if kind in ("g20", "g50"):
        return icebin_amd.from_synthetic(smc.grids(kind)[0])
    return icebin_amd.from_synthetic(smc.scene(kind, *args)[0])


def check_leg(mm, em, name, sigma, knobs, facts, plain, o, reference=None):
    """One build: the form the knobs and the input's facts decide (assert_input_side) is the one that ran; not conservative; dims, row and
    col exactly the oracle's; wM / Mw bitwise the unsmoothed oracle matrix's; entries within 1e-12 of the oracle and, with `reference`
    (row, col, long-double val), within the derived bound of the definition.  A fall-through is bitwise the build that asks for the
    serving form alone."""
    form = smc.serving_form(knobs, facts)
    smc.assert_input_side(form, knobs[1] > 0, knobs[0] > 0, facts["widest"], facts["longest"], facts["longest_smoothed"])
    w = smoothed_build(mm, em, name, sigma, knobs)
    assert w.smoothed_by() == form
    assert not w.conservative and not o.conservative
    assert (w.nrow_d, w.ncol_d, w.nnz) == (o.nrow, o.ncol, o.nnz)
    np.testing.assert_array_equal(w.dim(0), o.dims[0])
    np.testing.assert_array_equal(w.dim(1), o.dims[1])
    row, col, val = w.coo_dense()
    np.testing.assert_array_equal(row, o.row)
    np.testing.assert_array_equal(col, o.col)
    np.testing.assert_array_equal(w.wM.view(np.uint64), plain.wM.view(np.uint64))
    np.testing.assert_array_equal(w.Mw.view(np.uint64), plain.Mw.view(np.uint64))
    worst = float(np.max(np.abs(val - o.val) / np.abs(o.val))) if o.nnz else 0.0
    print("form %d knobs %s: worst relative difference from the oracle %.3g" % (form, knobs, worst))
    np.testing.assert_allclose(val, o.val, rtol=1e-12, atol=0)
    if reference is not None:
        rrow, rcol, ref = reference
        np.testing.assert_array_equal(row, rrow)
        np.testing.assert_array_equal(col, rcol)
        print("    worst error over the derived bound: device %.3g, oracle %.3g" % (
            smc.assert_entries_within_bound(val, facts["N"], rrow, ref), smc.assert_entries_within_bound(o.val, facts["N"], rrow, ref)))
    if knobs != FORM_KNOBS[form]:
        other = smoothed_build(mm, em, name, sigma, FORM_KNOBS[form])
        assert other.smoothed_by() == form
        assert same_bits(w, other)
    return w


def check_scene(name, sigma, knobs, kind, *args):
    g, em, plain, o, facts = smc.scene_case(name, sigma, kind, *args)
    return check_leg(model(kind, *args), em, name, sigma, knobs, facts, plain, o, smc.scene_reference(name, sigma, kind, *args))


# ---- 1, 2: grids with several waves in a bin of the tile form; the direct form's drain; SMT_KMAX with several waves --------------------
@pytest.mark.parametrize("knobs", smc.KNOBS, ids=["tile", "direct", "triplet"])
@pytest.mark.parametrize("leg", range(len(smc.BIG_LEGS)), ids=[l[0] for l in smc.BIG_LEGS])
def test_several_waves_per_bin_and_the_drain(leg, knobs):
    _, config, name, sigma, want = smc.BIG_LEGS[leg]
    g, em = smc.grids(config)
    plain, o, widest, longest, longest_smoothed = smc.oracle_case(config, name, sigma)
    members, _ = smc.bin_members(g, em, plain, sigma)
    assert members.max() > 64 and members.max() % 64 != 0 and int(members.max()) == want["fullest"]
    if config == "g20":
        assert smc.neighbour_counts(g, em, plain, sigma).max() > smc.SMD_HITS - 64
    else:
        assert widest == smc.SMT_KMAX
    facts = dict(widest=widest, longest=longest, longest_smoothed=longest_smoothed)
    w = check_leg(model(config), em, name, sigma, knobs, facts, plain, o)
    assert w.smoothed_by() == KNOB_FORM[knobs]


# ---- 3: the cluster scenes: every cell every cell's neighbour, one bin ---------------------------------------------------------------
# every scene with the knobs that ask for one form, and with both where the tiles fall through
CLUSTER_LEGS = [(c, k) for c in smc.CLUSTERS_IVA for k in ALL_KNOBS if k != (1, 1) or smc.cluster_form(c[1], c[2], k) != smc.TILE]


@pytest.mark.parametrize("nKr,knobs", CLUSTER_LEGS, ids=["%d-%d-%d-knobs%d%d" % (c + k) for c, k in CLUSTER_LEGS])
def test_cluster_scenes_iva(nKr, knobs):
    n, K, rowlen = nKr
    w = check_scene("IvA", smc.SIGMA_C, knobs, "cluster", n, K, rowlen)
    assert w.smoothed_by() == smc.cluster_form(K, rowlen, knobs)


@pytest.mark.parametrize("knobs", smc.KNOBS, ids=["tile", "direct", "triplet"])
@pytest.mark.parametrize("nKr", smc.CLUSTERS_IVE, ids=lambda t: "%d-%d-%d" % t)
def test_cluster_scenes_ive(nKr, knobs):
    w = check_scene("IvE", smc.SIGMA_C, knobs, "cluster", *nKr)
    assert w.smoothed_by() == KNOB_FORM[knobs]


# ---- 4: the lattice at the cut -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", smc.KNOBS, ids=["tile", "direct", "triplet"])
def test_lattice_at_the_cut(knobs):
    g, em, plain, o, f = smc.scene_case("IvA", smc.SIGMA_C, "lattice")
    inside, outside = smc.cut_pairs(g, em, plain, smc.SIGMA_C)
    assert inside + outside >= 100 and inside > 0 and outside > 0
    w = check_scene("IvA", smc.SIGMA_C, knobs, "lattice")
    assert w.smoothed_by() == KNOB_FORM[knobs]


# ---- 5: degenerate bin grids -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", smc.KNOBS, ids=["tile", "direct", "triplet"])
@pytest.mark.parametrize("kind", ["one_column", "one_point", "one_cell"])
def test_degenerate_bin_grids(kind, knobs):
    _, _, _, _, f = smc.scene_case("IvA", smc.SIGMA_C, kind)
    assert (f["nbx"], f["nby"]) == (1, 1)
    w = check_scene("IvA", smc.SIGMA_C, knobs, kind)
    assert w.smoothed_by() == KNOB_FORM[knobs]


@pytest.mark.parametrize("knobs", smc.KNOBS, ids=["tile", "direct", "triplet"])
def test_all_cells_masked(knobs):
    g, em, plain, o, _ = smc.scene_case("IvA", smc.SIGMA_C, "all_masked")
    assert o.nnz == 0
    w = smoothed_build(model("all_masked"), em, "IvA", smc.SIGMA_C, knobs)
    assert (w.nrow_d, w.ncol_d, w.nnz) == (o.nrow, o.ncol, 0)
    assert w.conservative == o.conservative
    np.testing.assert_array_equal(w.dim(0), o.dims[0])
    np.testing.assert_array_equal(w.dim(1), o.dims[1])


@pytest.mark.parametrize("knobs", smc.KNOBS, ids=["tile", "direct", "triplet"])
def test_capped_bin_grid_on_one_axis(knobs):
    g, em = smc.scene("cluster", 65, 3, 1)
    sigma = smc.capped_sigma(g)
    _, _, _, _, f = smc.scene_case("IvA", sigma, "cluster", 65, 3, 1)
    assert (f["nbx"], f["nby"]) == (smc.MAX_BINS, 1) and f["N"].max() <= 3
    w = check_scene("IvA", sigma, knobs, "cluster", 65, 3, 1)
    assert w.smoothed_by() == KNOB_FORM[knobs]


# ---- 6: the pair across two bins ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", smc.KNOBS, ids=["tile", "direct", "triplet"])
def test_neighbours_two_bins_of_two_sigmas_apart(knobs):
    """Two cells less than two sigmas apart whose truncated quotients under bins of exactly two sigmas differ by two: the reference's RTree
    box holds the pair, so must the 3 x 3 bins (smooth_plan.h: a bin is SMOOTH_BIN_MARGIN wider than two sigmas)."""
    g, em, a, b = smc.far_pair_scene()
    _, _, plain, o, f = smc.scene_case("IvA", smc.FAR_SIGMA, "far")
    (qa, qb), neighbours, brings = smc.far_pair_facts(g, em, plain, a, b)
    assert qb - qa == 2 and neighbours and len(brings) >= 1
    da = int(np.nonzero(np.asarray(plain.dims[0]) == a)[0][0])
    row, col, _ = smoothed_build(model("far"), em, "IvA", smc.FAR_SIGMA, knobs).coo_dense()
    print("row of cell a: device columns %s, oracle columns %s, the partner's own %s" % (col[row == da].tolist(), o.col[o.row == da].tolist(), brings))
    w = check_leg(model("far"), em, "IvA", smc.FAR_SIGMA, knobs, f, plain, o)
    assert w.smoothed_by() == KNOB_FORM[knobs]


# ---- 7: zero area ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", smc.KNOBS, ids=["tile", "direct", "triplet"])
@pytest.mark.parametrize("cells", [(smc.ZERO_AREA_ONE,), smc.ZERO_AREA_PAIR], ids=["one", "two"])
def test_zero_area_refusal_names_the_references_cell(cells, knobs):
    """smoother.cpp:89-90: the reference walks the cells in ascending index, so of two cells without area it names the smaller index --
    whose dense row here is the later one"""
    g, em = smc.zero_area_scene(list(cells))
    rg = orc.Regridder(g)
    plain = rg.matrix_d("IvE", em, scale=True, correctA=True)
    s = np.asarray(plain.dims[0], np.int64).tolist()
    assert all(plain.wM[s.index(c)] == 0.0 for c in cells) and np.count_nonzero(plain.wM == 0.0) == len(cells)
    if len(cells) == 2:
        assert cells[0] < cells[1] and s.index(cells[1]) < s.index(cells[0])
    with pytest.raises(orc.OracleError, match="Area of cell %d must be non-zero" % min(cells)):
        rg.matrix_d("IvE", em, scale=True, correctA=True, sigma=smc.SIGMA_C)
    mm = icebin_amd.from_synthetic(g)
    with pytest.raises(icebin_amd.IcebinHipError) as ei:
        smoothed_build(mm, em, "IvE", smc.SIGMA_C, knobs)
    print("device: %s" % ei.value)
    assert ei.value.code == _capi.IBH_EINVAL
    assert "Area of cell %d must be non-zero" % min(cells) in str(ei.value)
    w = mm.regrid_matrices("greenland", em, scale=True, correctA=True).matrix("IvE")      # the handle stays usable
    assert w.conservative and (w.nrow_d, w.ncol_d, w.nnz) == (plain.nrow, plain.ncol, plain.nnz)
    row, col, _ = w.coo_dense()
    np.testing.assert_array_equal(row, plain.row)
    np.testing.assert_array_equal(col, plain.col)
    np.testing.assert_array_equal(w.wM.view(np.uint64), plain.wM.view(np.uint64))
