"""The inputs of tests/test_gpu_smoothing.py, checked on the CPU: every scene lies where its leg needs it -- members per bin, neighbours
per row, columns around a bin, row lengths, pairs at the cut, the bin grid's shape -- and the oracle's smoothed matrix has the structure
of the long-double definition with every entry inside the derived bound (smoothing_cases.entry_bound).  An input that drifts fails
here, on any machine, before a device build is asked what it made of it."""
import os
import sys

import numpy as np
import pytest

from oracle import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import smoothing_cases as smc
finally:
    sys.path.pop(0)


def assert_oracle_is_the_definition(g, em, plain, o, N, sigma):
    row, col, ref = smc.reference_ld(g, em, plain, sigma)
    np.testing.assert_array_equal(o.row, row)
    np.testing.assert_array_equal(o.col, col)
    return smc.assert_entries_within_bound(o.val, N, row, ref)


@pytest.mark.parametrize("nKr", smc.CLUSTERS_IVA, ids=lambda t: "%d-%d-%d" % t)
def test_cluster_scenes_iva(nKr):
    n, K, rowlen = nKr
    g, em, plain, o, f = smc.scene_case("IvA", smc.SIGMA_C, "cluster", n, K, rowlen)
    assert (plain.nrow, plain.ncol) == (n, K)
    assert f["widest"] == f["longest_smoothed"] == K and f["longest"] == rowlen
    assert np.all(f["N"] == n)                                   # every cell is every cell's neighbour ...
    assert (f["nbx"], f["nby"]) == (1, 1) and f["members"].max() == n      # ... and all share one bin
    for knobs in smc.KNOBS + ((1, 1),):
        smc.assert_input_side(smc.cluster_form(K, rowlen, knobs), knobs[1] > 0, knobs[0] > 0, f["widest"], f["longest"], f["longest_smoothed"])
    assert np.all(np.bincount(o.row, minlength=n) == K)
    assert_oracle_is_the_definition(g, em, plain, o, f["N"], smc.SIGMA_C)


def test_cluster_scenes_put_the_limits_where_the_legs_say():
    K = {c[1] for c in smc.CLUSTERS_IVA}
    assert {1, 64, 65, smc.SMT_KMAX, smc.SMT_KMAX + 1} <= K                 # slots / lanes 63 and 64, both tables full, and one more
    assert {smc.SMT_ROWMAX, smc.SMT_ROWMAX + 1} <= {c[2] for c in smc.CLUSTERS_IVA}
    n = {c[0] for c in smc.CLUSTERS_IVA}
    assert {1, 64, 65, smc.SMD_HITS, smc.SMD_HITS + 1, 32 * 64 + 1} <= n    # the hit list exactly full, drained, drained twice


@pytest.mark.parametrize("nKr,columns", list(zip(smc.CLUSTERS_IVE, (80, 128))), ids=lambda t: "-".join(map(str, t)) if isinstance(t, tuple) else str(t))
def test_cluster_scenes_ive(nKr, columns):
    n, K, rowlen = nKr
    g, em, plain, o, f = smc.scene_case("IvE", smc.SIGMA_C, "cluster", n, K, rowlen)
    assert plain.nrow == n and plain.ncol == columns
    assert f["widest"] == f["longest_smoothed"] == columns and f["longest"] == 2 and np.all(f["N"] == n)
    for knobs, form in zip(smc.KNOBS, (smc.TILE, smc.DIRECT, smc.TRIPLET)):
        smc.assert_input_side(form, knobs[1] > 0, knobs[0] > 0, f["widest"], f["longest"], f["longest_smoothed"])
    assert_oracle_is_the_definition(g, em, plain, o, f["N"], smc.SIGMA_C)


def test_lattice_scene_has_pairs_on_both_sides_of_the_cut():
    g, em, plain, o, f = smc.scene_case("IvA", smc.SIGMA_C, "lattice")
    assert plain.nrow == 256 and plain.ncol == 16 and f["longest"] == 1
    inside, outside = smc.cut_pairs(g, em, plain, smc.SIGMA_C)
    print("pairs within 1e-9 of the cut: %d inside, %d outside" % (inside, outside))
    assert inside + outside >= 100 and inside > 0 and outside > 0
    # the steps of LATTICE_STEPS are such pairs
    live, c = smc._tuples(g, em, plain)
    nds = smc._nds(c, 0, len(live), smc.SIGMA_C)
    s = np.asarray(plain.dims[0], np.int64)[live]
    ni, nj, nk = smc.LATTICE
    where = {int(v): q for q, v in enumerate(s)}
    for di, dj, dk in smc.LATTICE_STEPS:
        assert abs(nds[where[0], where[(di * nj + dj) * nk + dk]] - 4.0) < 1e-9
    assert f["nbx"] > 1 and f["nby"] > 1
    for knobs, form in zip(smc.KNOBS, (smc.TILE, smc.DIRECT, smc.TRIPLET)):
        smc.assert_input_side(form, knobs[1] > 0, knobs[0] > 0, f["widest"], f["longest"], f["longest_smoothed"])
    assert_oracle_is_the_definition(g, em, plain, o, f["N"], smc.SIGMA_C)


def test_far_pair_scene_spans_two_bins_of_two_sigmas():
    g, em, a, b = smc.far_pair_scene()
    _, _, plain, o, f = smc.scene_case("IvA", smc.FAR_SIGMA, "far")
    assert (smc.FAR_B - smc.FAR_A) / smc.FAR_SIGMA[0] < 2.0
    (qa, qb), neighbours, brings = smc.far_pair_facts(g, em, plain, a, b)
    assert qb - qa == 2, (qa, qb)
    assert neighbours and len(brings) >= 1
    s = np.asarray(plain.dims[0], np.int64)
    da = int(np.nonzero(s == a)[0][0])
    assert set(brings) <= set(o.col[o.row == da].tolist())      # the oracle keeps the pair: a's smoothed row holds b's own columns
    for knobs, form in zip(smc.KNOBS, (smc.TILE, smc.DIRECT, smc.TRIPLET)):
        smc.assert_input_side(form, knobs[1] > 0, knobs[0] > 0, f["widest"], f["longest"], f["longest_smoothed"])


@pytest.mark.parametrize("kind", ["one_column", "one_point", "one_cell", "all_masked"])
def test_degenerate_bin_grids(kind):
    g, em, plain, o, f = smc.scene_case("IvA", smc.SIGMA_C, kind)
    assert (f["nbx"], f["nby"]) == (1, 1)
    cen = np.asarray(g["I_centroid_xy"]).reshape(-1, 2)
    ext = cen.max(axis=0) - cen.min(axis=0)
    if kind == "one_column":
        assert ext[0] == 0 and ext[1] > 0
    if kind == "one_point":
        assert ext[0] == 0 and ext[1] == 0
    if kind == "all_masked":
        assert o.nnz == 0 and plain.nnz == 0
        return
    if kind == "one_cell":
        assert plain.nrow == 1 and np.all(f["N"] == 1)
        np.testing.assert_array_equal(o.col, plain.col)          # its row is its own row of M
    else:
        assert plain.nrow == 65 and np.all(f["N"] == 65) and f["members"].max() == 65
    for knobs, form in zip(smc.KNOBS, (smc.TILE, smc.DIRECT, smc.TRIPLET)):
        smc.assert_input_side(form, knobs[1] > 0, knobs[0] > 0, f["widest"], f["longest"], f["longest_smoothed"])
    assert_oracle_is_the_definition(g, em, plain, o, f["N"], smc.SIGMA_C)


def test_capped_bin_grid_on_one_axis():
    g, em = smc.scene("cluster", 65, 3, 1)
    sigma = smc.capped_sigma(g)
    _, _, plain, o, f = smc.scene_case("IvA", sigma, "cluster", 65, 3, 1)
    assert (f["nbx"], f["nby"]) == (smc.MAX_BINS, 1)
    cen = np.asarray(g["I_centroid_xy"]).reshape(-1, 2)
    x0, y0, bw, bh, nbx, nby = smc.smooth_grid(cen.min(axis=0), cen.max(axis=0), sigma)
    assert bw > 2.0 * sigma[0] and bh > 2.0 * sigma[1]          # the regrown bin width: bins only grow
    assert f["N"].min() == 1 and f["N"].max() <= 3               # a cell is its own neighbour in x, unless two share an x within 2 sigma_x
    for knobs, form in zip(smc.KNOBS, (smc.TILE, smc.DIRECT, smc.TRIPLET)):
        smc.assert_input_side(form, knobs[1] > 0, knobs[0] > 0, f["widest"], f["longest"], f["longest_smoothed"])
    assert_oracle_is_the_definition(g, em, plain, o, f["N"], sigma)


def test_bins_only_grow_and_neighbours_stay_within_one_bin():
    """smooth_grid: a bin is wider than two sigmas on every branch, the cap's included; and no two coordinates less than two sigmas
    apart fall more than one bin apart -- tried on coordinates a few ulps around the bin edges of grids far from the origin"""
    rng = np.random.default_rng(5)
    for _ in range(300):
        sx = 10.0 ** rng.uniform(1, 5)
        ext = sx * 10.0 ** rng.uniform(0, 4.5)
        x0 = (rng.random() - 0.5) * 10.0 ** rng.uniform(3, 9)
        _, _, bw, _, nbx, _ = smc.smooth_grid((x0, 0.0), (x0 + ext, 0.0), (sx, 1.0, 1.0))
        assert bw > 2.0 * sx and 1 <= nbx <= smc.MAX_BINS
        assert int((x0 + ext - x0) / bw) <= nbx - 1
        k = rng.integers(1, max(nbx, 2), 64)
        a = x0 + k * (2.0 * sx)
        for _ in range(int(rng.integers(0, 4))):
            a = np.nextafter(a, -np.inf)
        b = a + np.nextafter(2.0 * sx, 0.0)
        ok = (b <= x0 + ext) & ((b - a) / sx < 2.0)
        qa, qb = ((a - x0) / bw).astype(np.int64), ((b - x0) / bw).astype(np.int64)
        assert np.all((qb - qa)[ok] <= 1)


def test_zero_area_scenes():
    # one unmasked cell without area: the reference's refusal, naming the cell
    one = smc.ZERO_AREA_ONE
    g, em = smc.zero_area_scene([one])
    plain = orc.Regridder(g).matrix_d("IvE", em, scale=True, correctA=True)
    assert plain.nrow == 65 and np.nonzero(plain.wM == 0.0)[0].tolist() == [list(plain.dims[0]).index(one)]
    with pytest.raises(orc.OracleError, match="Area of cell %d must be non-zero" % one):
        orc.Regridder(g).matrix_d("IvE", em, scale=True, correctA=True, sigma=smc.SIGMA_C)
    # two: the reference walks the cells in ascending index and names the smaller; their dense rows are in the opposite order
    lo, hi = smc.ZERO_AREA_PAIR
    g, em = smc.zero_area_scene([lo, hi])
    plain = orc.Regridder(g).matrix_d("IvE", em, scale=True, correctA=True)
    s = np.asarray(plain.dims[0], np.int64).tolist()
    assert lo < hi and s.index(hi) < s.index(lo)
    assert plain.wM[s.index(lo)] == 0.0 and plain.wM[s.index(hi)] == 0.0 and np.count_nonzero(plain.wM == 0.0) == 2
    with pytest.raises(orc.OracleError, match="Area of cell %d must be non-zero" % lo):
        orc.Regridder(g).matrix_d("IvE", em, scale=True, correctA=True, sigma=smc.SIGMA_C)


@pytest.mark.parametrize("leg", range(len(smc.BIG_LEGS)), ids=[l[0] for l in smc.BIG_LEGS])
def test_grid_legs_with_several_waves_per_bin(leg):
    _, config, name, sigma, want = smc.BIG_LEGS[leg]
    g, em = smc.grids(config)
    plain, o, widest, longest, longest_smoothed = smc.oracle_case(config, name, sigma)
    members, nb = smc.bin_members(g, em, plain, sigma)
    N = smc.neighbour_counts(g, em, plain, sigma)
    got = dict(rows=int((N > 0).sum()), bins=nb, fullest=int(members.max()), widest=widest, longest=longest, longest_smoothed=longest_smoothed,
               neighbours=int(N.max()))
    print(got)
    assert got == want
    assert members.max() > 64                                    # several waves in one bin of the tile form, the last with dead lanes
    assert members.max() % 64 != 0
    if config == "g20":
        assert N.max() > smc.SMD_HITS - 64                       # the direct form's hit list drains before the end of pass 2
    else:
        assert widest == smc.SMT_KMAX                            # the tile form's column table exactly full
    for knobs, form in zip(smc.KNOBS, (smc.TILE, smc.DIRECT, smc.TRIPLET)):
        smc.assert_input_side(form, knobs[1] > 0, knobs[0] > 0, widest, longest, longest_smoothed)
