"""CPU-only: every grid of tests/assembly_limit_cases.py has the property its case claims, measured here with numpy from the
exchange cells, the areas and the elevation mask (no library), and every THRESHOLDS row has a case on each side."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import assembly_limit_cases as alc
finally:
    sys.path.pop(0)


class ElevationOutOfBounds(ValueError):
    """linterp_1d_b's refusal: .ice is the ice cell, .elevation the clamped elevation"""

    def __init__(self, ice, elevation):
        ValueError.__init__(self, "ice cell %d elevation %r" % (ice, elevation))
        self.ice, self.elevation = ice, elevation


def class_pattern(hc, em, interp_style=0):
    """Per ice cell: the classes (i0, i1) and weights (w0, w1) of its elevation, in the operation order of the oracle's linterp_1d_b
    and IceRegridder_L0::GvEp (float64 numpy, no library).  Masked cells (NaN): classes -1, weights 0.  ELEV_CLASS_INTERP
    (interp_style 1): the nearest class, the lower one on a tie, as (i0, i0, 1, 0).  Raises ElevationOutOfBounds for the first ice
    cell (by index) beyond the last class."""
    hc, em = np.asarray(hc, np.float64), np.asarray(em, np.float64)
    nhc, n = len(hc), len(em)
    i0, i1 = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    w0, w1 = np.zeros(n), np.zeros(n)
    on = np.flatnonzero(~np.isnan(em))
    e = em[on]
    elevation = np.where(e < 0.0, 0.0, e)                          # std::max(elevation, 0.0): -0.0 stays -0.0
    lb = np.searchsorted(hc, elevation, side="left")               # std::lower_bound
    if interp_style == 0:
        hi = np.maximum(lb, 1)
        bad = np.flatnonzero(hi >= nhc)
        if len(bad):
            raise ElevationOutOfBounds(int(on[bad[0]]), float(elevation[bad[0]]))
        lo = hi - 1
        ratio = (elevation - hc[lo]) / (hc[hi] - hc[lo])
        i0[on], i1[on], w0[on], w1[on] = lo, hi, 1.0 - ratio, ratio
    else:
        hi = np.clip(lb, 1, max(nhc - 1, 1)) if nhc > 1 else np.ones(len(e), np.int64)
        lo = hi - 1
        if nhc > 1:
            d0, d1 = np.abs(elevation - hc[lo]), np.abs(hc[hi] - elevation)
            near = np.where(lb <= 0, 0, np.where(lb >= nhc, nhc - 1, np.where(d0 <= d1, lo, hi)))
        else:
            near = np.zeros(len(e), np.int64)
        i0[on], i1[on], w0[on], w1[on] = near, near, 1.0, 0.0
    return i0, i1, w0, w1


def cell_entries(g, em):
    """Per exchange cell: has0 / has1 (an entry of class c0 / c1 exists: weight != 0 and area * weight != 0), the classes, and
    under0 / under1 (area != 0, weight != 0, area * weight == 0)."""
    ex = g["ex_indices"].astype(np.int64)
    iI, area = ex[:, 1], np.asarray(g["ex_area"], np.float64)
    i0, i1, w0, w1 = class_pattern(g["hcdefs"], em, int(g.get("interp_style", 0)))
    with np.errstate(under="ignore"):
        v0, v1 = area * w0[iI], area * w1[iI]
    has0, has1 = (w0[iI] != 0) & (v0 != 0), (w1[iI] != 0) & (v1 != 0)
    under0, under1 = (area != 0) & (w0[iI] != 0) & (v0 == 0), (area != 0) & (w1[iI] != 0) & (v1 == 0)
    return dict(has0=has0, has1=has1, c0=i0[iI], c1=i1[iI], under0=under0, under1=under1, w0nz=w0[iI] != 0, w1nz=w1[iI] != 0)


def measure(g, em):
    """Every quantity a THRESHOLDS row speaks of, for grid g (sorted or not: ranges are runs of one atmosphere cell).  Entries are
    counted as the E-keyed matrices have them: per (range, ice cell) one for every class with a nonzero area * weight."""
    ex = g["ex_indices"].astype(np.int64)
    iA, iI, area = ex[:, 0], ex[:, 1], g["ex_area"]
    nX, nhc = len(iA), len(g["hcdefs"])
    key = iA * (int(g["nI"]) + 1) + iI
    head = np.r_[True, iA[1:] != iA[:-1]]
    rng_of = np.cumsum(head) - 1                                   # range of every exchange cell
    nAr = int(rng_of[-1]) + 1
    lengths = np.bincount(rng_of, minlength=nAr)
    newrun = np.r_[True, key[1:] != key[:-1]]
    runs = np.diff(np.r_[np.flatnonzero(newrun), nX])
    # first-seen exchange cell of every ice cell: the first one with a nonzero area
    nz = np.flatnonzero(area != 0)
    first = np.full(int(g["nI"]), nX, np.int64)
    np.minimum.at(first, iI[nz], nz)
    seen = first[iI] < nX
    old = seen & (rng_of[np.minimum(first[iI], nX - 1)] < rng_of)
    ce = cell_entries(g, em)
    # the entries of the E-keyed matrices, one row (range, ice cell, class, straddler) each: the cells of one (range, ice cell) merge.
    # A cell lists the classes of its nonzero weights, but not one whose product with a nonzero area underflows; a cell WITHOUT
    # area is counted with its classes (as the grids of one class per cell always were): no case that claims a count has one.
    lists0, lists1 = ce["w0nz"] & ~ce["under0"], ce["w1nz"] & ~ce["under1"]
    rows = np.concatenate([np.stack([rng_of[m], iI[m], c[m], old[m]], axis=1) for m, c in ((lists0, ce["c0"]), (lists1, ce["c1"]))])
    rows = np.unique(rows, axis=0)
    entries = np.bincount(rows[:, 0], minlength=nAr)                # entries of every range
    so = rows[rows[:, 3] == 1]
    seg = np.bincount(so[:, 0] * nhc + so[:, 2], minlength=nAr * nhc) if len(so) else np.zeros(1, np.int64)
    per_range_old = np.bincount(so[:, 0], minlength=nAr) if len(so) else np.zeros(1, np.int64)
    order_keys = iA * (int(g["nI"]) + 1) + iI
    mult = np.bincount(iI, minlength=int(g["nI"]))
    nzabs = np.abs(area[area != 0])
    rel16 = 2 * int(lengths.max()) <= 65535
    return {
        "sorted": int(np.count_nonzero(order_keys[1:] < order_keys[:-1])),
        "nhc": nhc,
        "ilmax": int(mult.max()),
        "dupmax": int(runs.max()),
        "tiny": float(nzabs.min()),
        "rel32_ep": 2 * int(lengths.max()),
        "rel32": int(lengths.max()),
        "emit_blocks": nX if 2 * lengths.max() > 65535 else 0,
        "oldseg_s": int(seg.max()),
        "oldseg_l": int(seg.max()),
        "default_oldseg": nX // nAr,
        "default_wpr4": nX // nAr,
        "default_wpr16": nX // nAr,
        "default_rowsl": nAr,
        "fa_oldmax": int(per_range_old.max()),
        "lcap_s0": set(entries.tolist()), "lcap_s1": set(entries.tolist()), "lcap_s2": set(entries.tolist()),
        "lcap_s3": set(entries.tolist()),
        "pass_s0": set(lengths.tolist()), "pass_s1": set(lengths.tolist()), "pass_s2": set(lengths.tolist()),
        "pass_s3": set(lengths.tolist()),
        "stream_default": nX,
        "optimistic": nX,
        "chained": nAr,
        "rscan_many": nAr,
        "psums": int(np.count_nonzero(mult > 1)),
        "entries_max": int(entries.max()),
        "entries_total": int(entries.sum()),
        "rel16_used": int(entries.max()) - 1 if rel16 else 0,
        "two_class": float(np.count_nonzero(ce["has0"] & ce["has1"])) / nX,
        "weight_underflow": int(np.count_nonzero(ce["under0"] | ce["under1"])),
    }


def _grid(case, cache={}):
    name = case["name"]
    if name not in cache:
        g, em = alc.build_grid(case["grid"])
        cache.clear()                                              # (one grid at a time: some hold millions of cells)
        cache[name] = (g, em, measure(g, em))
    return cache[name]


@pytest.mark.parametrize("case", alc.CASES, ids=[c["name"] for c in alc.CASES])
def test_every_grid_has_the_properties_its_case_claims(case):
    g, em, m = _grid(case)
    assert case["covers"], case["name"]
    for row, claim in case["covers"].items():
        assert row in alc.THRESHOLDS, row
        v = m[row]
        if row in alc.PER_RANGE:
            # a grid holds ranges on both sides: the claimed length, and the pass / LCAP limits one below and one above it
            lim = alc.THRESHOLDS[row][2]
            assert claim in v, (row, claim, sorted(v))
            if claim == lim:
                assert {lim - 1 if row.startswith("pass") else lim, lim} <= v | {lim}, (row, sorted(v))
            continue
        if claim == "in":
            assert alc.INSIDE[row](v), (case["name"], row, v)
        elif claim == "over":
            assert not alc.INSIDE[row](v), (case["name"], row, v)
        else:
            assert v == claim, (case["name"], row, v, claim)
    # the builds and paths are well-formed
    paths = case["path"] if isinstance(case["path"], list) else [case["path"]] * len(case["knobs"])
    assert len(paths) == len(case["knobs"]) and set(paths) <= {0, 1, 2}, case["name"]
    for name, branches, dims in case["builds"]:
        assert name in ("AvI", "IvA", "EvI", "IvE", "AvX", "XvA", "EvX", "XvE") and dims in ("own", "identity") and branches
    assert case.get("reference", "oracle") in ("oracle", "general")


def test_every_threshold_has_a_case_on_each_side():
    sides = {row: set() for row in alc.THRESHOLDS}
    exact = {row: set() for row in alc.THRESHOLDS}
    for case in alc.CASES:
        _, _, m = _grid(case)
        for row, claim in case["covers"].items():
            vals = [claim] if row in alc.PER_RANGE else [m[row]]
            if row in alc.PER_RANGE:
                lim, over = alc.THRESHOLDS[row][2], alc.THRESHOLDS[row][3]
                vals = [v for v in (lim - 1, lim, over) if v in m[row]]
            for v in vals:
                sides[row].add(bool(alc.INSIDE[row](v)))
                exact[row].add(v)
    for row, (where, what, inside, over) in alc.THRESHOLDS.items():
        assert sides[row] == {True, False}, ("a side without a case", row, sides[row])
        for v in (inside, over):
            if v not in ("in", "over"):
                assert v in exact[row], ("no case at", row, v, sorted(exact[row], key=str))
    for row in ("pass_s0", "pass_s1", "pass_s2", "pass_s3"):         # pass - 1, pass and pass + 1
        lim = alc.THRESHOLDS[row][2]
        assert {lim - 1, lim, lim + 1} <= exact[row], (row, exact[row])


def test_kernels_name_cases_that_exist():
    names = {c["name"] for c in alc.CASES}
    for kernel, test in alc.KERNELS.items():
        m = test.split("::")[1]
        if "[" in m and m.startswith("test_sorted_grid_limits"):
            assert m[m.index("[") + 1:-1] in names, (kernel, test)
    assert alc.SHARDED_CASE in names


# ---- the grids and the measured values of the cases from before the elevation spec ------------------------------------------------
# sha256 of em and of ex_area as build_grid made them before it knew `elev`
ARRAYS_BEFORE = {
    "sorted": ("6fce4d985774679bb383c8ef873da293d99c4019bb9230210b4591c67a008c15", "1c2bfc94b39a7fabfdb28bcc618ac9994e2654b4304cd0b5668dbb02f003fb58"),
    "rel32_ep_in": ("4466fc50e937679109fa5d92d6ab0bcdda911d7bf25dc2a22149bfc2e3284cad", "0187f23d0de19e79db4779d4879141e7d77f84f03c59f70a7284bc006c243c29"),
}
# the rows measure() had when it counted cells, and a digest of their values per case as it measured them then
ROWS_BEFORE = ("sorted", "nhc", "ilmax", "dupmax", "tiny", "rel32_ep", "rel32", "emit_blocks", "oldseg_s", "oldseg_l", "default_oldseg",
               "default_wpr4", "default_wpr16", "default_rowsl", "fa_oldmax", "lcap_s0", "lcap_s1", "lcap_s2", "lcap_s3", "pass_s0", "pass_s1",
               "pass_s2", "pass_s3", "stream_default", "optimistic", "chained", "rscan_many", "psums")
MEASURED_BEFORE = {
    "sorted": "5d4509f45f13f675",
    "inversion_first": "f1d0a3880bc9e36c",
    "inversion_last": "f1d0a3880bc9e36c",
    "nhc64": "74200424a58d6194",
    "nhc65": "8f0068f56d8486b3",
    "ilmax8": "6945ff65c8511330",
    "ilmax9": "4374d948617ebeee",
    "dup4": "69ee135460e72eb5",
    "dup5": "0c4e43495f7346c3",
    "area_at_cut": "99ce367ba70dae82",
    "area_above_cut": "613793f7a556e80d",
    "area_below_cut": "ffd2dc48c99aff82",
    "area_subnormal": "cadb8da00d0eb5e5",
    "rel32_ep_in": "6bc8cbf23332c94b",
    "rel32_ep_out": "c2f3143e6482b75c",
    "rel32_in": "144466ccb6aba1c5",
    "rel32_out": "3de91c1a11e8a2a7",
    "oldseg_s_128": "5a1fcb96befd57ea",
    "oldseg_s_129": "4692f09519954cc9",
    "oldseg_l_512": "a6f53280dcf07f90",
    "oldseg_l_513": "81a1d133d7fb4ac4",
    "oldseg_l_forced_512": "d8b7d8c060ef5421",
    "oldseg_l_forced_513": "fc0cc5677be82c5a",
    "fa_oldmax_512": "2fd7df84248a2e20",
    "fa_oldmax_513": "e5a7e8d7b2687bd4",
    "lcap_and_passes": "c730c4ad3dc84c9a",
    "lcap_and_passes_over": "057fd245e2dbe88b",
    "nx_2p20_minus_1": "9e2809a56deae6bb",
    "nx_2p20": "6d734a277af935b9",
    "nx_2p20_discard": "679248b77ce37c02",
    "nx_2p20_plus_1_discard": "b21bae3edacfeb5a",
    "chained_32767": "1c03cb3fbd5e3400",
    "chained_32768": "233104ff6d9c8b29",
    "rscan_4096": "f87d02d40b19a21d",
    "rscan_4097": "fded5d4fe7f2425e",
    "emit_blocks_and_psums": "750f2183174a8c26",
}


def test_the_default_elevations_build_the_same_arrays():
    by_name = {c["name"]: c for c in alc.CASES}
    for name, (h_em, h_area) in ARRAYS_BEFORE.items():
        g, em = alc.build_grid(by_name[name]["grid"])
        assert hashlib.sha256(em.tobytes()).hexdigest() == h_em, name
        assert hashlib.sha256(g["ex_area"].tobytes()).hexdigest() == h_area, name


def test_counting_entries_leaves_the_one_class_cases_as_measured():
    seen = set()
    for case in alc.CASES:
        if case["name"] not in MEASURED_BEFORE:
            continue
        _, _, m = _grid(case)
        text = repr([(k, sorted(m[k]) if isinstance(m[k], set) else m[k]) for k in ROWS_BEFORE])
        assert hashlib.sha256(text.encode()).hexdigest()[:16] == MEASURED_BEFORE[case["name"]], case["name"]
        assert m["two_class"] == 0 and m["weight_underflow"] == 0, case["name"]
        seen.add(case["name"])
    assert seen == set(MEASURED_BEFORE)


NEW_CASES = [c for c in alc.CASES if "elev" in c["grid"]]


@pytest.mark.parametrize("case", NEW_CASES, ids=[c["name"] for c in NEW_CASES])
def test_the_oracle_has_the_entries_the_restatement_counts(case):
    """EvX keeps every entry apart (nothing merges on X): its nonzeros are the restatement's entries; EvI merges the cells of one
    (GCM cell, ice cell): its nonzeros are the distinct (range, ice cell, class) with an entry."""
    from oracle import oracle as orc
    g, em, m = _grid(case)
    ce = cell_entries(g, em)
    ex = g["ex_indices"].astype(np.int64)
    rg = orc.Regridder(g)
    evx = rg.matrix_d("EvX", em, scale=False, correctA=False)
    assert evx.nnz == int(np.count_nonzero(ce["has0"]) + np.count_nonzero(ce["has1"])), case["name"]
    keys = np.concatenate([np.stack([ex[h, 0], ex[h, 1], c[h]], axis=1) for h, c in ((ce["has0"], ce["c0"]), (ce["has1"], ce["c1"]))])
    evi = rg.matrix_d("EvI", em, scale=False, correctA=False)
    assert evi.nnz == len(np.unique(keys, axis=0)), case["name"]
    if np.all(g["ex_area"] != 0):                                 # ... which is what measure() counts per range
        assert evi.nnz == m["entries_total"], case["name"]


def test_an_underflowing_product_drops_the_entry_in_the_oracle():
    from oracle import oracle as orc
    got = {}
    for case in alc.CASES:
        if case["name"] in ("weight_underflow", "weight_subnormal", "weight_on_class"):
            g, em = alc.build_grid(case["grid"])
            rg = orc.Regridder(g)
            got[case["name"]] = (rg.matrix_d("EvI", em, scale=False).nnz, rg.matrix_d("EvX", em, scale=False).nnz)
    assert got == {"weight_underflow": (806, 823), "weight_subnormal": (807, 824), "weight_on_class": (806, 823)}
