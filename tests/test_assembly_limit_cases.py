"""CPU-only: every grid of tests/assembly_limit_cases.py has the property its case claims, measured here with numpy from the
exchange cells, the areas and the elevation mask (no library), and every THRESHOLDS row has a case on each side."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import assembly_limit_cases as alc
finally:
    sys.path.pop(0)


def measure(g, em):
    """Every quantity a THRESHOLDS row speaks of, for grid g (sorted or not: ranges are runs of one atmosphere cell)."""
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
    cls = np.full(len(em), -1, np.int64)
    on = np.isfinite(em)
    cls[on] = np.searchsorted(g["hcdefs"], em[on])
    assert np.array_equal(g["hcdefs"][cls[on]], em[on]), "every ice cell sits exactly on a class"
    # straddling entries: distinct (range, ice cell) among the old cells (duplicates merge), by class
    sx = np.flatnonzero(old & (cls[iI] >= 0))
    pairs = np.unique(np.stack([rng_of[sx], iI[sx]], axis=1), axis=0) if len(sx) else np.zeros((0, 2), np.int64)
    seg = np.bincount(pairs[:, 0] * nhc + cls[pairs[:, 1]], minlength=nAr * nhc) if len(pairs) else np.zeros(1, np.int64)
    per_range_old = np.bincount(pairs[:, 0], minlength=nAr) if len(pairs) else np.zeros(1, np.int64)
    entries = np.bincount(rng_of[newrun], minlength=nAr)          # distinct (iA, iI) of every range: its entries (one class each)
    order_keys = iA * (int(g["nI"]) + 1) + iI
    mult = np.bincount(iI, minlength=int(g["nI"]))
    nzabs = np.abs(area[area != 0])
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
