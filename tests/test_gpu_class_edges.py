"""Elevations at the edges of the class table (tests/class_edge_cases.py) on a real MI355X: every scene through the general
pipeline, the per-range build and the streamed build -- the path asserted, every matrix bitwise the oracle's -- and every refusal
with the oracle's words, after which the same object still builds."""
import os
import sys

import numpy as np
import pytest

import icebin_amd
from oracle import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import class_edge_cases as cec
    from test_gpu_assembly_limits import path_of, reset_knobs
    from test_gpu_parity import assert_same_weighted
finally:
    sys.path.pop(0)

pytestmark = pytest.mark.gpu

# knobs -> the path of a G/P build: the general pipeline, the per-range build, the streamed build (None: the scene's stream_path)
PATHS = {"general": ({"assemble_fast": 0}, 0), "range": ({"assemble_stream": 0}, 1), "stream": ({"assemble_stream": 1}, None)}
BRANCHES = [(True, True), (False, False)]


def set_knobs(knobs):
    reset_knobs()
    for k, v in knobs.items():
        icebin_amd.set_tuning(k, v)


def oracle_of(name, cache={}):
    """The scene and the oracle's matrices, made once for the paths that share them (and never written)."""
    if name not in cache:
        g, em = cec.scene(**cec.LEGAL[name]["args"])
        rg = orc.Regridder(g)
        refs = {(m, sc, cA): rg.matrix_d(m, em, scale=sc, correctA=cA) for m in cec.E_MATRICES + ("AvI", "IvA") for sc, cA in BRANCHES}
        cache.clear()
        cache[name] = (g, em, refs)
    return cache[name]


@pytest.mark.parametrize("how", ["general", "range", "stream", "stream_device_mask"])
@pytest.mark.parametrize("name", list(cec.LEGAL))
def test_class_edges_bitwise(name, how):
    g, em, refs = oracle_of(name)
    knobs, path = PATHS[how.split("_")[0]]
    if path is None:
        path = cec.LEGAL[name]["stream_path"]
    mm = icebin_amd.from_synthetic(g)
    try:
        set_knobs(knobs)
        if how == "stream_device_mask":                           # the class bytes made in the pass that copies a device-resident mask
            import torch
            rm = mm.regrid_matrices("greenland", torch.from_numpy(em).cuda())
        else:
            rm = mm.regrid_matrices("greenland", em)
        for (m, sc, cA), ref in refs.items():
            what = "%s %s %s scale=%d correctA=%d" % (name, how, m, sc, cA)
            w = rm.matrix_d(m, scale=sc, correctA=cA)
            # (EvA / AvE have a per-range build of their own and no streamed one: they report 1 whenever a fast build is allowed)
            # (... and a matrix without classes reads no weights: the streamed build keeps it whatever the mask holds)
            plain = PATHS[how.split("_")[0]][1]
            want = min(path, 1) if m in ("EvA", "AvE") else path if m in cec.E_MATRICES else 2 if plain is None else plain
            assert path_of(w) == want, (what, path_of(w))
            assert_same_weighted(w, ref, what)
    finally:
        reset_knobs()


@pytest.mark.parametrize("how", ["general", "range", "stream"])
@pytest.mark.parametrize("name", list(cec.REFUSED))
def test_class_edge_refusals(name, how):
    args, _ = cec.REFUSED[name]
    g, em = cec.scene(**args)
    rg = orc.Regridder(g)
    mm = icebin_amd.from_synthetic(g)
    try:
        set_knobs(PATHS[how][0])
        rm = mm.regrid_matrices("greenland", em)
        for m in cec.E_MATRICES:
            with pytest.raises(orc.OracleError) as eo:
                rg.matrix_d(m, em)
            with pytest.raises(icebin_amd.IcebinHipError) as ei:
                rm.matrix_d(m)
            assert str(ei.value) == str(eo.value), (m, str(ei.value), str(eo.value))
            assert ei.value.code == -4, m
            # the same object still builds, through the path the knobs name -- AvI and IvA: every matrix with classes of this mask
            # is refused, those two ask for none
            for legal in ("AvI", "IvA"):
                w = rm.matrix_d(legal, scale=True, correctA=True)
                assert path_of(w) == {"general": 0, "range": 1, "stream": 2}[how], (name, how, legal, path_of(w))
                assert_same_weighted(w, rg.matrix_d(legal, em, scale=True, correctA=True), "%s %s %s after %s" % (name, how, legal, m))
        if "cells" in args:
            # the contrast: the same offenders under the mask are nobody's concern -- the scene builds, bitwise, through the same path
            masked = em.copy()
            masked[list(args["cells"])] = np.nan
            rm = mm.regrid_matrices("greenland", masked)
            for m in ("EvI", "IvE", "EvX", "XvE"):
                w = rm.matrix_d(m, scale=True, correctA=True)
                assert path_of(w) == {"general": 0, "range": 1, "stream": 2}[how], (name, how, m, path_of(w))
                assert_same_weighted(w, rg.matrix_d(m, masked, scale=True, correctA=True), "%s %s %s offenders masked" % (name, how, m))
    finally:
        reset_knobs()
