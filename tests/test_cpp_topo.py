"""Compiles the C++ test of update_topo's field handling (tests/cpp/test_topo.cpp: merge_topoO, make_topoA and
GCMRegridder_ModelE::update_topo of icebin_amd/host/icebin_hip.hpp) against libicebin_hip.so (g++, no HIP headers needed), runs
it, and compares its planes and sanity-check strings with the Python surface, bitwise."""
import numpy as np
import pytest

import cpp_programs as cpp
from cpp_programs import read


def lines(path):
    with open(path) as f:
        return f.read().splitlines()


def test_cpp_topo_compiles_and_fails_loudly_without_gpu(tmp_path):
    cpp.fails_loudly_without_gpu("test_topo", tmp_path, timeout=300)


TOPOO = ("FOCEANF", "FGICEF", "ZATMOF", "FOCEAN", "FLAKE", "FGRND", "FGICE", "ZATMO", "ZICETOP", "ZLAND_MIN", "ZLAND_MAX")
TOPOA = ("focean", "flake", "fgrnd", "fgice", "zatmo", "hlake", "zicetop", "zland_min", "zland_max", "fhc", "elevE")


def same_topoo(tmp_path, name, topoo, mask):
    for k in TOPOO:
        assert read(tmp_path / (name + "." + k), np.float64).tobytes() == np.ascontiguousarray(topoo[k], np.float64).tobytes(), (name, k)
    assert np.array_equal(read(tmp_path / (name + ".mergemask"), np.int16), np.asarray(mask).reshape(-1)), name


def same_topoa(tmp_path, name, a):
    for k in TOPOA:
        assert read(tmp_path / (name + "." + k), np.float64).tobytes() == np.ascontiguousarray(a[k], np.float64).tobytes(), (name, k)
    for k in ("mergemask", "underice"):
        assert np.array_equal(read(tmp_path / (name + "." + k), np.int16), np.asarray(a[k]).reshape(-1)), (name, k)


@pytest.mark.gpu
def test_cpp_topo_on_gpu(tmp_path):
    from icebin_amd import GCMRegridder, HntrSpec, global_ec, make_topoA, merge_topoO
    r = cpp.run(cpp.exe("test_topo", allow_compile=False), tmp_path, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    R = 6371000.
    O, Is = HntrSpec(8, 6, 0., 1800.), (HntrSpec(48, 36, 0.5, 300.), HntrSpec(24, 18, 0.25, 600.))
    i0, i1 = np.arange(Is[0].size), np.arange(Is[1].size)
    lands = [np.where((i0 * 7) % 5 == 0, np.nan, (i0 % 3000) - 100.), np.where((i1 * 3) % 4 == 0, np.nan, ((i1 * 5) % 3000) + 200.)]
    with np.errstate(invalid="ignore"):
        ices = [np.where((i % 3 == 0) | ~((e >= 0.) & (e <= 3000.)), np.nan, e) for i, e in zip((i0, i1), lands)]
    o = np.arange(O.size)
    ocean = o % 5 == 0
    op = np.where(ocean, 1., np.where(o % 5 == 1, 0.25, 0.))
    land = lambda v: np.where(ocean, 0., v)     # noqa: E731

    def topoo():
        return dict(FOCEAN=np.where(ocean, 1., 0.), FOCEANF=op.copy(), FGICE=land(0.25), FLAKE=land(0.125), FGRND=land(0.625),
                    FGICEF=land(0.25 * (1. - op)), ZATMO=land(100. + o), ZATMOF=land((100. + o) * (1. - op)), ZICETOP=land(150. + o),
                    ZLAKE=land(5.))
    c = np.arange(17, 32, 3)
    base = ([1500., 4000.], (c + O.size * (c % 2 == 0), c, 1e9 * (c + 1.)), (2 * O.size, O.size))
    hc = [0., 1500., 3000.]
    gcm = GCMRegridder(dict(nA=O.size, to_sparse=o, native_area=np.full(O.size, 1.e13)), hc, True)
    for k in (0, 1):
        idx, area = global_ec.gcm_from_hntr(O, Is[k], lands[k], hc, True, R).exgrid()
        gcm.add_sheet("sheet%d" % k, dict(nI=Is[k].size), dict(indices=idx.copy(), overlaps=area.copy()))
    t = topoo()
    mask, errors = merge_topoO(t, gcm, lands, ices, O, R)
    assert errors == []
    same_topoo(tmp_path, "merged", t, mask)
    m = gcm.to_modele((op, np.where(ocean, 1., 0.)), hspecO=O, eq_rad=R, global_ec=base)
    w, offsetE = m.global_AvE(lands, ices, t["FOCEANF"].reshape(-1), t["FOCEAN"].reshape(-1), scale=True)
    a, errors2 = make_topoA(t, mask, O, m.hspecA, (1, m.hspecA.size), m.hcdefs, [m.underice(k) for k in range(5)], w)
    same_topoa(tmp_path, "topoa", a)
    assert lines(tmp_path / "topoa.errors.txt") == errors2
    threw = lines(tmp_path / "update.thrown.txt") == ["thrown"]
    assert threw == bool(errors2)
    t2 = topoo()
    if threw:
        with pytest.raises(RuntimeError, match="halting!"):
            m.update_topo(t2, lands, ices)
    else:
        out = m.update_topo(t2, lands, ices)
        same_topoa(tmp_path, "update", out)
        assert np.array_equal(read(tmp_path / "update.wEAm_base.iE", np.int64), out["wEAm_base"][0])
        assert read(tmp_path / "update.wEAm_base.w", np.float64).tobytes() == out["wEAm_base"][1].tobytes()
    # the planted errors
    bad = topoo()
    bad["ZATMOF"][[13, 2]] = np.nan
    bad["FLAKE"][30] = np.nan
    bad["FGRND"][11] += 1e-10
    mask, errors = merge_topoO(bad, gcm, lands, ices, O, R)
    assert errors == lines(tmp_path / "merged.errors.txt") and len(errors) >= 6
    same_topoo(tmp_path, "bad", bad, mask)
