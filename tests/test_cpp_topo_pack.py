"""Compiles the C++ test of update_topo's packing (tests/cpp/test_topo_pack.cpp: VectorMultivec::append_planes / affine and
modele::TopoPacker of icebin_amd/host/icebin_hip.hpp) against libicebin_hip.so (g++, no HIP headers needed), runs it, and compares
the vectors of its two coupling steps with the Python surface, bitwise."""
import numpy as np
import pytest

import cpp_programs as cpp
from cpp_programs import read
from icebin_amd.build import build_library


def test_cpp_topo_pack_compiles_and_fails_loudly_without_gpu(tmp_path):
    cpp.fails_loudly_without_gpu("test_topo_pack", tmp_path, timeout=300)


def test_pack_kernels_are_wave64_without_scratch(tmp_path):
    """The gfx950 code object of multivec.hip by its metadata notes: the packing's kernels are there, every kernel
    of the unit is wave64 and none uses scratch memory."""
    import re
    from test_capi_symbols import code_object_notes
    build_library()
    notes = code_object_notes(tmp_path, "multivec")
    names = re.findall(r"^    \.name:\s+(\S+)", notes, re.M)
    scratch = [int(s) for s in re.findall(r"^    \.private_segment_fixed_size:\s+(\d+)", notes, re.M)]
    waves = [int(s) for s in re.findall(r"^    \.wavefront_size:\s+(\d+)", notes, re.M)]
    assert len(names) == len(scratch) == len(waves) and all("k_mv_" in n for n in names), names
    for kernel, count in (("k_mv_pack_count", 1), ("k_mv_pack_rank", 2), ("k_mv_packE", 1), ("k_mv_affine", 1)):
        assert sum(kernel in n for n in names) == count, (kernel, names)
    assert not [(n, s) for n, s in zip(names, scratch) if s != 0]
    assert set(waves) == {64}


@pytest.mark.gpu
def test_cpp_topo_pack_on_gpu(tmp_path):
    from icebin_amd import GCMRegridder, HntrSpec, TopoPacker, global_ec, make_topoA, merge_topoO
    r = cpp.run(cpp.exe("test_topo_pack", allow_compile=False), tmp_path, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    print(r.stdout)
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

    def retreated(em, I):
        em = em.copy()
        em.reshape(I.jm, I.im)[:, I.im // 2:] = np.nan
        return em
    c = np.arange(17, 32, 3)
    base = ([1500., 4000.], (c + O.size * (c % 2 == 0), c, 1e9 * (c + 1.)), (2 * O.size, O.size))
    hc = [0., 1500., 3000.]
    gcm = GCMRegridder(dict(nA=O.size, to_sparse=o, native_area=np.full(O.size, 1.e13)), hc, True)
    for k in (0, 1):
        idx, area = global_ec.gcm_from_hntr(O, Is[k], lands[k], hc, True, R).exgrid()
        gcm.add_sheet("sheet%d" % k, dict(nI=Is[k].size), dict(indices=idx.copy(), overlaps=area.copy()))
    m = gcm.to_modele((op, np.where(ocean, 1., 0.)), hspecO=O, eq_rad=R, global_ec=base)
    nA = m.hspecA.size
    packer = TopoPacker(("focean", "flake", "fgrnd", "fgice", "zatmo", "hlake"), ("fhc", "elevE", "underice_d"), (1, nA),
                        mmA=[1., 1., 1., 1., 9.80665, 1.], bbA=[0., 0., 0., 0., -3.5, 0.], mmE=[1., 2., 1.], bbE=[0., .5, 0.])
    masks = []
    for step in (1, 2):
        la = lands if step == 1 else [retreated(e, I) for e, I in zip(lands, Is)]
        ic = ices if step == 1 else [retreated(e, I) for e, I in zip(ices, Is)]
        t = topoo()
        mask, _ = merge_topoO(t, gcm, la, ic, O, R)
        w, _ = m.global_AvE(la, ic, t["FOCEANF"].reshape(-1), t["FOCEAN"].reshape(-1), scale=True)
        a, _ = make_topoA(t, mask, O, m.hspecA, (1, nA), m.hcdefs, [m.underice(k) for k in range(5)], w)
        A, E = packer.pack(a, 5, run_ice=step == 2)
        assert np.array_equal(read(tmp_path / ("step%d.mergemask" % step), np.int16), np.asarray(a["mergemask"]).reshape(-1))
        masks.append(np.asarray(a["mergemask"]).reshape(-1) != 0)
        for name, v in (("A", A), ("E", E)):
            p = str(tmp_path / ("step%d.%s" % (step, name)))
            assert np.array_equal(read(p + ".index", np.int64), v.index), (step, name)
            assert read(p + ".weights", np.float64).tobytes() == v.weights.tobytes(), (step, name)
            assert read(p + ".vals", np.float64).tobytes() == v.vals.tobytes() and len(v) > 0, (step, name)
    print("step 2: %d cells by the new mask, %d by the previous one alone" % (masks[1].sum(), (masks[0] & ~masks[1]).sum()))
