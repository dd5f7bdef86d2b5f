"""Compiles the C++ test of the chunked global_ec (tests/cpp/test_global_ec_chunks.cpp) against libicebin_hip.so (g++, no HIP
headers needed), runs it, and compares its plan, masks and combined AvI / EvA with the Python surface (icebin_amd.global_ec),
bitwise."""
import numpy as np
import pytest

import cpp_programs as cpp
from cpp_programs import bits, read


def test_cpp_global_ec_chunks_compiles_and_fails_loudly_without_gpu(tmp_path):
    cpp.fails_loudly_without_gpu("test_global_ec_chunks", tmp_path, timeout=300)


@pytest.mark.gpu
def test_cpp_global_ec_chunks_on_gpu(tmp_path):
    from icebin_amd import HntrSpec, SparseSet, global_ec
    r = cpp.run(cpp.exe("test_global_ec_chunks", allow_compile=False), tmp_path, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    O, I = HntrSpec(8, 4, 0., 2700.), HntrSpec(32, 16, 0., 675.)
    x = np.arange(I.size)
    fg = np.where((x * 7 + x // 13) % 3 == 0, 0, 1 + x % 2).astype(np.int16).reshape(I.jm, I.im)
    el = ((x * 37) % 3000 - 200).astype(np.int16).reshape(I.jm, I.im)
    scan = global_ec.IceScan(O, I, fg, el)
    plan = scan.chunks(70)
    assert read(tmp_path / "chunks", np.int32).reshape(-1, 5).tolist() == [list(ch) for ch, _ in plan]
    assert read(tmp_path / "chunks.nice", np.int64).tolist() == [n for _, n in plan]
    assert np.array_equal(bits(read(tmp_path / "fgiceO", np.float64)), bits(scan.fgiceO.cpu().numpy().reshape(-1)))
    hc = global_ec.hcdefs(*scan.ec_range(500.), 500.)
    res = []
    for ch, _ in plan:
        mask = scan.chunk_mask(ch)
        assert np.array_equal(bits(read(tmp_path / ("mask%d" % ch[0]), np.float64)), bits(mask.cpu().numpy()))
        gcm = global_ec.gcm_from_hntr(O, I, mask, hc, True, 6371000.)
        rm = gcm.regrid_matrices("globalI", mask, scale=False, correctA=True)
        dimA, dimI, dimE = SparseSet(), SparseSet(), SparseSet()
        res.append(dict(AvI=rm.matrix_d("AvI", (dimA, dimI), scale=False, correctA=True),
                        EvA=rm.matrix_d("EvA", (dimE, dimA), scale=False, correctA=True), keep=(gcm, rm)))
    for name, mname, scale in (("AvI", "AvI", False), ("EvA", "EvA", False), ("EvA_scaled", "EvA", True)):
        w = global_ec.combine_chunks(res, mname, scale=scale)
        row, col, val = w.coo_dense()
        p = lambda ext: tmp_path / (name + ext)       # noqa: E731
        assert np.array_equal(read(p(".row"), np.int32), row), name
        assert np.array_equal(read(p(".col"), np.int32), col), name
        assert np.array_equal(bits(read(p(".val"), np.float64)), bits(val)), name
        assert np.array_equal(bits(read(p(".wM"), np.float64)), bits(w.wM)), name
        assert np.array_equal(bits(read(p(".Mw"), np.float64)), bits(w.Mw)), name
        assert np.array_equal(read(p(".dim0"), np.int64), w.dim(0)), name
        assert np.array_equal(read(p(".dim1"), np.int64), w.dim(1)), name
        if mname == "EvA":
            iB, iA, sv = w.coo_sparse()
            assert np.array_equal(bits(read(p(".stream"), np.float64)), bits(sv)), name
            if not scale:
                assert np.array_equal(read(p(".iB"), np.int64), iB) and np.array_equal(read(p(".iA"), np.int64), iA)
