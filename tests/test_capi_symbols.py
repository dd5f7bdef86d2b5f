"""CPU-only checks of the drop-in boundary: the C-ABI library loads, exports every symbol
include/icebin_hip.h declares, and fails loudly (no fallback) without a GPU."""
import ctypes as C
import os
import re

import pytest

from icebin_amd import _capi
from icebin_amd.build import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build_library()
    return _capi.lib()


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "icebin_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ibh_[A-Za-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported(lib):
    names = declared_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), "libicebin_hip.so does not export %s" % n
    assert set(_capi.exported_symbols()) == set(names), set(_capi.exported_symbols()) ^ set(names)


def test_sparse_set_host_logic(lib):
    from icebin_amd import SparseSet
    import numpy as np
    s = SparseSet(100, [7, 3, 99])
    assert s.sparse_extent() == 100 and s.dense_extent() == 3 and s.to_sparse().tolist() == [7, 3, 99]
    i = SparseSet.identity(5)
    assert i.to_sparse().tolist() == [0, 1, 2, 3, 4] and i.sparse_extent() == 5
    with pytest.raises(_capi.IcebinHipError, match="duplicate sparse index"):
        SparseSet(100, [1, 1])
    with pytest.raises(_capi.IcebinHipError, match="outside extent"):
        SparseSet(10, [11])


@pytest.mark.skipif(_capi.device_count() > 0, reason="checks the no-GPU failure mode")
def test_no_gpu_fails_loudly(lib):
    import numpy as np
    from icebin_amd import linear_Weighted, from_synthetic, synthetic
    with pytest.raises(_capi.IcebinHipError, match="no CPU fallback") as ei:
        linear_Weighted.from_coo((1, 1), [0], [0], [1.0], [1.0], [1.0])
    assert ei.value.code == _capi.IBH_ENODEVICE
    with pytest.raises(_capi.IcebinHipError, match="no CPU fallback"):
        from_synthetic(synthetic.make_grids("tiny"))


def test_product_never_imports_oracle():
    # the oracle is test infrastructure: nothing under icebin_amd/ may reference it
    pkg = os.path.join(ROOT, "icebin_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".hpp", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, re.M), f
                assert "liboracle" not in text and "icebin_oracle.h" not in text, f


def test_cython_module_builds_and_has_the_reference_surface():
    # pylib/_icebin.pyx:50-175: `import icebin` gives GCMRegridder / RegridMatrices with the reference's
    # method names and keyword defaults; compute fails loudly without a GPU (RuntimeError via `except +`)
    import sys
    from icebin_amd.cython.build_ext import build
    build()
    sys.path.insert(0, os.path.join(ROOT, "icebin_amd", "cython"))
    import icebin
    for cls, names in ((icebin.GCMRegridder, ("nA", "nE", "nhc", "wA", "add_sheet", "regrid_matrices")),
                       (icebin.RegridMatrices, ("matrix",)),
                       (icebin.linear_Weighted, ("apply_M", "apply_weight", "apply_wM", "apply_Mw", "to_coo", "get_weights", "shape"))):
        for n in names:
            assert hasattr(cls, n), (cls, n)
    g = icebin.GCMRegridder(dict(nA=4, to_sparse=[0, 1], native_area=[1., 1.]), [0., 100.], True)
    assert (g.nA, g.nE, g.nhc) == (4, 8, 2)
    with pytest.raises(ValueError, match="Invalid arguments"):
        icebin.GCMRegridder(1, 2)
    with pytest.raises(ValueError, match="snative"):
        g.wA("s", "bogus")
    if _capi.device_count() == 0:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            g.add_sheet("s", dict(nI=2), dict(indices=[[0, 0], [1, 1]], overlaps=[1., 1.]))


def test_missing_rccl_is_enotimpl_not_a_crash(lib):
    # with no librccl to be found, ibh_comm_unique_id must return IBH_ENOTIMPL ("multi-GPU exchange needs RCCL")
    # -- it used to build a std::string from dlerror()'s second, NULL, return.  A fresh process without torch (whose bundled
    # librccl would already be in the process), ICEBIN_RCCL_LIB naming a file that does not exist.
    import subprocess
    import sys
    code = (
        "import ctypes as C, sys\n"
        "L = C.CDLL(%r)\n"
        "L.ibh_last_error.restype = C.c_char_p\n"
        "buf = C.create_string_buffer(128)\n"
        "rc = L.ibh_comm_unique_id(buf)\n"
        "print(rc, L.ibh_last_error().decode())\n" % os.path.join(ROOT, "icebin_amd", "lib", "libicebin_hip.so"))
    env = dict(os.environ, ICEBIN_RCCL_LIB="/nonexistent/librccl.so")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rc, msg = r.stdout.strip().split(" ", 1)
    assert int(rc) == _capi.IBH_ENOTIMPL and "needs RCCL" in msg and "/nonexistent/librccl.so" in msg, r.stdout


def code_object_notes(tmp_path, name):
    """The metadata notes of the gfx950 code object in icebin_amd/lib/<name>.o: every kernel with its resource usage."""
    import subprocess
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    obj = os.path.join(ROOT, "icebin_amd", "lib", name + ".o")
    fatbin, dev = str(tmp_path / (name + ".hip_fatbin")), str(tmp_path / (name + "_gfx950.o"))
    subprocess.run([os.path.join(llvm, "llvm-objcopy"), "--dump-section=.hip_fatbin=" + fatbin, obj, str(tmp_path / "host.o")], check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--input=" + fatbin, "--output=" + dev], check=True)
    return subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", dev], check=True, capture_output=True, text=True).stdout


def spmm_code_object_notes(tmp_path):
    return code_object_notes(tmp_path, "spmm")


def test_no_apply_kernel_uses_scratch_memory(lib, tmp_path):
    # a kernel that spills registers to scratch is slow whether or not the dispatch picks it: no instantiation in spmm.hip may.
    # The code object's metadata lists every kernel with its private segment (scratch) size per lane.
    notes = spmm_code_object_notes(tmp_path)
    names = re.findall(r"^    \.name:\s+(\S+)", notes, re.M)
    sizes = [int(s) for s in re.findall(r"^    \.private_segment_fixed_size:\s+(\d+)", notes, re.M)]
    assert len(names) == len(sizes) and len(names) > 100, (len(names), len(sizes))
    spilling = [(n, s) for n, s in zip(names, sizes) if s != 0]
    assert not spilling, spilling


def demangle_template_args(mangled):
    """"_ZN3ibh20spmm_rowone_kernelILi8ELi14EEEvPKiS2_..." -> ("spmm_rowone_kernel", "<8, 14>"): the integer and bool template
    arguments of a kernel in namespace ibh, spelled as the demangler (and ibh_weighted_last_launch) spells them."""
    m = re.match(r"_ZN3ibh(\d+)", mangled)
    if not m:
        return None
    n = int(m.group(1))
    start = m.end()
    name, rest = mangled[start:start + n], mangled[start + n:]
    if not rest.startswith("I"):
        return None
    args = []
    for a in re.finditer(r"L([ib])(n?\d+)E", rest[1:rest.index("EE") + 2]):
        kind, v = a.group(1), a.group(2).replace("n", "-")
        args.append(("true" if v == "1" else "false") if kind == "b" else v)
    return name, "<" + ", ".join(args) + ">"


def test_every_apply_kernel_has_a_recipe(lib, tmp_path):
    # tests/apply_kernel_recipes.py holds one recipe per apply-kernel instantiation (tests/test_gpu_apply_kernels.py runs them all
    # against an exact reference): a kernel instantiated without a recipe, or a recipe for a kernel no longer built, fails here
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    try:
        import apply_kernel_recipes as akr
    finally:
        sys.path.pop(0)
    notes = spmm_code_object_notes(tmp_path)
    built = set()
    for mangled in re.findall(r"^    \.name:\s+(\S+)", notes, re.M):
        d = demangle_template_args(mangled)
        if d and re.fullmatch(r"spmm_\w+_kernel", d[0]):
            built.add(d[0] + d[1])
    recipes = {r["name"] for r in akr.RECIPES}
    assert built == recipes, ("built without a recipe", sorted(built - recipes), "recipe without a kernel", sorted(recipes - built))
    print("%d apply-kernel instantiations, one recipe each" % len(built))


PRIMS_TYPE_ARGS = {"j": "unsigned int", "h": "unsigned char", "t": "unsigned short", "i": "int", "m": "unsigned long", "y": "unsigned long long"}


def prims_kernel_name(mangled):
    """"_ZN3ibh12scan_chainedIjEEvPKT_..." -> "scan_chained<unsigned int>", "_ZN3ibh13oa_chunk_sortILi8192ELi4096ELi1024EEEv..." ->
    "oa_chunk_sort<8192, 4096, 1024>", "_ZN3ibh7rs_histEPKm..." -> "rs_hist": a kernel of namespace ibh as the demangler spells it
    (integer and builtin-type template arguments; anything else gives None)."""
    m = re.match(r"_ZN3ibh(\d+)", mangled)
    if not m:
        return None
    n = int(m.group(1))
    name, rest = mangled[m.end():m.end() + n], mangled[m.end() + n:]
    if rest.startswith("E"):
        return name
    m = re.match(r"I((?:Li\d+E|[a-z])+)EE", rest)
    if not m:
        return None
    args = [a[2:-1] if a.startswith("L") else PRIMS_TYPE_ARGS.get(a, a) for a in re.findall(r"Li\d+E|[a-z]", m.group(1))]
    return name + "<" + ", ".join(args) + ">"


def test_every_prims_kernel_is_exercised(lib, tmp_path):
    # tests/prims_kernel_cases.py names, for every kernel in prims.o, the case of tests/test_gpu_prims.py that runs it against an exact
    # reference: a kernel built without a case, or a case for a kernel no longer built, fails here
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    try:
        import prims_kernel_cases as pkc
    finally:
        sys.path.pop(0)
    mangled = re.findall(r"^    \.name:\s+(\S+)", code_object_notes(tmp_path, "prims"), re.M)
    built = {prims_kernel_name(m) for m in mangled}
    assert None not in built and len(built) == len(mangled), (sorted(mangled), sorted(map(str, built)))
    assert built == set(pkc.CASES), ("built without a case", sorted(built - set(pkc.CASES)), "case without a kernel",
                                     sorted(set(pkc.CASES) - built))
    module = open(os.path.join(ROOT, "tests", "test_gpu_prims.py")).read()
    for kernel, case in pkc.CASES.items():
        assert re.search(r"^def %s\(" % case, module, re.M), (kernel, case)


# the ibh_selftest_* entries of the integer primitives validate every argument before they touch a device
def test_selftest_scan_rejects_bad_arguments(lib):
    import numpy as np
    x = np.zeros(4, np.uint32)
    out, tot = np.zeros(16, np.uint32), np.zeros(3, np.uint32)
    for kind, n, flags in ((3, 4, 0), (-1, 4, 0), (0, -1, 0), (0, 1 << 31, 0), (1, 4, 1), (2, 4, 1), (0, 4, 8)):
        rc = lib.ibh_selftest_scan(kind, x.ctypes.data, n, out.ctypes.data, tot.ctypes.data, flags)
        assert rc == _capi.IBH_EINVAL, (kind, n, flags, rc)
    assert lib.ibh_selftest_scan(0, x.ctypes.data, 4, out.ctypes.data, None, 0) == _capi.IBH_EINVAL


def test_selftest_radix_sort_rejects_bad_fields(lib):
    import numpy as np
    k, kout, perm = np.arange(10, dtype=np.uint64), np.zeros(10, np.uint64), np.zeros(10, np.uint32)
    for fields in ([(0, 0)], [(0, 33)], [(40, 25)], [(33, 32)], [(-1, 4)], [(0, 4)] * 9):
        f = np.asarray(fields, np.int32).reshape(-1)
        rc = lib.ibh_selftest_radix_sort(k.ctypes.data, 10, f.ctypes.data, len(fields), kout.ctypes.data, perm.ctypes.data)
        assert rc == _capi.IBH_EINVAL, (fields, rc)
    f = np.asarray([0, 8], np.int32)
    assert lib.ibh_selftest_radix_sort(k.ctypes.data, -1, f.ctypes.data, 1, kout.ctypes.data, perm.ctypes.data) == _capi.IBH_EINVAL


def test_selftest_order_rejects_bad_arguments(lib):
    import ctypes as C
    import numpy as np
    perm, info, path = np.zeros(2, np.uint32), np.zeros(6, np.uint32), C.c_int(-1)
    for keys, lo, hi in (([1 << 40, 3], 20, 8), ([1 << 20, 3], 20, 12), ([3, 1], 33, 0), ([3, 1], 8, -1)):
        k = np.asarray(keys, np.uint64)
        rc = lib.ibh_selftest_order(k.ctypes.data, 2, lo, hi, 1, perm.ctypes.data, info.ctypes.data, C.byref(path))
        assert rc == _capi.IBH_EINVAL, (keys, lo, hi, rc)
    k = np.asarray([3, 1], np.uint64)
    assert lib.ibh_selftest_order(k.ctypes.data, 2, 20, 12, 2, perm.ctypes.data, info.ctypes.data, C.byref(path)) == _capi.IBH_EINVAL


def test_selftest_number_keys_rejects_bad_arguments(lib):
    import ctypes as C
    import numpy as np
    keys, ts = np.asarray([1, 2, 3, 0], np.int64), np.asarray([2, 0], np.int64)
    dense, table, n_new, status = np.zeros(4, np.int32), np.zeros(16, np.int64), C.c_int32(0), C.c_uint32(0)

    def call(key_bytes=8, stride=1, n=4, extent=8, to_sparse=ts.ctypes.data, n_old=2, identity=0, transform=0, check_range=0,
             k=keys.ctypes.data, d=dense.ctypes.data, t=table.ctypes.data, nn=C.byref(n_new), s=C.byref(status)):
        return lib.ibh_selftest_number_keys(k, key_bytes, stride, n, None, extent, to_sparse, n_old, identity, transform, check_range, d, t, nn, s)

    for bad in (dict(key_bytes=2), dict(key_bytes=16), dict(stride=0), dict(stride=-1), dict(n=-1), dict(n=1 << 31), dict(extent=-1),
                dict(extent=1 << 31), dict(transform=3), dict(transform=-1), dict(n_old=-2), dict(n_old=9), dict(identity=2),
                dict(check_range=2), dict(k=None), dict(d=None), dict(t=None), dict(nn=None), dict(s=None), dict(to_sparse=None),
                dict(extent=3),                     # key 3 outside [0, 3) without the range check (the old set's entries lie inside)
                dict(extent=2)):                    # ... and the old set's entry 2 outside its extent
        assert call(**bad) == _capi.IBH_EINVAL, bad
    dup = np.asarray([2, 2], np.int64)
    assert call(to_sparse=dup.ctypes.data) == _capi.IBH_EINVAL
    neg = np.asarray([1, -1, 3, 0], np.int64)
    assert call(k=neg.ctypes.data) == _capi.IBH_EINVAL


def assembly_kernel_name(mangled):
    """"_ZN3ibh9k_sa_emitILb1ELb0EjLi4EEEv..." -> "k_sa_emit<true, false, unsigned int, 4>": prims_kernel_name's spelling, with bool
    template arguments as well."""
    m = re.match(r"_ZN3ibh(\d+)", mangled)
    if not m:
        return None
    n = int(m.group(1))
    name, rest = mangled[m.end():m.end() + n], mangled[m.end() + n:]
    if rest.startswith("E"):
        return name
    m = re.match(r"I((?:Li\d+E|Lb[01]E|[a-z])+)EE", rest)
    if not m:
        return None
    args = []
    for a in re.findall(r"Li\d+E|Lb[01]E|[a-z]", m.group(1)):
        if a.startswith("Lb"):
            args.append("true" if a[2] == "1" else "false")
        elif a.startswith("L"):
            args.append(a[2:-1])
        else:
            args.append(PRIMS_TYPE_ARGS.get(a, a))
    return name + "<" + ", ".join(args) + ">"


def test_every_sorted_grid_assembly_kernel_has_a_case(lib, tmp_path):
    # tests/assembly_limit_cases.py names, for every kernel of the sorted-grid builds in assemble.o (the static plan k_plan_*, the
    # per-range build k_fa_*, the streamed build k_sa_*), a test that launches it: a kernel built without a case, or a case for a
    # kernel no longer built, fails here; so does a test named there that does not exist
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    try:
        import assembly_limit_cases as alc
    finally:
        sys.path.pop(0)
    mangled = [m for m in re.findall(r"^    \.name:\s+(\S+)", code_object_notes(tmp_path, "assemble"), re.M)
               if re.match(r"_ZN3ibh\d+k_(plan|fa|sa)_", m)]
    built = {assembly_kernel_name(m) for m in mangled}
    assert None not in built and len(built) == len(mangled) and len(built) > 80, (sorted(mangled), sorted(map(str, built)))
    named = set(alc.KERNELS) | set(alc.UNREACHABLE)
    assert not set(alc.KERNELS) & set(alc.UNREACHABLE)
    assert built == named, ("built without a case", sorted(built - named), "case without a kernel", sorted(named - built))
    modules = {}
    for kernel, test in alc.KERNELS.items():
        module, func = test.split("::")
        if module not in modules:
            modules[module] = open(os.path.join(ROOT, "tests", module)).read()
        base = func.split("[")[0]
        assert re.search(r"^def %s\(" % base, modules[module], re.M), (kernel, test)
        if "[" in func:
            case = func[func.index("[") + 1:-1]
            assert module == "test_gpu_assembly_limits.py" and case in {c["name"] for c in alc.CASES}, (kernel, test)


def test_smoother_and_apply_structure_kernels_live_in_their_own_units(lib, tmp_path):
    # the unit boundary, by kernel name: smooth.o holds the smoother's kernels and nothing else, applystruct.o the kernels of the
    # apply-structure builders (bands, sweep, row groups, tiles, the row expansions and the run heads the builders share; it
    # includes sweep_kernel.inl for the item meta bits only and instantiates no kernel of it), and assemble.o holds none of either
    smoother = r"k_smooth_|k_smt_"
    builders = r"k_band_|k_sw_|k_rg_|k_gt_|k_expand_|k_key_heads$"

    def names(unit):
        mangled = re.findall(r"^    \.name:\s+(\S+)", code_object_notes(tmp_path, unit), re.M)
        heads = [re.match(r"_ZN3ibh(\d+)", m) for m in mangled]
        assert all(heads), sorted(mangled)              # every kernel is named directly in namespace ibh
        return sorted(m[h.end():h.end() + int(h.group(1))] for m, h in zip(mangled, heads))

    in_smooth, in_builders, in_assembly = names("smooth"), names("applystruct"), names("assemble")
    assert len(in_smooth) >= 18 and all(re.match(smoother, n) for n in in_smooth), in_smooth
    assert len(in_builders) >= 20 and all(re.match(builders, n) for n in in_builders), in_builders
    strays = [n for n in in_assembly if re.match(smoother + "|" + builders, n)]
    assert not strays, strays


def csr_build_cases_module():
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    try:
        import csr_build_cases as cbc
    finally:
        sys.path.pop(0)
    return cbc


def assert_named_tests_exist(table):
    modules = {}
    for kernel, test in table.items():
        module, func = test.split("::")
        if module not in modules:
            modules[module] = open(os.path.join(ROOT, "tests", module)).read()
        assert re.search(r"^def %s\(" % func, modules[module], re.M), (kernel, test)


def test_every_csrops_kernel_and_every_triplet_build_kernel_has_a_case(lib, tmp_path):
    # tests/csr_build_cases.py names, for every kernel of csrops.o and every kernel of the triplets -> CSR layer, csrbuild.o, the
    # test that runs it against an exact reference: a kernel built without a case, or a case for a kernel no longer built, fails
    # here; so does a test named there that does not exist
    cbc = csr_build_cases_module()
    mangled = re.findall(r"^    \.name:\s+(\S+)", code_object_notes(tmp_path, "csrops"), re.M)
    built = {assembly_kernel_name(m.replace("12_GLOBAL__N_1", "", 1)) for m in mangled}
    assert None not in built and len(built) == len(mangled) >= 14, (sorted(mangled), sorted(map(str, built)))
    assert built == set(cbc.CSROPS_KERNELS), ("built without a case", sorted(built - set(cbc.CSROPS_KERNELS)), "case without a kernel",
                                              sorted(set(cbc.CSROPS_KERNELS) - built))
    mangled = re.findall(r"^    \.name:\s+(\S+)", code_object_notes(tmp_path, "csrbuild"), re.M)
    layer = {assembly_kernel_name(m) for m in mangled}
    assert None not in layer and len(layer) == len(mangled) >= 20, (sorted(mangled), sorted(map(str, layer)))
    assert layer == set(cbc.LAYER_KERNELS), ("built without a case", sorted(layer - set(cbc.LAYER_KERNELS)), "case without a kernel",
                                            sorted(set(cbc.LAYER_KERNELS) - layer))
    assert_named_tests_exist(cbc.CSROPS_KERNELS)
    assert_named_tests_exist(cbc.LAYER_KERNELS)


def test_selftest_triplets_rejects_bad_arguments(lib):
    import ctypes as C
    import numpy as np
    cbc = csr_build_cases_module()
    row, col, val = np.asarray([0, 1], np.int32), np.asarray([2, 0], np.int32), np.asarray([1., 2.])
    info, h = np.zeros(len(cbc.INFO), np.int32), C.c_void_p()

    def call(nrow=2, ncol=3, n=2, r=row, c=col, v=val, mode=0, out=C.byref(h), inf=info):
        p = lambda a: None if a is None else a.ctypes.data
        return lib.ibh_selftest_triplets(nrow, ncol, n, p(r), p(c), p(v), mode, out, p(inf))

    for bad in (dict(nrow=-1), dict(ncol=-1), dict(n=-1), dict(n=1 << 31), dict(mode=2), dict(mode=-1), dict(r=None), dict(c=None),
                dict(v=None), dict(out=None), dict(inf=None), dict(nrow=1), dict(ncol=2), dict(r=np.asarray([0, -1], np.int32)),
                dict(c=np.asarray([3, 0], np.int32)), dict(nrow=0, ncol=0)):
        assert call(**bad) == _capi.IBH_EINVAL, bad
        assert not h.value


def test_selftest_csr_op_rejects_bad_arguments(lib):
    import ctypes as C
    import numpy as np
    cbc = csr_build_cases_module()
    op = cbc.OPS
    i32, f64 = (lambda *x: np.asarray(x, np.int32)), (lambda *x: np.asarray(x, np.float64))
    h, vec = C.c_void_p(), np.zeros(8)
    # a handle is only looked at once the other arguments hold: without a GPU no matrix can be made, so the checks that need one
    # (lengths against its shape) are left to the GPU tests; here, everything that is wrong whatever the matrix

    def call(code, m=None, idx=None, a=None, b=None, nout=0, nidx=None, na=None, nb=None, out=C.byref(h), v=vec.ctypes.data):
        p = lambda x: None if x is None else x.ctypes.data
        n = lambda x, k: (0 if x is None else len(x)) if k is None else k
        return lib.ibh_selftest_csr_op(code, m, p(idx), n(idx, nidx), p(a), n(a, na), p(b), n(b, nb), nout, out, v)

    for bad in (dict(code=-1), dict(code=10), dict(code=op["recip"], a=f64(1, 2), nout=2, na=-1), dict(code=op["recip"], a=f64(1, 2), nout=3),
                dict(code=op["recip"], a=f64(1, 2), nout=2, v=None), dict(code=op["recip"], nout=2, na=2),
                dict(code=op["recip"], a=f64(1, 2), nout=2, idx=i32(0)), dict(code=op["mul"], a=f64(1, 2), b=f64(1), nout=2),
                dict(code=op["mul"], a=f64(1, 2), nout=2), dict(code=op["gather"], a=f64(1, 2), idx=i32(0, 2), nout=2),
                dict(code=op["gather"], a=f64(1, 2), idx=i32(0, -1), nout=2), dict(code=op["gather"], a=f64(1, 2), idx=i32(0), nout=2),
                dict(code=op["gather"], a=f64(1, 2), idx=i32(0, 1), nout=2, nidx=1 << 31), dict(code=op["transpose"]),
                dict(code=op["crop_rows"]), dict(code=op["crop_cols"]), dict(code=op["scale_rows"], a=f64(1)), dict(code=op["scale_cols"]),
                dict(code=op["scale_rows_recip"]), dict(code=op["expand_rows"]), dict(code=op["transpose"], out=None)):
        assert call(**bad) == _capi.IBH_EINVAL, bad
        assert not h.value
