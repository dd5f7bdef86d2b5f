"""update_topo's packing on the GPU (ibh_multivec_append_planes_*, ibh_multivec_affine_device, VectorMultivec.append_planes /
.affine, modele.TopoPacker, GCMRegridder_ModelE.update_topo(packer=...)) against the plain-Python restatement of the reference's
loops (tests/topo_pack_restatement.py, pinned by tests/test_topo_pack_restatement.py).  Every comparison is exact: index equal,
weights and vals as uint64 bit patterns."""
import ctypes as C
import itertools
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topo_pack_restatement as pr  # noqa: E402

# the launch shapes of icebin_amd/csrc/multivec.hip: a rank block takes PK_TILE = 256 threads x 8 passes cells and, up to
# PK_SELF_TILES tiles, sums the counts of the tiles before it itself (beyond, a scan does); a pack block takes AP_ROWS kept cells of
# one class and walks the variables in chunks of AP_VC through LDS
PK_TILE, PK_SELF_TILES, AP_ROWS, AP_VC = 2048, 1024, 64, 32
DENSITIES = (0., 0.03, 0.5, 1.)
NCLASS = (1, 3)
NVAR = (1, 3, 6, AP_VC - 1, AP_VC, AP_VC + 1)         # 6 and 3: the contract's widths; the rest straddle the LDS variable chunk
COMBOS = list(itertools.product(DENSITIES, NCLASS, NVAR))


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64).reshape(-1)).view(np.uint64)


def make_mask(rng, ncell, density):
    """int16 with kept values out of {1, -1, 7}"""
    return np.where(rng.random(ncell) < density, rng.choice(np.asarray([1, -1, 7], np.int16), ncell), np.int16(0)).astype(np.int16)


def make_planes(nvar, n):
    """plane k holds k * 1e7 + position + 0.25: every value names where it came from"""
    return np.arange(n, dtype=np.float64)[None, :] + 1e7 * np.arange(nvar, dtype=np.float64)[:, None] + 0.25


def reference(planes, mask, mask0, nclass, strides, into=None):
    """The restatement's pack_E on a 1 x ncell grid (pack_A is its nclass = 1): planes as lists (an int16 plane through
    underice_d), a missing mask0 as zeros (:1122 then reads the mask alone)."""
    ncell = len(mask)
    lists = [pr.underice_d(p.tolist()) if p.dtype == np.int16 else p.tolist() for p in planes]
    v = pr.VectorMultivec(len(planes)) if into is None else into
    pr.pack_E(v, lists, nclass, mask.tolist(), [0] * ncell if mask0 is None else mask0.tolist(), ncell, 1,
              lambda i, j, ihc: i * strides[0] + ihc * strides[1])
    return v


def same(vec, ref, what):
    assert vec.size() == ref.size(), (what, vec.size(), ref.size())
    assert np.array_equal(vec.index, np.asarray(ref.index, np.int64)), what
    assert np.array_equal(bits(vec.weights), bits(ref.weights)), what
    assert np.array_equal(bits(vec.vals), bits(ref.vals)), what


def to_device(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pack(vec, planes, mask, mask0, device=True, **kw):
    if device:
        planes, mask, mask0 = [to_device(p) for p in planes], to_device(mask), to_device(mask0)
    return vec.append_planes(list(planes), mask, mask0, **kw)


def one_case(vecs, rng, ncell, density, nclass, nvar, with_mask0, device=True, strides=None):
    from icebin_amd import VectorMultivec
    mask = make_mask(rng, ncell, density)
    mask0 = make_mask(rng, ncell, density / 2 if density < 1 else 0.5) if with_mask0 else None
    planes = make_planes(nvar, nclass * ncell)
    strides = (1, ncell) if strides is None else strides
    if nvar not in vecs:
        vecs[nvar] = VectorMultivec(nvar)
    vec = vecs[nvar]
    vec.clear()
    nkept = pack(vec, planes, mask, mask0, device, nclass=nclass, index_strides=strides)
    ref = reference(list(planes), mask, mask0, nclass, strides)
    what = dict(ncell=ncell, density=density, nclass=nclass, nvar=nvar, mask0=with_mask0, device=device)
    assert nkept * nclass == ref.size() and nkept == np.count_nonzero((mask != 0) | (mask0 != 0 if with_mask0 else False)), what
    same(vec, ref, what)
    return nkept


# ---- 1. kernel edges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_mask0", [False, True])
def test_every_ncell_up_to_600(with_mask0):
    """Every ncell 1 .. 600: below, at and above a wave, a pack block (64 kept cells) and the passes of a rank block; density,
    nclass and nvar cycle through all their combinations (7 is coprime to their number, so each meets a dozen sizes)."""
    rng = np.random.default_rng(11 + with_mask0)
    vecs, seen = {}, set()
    for ncell in range(1, 601):
        density, nclass, nvar = COMBOS[(ncell * 7 + 5 * with_mask0) % len(COMBOS)]
        one_case(vecs, rng, ncell, density, nclass, nvar, with_mask0)
        seen.add((density, nclass, nvar))
    assert seen == set(COMBOS)


@pytest.mark.parametrize("ncell", [4095, 4096, 4097])
def test_around_two_rank_blocks(ncell):
    """Two rank blocks, exactly and one cell either way (PK_TILE = 2048): every (nclass, nvar) pair over the three sizes."""
    rng = np.random.default_rng(ncell)
    pairs = list(itertools.product(NCLASS, NVAR))
    vecs = {}
    for k, density in enumerate(DENSITIES):
        nclass, nvar = pairs[((ncell - 4095) * len(DENSITIES) + k) % len(pairs)]
        one_case(vecs, rng, ncell, density, nclass, nvar, with_mask0=bool(k % 2))


def test_rank_spans_many_blocks():
    """70 001 cells: a rank block takes PK_TILE = 2048 cells, so the rank spans 35 blocks (the issue asks for at least three) and
    the last holds 369 cells."""
    ncell = 70001
    assert -(-ncell // PK_TILE) == 35 >= 3 and ncell % PK_TILE == 369
    rng = np.random.default_rng(70001)
    vecs = {}
    for density, nclass, nvar, with_mask0 in ((0., 3, 33, False), (0.03, 3, 31, True), (0.5, 3, 3, True), (1., 1, 6, False)):
        nkept = one_case(vecs, rng, ncell, density, nclass, nvar, with_mask0)
        assert (nkept == 0) == (density == 0.) and (nkept == ncell) == (density == 1.)


@pytest.mark.parametrize("over", [0, 1])
def test_both_sides_of_the_self_summing_limit(over):
    """PK_SELF_TILES tiles: the rank blocks sum the counts of the tiles before them themselves; one more: the counts are scanned."""
    ncell = PK_SELF_TILES * PK_TILE + over
    assert -(-ncell // PK_TILE) == PK_SELF_TILES + over
    nkept = one_case({}, np.random.default_rng(5 + over), ncell, 0.03, 1, 1, with_mask0=False)
    assert 0.02 * ncell < nkept < 0.04 * ncell


@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("ncell", [333, 2500])
def test_every_width_and_class_count(ncell, device):
    """nvar x nclass x mask0 in full, on one and on two rank blocks, from device tensors and from numpy arrays (the host entry);
    index strides (1, ncell) and (nclass, 1) alternate."""
    rng = np.random.default_rng(ncell + device)
    vecs = {}
    for k, (nclass, nvar, with_mask0) in enumerate(itertools.product(NCLASS, NVAR, (False, True))):
        one_case(vecs, rng, ncell, 0.5, nclass, nvar, with_mask0, device=device, strides=(nclass, 1) if k % 2 else None)


@pytest.mark.parametrize("device", [True, False])
def test_behind_existing_entries_and_twice(device):
    """A vector that already holds 5 entries, then two packs in a row with the two index orders: the entries lie behind one
    another, the first five are untouched."""
    from icebin_amd import VectorMultivec
    rng = np.random.default_rng(3)
    ncell, nvar = 700, 6
    vec, ref = VectorMultivec(nvar), pr.VectorMultivec(nvar)
    ix, w, v = np.arange(5) * 11 + 100000, rng.random(5), rng.standard_normal((5, nvar))
    vec.add(ix, v, w)
    for k in range(5):
        ref.add(int(ix[k]), v[k].tolist(), float(w[k]))
    for nclass, strides, seed in ((3, (1, ncell), 1), (2, (2, 1), 2)):
        mask, mask0 = make_mask(np.random.default_rng(seed), ncell, 0.4), make_mask(np.random.default_rng(seed + 10), ncell, 0.1)
        planes = make_planes(nvar, nclass * ncell) * (seed + 1)
        nkept = pack(vec, planes, mask, mask0, device, nclass=nclass, index_strides=strides)
        before = ref.size()
        reference(list(planes), mask, mask0, nclass, strides, into=ref)
        assert nkept * nclass == ref.size() - before
        same(vec, ref, (device, nclass))


@pytest.mark.parametrize("device", [True, False])
def test_int16_plane_and_special_doubles_keep_their_bits(device):
    """One int16 plane among doubles, holding -32768 and 32767; doubles with NaN payloads of both signs, -0.0, denormals and
    infinities: copied bit for bit."""
    from icebin_amd import VectorMultivec
    rng = np.random.default_rng(8)
    ncell, nclass = 300, 2
    n = ncell * nclass
    special = np.asarray([0x7ff8000000000001, 0xfff8000000abcdef, 0x7ffc0000deadbeef, 0x8000000000000000, 0x0000000000000001,
                          0x800fffffffffffff, 0x7ff0000000000000, 0xfff0000000000000, 0x0010000000000000], np.uint64)
    p0 = special[rng.integers(0, len(special), n)].view(np.float64)
    p1 = rng.integers(-32768, 32768, n).astype(np.int16)
    p1[[0, 1, ncell, n - 1]] = [-32768, 32767, 32767, -32768]
    p2 = rng.standard_normal(n)
    mask = make_mask(rng, ncell, 0.6)
    mask[[0, 1, ncell - 1]] = 7
    vec = VectorMultivec(3)
    nkept = pack(vec, [p0, p1, p2], mask, None, device, nclass=nclass)
    ref = reference([p0, p1, p2], mask, None, nclass, (1, ncell))
    same(vec, ref, device)
    got = vec.vals
    assert nkept == np.count_nonzero(mask) and set(bits(got[:, 0]).tolist()) == set(special.tolist())
    assert got[0, 1] == -32768. and got[1, 1] == 32767. and got[nkept, 1] == 32767. and got[-1, 1] == -32768.
    # an int16 plane named as such explicitly, and the default (by dtype), are the same call
    vec2 = VectorMultivec(3)
    pack(vec2, [p0, p1, p2], mask, None, device, nclass=nclass, types=[0, 1, 0])
    assert np.array_equal(bits(vec2.vals), bits(got))


@pytest.mark.parametrize("device", [True, False])
def test_no_cells_and_no_classes_append_nothing(device):
    from icebin_amd import VectorMultivec
    vec = VectorMultivec(2)
    vec.add([4], [[1., 2.]], [.5])
    empty, mask = np.zeros(0), np.asarray([1, 0, 1], np.int16)
    assert pack(vec, [empty, empty], np.zeros(0, np.int16), None, device) == 0
    assert pack(vec, [np.ones(3), np.ones(3)], mask, None, device, nclass=0) == 2       # the kept cells are still counted
    assert pack(vec, [np.ones(3), np.ones(3)], np.zeros(3, np.int16), np.zeros(3, np.int16), device, nclass=2, plane_class_stride=0) == 0
    assert vec.size() == 1 and vec.index.tolist() == [4] and vec.vals.tolist() == [[1., 2.]] and vec.weights.tolist() == [.5]


# ---- 2. round trip ----------------------------------------------------------------------------------------------------------
def test_round_trip_through_update_dense():
    """append_planes with nclass = 1, then update_dense with a scale of ones onto sentinel-filled arrays: 0.0 + v = v on the kept
    cells (no -0.0 among the values), the sentinel everywhere else."""
    import torch
    from icebin_amd import VectorMultivec
    rng = np.random.default_rng(21)
    ncell, nvar, sentinel = 5000, 6, -7.25
    planes = rng.standard_normal((nvar, ncell))
    planes[1, ::5] = 5e-324
    assert not np.any((planes == 0.) & np.signbit(planes))
    mask, mask0 = make_mask(rng, ncell, 0.3), make_mask(rng, ncell, 0.1)
    kept = (mask != 0) | (mask0 != 0)
    vec = VectorMultivec(nvar)
    assert pack(vec, planes, mask, mask0, nclass=1) == kept.sum()
    out = torch.full((nvar, ncell), sentinel, dtype=torch.float64, device="cuda")
    vec.update_dense(torch.ones(ncell, dtype=torch.float64, device="cuda"), out)
    got = out.cpu().numpy()
    assert np.array_equal(bits(got[:, kept]), bits(planes[:, kept]))
    assert np.all(got[:, ~kept] == sentinel) and 0 < kept.sum() < ncell


# ---- 3. affine --------------------------------------------------------------------------------------------------------------
def test_affine_is_a_product_then_an_add_and_keeps_the_grouping():
    import torch
    from icebin_amd import VectorMultivec
    rng = np.random.default_rng(31)
    nvar, n, nE = 19, 3000, 500                  # 19 variables: two launches of the 16-variable coefficient chunk
    x = 1. + 2. ** -30
    vals = rng.standard_normal((n, nvar)) * 10. ** rng.integers(-3, 4, (n, nvar))
    mm, bb = rng.uniform(-3., 3., nvar), rng.uniform(-100., 100., nvar)
    vals[::7, 2], mm[2], bb[2] = x, x, -1.       # x * x + -1: the product rounds 2^-60 away, a fused multiply-add would keep it
    vals[::11, 17], mm[17], bb[17] = x, x, -1.
    vals[6, 1] = -0.
    index, weights = rng.integers(0, nE, n), rng.uniform(.5, 2., n)
    # the test shows something only if, somewhere, the correctly rounded v * mm + bb differs from the two-step result
    differs = 0
    for ix in range(0, n, 7):
        exact = Fraction(float(vals[ix, 2])) * Fraction(float(mm[2])) + Fraction(float(bb[2]))
        two_step = float(vals[ix, 2]) * float(mm[2]) + float(bb[2])
        fused = float(exact)                     # Fraction -> float rounds to nearest even, as a fused multiply-add does
        differs += fused != two_step
    assert differs > 0 and two_step == 2. ** -29 and fused == 2. ** -29 + 2. ** -60
    vec, ref = VectorMultivec(nvar), pr.VectorMultivec(nvar)
    vec.add(index, vals, weights)
    for k in range(n):
        ref.add(int(index[k]), vals[k].tolist(), float(weights[k]))
    scale0 = vec.to_dense_scale(nE).cpu().numpy()
    dense0 = vec.to_dense(torch.from_numpy(scale0).cuda(), -1.).cpu().numpy()
    vec.affine(mm, bb)
    pr.convert_units(ref, mm.tolist(), bb.tolist())
    same(vec, ref, "affine")
    assert vec.vals[0, 2] == 2. ** -29
    # the grouping survives (no index changed): the scale has the same bits, and to_dense is the converted values merged
    scale1 = vec.to_dense_scale(nE).cpu().numpy()
    assert np.array_equal(bits(scale0), bits(scale1))
    fresh = VectorMultivec(nvar)
    fresh.add(index, np.asarray(ref.vals).reshape(n, nvar), weights)
    want = fresh.to_dense(torch.from_numpy(scale0).cuda(), -1.).cpu().numpy()
    got = vec.to_dense(torch.from_numpy(scale1).cuda(), -1.).cpu().numpy()
    assert np.array_equal(bits(got), bits(want)) and not np.array_equal(bits(got), bits(dense0))
    # an empty vector is left alone
    VectorMultivec(2).affine([1., 2.], [0., 0.])


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_vector_alone():
    import torch
    from icebin_amd import VectorMultivec, _capi
    L = _capi.lib()
    ncell = 100
    vec, other = VectorMultivec(2), VectorMultivec(3)
    vec.add([4, 9], [[1., 2.], [3., 4.]], [.5, .25])
    planes = [torch.ones(ncell, dtype=torch.float64, device="cuda") for _ in range(2)]
    mask = torch.ones(ncell, dtype=torch.int16, device="cuda")
    table = (C.c_void_p * 2)(*[p.data_ptr() for p in planes])
    holed = (C.c_void_p * 2)(planes[0].data_ptr(), None)
    types_bad = np.asarray([0, 2], np.int32)
    m = C.c_void_p(mask.data_ptr())
    nkept = C.c_int64(-5)

    def call(mv=vec._h, tab=table, types=None, nvar=2, n=ncell, nclass=1, stride=ncell, mask=m, mask0=None, sc=1, sh=ncell):
        return L.ibh_multivec_append_planes_device(mv, tab, types, nvar, n, nclass, stride, mask, mask0, sc, sh, C.byref(nkept), None)

    cases = [(dict(mv=None), "null VectorMultivec handle"), (dict(mask=None), "null mask"), (dict(tab=None), "null plane array"),
             (dict(tab=holed), "plane 1 is null"), (dict(nvar=3), "Inconsistant nvar: 2 vs 3"), (dict(mv=other._h), "Inconsistant nvar: 3 vs 2"),
             (dict(types=types_bad.ctypes.data_as(C.c_void_p)), "plane 1 has type 2"), (dict(n=-1), "ncell=-1"), (dict(nclass=-1), "nclass=-1"),
             (dict(n=1 << 31), "ncell=2147483648"), (dict(stride=-1), "plane_class_stride=-1"),
             # 100 kept cells x 2^25 classes of stride 0 = 100 * 2^25 > 2^31 entries: refused once the count is known
             (dict(nclass=1 << 25, stride=0), "entries \\(fewer than 2\\^31 supported\\)")]
    import re
    for kw, msg in cases:
        rc = call(**kw)
        err = L.ibh_last_error().decode()
        assert rc == _capi.IBH_EINVAL and re.search(msg, err), (kw, rc, err)
        assert vec.size() == 2 and vec.index.tolist() == [4, 9] and vec.vals.tolist() == [[1., 2.], [3., 4.]] and vec.weights.tolist() == [.5, .25]
        assert other.size() == 0
    # the host entry refuses the same way, and the two-pack form refuses a vector named twice
    hp = [np.ones(ncell), np.ones(ncell)]
    htab = (C.c_void_p * 2)(hp[0].ctypes.data, None)
    hmask = np.ones(ncell, np.int16)
    rc = L.ibh_multivec_append_planes_host(vec._h, htab, None, 2, ncell, 1, ncell, hmask.ctypes.data_as(C.c_void_p), None, 1, ncell, None)
    assert rc == _capi.IBH_EINVAL and "plane 1 is null" in L.ibh_last_error().decode()
    packs = (_capi.PlanePack * 2)()
    for s in packs:
        s.mv, s.planes, s.plane_type, s.nvar, s.nclass = vec._h.value, C.cast(table, C.c_void_p).value, None, 2, 1
        s.plane_class_stride, s.index_stride_cell, s.index_stride_class = ncell, 1, ncell
    rc = L.ibh_multivec_append_planes_many_device(C.cast(packs, C.c_void_p), 2, ncell, m, None, None, None)
    assert rc == _capi.IBH_EINVAL and "name the same VectorMultivec" in L.ibh_last_error().decode()
    assert L.ibh_multivec_affine_device(None, None, None, None) == _capi.IBH_EINVAL
    assert L.ibh_multivec_affine_device(vec._h, None, None, None) == _capi.IBH_EINVAL and "null coefficient" in L.ibh_last_error().decode()
    assert vec.size() == 2 and vec.vals.tolist() == [[1., 2.], [3., 4.]]
    # the Python surface: mixed host and device arrays, a plane too short for its classes, a type that contradicts the dtype
    with pytest.raises(ValueError, match="mixed"):
        vec.append_planes([planes[0], np.ones(ncell)], mask)
    with pytest.raises(ValueError, match="2 classes of stride 100 over 100 cells need 200"):
        vec.append_planes(planes, mask, nclass=2)
    with pytest.raises(ValueError, match="types"):
        vec.append_planes(planes, mask, types=[0, 1])
    with pytest.raises(ValueError, match="affine"):
        vec.affine([1.], [0.])
    # and the call that all of these were variations of goes through
    assert call() == 0 and nkept.value == ncell and vec.size() == 2 + ncell


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------
VARS_A = ("focean", "flake", "fgrnd", "fgice", "zatmo", "hlake")           # LISheetIceBin.F90's ATOPO contract
VARS_E = ("fhc", "elevE", "underice_d")
MM_A, BB_A = [1., 1., 1., 1., 9.80665, 1.], [0., 0., 0., 0., -3.5, 0.]       # zatmo [m] -> [m^2 s-2], and an offset to see it
BASE_KEYS = {"focean", "flake", "fgrnd", "fgice", "zatmo", "hlake", "zicetop", "zland_min", "zland_max", "mergemask", "fhc", "elevE",
             "underice", "wEAm_base", "offsetE"}


def retreated(em, I):
    """No land and no ice in the ice-grid columns >= im // 2"""
    em = np.array(em, np.float64)
    em.reshape(I.jm, I.im)[:, I.im // 2:] = np.nan
    return em


def host(x):
    return x.cpu().numpy() if hasattr(x, "is_cuda") else np.asarray(x)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("name", ["t1", "t2"])
def test_update_topo_packs_two_steps(name, device):
    """Initialisation (run_ice = False) on the fixture's masks, then a step on fresh TOPOO planes after every sheet has lost the
    eastern half of its land and ice: cells kept by the new mask, cells kept by the previous mask alone and (t2) cells that
    neither keeps.  gcm_ivalsA / gcm_ivalsE of both steps against the restatement applied to the planes update_topo returned."""
    import topo_cases as tc
    from icebin_amd import TopoPacker
    from test_gpu_topo import get_G
    g = get_G(name)
    c = g.c
    m = g.gcm.to_modele((c["planes"]["foceanOp"], c["planes"]["foceanOm"]), hspecO=g.O, eq_rad=tc.R, global_ec=g.base)
    nA, im, jm, nhc = m.hspecA.size, m.hspecA.im, m.hspecA.jm, len(m.hcdefs)
    strides_E = (nhc, 1) if device else (1, nA)              # the two orders of indexingE
    packer = TopoPacker(VARS_A, VARS_E, strides_E, mmA=MM_A, bbA=BB_A)
    ref = pr.Coupler()
    steps = [(False, c["lands"], c["ices"]),
             (True, [retreated(e, I) for e, I in zip(c["lands"], c["Is"])], [retreated(e, I) for e, I in zip(c["ices"], c["Is"])])]
    masks = []
    for run_ice, lands, ices in steps:
        if device:
            import torch
            lands, ices = [torch.from_numpy(e).cuda() for e in lands], [torch.from_numpy(e).cuda() for e in ices]
        out = m.update_topo(g.topoo(device=device), lands, ices, run_ice=run_ice, packer=packer)
        assert set(out) == BASE_KEYS | {"gcm_ivalsA", "gcm_ivalsE"}
        mask = host(out["mergemask"]).reshape(-1)
        masks.append(mask != 0)
        if run_ice:             # what the second step is for
            new, old_only, neither = masks[1], masks[0] & ~masks[1], ~masks[0] & ~masks[1]
            print("%s: step 1 keeps %d of %d cells, step 2 %d by the new mask, %d by the previous one alone, %d by neither"
                  % (name, masks[0].sum(), nA, new.sum(), old_only.sum(), neither.sum()))
            assert new.any() and old_only.any() and (name != "t2" or neither.any())
        arraysA = [host(out[k]).reshape(-1).tolist() for k in VARS_A]
        arraysE = [host(out["fhc"]).reshape(-1).tolist(), host(out["elevE"]).reshape(-1).tolist(),
                   pr.underice_d(host(out["underice"]).reshape(-1).tolist())]
        A, E = ref.pack(run_ice, mask.tolist(), arraysA, arraysE, nhc, im, jm, lambda i, j: j * im + i,
                        lambda i, j, ihc: (j * im + i) * strides_E[0] + ihc * strides_E[1], unitsA=(MM_A, BB_A))
        same(out["gcm_ivalsA"], A, (name, device, run_ice, "A"))
        same(out["gcm_ivalsE"], E, (name, device, run_ice, "E"))
        kept = masks[-1] | masks[0] if run_ice else masks[-1]
        assert out["gcm_ivalsA"].size() == kept.sum() > 0 and out["gcm_ivalsE"].size() == nhc * kept.sum()
        assert packer.mergemaskA0 is out["mergemask"]
    # without a packer: exactly the keys of before
    if not device:
        plain = m.update_topo(g.topoo(), c["lands"], c["ices"], run_ice=True)
        assert set(plain) == BASE_KEYS


def test_packer_names_and_first_step():
    from icebin_amd import TopoPacker
    with pytest.raises(KeyError, match="fland"):
        TopoPacker(("focean", "fland"), VARS_E, (1, 12))
    with pytest.raises(KeyError, match="underice"):
        TopoPacker(VARS_A, ("fhc", "underice"), (1, 12))
    with pytest.raises(ValueError, match="variables"):
        TopoPacker(VARS_A, VARS_E, (1, 12), mmA=[1., 2.])
    p = TopoPacker(VARS_A, VARS_E, (1, 12))
    with pytest.raises(RuntimeError, match="run_ice"):
        p.pack(dict(mergemask=np.zeros((3, 4), np.int16)), 2, run_ice=True)
