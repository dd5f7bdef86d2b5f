"""global_ec in chunks on the GPU (icebin_amd.global_ec: IceScan, run_chunk, combine_chunks, combine_chunk_files) against the
plain-loop restatement of modele/global_ec.cpp:752-893 and combine_global_ec.cpp:94-262 (tests/global_ec_chunks_restatement.py),
bit for bit, and against one unchunked write_matrices over the whole mask."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_ec_chunks_restatement as gr  # noqa: E402

NAMES = ("IvE", "EvI", "IvA", "AvI", "AvE", "EvA")
EC_SKIP = 500.


def specs():
    from icebin_amd import HntrSpec
    O8, O4, Ooff = HntrSpec(8, 4, 0., 2700.), HntrSpec(4, 2, 0., 5400.), HntrSpec(8, 4, .5, 2700.)
    return {"m4": (O8, HntrSpec(32, 16, 0., 675.)), "m3": (O8, HntrSpec(24, 12, 0., 900.)), "m5": (O8, HntrSpec(40, 20, 0., 540.)),
            "m30": (O4, HntrSpec(120, 60, 0., 180.)), "offi": (Ooff, HntrSpec(32, 16, 2., 675.))}


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def tile(a, O, I, jO, iO):
    mi, mj = I.im // O.im, I.jm // O.jm
    return a[jO * mj:(jO + 1) * mj, iO * mi:(iO + 1) * mi]


def make_planes(O, I, seed, binary):
    """Random int16 planes with about half the cells set, then: single ice cells at the four corners of the grid (their tiles
    otherwise empty), an all-ice tile, a run of empty tiles, a tile with ice only in its first and last row and column; the
    non-binary plane holds values other than 0 / 1 and a tile whose values cancel within one row (fgiceO == 0, nice > 0)."""
    rng = np.random.default_rng(seed)
    on = rng.random((I.jm, I.im)) < 0.5
    fg = np.where(on, 1 if binary else rng.integers(1, 4, on.shape), 0).astype(np.int16)
    el = rng.integers(-300, 3200, on.shape).astype(np.int16)
    for (jO, iO), (j, i) in (((0, 0), (0, 0)), ((0, O.im - 1), (0, -1)), ((O.jm - 1, 0), (-1, 0)), ((O.jm - 1, O.im - 1), (-1, -1))):
        t = tile(fg, O, I, jO, iO)
        t[:] = 0
        t[j, i] = 1
    tile(fg, O, I, 0, 1)[:] = 1                                 # all ice
    tile(fg, O, I, 1, 1)[:] = 0                                 # empty, two in a row
    tile(fg, O, I, 1, 2)[:] = 0
    t = tile(fg, O, I, 0, 2)                                    # the frame of a tile
    t[1:-1, 1:-1] = 0
    t[0, :] = t[-1, :] = 1
    t[:, 0] = t[:, -1] = 1
    if not binary:
        t = tile(fg, O, I, 1, O.im - 1) if O.jm > 2 else tile(fg, O, I, 1, 1)
        t[:] = 0
        t[1, 0], t[1, 1] = 7, -7                                # equal areas in one row: they cancel in fgiceO
    return fg, el


CASES = [(g, b) for g in ("m4", "m3", "m5", "m30", "offi") for b in (True, False)]
_scans = {}


def scanned(grid, binary):
    """(O, I, fg, el, fgiceO reference, scan), made once."""
    from icebin_amd import Hntr, global_ec
    key = (grid, binary)
    if key not in _scans:
        O, I = specs()[grid]
        fg, el = make_planes(O, I, 11 + CASES.index(key), binary)
        fgO = Hntr(17.17, O, I).regrid(1.0, fg)
        _scans[key] = (O, I, fg, el, fgO, global_ec.IceScan(O, I, fg, el))
    return _scans[key]


# ---- 2. the scan -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,binary", CASES)
def test_scan(grid, binary):
    import torch
    from icebin_amd import global_ec
    O, I, fg, el, fgO, scan = scanned(grid, binary)
    nice = gr.tile_counts(fg, O.im, O.jm)
    rng = gr.elev_range(fg, el)
    assert nice.max() == (I.im // O.im) * (I.jm // O.jm) and nice.min() == 0 and (nice == 1).sum() >= 4
    assert np.array_equal(scan.nice.cpu().numpy(), nice)
    assert scan.nice.dtype == torch.int32 and scan.fgiceO.dtype == torch.float64
    assert scan.elevI_range == rng
    assert scan.ec_range(EC_SKIP) == gr.ec_range(rng, EC_SKIP)
    assert np.array_equal(bits(scan.fgiceO.cpu().numpy()), bits(fgO))
    if not binary:
        cancel = (fgO == 0) & (nice > 0)
        assert cancel.sum() == 1, "the fixture's cancelling tile"
    dev = global_ec.IceScan(O, I, torch.from_numpy(fg).cuda(), torch.from_numpy(el).cuda())
    assert np.array_equal(dev.nice.cpu().numpy(), nice) and dev.elevI_range == rng
    assert np.array_equal(bits(dev.fgiceO.cpu().numpy()), bits(fgO))
    # planes whose rows start off the 16-byte pieces: a device view one cell into a longer buffer
    buf = torch.zeros(2 * I.size + 2, dtype=torch.int16, device="cuda")
    buf[1:I.size + 1] = torch.from_numpy(fg.reshape(-1)).cuda()
    buf[I.size + 2:] = torch.from_numpy(el.reshape(-1)).cuda()[:I.size]
    odd = global_ec.IceScan(O, I, buf[1:I.size + 1], buf[I.size + 2:2 * I.size + 2])
    assert np.array_equal(odd.nice.cpu().numpy(), nice) and odd.elevI_range == rng
    ch = odd.chunks(10 ** 6)[0][0]
    assert np.array_equal(odd.chunk_mask(ch).cpu().numpy().reshape(fg.shape), gr.chunk_mask(fg, el, fgO, ch), equal_nan=True)


@pytest.mark.parametrize("mult", [3, 5, 30])
def test_scan_with_several_ocean_cells_per_workgroup(mult):
    # the scan gives a workgroup one ocean row's slice of ceil(imO / min(imO, max(ceil(imO / 2048), ceil(1024 / jmO)))) cells:
    # one cell on the small grids above, here 2 with a last slice of 1 (imO = 67 is odd, jmO = 16), so that tile indices above 0,
    # 16-byte pieces that straddle two ocean cells (mult 3, 5 and 30 against pieces of 8), rows that start off a piece (imI odd
    # for mult 3 and 5) and the short last slice all run.  Random planes, half the cells set, values other than 0 / 1.
    import torch
    from icebin_amd import Hntr, HntrSpec, global_ec
    O = HntrSpec(67, 16, 0., 675.)
    I = HntrSpec(67 * mult, 16 * mult, 0., 675. / mult)
    assert -(-1024 // O.jm) < O.im and O.im % 2 == 1
    rng = np.random.default_rng(100 + mult)
    fg = (rng.choice([-2, -1, 1, 2, 3], (I.jm, I.im)) * (rng.random((I.jm, I.im)) < 0.5)).astype(np.int16)
    el = rng.integers(-300, 3200, fg.shape).astype(np.int16)
    nice, erange = gr.tile_counts(fg, O.im, O.jm), gr.elev_range(fg, el)
    assert len(np.unique(nice)) > 3
    fgO = Hntr(17.17, O, I).regrid(1.0, fg)
    buf = torch.zeros(2 * I.size + 4, dtype=torch.int16, device="cuda")
    buf[1:I.size + 1] = torch.from_numpy(fg.reshape(-1)).cuda()
    buf[I.size + 4:] = torch.from_numpy(el.reshape(-1)).cuda()
    scans = {"host": global_ec.IceScan(O, I, fg, el),
             "device": global_ec.IceScan(O, I, torch.from_numpy(fg).cuda(), torch.from_numpy(el).cuda()),
             "device, off the pieces": global_ec.IceScan(O, I, buf[1:I.size + 1], buf[I.size + 4:])}
    for what, scan in scans.items():
        assert np.array_equal(scan.nice.cpu().numpy(), nice), what
        assert scan.elevI_range == erange, what
        assert np.array_equal(bits(scan.fgiceO.cpu().numpy()), bits(fgO)), what
    if mult != 30:          # (the restatement's mask loop over the 30-fold grid takes seconds; the masks at 30: test_plan_and_masks)
        for what, scan in scans.items():
            plan = scan.chunks(40 * mult * mult)
            assert plan == gr.chunk_plan(fg, fgO, 40 * mult * mult) and len(plan) >= 3
            for ch in plan[:2] + plan[-1:]:
                em = scan.chunk_mask(ch).cpu().numpy().reshape(fg.shape)
                assert np.array_equal(bits(em), bits(gr.chunk_mask(fg, el, fgO, ch[0]))), (what, ch)


def test_scan_without_ice():
    from icebin_amd import global_ec
    O, I = specs()["m3"]
    z = np.zeros((I.jm, I.im), np.int16)
    scan = global_ec.IceScan(O, I, z, z + 5)
    assert scan.elevI_range == (10000, -10000) and int(scan.nice.sum()) == 0
    assert scan.chunks(100) == [((0, 0, 0, O.jm, 0), 0)]
    assert bool(scan.chunk_mask(scan.chunks(100)[0]).isnan().all())


# ---- 3. the plan and the masks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,binary", [("m4", False), ("m30", True), ("offi", True), ("m3", False), ("m5", True)])
def test_plan_and_masks(grid, binary):
    O, I, fg, el, fgO, scan = scanned(grid, binary)
    mult2 = (I.im // O.im) * (I.jm // O.jm)
    c = np.where(fgO != 0, gr.tile_counts(fg, O.im, O.jm), 0).reshape(-1)
    total = int(c.sum())
    incl = np.cumsum(c)
    # the chunk sizes at which the first chunk ends at cell k, for every k that can end one, and the two extremes
    sizes = sorted({int(incl[k]) for k in range(O.size) if c[k] > 0 and incl[k] > mult2} | {mult2 + 1, total + 1})
    assert scan.chunks(sizes[1]) == gr.chunk_plan(fg, fgO, sizes[1])
    seen = set()
    for size in sizes:
        plan = scan.chunks(size)
        assert plan == gr.chunk_plan_counts(c, O.im, O.jm, size), size
        ks = [(ch[1] * O.im + ch[2], ch[3] * O.im + ch[4]) for ch, _ in plan]
        assert ks[0][0] == 0 and ks[-1][1] == O.size and all(a[1] == b[0] and a[0] < a[1] for a, b in zip(ks, ks[1:] + [(O.size, 0)]))
        assert all(c[k0:k1].sum() < size for k0, k1 in ks)
        for (ch, _), (k0, k1) in zip(plan[:-1], ks[:-1]):
            seen.add("mid-row" if ch[4] else "row end")
            if c[k1 - 1] == 0:
                seen.add("after empty cells")
        if any(ch[3] - ch[1] >= 2 for ch, _ in plan):
            seen.add("several rows")
    assert seen == {"mid-row", "row end", "after empty cells", "several rows"}, seen
    whole = gr.chunk_mask(fg, el, fgO, (0, 0, 0, O.jm, 0))
    assert np.array_equal(np.isnan(whole), ~((fg != 0) & (np.kron(fgO != 0, np.ones((I.jm // O.jm, I.im // O.im))) != 0)))
    for size in (mult2 + 1, sizes[len(sizes) // 2], int(incl[(O.jm - 1) * O.im]), total + 1):
        plan = scan.chunks(size)
        union = np.full(fg.shape, np.nan)
        for ch in plan:
            em = scan.chunk_mask(ch).cpu().numpy().reshape(fg.shape)
            assert np.array_equal(bits(em), bits(gr.chunk_mask(fg, el, fgO, ch[0]))), (size, ch)
            on = ~np.isnan(em)
            assert np.isnan(union[on]).all(), "masks overlap"
            union[on] = em[on]
        assert np.array_equal(bits(union), bits(whole)), size


# ---- 4. - 7. the chunks' matrices, combined ------------------------------------------------------------------------------------------
_runs = {}


def hspecI2():
    from icebin_amd import HntrSpec
    return HntrSpec(16, 8, 0., 1350.)


def chunk_runs(option, which, tmp=None):
    """The results of run_chunk over the m4 grid, made once per (option, which): `ocean` or `atmosphere`; which = "many" (the
    plan's chunks for a chunk size that gives at least three, the one that holds the run of empty cells split in three so
    that its middle has no ice) or "one" (a single chunk: one unchunked write_matrices over the whole mask)."""
    from icebin_amd import global_ec
    from icebin_amd.modele import make_hntrA
    key = (option, which)
    if key in _runs and tmp is None:
        return _runs[key]
    O, I, fg, el, fgO, scan = scanned("m4", False)
    A = O if option == "ocean" else make_hntrA(O)
    if which == "many":
        plan = [ch for ch, _ in scan.chunks(70)]
        assert len(plan) >= 3
        e0, e1 = 1 * O.im + 1, 1 * O.im + 3                     # make_planes' two empty tiles
        chunks = []
        for ch in plan:
            k0, k1 = ch[1] * O.im + ch[2], ch[3] * O.im + ch[4]
            cuts = [k0] + [k for k in (e0, e1) if k0 < k < k1] + [k1]
            chunks += [(a // O.im, a % O.im, b // O.im, b % O.im) for a, b in zip(cuts, cuts[1:])]
        chunks = [(n,) + ch for n, ch in enumerate(chunks)]
        assert any(ch[1] * O.im + ch[2] == e0 and ch[3] * O.im + ch[4] == e1 for ch in chunks), "the chunk with no ice"
    else:
        chunks = [(0, 0, 0, O.jm, 0)]
    res = [global_ec.run_chunk(scan, ch, A, hspecI2(), EC_SKIP, ofname=None if tmp is None else str(tmp), names=NAMES) for ch in chunks]
    if tmp is None:
        _runs[key] = (chunks, res)
    return chunks, res


def vname(name, option):
    return name.replace("A", "O") if option == "ocean" else name


def restate_input(mat):
    row, col, val = mat.coo_dense()
    return dict(dimB=mat.dim(0), dimA=mat.dim(1), wM=mat.wM, Mw=mat.Mw, row=row, col=col, val=val,
                extents=(mat.sparse_extent(0), mat.sparse_extent(1)))


def assert_is_restatement(comb, r, scale, what):
    iB, iA, val = comb.coo_sparse()
    assert np.array_equal(iB, r["iB"]) and np.array_equal(iA, r["iA"]), what
    assert np.array_equal(bits(val), bits(r["val"])), what
    assert np.array_equal(comb.dim(0), r["dimB"]) and np.array_equal(comb.dim(1), r["dimA"]), what
    assert np.array_equal(bits(comb.wM), bits(r["wM"])) and np.array_equal(bits(comb.Mw), bits(r["Mw"])), what
    row, col, v = gr.set_from_triplets(r["dimB"], r["dimA"], r["iB"], r["iA"], r["val"])
    crow, ccol, cv = comb.coo_dense()
    assert np.array_equal(crow, row) and np.array_equal(ccol, col) and np.array_equal(bits(cv), bits(v)), what
    assert comb.scaled == scale and comb.nnz == len(v), what


@pytest.mark.parametrize("option", ["ocean", "atmosphere"])
@pytest.mark.parametrize("which", ["many", "one"])
def test_combine_is_the_restatement(option, which):
    from icebin_amd import global_ec
    chunks, res = chunk_runs(option, which)
    if which == "many":
        assert len(chunks) >= 3 and any(r[vname("AvI", option)].nnz == 0 for r in res)
    for name in NAMES:
        ins = [restate_input(r[vname(name, option)]) for r in res]
        for scale in (False, True):
            comb = global_ec.combine_chunks(res, name, scale=scale)
            assert_is_restatement(comb, gr.combine(ins, scale), scale, (option, which, name, scale))
            if which == "one" and not scale:                   # a single chunk: the identity
                m = res[0][vname(name, option)]
                assert all(np.array_equal(a, b) for a, b in zip(comb.coo_dense(), m.coo_dense()))
                assert np.array_equal(bits(comb.wM), bits(m.wM)) and np.array_equal(comb.dim(0), m.dim(0))


def keyed(mat):
    """(entries sorted by (row key, col key) as [n, 2] keys and values; {0: (keys, wM), 1: (keys, Mw)} sorted by key)."""
    row, col, val = mat.coo_dense()
    kB, kA = mat.dim(0)[row], mat.dim(1)[col]
    o = np.lexsort((kA, kB))
    w = {}
    for d, wt in ((0, mat.wM), (1, mat.Mw)):
        p = np.argsort(mat.dim(d))
        w[d] = (mat.dim(d)[p], wt[p])
    return np.stack([kB[o], kA[o]], 1), val[o], w


@pytest.mark.parametrize("option", ["ocean", "atmosphere"])
def test_combined_equals_the_unchunked_build(option):
    # independent of the restatement: one write_matrices over the whole mask
    from icebin_amd import global_ec
    chunks, res = chunk_runs(option, "many")
    _, whole = chunk_runs(option, "one")
    # the terms behind a weight or an AvE / EvA entry: the ice cells of the GCM cell (AvI's row) or of the class (EvI's row)
    nterms = {}
    for side, name in (("A", "AvI"), ("E", "EvI")):
        m = whole[0][vname(name, option)]
        rp = m.csr_dense()[0]
        nterms[side] = dict(zip(m.dim(0).tolist(), np.diff(rp).tolist()))
    named = {}
    for r in res:
        for a in r[vname("AvI", option)].dim(0).tolist():
            named[a] = named.get(a, 0) + 1
    straddlers = sum(1 for n in named.values() if n > 1)
    assert (straddlers == 0) if option == "ocean" else (straddlers >= 1)
    for name in NAMES:
        comb = global_ec.combine_chunks(res, name, scale=False)
        iB, iA, _ = comb.coo_sparse()
        dups = len(iB) - len(set(zip(iB.tolist(), iA.tolist())))           # entries of the stream that name a pair already named
        assert dups == len(iB) - comb.nnz
        assert (dups >= 1) if (option == "atmosphere" and name in ("AvE", "EvA")) else (dups == 0), (name, dups)
        k1, v1, w1 = keyed(comb)
        k0, v0, w0 = keyed(whole[0][vname(name, option)])
        assert np.array_equal(k1, k0), name
        exact = option == "ocean" or name not in ("AvE", "EvA")
        if exact:
            assert np.array_equal(bits(v1), bits(v0)), name
        else:
            kE = [nterms["E"][int(k[0 if name[0] == "E" else 1])] for k in k0]
            bound = np.asarray([2 * (k - 1) * 2. ** -53 for k in kE])
            print(name, "entries: largest relative difference", np.max(np.abs(v1 - v0) / np.abs(v0)), "bound", bound.max())
            assert np.all(np.abs(v1 - v0) <= bound * np.abs(v0)), name
        for d in (0, 1):
            side = name[2 * d]
            assert np.array_equal(w1[d][0], w0[d][0]), (name, d)
            if option == "ocean" or side == "I":
                assert np.array_equal(bits(w1[d][1]), bits(w0[d][1])), (name, d)
            else:
                bound = np.asarray([2 * (nterms[side][int(k)] - 1) * 2. ** -53 for k in w0[d][0]])
                print(name, d, "weights: largest relative difference", np.max(np.abs(w1[d][1] - w0[d][1]) / np.abs(w0[d][1])), "bound", bound.max())
                assert np.all(np.abs(w1[d][1] - w0[d][1]) <= bound * np.abs(w0[d][1])), (name, d)


def test_end_to_end_base_of_EOpvAOp():
    from icebin_amd import global_ec
    from icebin_amd.modele import compute_EOpvAOp_merged
    O, I, fg, el, fgO, scan = scanned("m4", False)
    chunks, res = chunk_runs("ocean", "many")
    comb = global_ec.combine_chunks(res, "EvA")
    iE, iO, val = comb.coo_sparse()
    hc = global_ec.hcdefs(*scan.ec_range(EC_SKIP), EC_SKIP)
    r = compute_EOpvAOp_merged([], base=(hc, (iE, iO, val), comb.shape))
    assert r.offsetE == 0 and np.array_equal(r.hcdefs, hc)
    row, col, v = r.EOpvAOp.coo_dense()
    got = sorted(zip(r.EOpvAOp.dim(0)[row].tolist(), r.EOpvAOp.dim(1)[col].tolist(), bits(v).tolist()))
    crow, ccol, cv = comb.coo_dense()
    want = sorted(zip(comb.dim(0)[crow].tolist(), comb.dim(1)[ccol].tolist(), bits(cv).tolist()))
    assert got == want and len(got) == len(val) > 0


def test_chunk_files_round_trip(tmp_path):
    from icebin_amd import global_ec
    from icebin_amd.linear import nc_read_weighted
    chunks, res = chunk_runs("ocean", "many", tmp_path / "global_ecO")
    names = [str(tmp_path / ("global_ecO-%02d" % ch[0])) for ch in chunks]
    assert all(os.path.exists(n) for n in names)
    for scale in (False, True):
        out = str(tmp_path / ("combined%d" % scale))
        combined = global_ec.combine_chunk_files(names, out, NAMES, scale)
        assert sorted(combined) == sorted(vname(n, "ocean") for n in NAMES)
        for name in NAMES:
            direct = global_ec.combine_chunks(res, name, scale=scale)
            back = nc_read_weighted(out, vname(name, "ocean"))
            for m in (combined[vname(name, "ocean")], back):
                assert all(np.array_equal(a, b) for a, b in zip(m.coo_dense()[:2], direct.coo_dense()[:2])), name
                assert np.array_equal(bits(m.coo_dense()[2]), bits(direct.coo_dense()[2])), name
                assert np.array_equal(bits(m.wM), bits(direct.wM)) and np.array_equal(bits(m.Mw), bits(direct.Mw)), name
                assert np.array_equal(m.dim(0), direct.dim(0)) and np.array_equal(m.dim(1), direct.dim(1)), name
                assert m.scaled == scale and m.shape == direct.shape, name
            assert all(np.array_equal(a, b) for a, b in zip(combined[vname(name, "ocean")].coo_sparse()[:2], direct.coo_sparse()[:2]))


# ---- 8. the errors that need matrices -------------------------------------------------------------------------------------------------
def test_combine_rejects_scaled_and_mismatched_chunks():
    from icebin_amd import _capi, global_ec
    from icebin_amd.modele import make_hntrA
    O, I, fg, el, fgO, scan = scanned("m4", False)
    chunks, res = chunk_runs("ocean", "many")
    gcm = global_ec.gcm_from_hntr(O, I, scan.chunk_mask(chunks[0]), global_ec.hcdefs(*scan.ec_range(EC_SKIP), EC_SKIP))
    scaled = gcm.regrid_matrices("globalI", scan.chunk_mask(chunks[0]), scale=True).matrix_d("AvI", scale=True)
    with pytest.raises(_capi.IcebinHipError, match="mats: chunk 1's matrix is scaled") as ei:
        global_ec.combine_chunks([res[0], {"AvI": scaled}], "AvI")
    assert ei.value.code == _capi.IBH_EINVAL
    _, other = chunk_runs("atmosphere", "one")
    with pytest.raises(_capi.IcebinHipError, match=r"mats: chunk 1 has sparse extents \(\d+, \d+\), chunk 0 \(\d+, \d+\)") as ei:
        global_ec.combine_chunks([res[0], other[0]], "AvI")
    assert ei.value.code == _capi.IBH_EINVAL
    with pytest.raises(_capi.IcebinHipError, match="name: chunk 0 holds no matrix 'XvY'"):
        global_ec.combine_chunks(res, "XvY")
    with pytest.raises(_capi.IcebinHipError, match="chunk: "):
        scan.chunk_mask((0, 0, 0, O.jm + 1, 0))
    import torch
    for bad in (torch.empty(I.size, dtype=torch.float32, device="cuda"), torch.empty(I.size, dtype=torch.float64),
                torch.empty(2 * I.size, dtype=torch.float64, device="cuda")[::2], np.empty(I.size)):
        with pytest.raises(_capi.IcebinHipError, match="out: ") as ei:
            scan.chunk_mask(chunks[0], out=bad)
        assert ei.value.code == _capi.IBH_EINVAL
    with pytest.raises(_capi.IcebinHipError, match="d_elevmaskI: 511 cells") as ei:
        scan.chunk_mask(chunks[0], out=torch.empty(I.size - 1, dtype=torch.float64, device="cuda"))
    # a table read from a file that names a sparse index twice (a set cannot)
    m = res[0]["OvI"]
    host = [(m.dim(0), m.dim(1), m.sparse_extent(0), m.sparse_extent(1))]
    assert global_ec._combine([m], False, host).nnz == m.nnz
    twice = m.dim(1).copy()
    twice[-1] = twice[0]
    with pytest.raises(_capi.IcebinHipError, match="dims_host: chunk 0, dimension 1 names the sparse index %d twice" % twice[0]) as ei:
        global_ec._combine([m], False, [(m.dim(0), twice, m.sparse_extent(0), m.sparse_extent(1))])
    assert ei.value.code == _capi.IBH_EINVAL
    assert make_hntrA(O).size * 4 == O.size
