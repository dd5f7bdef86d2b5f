"""The apply's side paths (spmm.hip below the conservation banner) at their table, wave and chunk edges, each against the plain
long-double references of tests/apply_sidepath_cases.py (pinned against the CPU oracle by tests/test_apply_sidepath_cases.py):

  A  transform_kernel<INLINE>, rowsum_kernel, spmm_transformed_launch: M (V T + b) on both sides of M, of the 256-thread block and of
     the inline table (384 coefficients), two tables in a row on one handle, padded planes, a captured apply;
  B  matvec_legacy_kernel<WAVE>: the thread and the wave form of the same rows, nvar 1 and 3, leading dimensions, both NaN modes;
  C  weight_dot_kernel / weight_dot_final_kernel through apply_weight: 1 .. 256 chunks, the cap, both weight vectors;
  D  the conservation correction: the row side chunked, batches across the 32-batch split, padded planes, the exact variant, a
     conservative matrix, the host entry, a captured apply;
  E  rowperm_kernel: 8192 rows (built), 8193 and 1 (declined), ties by index;
  F  the leading dimension of a field batch: a broadcast batch is refused before any launch, a slice of a wider buffer is taken.

Every gated case prints its largest err / bound (pytest -s); the bounds are derived in apply_sidepath_cases' docstring.  No row or
element is left out of a comparison: dead rows hold fill exactly, NaN sits exactly where the reference has it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import icebin_amd
from icebin_amd._capi import check, lib, ptr
from icebin_amd.linear import linear_Weighted

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import apply_kernel_recipes as akr  # noqa: E402
import apply_sidepath_cases as asc  # noqa: E402
from test_gpu_apply_kernels import CANARY, PaddedOutput, padded_input, setup_recipe  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = asc.FILL


def handle(m, conservative=True):
    """the case's matrix on the device; the references are computed from what the handle says it holds"""
    w = linear_Weighted.from_csr((m.nrow, m.ncol), m.rowptr, m.colind, m.val, m.wM, m.Mw, conservative=conservative)
    row, col, val = w.coo_dense()
    assert np.array_equal(row, m.row) and np.array_equal(col, m.colind) and asc.same_bits(val, m.val)
    assert asc.same_bits(w.wM, m.wM) and asc.same_bits(w.Mw, m.Mw) and w.conservative == conservative
    return w


def own_csr(w):
    row, col, val = w.coo_dense()
    return asc.csr_from_coo(w.nrow_d, w.ncol_d, row, col, val, w.wM, w.Mw)


def stream_of(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def report(what, ratio):
    print("err/bound %-60s %.2e" % (what, ratio))
    return ratio


# ---- A: transformed product -------------------------------------------------------------------------------------------------------
def run_transformed(torch, w, m, V, T, b, fill, what):
    x = padded_input(torch, V)                                           # row stride ncol + 3, NaN in the padding
    out = PaddedOutput(torch, T.shape[1], m.nrow)                        # canaries before, between and after the planes
    w.apply_transformed_device(x, T, b, out=out.view, fill=fill)
    torch.cuda.synchronize()
    y = out.result(what)                                                 # every element written, no canary touched
    return asc.check_transformed(m, y, V, T, b, fill, what)


@pytest.mark.parametrize("size", asc.SIZES_A, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("shape", asc.SHAPES_A, ids=lambda s: "%dx%d" % s)
def test_transformed_product(shape, size):
    """M (V T + b) at 255 / 256 / 257 on the transformed side (one block of the transform, exactly one, two), inputs side for
    ncol <= nrow (the tie included) and outputs side otherwise; (23, 16) and (31, 12) fill the inline table, (24, 16) goes through the
    device copy.  NaN of variable 0 at one column reaches the rows that store it; the all-NaN variable behind the zero row of the
    (5, 3) transform reaches nothing."""
    import torch
    m = asc.side_matrix(*shape, seed=sum(shape))
    w = handle(m)
    T, b = asc.transform(*size, 0)
    V = asc.transform_inputs(m, size[0], seed=11, T=T)
    worst = 0.0
    for fill in (FILL, float("nan")):
        what = "transformed %dx%d T %dx%d fill %s" % (shape + size + (fill,))
        worst = max(worst, run_transformed(torch, w, m, V, T, b, fill, what))
    report("transformed %dx%d T %dx%d" % (shape + size), worst)


@pytest.mark.parametrize("shape", [(400, 256), (256, 400)], ids=lambda s: "%dx%d" % s)
def test_transformed_tables_in_a_row_on_one_handle(shape):
    """(24, 16), another (24, 16), then (5, 3) on one handle, each against its own reference: the device copy of the coefficients is
    reused and then left for the inline table."""
    import torch
    m = asc.side_matrix(*shape, seed=sum(shape))
    w = handle(m)
    for step, (size, seed) in enumerate((((24, 16), 0), ((24, 16), 1), ((5, 3), 1))):
        T, b = asc.transform(*size, seed)
        V = asc.transform_inputs(m, size[0], seed=20 + step, T=T)
        what = "transformed %dx%d step %d T %dx%d" % (shape + (step,) + size)
        report(what, run_transformed(torch, w, m, V, T, b, FILL, what))


@pytest.mark.parametrize("shape", [(400, 256), (256, 400)], ids=lambda s: "%dx%d" % s)
def test_transformed_product_in_a_graph_keeps_the_coefficients_of_the_capture(shape):
    """The inline table travels with the launch: a captured apply replays the T and b it was given, whatever the host arrays hold by
    then."""
    import torch
    m = asc.side_matrix(*shape, seed=sum(shape))
    w = handle(m)
    nin, nout = 23, 16
    T0, b0 = asc.transform(nin, nout, 0)
    T, b = T0.copy(), b0.copy()
    V = asc.transform_inputs(m, nin, seed=31, T=T)
    w.reserve(max(nin, nout))
    x = torch.from_numpy(V).cuda()
    out = torch.full((nout, m.nrow), CANARY, dtype=torch.float64, device="cuda")
    w.apply_transformed_device(x, T, b, out=out, fill=FILL)              # warm-up
    torch.cuda.synchronize()
    asc.check_transformed(m, out.cpu().numpy(), V, T0, b0, FILL, "warm-up")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        w.apply_transformed_device(x, T, b, out=out, fill=FILL)
    T[:], b[:] = asc.transform(nin, nout, 1)                             # the host arrays move on
    assert not np.array_equal(T, T0) and not np.array_equal(b, b0)
    V2 = asc.transform_inputs(m, nin, seed=32, T=T0)
    x.copy_(torch.from_numpy(V2).cuda())
    out.fill_(CANARY)
    graph.replay()
    torch.cuda.synchronize()
    y = out.cpu().numpy()
    assert not np.any(y == CANARY)
    report("transformed %dx%d replayed" % shape, asc.check_transformed(m, y, V2, T0, b0, FILL, "replay"))


# ---- B: legacy matvec -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ignore_nan", [0, 1])
@pytest.mark.parametrize("nvar", [1, 3])
@pytest.mark.parametrize("form", [0, 1], ids=["thread", "wave"])
def test_legacy_matvec_device(form, nvar, ignore_nan):
    """ibh_weighted_matvec_device on the two matrices of asc.matvec_matrices(): the same rows but for one entry of one short row, so
    that nnz == 8 nrow - 1 takes one thread a row and nnz == 8 nrow one wave a row.  yy is preset to a value of its own in every
    element: rows without a surviving term and the padding keep theirs."""
    import torch
    m = asc.matvec_matrices()[form]
    assert m.nnz == 8 * m.nrow - 1 + form
    w = handle(m)
    X = asc.matvec_inputs(m, nvar, seed=5)
    ldx, ldy = m.ncol + 3, m.nrow + 5
    Y0 = asc.matvec_canaries(nvar, ldy)
    xb = torch.full((nvar, ldx), float("nan"), dtype=torch.float64, device="cuda")
    xb[:, :m.ncol] = torch.from_numpy(X).cuda()
    yb = torch.from_numpy(Y0).cuda()
    check(lib().ibh_weighted_matvec_device(w._h, C.c_void_p(xb.data_ptr()), nvar, ldx, C.c_void_p(yb.data_ptr()), ldy, ignore_nan,
                                           stream_of(torch)))
    torch.cuda.synchronize()
    y = yb.cpu().numpy()
    assert np.array_equal(y[:, m.nrow:], Y0[:, m.nrow:]), "wrote beyond nrow"
    ref, tol, written = asc.matvec_ref(m, X, Y0[:, :m.nrow], ignore_nan)
    what = "matvec %s nvar %d ignore_nan %d" % (("thread", "wave")[form], nvar, ignore_nan)
    report(what, asc.gate(y[:, :m.nrow], ref, tol, what))               # tol is 0 where nothing is written: the canary, exactly
    r0, r65, r130 = (m.where[k] for k in ("len0", "len65", "len130"))
    gone = asc.matvec_all_nan_rows(m)
    assert np.all(y[:, r0] == Y0[:, r0])
    if ignore_nan:
        assert np.all(y[0, gone] == Y0[0, gone]) and not np.isnan(y[:, :m.nrow]).any()
        assert y[0, r130] != Y0[0, r130]
    else:
        assert np.isnan(y[0, gone + [r130]]).all() and not np.isnan(y[0, r65])


@pytest.mark.parametrize("ignore_nan", [False, True])
@pytest.mark.parametrize("form", [0, 1], ids=["thread", "wave"])
def test_coo_multiply_shuffled_duplicates(form, ignore_nan):
    """the same matrices as shuffled triplets with duplicates (halves that add up exactly) through icebin_amd.coo_multiply"""
    import scipy.sparse
    m = asc.matvec_matrices()[form]
    row, col, val = asc.shuffled_duplicate_triplets(m, seed=9)
    M = scipy.sparse.coo_matrix((val, (row, col)), shape=(m.nrow, m.ncol))
    X = asc.matvec_inputs(m, 1, seed=5)
    y = icebin_amd.coo_multiply(M, X[0], fill=FILL, ignore_nan=ignore_nan)
    ref, tol, _ = asc.matvec_ref(m, X, np.full((1, m.nrow), FILL), int(ignore_nan))
    what = "coo_multiply %s ignore_nan %d" % (("thread", "wave")[form], ignore_nan)
    report(what, asc.gate(y[None, :], ref, tol, what))


# ---- C: weight dots ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", asc.SIZES_C)
def test_weight_dots(n):
    """apply_weight on a matrix without entries: one chunk up to 4096 elements, two of 2049 at 4097, three at 8193, 256 of 4096 at
    2^20 and the cap (256 of 4097) one beyond.  A tenth of the weights are 0 with NaN in the field there.  Exact variant (powers of
    two times small integers): the sum, bitwise; random variant: the dot bound against math.fsum.  Then the C entry with lda > n and
    NaN in the padding."""
    worst = 0.0
    for exact in (True, False):
        m = asc.empty_matrix(n, seed=n, exact=exact)
        w = handle(m)
        for dim, wt in ((0, m.wM), (1, m.Mw)):
            A = asc.weight_fields(wt, 3, seed=n + dim, exact=exact)
            ref, tol = asc.weight_dot_ref(wt, A)
            pad = np.full((3, n + 7), np.nan)
            pad[:, :n] = A
            for nvar in (1, 3):
                got = np.atleast_1d(w.apply_weight(dim, A[0] if nvar == 1 else A))
                via_c = np.full(nvar + 1, CANARY)
                check(lib().ibh_weighted_apply_weight_host(w._h, dim, ptr(pad), nvar, n + 7, ptr(via_c)))
                assert via_c[nvar] == CANARY
                for y, how in ((got, "apply_weight"), (via_c[:nvar], "lda > n")):
                    what = "weight dot n=%d dim=%d nvar=%d %s %s" % (n, dim, nvar, "exact" if exact else "random", how)
                    assert y.shape == (nvar,) and np.all(np.isfinite(y)), what
                    if exact:
                        assert asc.same_bits(y, ref[:nvar].astype(np.float64)), what
                    else:
                        worst = max(worst, asc.gate(y, ref[:nvar], tol[:nvar], what))
    report("weight dot n=%d" % n, worst)


# ---- D: conservation correction ---------------------------------------------------------------------------------------------------
def corrected_gate(y1, y0, X, wM, Mw, fill, what):
    exact, tol, _ = asc.correction_ref(y0, X, wM, Mw)
    dead = wM == 0.0
    assert asc.holds(y1[:, dead], fill) and asc.holds(y0[:, dead], fill), "%s: dead rows do not hold fill" % what
    return asc.gate(y1[:, ~dead], exact[:, ~dead], tol[:, ~dead], what)


def noncons(nrow, ncol=900, nvar=3):
    row, col, val, wM, Mw, nan_cols = asc.random_coo(nrow, ncol, 8, seed=nrow)
    w = linear_Weighted.from_coo((nrow, ncol), row, col, val, wM, Mw, conservative=False)
    return w, wM, Mw, asc.correction_fields(nvar, ncol, nan_cols)


@pytest.mark.parametrize("nrow", [4096, 4097])
def test_correction_with_the_row_side_chunked(nrow):
    """nrow x 900: wM . B runs in one chunk at 4096 rows and in two at 4097, Mw . A in one; the scratch is sized by the larger side.
    Then the same apply with padded planes (same bits where the same kernel ran), and the host entry with lda > ncol, ldb > nrow."""
    import torch
    w, wM, Mw, X = noncons(nrow)
    nvar, ncol = X.shape
    m = own_csr(w)
    x = torch.from_numpy(X).cuda()
    y0 = w.apply_device(x, fill=FILL, force_conservation=False).cpu().numpy()
    report("uncorrected %d x %d" % (nrow, ncol), asc.check_product(m, y0, X, FILL, "uncorrected"))
    y1 = w.apply_device(x, fill=FILL, force_conservation=True).cpu().numpy()
    plain = w.last_launch()
    report("corrected %d x %d" % (nrow, ncol), corrected_gate(y1, y0, X, wM, Mw, FILL, "corrected"))
    assert np.max(np.abs(y1[:, wM != 0.0] / y0[:, wM != 0.0] - 1.0)) > 1e-3           # a factor that a missing correction would miss

    out = PaddedOutput(torch, nvar, nrow)
    w.apply_device(padded_input(torch, X), out=out.view, fill=FILL, force_conservation=True)
    torch.cuda.synchronize()
    yp = out.result("padded corrected")
    if w.last_launch() == plain:
        assert asc.same_bits(yp, y1), "padded planes, the same kernel, other bits"
    report("corrected %d x %d padded" % (nrow, ncol), corrected_gate(yp, y0, X, wM, Mw, FILL, "padded corrected"))

    lda, ldb = ncol + 3, nrow + 5
    A = np.full((nvar, lda), np.nan)
    A[:, :ncol] = X
    B = asc.matvec_canaries(nvar, ldb)
    B0 = B.copy()
    check(lib().ibh_weighted_apply_host(w._h, ptr(A), nvar, lda, ptr(B), ldb, FILL, 1))
    assert np.array_equal(B[:, nrow:], B0[:, nrow:]), "the host apply wrote into the padding"
    h0 = w.apply(X, fill=FILL, force_conservation=False)
    asc.check_product(m, h0, X, FILL, "host uncorrected")
    report("corrected %d x %d host, padded" % (nrow, ncol), corrected_gate(B[:, :nrow], h0, X, wM, Mw, FILL, "host corrected"))


@pytest.mark.parametrize("nbatch", [2, 33])
def test_correction_in_batches(nbatch):
    """apply_many_device with the correction: one scratch of dot products serves every batch of a launch in turn (33 batches: two
    launches).  A different field per batch and variable; every batch bitwise its own corrected apply_device, batch 0 within the
    bound."""
    import torch
    w, wM, Mw, X = noncons(4097)
    nvar, ncol = X.shape
    Xs = asc.batch_fields(X, nbatch)
    xs = [torch.from_numpy(a).cuda() for a in Xs]
    sep = [w.apply_device(x, fill=FILL, force_conservation=True).cpu().numpy() for x in xs]
    y0 = w.apply_device(xs[0], fill=FILL, force_conservation=False).cpu().numpy()
    outs = [torch.full((nvar, w.nrow_d), CANARY, dtype=torch.float64, device="cuda") for _ in xs]
    w.apply_many_device(xs, outs, fill=FILL, force_conservation=True)
    torch.cuda.synchronize()
    for q in range(nbatch):
        assert asc.same_bits(outs[q].cpu().numpy(), sep[q]), "batch %d of %d differs from its own corrected apply" % (q, nbatch)
    asc.check_product(own_csr(w), y0, X, FILL, "uncorrected")
    report("corrected batch 0 of %d" % nbatch, corrected_gate(outs[0].cpu().numpy(), y0, X, wM, Mw, FILL, "batch 0"))


@pytest.mark.parametrize("fill", [FILL, float("nan")])
def test_correction_exact_variant(fill):
    """Powers of two and small integers: every sum is exact in any order, so the corrected apply is bitwise y0 * (TA / TB) in float64
    -- one division, one multiplication.  Dead rows hold fill and are not scaled."""
    import torch
    m = asc.side_matrix(400, 1100, seed=77, exact=True)
    w = handle(m, conservative=False)
    X = asc.exact_fields(3, m.ncol, seed=8)
    x = padded_input(torch, X)
    y0 = w.apply_device(x, fill=fill, force_conservation=False).cpu().numpy()
    y1 = w.apply_device(x, fill=fill, force_conservation=True).cpu().numpy()
    live = m.wM != 0.0
    ref, _ = asc.product_ref(m, X)
    assert asc.same_bits(y0[:, live], ref[:, live].astype(np.float64))
    _, _, factor = asc.correction_ref(y0, X, m.wM, m.Mw)
    assert np.all(factor != 1.0) and len(set(factor.tolist())) == 3                     # a factor of its own per variable
    assert asc.same_bits(y1[:, live], y0[:, live] * factor[:, None])
    assert asc.holds(y0[:, ~live], fill) and asc.holds(y1[:, ~live], fill)


def test_conservative_matrix_is_not_corrected():
    import torch
    m = asc.side_matrix(400, 1100, seed=78)
    w = handle(m, conservative=True)
    X = asc.transform_inputs(m, 3, seed=4)
    x = torch.from_numpy(X).cuda()
    y0 = w.apply_device(x, fill=FILL, force_conservation=False).cpu().numpy()
    y1 = w.apply_device(x, fill=FILL, force_conservation=True).cpu().numpy()
    assert asc.same_bits(y0, y1)
    report("conservative 400 x 1100", asc.check_product(m, y0, X, FILL, "conservative"))


def test_correction_in_a_graph():
    """after reserve(nvar) and a warm-up, one corrected apply captured in a single-stream graph; two replays on new inputs, each
    bitwise the eager result on that input"""
    import torch
    w, wM, Mw, X = noncons(4097)
    nvar, ncol = X.shape
    w.reserve(nvar)
    x = torch.from_numpy(X).cuda()
    out = torch.empty((nvar, w.nrow_d), dtype=torch.float64, device="cuda")
    w.apply_device(x, out=out, fill=FILL, force_conservation=True)                      # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        w.apply_device(x, out=out, fill=FILL, force_conservation=True)
    rng = np.random.default_rng(12)
    for rep in range(2):
        Xr = rng.uniform(0.5, 2.0, (nvar, ncol)) * (rep + 2.0)
        x.copy_(torch.from_numpy(Xr).cuda())
        out.fill_(CANARY)
        graph.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        eager = w.apply_device(x, fill=FILL, force_conservation=True).cpu().numpy()
        assert asc.same_bits(got, eager), "replay %d differs from the eager corrected apply" % rep
        y0 = w.apply_device(x, fill=FILL, force_conservation=False).cpu().numpy()
        report("corrected replay %d" % rep, corrected_gate(got, y0, Xr, wM, Mw, FILL, "replay %d" % rep))


# ---- E: longest rows first --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrow", [8192, 8193, 1])
def test_longest_rows_first_is_the_same_apply(nrow):
    """rowblock_lpt on a batched rowblock launch: at 8192 rows rowperm_kernel ranks the rows (most of them of 3 entries: ties by
    index), at 8193 rows and at 1 row the order is declined.  Either way the result is bitwise the apply without the option, and every
    row is written."""
    import torch
    recipe = akr.BY_NAME["spmm_rowblock_kernel<1, 1, 4, 4, false>"]
    m = asc.lpt_matrix(nrow, seed=nrow)
    w = handle(m)
    setup_recipe(recipe, w)
    nv = recipe["batch_nvar"]
    rng = np.random.default_rng(nrow)
    Xs = [rng.uniform(0.5, 2.0, (nv, m.ncol)) * rng.choice([-1.0, 1.0], (nv, m.ncol)) for _ in range(2)]
    for X in Xs:
        X[:, m.ncol - 1] = np.nan
    xs = [torch.from_numpy(X).cuda() for X in Xs]
    got = []
    for lpt in (None, 1):
        w.set_option("rowblock_lpt", lpt)
        outs = [torch.full((nv, nrow), CANARY, dtype=torch.float64, device="cuda") for _ in xs]
        w.apply_many_device(xs, outs, fill=FILL, force_conservation=False)
        torch.cuda.synchronize()
        got.append(([o.cpu().numpy() for o in outs], w.last_launch()))
    (base, name0), (lpt, name1) = got
    assert name0 == name1 and name0.startswith("spmm_rowblock_kernel") and (nrow == 1 or name0 == recipe["name"]), (name0, name1)
    for q in range(2):
        assert not np.any(base[q] == CANARY) and not np.any(lpt[q] == CANARY)
        assert asc.same_bits(lpt[q], base[q]), "batch %d: longest rows first changed the result" % q
        report("rowblock %d rows batch %d" % (nrow, q), asc.check_product(m, base[q], Xs[q], FILL, "rowblock %d rows" % nrow))


# ---- F: the leading dimension of a field batch ------------------------------------------------------------------------------------
def test_broadcast_fields_are_refused_and_a_slice_of_a_wider_buffer_is_taken():
    """Three fields on the 50 km IvA through apply_many_device, apply_transformed_device and apply_sharded (world 1): a broadcast
    batch (x.expand(3, -1), row stride 0) raises ValueError before anything is launched -- the result array keeps its canaries --, and
    a [3, n] slice of a [3, n + 5] buffer gives bitwise the result of the contiguous batch."""
    import torch
    from icebin_amd import synthetic as syn
    from icebin_amd.distributed import Communicator, apply_sharded
    g = syn.make_grids("g50")
    w = icebin_amd.from_synthetic(g).regrid_matrices("greenland", syn.dome_elevmask(g)).matrix("IvA")
    n, nrow = w.ncol_d, w.nrow_d
    x = torch.from_numpy(syn.fields(3, n)).cuda()
    wide = torch.full((3, n + 5), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, :n] = x
    T, b, comm = np.eye(3), np.zeros(3), Communicator()
    calls = {"apply_many_device": lambda a, out: w.apply_many_device([a], [out], fill=FILL)[0],
             "apply_transformed_device": lambda a, out: w.apply_transformed_device(a, T, b, out=out, fill=FILL),
             "apply_sharded": lambda a, out: apply_sharded(w, comm, a, out_all=out, fill=FILL)}
    for name, call in calls.items():
        outs = [torch.full((3, nrow), CANARY, dtype=torch.float64, device="cuda") for _ in range(3)]
        with pytest.raises(ValueError, match="planes overlap: stride 0 < %d cells" % n):
            call(x[:1].expand(3, -1), outs[0])
        torch.cuda.synchronize()
        assert bool((outs[0] == CANARY).all()), name + ": the refused call wrote its result array"
        assert call(x, outs[1]) is outs[1] and call(wide[:, :n], outs[2]) is outs[2]
        comm.wait()
        torch.cuda.synchronize()
        assert not bool((outs[1] == CANARY).any()), name
        assert torch.equal(outs[1].view(torch.int64), outs[2].view(torch.int64)), name + ": the slice of a wider buffer differs"
    comm.close()
