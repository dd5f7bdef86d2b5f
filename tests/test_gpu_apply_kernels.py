"""Every apply-kernel instantiation (tests/apply_kernel_recipes.py: one recipe each) against an exact row-by-row reference.

The reference is the matrix's own CSR (coo_dense) summed in long double.  Each row and field must satisfy
    |y_i - ref_i| <= (n_i + 8) * 2^-53 * S_i,   S_i = sum_j |a_ij x_j|,   n_i = entries of row i,
dead rows (wM == 0) hold `fill` exactly and live rows without entries exactly 0.  The synthetic matrices have rows of one magnitude
with mixed signs and magnitudes spread over 10^+-100: a dropped, doubled or misplaced entry misses the bound by orders of magnitude,
and no global normalisation can hide a row.  Every apply also checks that it launched the recipe's instantiation, wrote every
element of its result and nothing around it (padded leading dimensions, a base offset, one plane beyond nvar, NaN in the input's
padding columns)."""
import os
import sys

import numpy as np
import pytest

import icebin_amd
from icebin_amd import synthetic as syn
from icebin_amd.linear import linear_Weighted

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import apply_kernel_recipes as akr  # noqa: E402

pytestmark = pytest.mark.gpu

U = np.longdouble(2.0) ** -53
FILL = -7.25
CANARY = 1234.5e-3


# ---- matrices --------------------------------------------------------------------------------------------------------------
def _csr_from_rows(cols, rng, ncol, dead=()):
    """rows of one magnitude (10^e, e in [-100, 100]) with mixed signs; wM = 0 on the dead rows."""
    nrow = len(cols)
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    colind = np.concatenate([np.asarray(c, np.int64) for c in cols] + [np.zeros(0, np.int64)]).astype(np.int32)
    mag = 10.0 ** rng.integers(-100, 101, nrow)
    val = np.repeat(mag, np.diff(rowptr)) * rng.uniform(1.0, 2.0, len(colind)) * rng.choice([-1.0, 1.0], len(colind))
    wM = np.ones(nrow)
    wM[list(dead)] = 0.0
    return linear_Weighted.from_csr((nrow, ncol), rowptr, colind, val, wM, np.ones(ncol))


def synthetic_lengths(unroll, wk):
    b = unroll * 64 * wk
    return sorted({0, 1, 63, 64, 65, b - 1, b, b + 1, 1023, 1024, 1025, 2049, 5000} - {-1})


def make_synthetic(unroll, wk):
    """The rows the row kernels' control flow turns on: 0, 1, 63..65, the instantiation's own batch UNROLL*64*WK +-1, one
    staged segment (1024) +-1, 2049, ~5000 (several prefetched segments), a dead row of 1025 entries, an empty dead row -- shuffled
    among 300 short rows numbered cell by cell (runs of 45 rows sharing two columns, edge rows of 3-4 entries: the shortrow kernel's
    shared-column form).  Column ncol - 1 is never referenced."""
    rng = np.random.default_rng(1000 * unroll + wk)
    ncol = 6001
    cols = [np.sort(rng.choice(ncol - 1, n, replace=False)) for n in synthetic_lengths(unroll, wk)]
    cols += [np.sort(rng.choice(ncol - 1, 1025, replace=False)), np.zeros(0, np.int64)]
    for k in range(300):
        c = 2 * (k // 45)
        cols.append([c, c + 1] if k % 45 not in (0, 44) else [c, c + 1, c + 2, c + 3][: 3 + (k % 2)])
    order = rng.permutation(len(cols))
    cols = [cols[i] for i in order]
    nl = len(synthetic_lengths(unroll, wk))
    dead = [int(np.flatnonzero(order == nl)[0]), int(np.flatnonzero(order == nl + 1)[0])]
    return _csr_from_rows(cols, rng, ncol, dead)


def make_banded():
    """Columns of one or two entries (neighbouring rows overlap by 8 columns): a column sweep takes it, one item per column.  One
    dead row, one live row without entries."""
    rng = np.random.default_rng(97)
    ncol = 6000
    cols = [np.arange(max(0, 20 * r - 4), min(ncol, 20 * r + 24)) for r in range(300)]
    cols.insert(150, np.zeros(0, np.int64))
    return _csr_from_rows(cols, rng, ncol, dead=[7])


_rm_cache = {}


def regrid_matrices(family):
    if family not in _rm_cache:
        cfg, kw, spacing = akr.FAMILIES[family]
        g = syn.make_grids(cfg, **kw)
        if spacing is not None:
            g["hcdefs"] = np.arange(len(g["hcdefs"]), dtype=np.float64) * spacing - 30.0
        em = syn.dome_elevmask(g)
        _rm_cache[family] = icebin_amd.from_synthetic(g).regrid_matrices("greenland", em, scale=True, correctA=True)
    return _rm_cache[family]


def make_matrix(recipe):
    fam = recipe["family"]
    if fam == "synthetic":
        return make_synthetic(recipe.get("unroll", 1), recipe.get("wk", 1))
    if fam == "banded":
        return make_banded()
    return regrid_matrices(fam).matrix("EvI")


# ---- reference -------------------------------------------------------------------------------------------------------------
class Reference:
    """y = M x row by row in long double from the matrix's own CSR, with S = sum |a x| and the entry count of every row."""

    def __init__(self, w):
        self.row, self.col, self.val = w.coo_dense()
        self.nrow, self.ncol = w.nrow_d, w.ncol_d
        self.cnt = np.bincount(self.row, minlength=self.nrow)
        self.starts = np.concatenate([[0], np.cumsum(self.cnt)[:-1]])
        self.wM = w.wM.copy()
        self.v = self.val.astype(np.longdouble)

    def __call__(self, X):
        nv = X.shape[0]
        ref = np.zeros((nv, self.nrow), np.longdouble)
        S = np.zeros((nv, self.nrow), np.longdouble)
        has = self.cnt > 0
        if len(self.val):
            for f in range(nv):
                p = self.v * X[f, self.col].astype(np.longdouble)
                ref[f, has] = np.add.reduceat(p, self.starts[has])
                S[f, has] = np.add.reduceat(np.abs(p), self.starts[has])
        return ref, S

    def check(self, y, X, fill, what):
        ref, S = self(X)
        assert_rows(y, ref, S, self.cnt, self.wM, fill, what)


def assert_rows(y, ref, S, cnt, wM, fill, what):
    dead = wM == 0.0
    live = ~dead
    if dead.any():
        d = y[:, dead]
        assert (np.all(np.isnan(d)) if np.isnan(fill) else np.all(d == fill)), "%s: dead rows do not hold fill" % what
    yl, rl, sl = y[:, live], ref[:, live], S[:, live]
    nan_ref = np.isnan(rl)
    bad = np.isnan(yl) != nan_ref
    assert not bad.any(), "%s: NaN pattern differs at (field, live row) %s" % (what, np.argwhere(bad)[:5].tolist())
    empty = cnt[live] == 0
    assert np.all(yl[:, empty] == 0.0), "%s: live rows without entries are not 0" % what
    ok = ~nan_ref
    err = np.abs(yl.astype(np.longdouble) - rl)
    tol = (cnt[live][None, :] + 8) * U * sl
    viol = ok & ~(err <= tol)
    if viol.any():
        f, r = np.argwhere(viol)[0]
        raise AssertionError("%s: %d (field, row) values outside the bound; first: field %d live row %d (%d entries) y=%r ref=%r "
                             "err=%.3Le tol=%.3Le" % (what, viol.sum(), f, r, cnt[live][r], yl[f, r], float(rl[f, r]), err[f, r], tol[f, r]))


def inputs(ref, nv, seed):
    """x in +-[0.5, 2]; field 0 carries NaN in one referenced column (the last entry of a row) and in every unreferenced one."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.5, 2.0, (nv, ref.ncol)) * rng.choice([-1.0, 1.0], (nv, ref.ncol))
    if len(ref.col):
        k = np.flatnonzero(ref.cnt > 1)
        r = k[len(k) // 2] if len(k) else ref.row[0]
        X[0, ref.col[ref.starts[r] + ref.cnt[r] - 1]] = np.nan
    X[0, np.setdiff1d(np.arange(ref.ncol), ref.col)] = np.nan
    return X


# ---- padded device buffers ---------------------------------------------------------------------------------------------------
def padded_input(torch, X, pad=3):
    nv, n = X.shape
    buf = torch.full((nv, n + pad), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :n] = torch.from_numpy(X).cuda()
    return buf[:, :n]


class PaddedOutput:
    """[nvar, n] result planes at a base offset inside a canary-filled buffer: leading dimension n + 5, one more plane beyond nvar."""

    def __init__(self, torch, nv, n, off=3, pad=5):
        self.nv, self.n, self.off, self.ld = nv, n, off, n + pad
        self.buf = torch.full((off + (nv + 1) * self.ld + 8,), CANARY, dtype=torch.float64, device="cuda")
        self.view = self.buf[off:off + nv * self.ld].view(nv, self.ld)[:, :n]

    def result(self, what):
        b = self.buf.cpu().numpy()
        planes = b[self.off:self.off + self.nv * self.ld].reshape(self.nv, self.ld)
        outside = np.concatenate([b[:self.off], planes[:, self.n:].ravel(), b[self.off + self.nv * self.ld:]])
        assert np.all(outside == CANARY), "%s: wrote outside its result planes" % what
        y = planes[:, :self.n].copy()
        assert not np.any(y == CANARY), "%s: result elements left unwritten" % what
        return y


# ---- one recipe --------------------------------------------------------------------------------------------------------------
def setup_recipe(recipe, w):
    for k, v in recipe["options"].items():
        w.set_option(k, v)
    if recipe["entry"] == "apply_pair_device":
        second = regrid_matrices(recipe["family"]).matrix("AvE")
        w.pair_prepare(second, 16)
        return second
    if recipe["kernel"] == "rowdual":
        w.prepare(4, 1)                 # the bands (rowdual_min_work = 1: at once), under the automatic choice that builds them
        w.set_kernel("rowdual")
    else:
        w.set_kernel(recipe["kernel"])
        if recipe["prepare"]:
            w.prepare(16, 1)
    return None


def uses_block_to_task(recipe):
    return not recipe["name"].startswith(("spmm_shortrow", "spmm_sweep"))


@pytest.mark.parametrize("name", [r["name"] for r in akr.RECIPES])
def test_apply_kernel_against_exact_rows(name):
    import torch
    recipe = akr.BY_NAME[name]
    w = make_matrix(recipe)
    second = setup_recipe(recipe, w)
    ref = Reference(w)
    nvmax = max(recipe["nvars"] + [recipe.get("batch_nvar", 1)])
    X = inputs(ref, nvmax, seed=len(name))

    def launched(what):
        assert w.last_launch() == name, "%s: launched %r" % (what, w.last_launch())

    cases = [(nv, None) for nv in recipe["nvars"]]
    if uses_block_to_task(recipe):      # (row, chunk) -> workgroup by contiguous ranges where an XCD would own whole chunks
        cases += [(nv, 0) for nv in (recipe["fb"], 8 * recipe["fb"])]
    for nv, xcd in cases:
        what = "%s nvar=%d xcd_mode=%s" % (name, nv, xcd)
        if xcd is not None:
            w.set_option("rowblock_xcd_mode", xcd)
        try:
            x = padded_input(torch, X[:nv])
            if second is None:
                out = PaddedOutput(torch, nv, ref.nrow)
                w.apply_device(x, out=out.view, fill=FILL, force_conservation=False)
                torch.cuda.synchronize()
                launched(what)
                ref.check(out.result(what), X[:nv], FILL, what)
            else:
                out1, out2 = PaddedOutput(torch, nv, ref.nrow), PaddedOutput(torch, nv, second.nrow_d)
                w.apply_pair_device(second, x, out1=out1.view, out2=out2.view, fill=FILL)
                torch.cuda.synchronize()
                launched(what)
                y1 = out1.result(what)
                ref.check(y1, X[:nv], FILL, what)
                # the second matrix reads the first one's rows (its own numbering of E): reference on the first result as computed
                perm = np.argsort(w.dim(0))[np.searchsorted(np.sort(w.dim(0)), second.dim(1))]
                Reference(second).check(out2.result(what + " (second)"), y1[:, perm], FILL, what + " (second)")
        finally:
            if xcd is not None:
                w.set_option("rowblock_xcd_mode", None)

    # batched launches: each batch its own input, bitwise the separate single applies (33 batches: two launches)
    if recipe["nbatch"]:
        nv = recipe["batch_nvar"]
        rng = np.random.default_rng(7)
        xs = [padded_input(torch, X[:nv] if q == 0 else rng.uniform(0.5, 2.0, (nv, ref.ncol)) * rng.choice([-1.0, 1.0], (nv, ref.ncol)))
              for q in range(max(recipe["nbatch"]))]
        sep = []
        for x in xs:
            sep.append(w.apply_device(x, fill=FILL, force_conservation=False).cpu().numpy())
            launched("%s single apply" % name)
        ref.check(sep[0], X[:nv], FILL, name + " single apply of batch 0")
        variants = [None]
        if name.startswith("spmm_rowblock") and name.endswith("false>"):
            variants.append(("rowblock_lpt", 1))             # longest rows first
        if name.startswith("spmm_shortrow"):
            variants.append(("shortrow_many", 2))            # two batches per launch
        for var in variants:
            if var:
                w.set_option(*var)
            try:
                for nb in recipe["nbatch"] if var is None else [max(recipe["nbatch"])]:
                    outs = w.apply_many_device(xs[:nb], fill=FILL, force_conservation=False)
                    torch.cuda.synchronize()
                    launched("%s nbatch=%d %s" % (name, nb, var))
                    for q in range(nb):
                        assert np.array_equal(outs[q].cpu().numpy().view(np.uint64), sep[q].view(np.uint64)), \
                            "%s nbatch=%d %s: batch %d differs from its single apply" % (name, nb, var, q)
            finally:
                if var:
                    w.set_option(var[0], None)


# ---- bitwise classes -------------------------------------------------------------------------------------------------------
def bitwise_class(name):
    """Lane l of a row kernel sums entries l, l + 64 WK, ... in order whatever FPW, UNROLL or NW (segments of 1024 are whole
    batches of 64 WK), then the same wave sum and, for WK > 1, the same cross-wave sum: one class per WK, the lean single-apply
    kernel in the WK = 1 class.  The shortrow forms (plain, transposed input, shared columns, re-aligned or non-temporal stores) add
    a row's entries in the row's order."""
    if name.startswith("spmm_rowone"):
        return "rowblock WK=1"
    if name.startswith("spmm_rowblock") and name.endswith("false>"):
        return "rowblock WK=%s" % name.split("<")[1].split(",")[1].strip()
    if name.startswith("spmm_shortrow"):
        return "shortrow"
    return None


def test_row_kernels_are_bitwise_identical_within_each_class():
    import torch
    w0 = make_synthetic(4, 1)
    ref = Reference(w0)
    nv = 9
    X = inputs(ref, nv, seed=3)
    rowptr, col, val = w0.csr_dense()
    x = torch.from_numpy(X).cuda()
    got = {}
    for r in akr.RECIPES:
        cls = bitwise_class(r["name"])
        if cls is None:
            continue
        w = linear_Weighted.from_csr((w0.nrow_d, w0.ncol_d), rowptr, col, val, w0.wM, w0.Mw)
        setup_recipe(r, w)
        y = w.apply_device(x, fill=FILL, force_conservation=False).cpu().numpy()
        assert w.last_launch() == r["name"], (r["name"], w.last_launch())
        got.setdefault(cls, []).append((r["name"], y))
    assert sorted((k, len(v)) for k, v in got.items()) == [("rowblock WK=1", 31 + 7), ("rowblock WK=2", 12), ("rowblock WK=4", 12),
                                                           ("shortrow", 24)]
    for cls, ys in got.items():
        base_name, base = ys[0]
        ref.check(base, X, FILL, base_name)
        for n, y in ys[1:]:
            assert np.array_equal(np.isnan(y), np.isnan(base)), (cls, n)
            m = ~np.isnan(base)
            diff = y[m].view(np.uint64) != base[m].view(np.uint64)
            assert not diff.any(), "%s: %s differs from %s in %d values" % (cls, n, base_name, diff.sum())


# ---- conservation correction -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncol", [4096, 4097, 2_000_003])
def test_conservation_correction_against_exact_dot_products(ncol):
    """A non-conservative matrix applied with force_conservation: B_k *= (Mw . A_k) / (wM . B_k) over the rows with wM != 0.  At
    4097 and 2e6 columns the dot products are cut into chunks (2 and the cap of 256) summed by weight_dot_final_kernel.  NaN in
    columns with Mw == 0 that no row reads must not reach the factor."""
    import torch
    rng = np.random.default_rng(ncol)
    nrow, per = 700, 40
    row = np.repeat(np.arange(nrow), per)
    col = rng.integers(0, ncol, nrow * per)
    val = rng.uniform(0.5, 2.0, nrow * per)
    wM = rng.uniform(0.5, 2.0, nrow)
    wM[::50] = 0.0
    Mw = rng.uniform(0.5, 2.0, ncol)
    free = np.setdiff1d(np.arange(ncol), col)
    Mw[free[::3]] = 0.0
    w = linear_Weighted.from_coo((nrow, ncol), row, col, val, wM, Mw, conservative=False)
    nv = 3
    X = rng.uniform(0.5, 2.0, (nv, ncol))
    X[1, free[::3]] = np.nan
    x = torch.from_numpy(X).cuda()
    y0 = w.apply_device(x, fill=FILL, force_conservation=False).cpu().numpy()
    y1 = w.apply_device(x, fill=FILL, force_conservation=True).cpu().numpy()
    ref = Reference(w)
    ref.check(y0, X, FILL, "uncorrected")
    live = wM != 0.0
    assert np.all(y1[:, ~live] == FILL)
    Xl = np.where(Mw[None, :] != 0.0, X, 0.0).astype(np.longdouble)
    TA = (Xl * Mw.astype(np.longdouble)).sum(axis=1)
    SA = (np.abs(Xl) * Mw.astype(np.longdouble)).sum(axis=1)
    Y0 = y0[:, live].astype(np.longdouble)
    TB = (Y0 * wM[live].astype(np.longdouble)).sum(axis=1)
    SB = (np.abs(Y0) * wM[live].astype(np.longdouble)).sum(axis=1)
    exact = Y0 * (TA / TB)[:, None]
    rel = ((ncol + 8) * U * SA / np.abs(TA) + (live.sum() + 8) * U * SB / np.abs(TB) + 4 * U)[:, None]
    err = np.abs(y1[:, live].astype(np.longdouble) - exact)
    assert np.all(err <= rel * np.abs(exact)), float(np.max(err / np.abs(exact) / rel))
