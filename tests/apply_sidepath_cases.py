"""The inputs and the plain references of tests/test_gpu_apply_sidepaths.py: the apply's side paths below spmm.hip's conservation
banner -- the transformed product M (V T + b), the legacy matvec, the weight dots, the conservation correction, the longest-rows-first
order.  numpy only (long double and math.fsum); the package under test is not imported, so tests/test_apply_sidepath_cases.py can pin
every reference against the CPU oracle on a machine without a GPU.

Bounds (u = 2^-53, n_i = stored entries of row i), all derived, none measured:
  dot products and row sums of products   |got - ref| <= (n + 8) u sum|terms|
  transformed product, either side of M   |y_ki - ref_ki| <= (n_i + nin + 12) u sum_j |a_ij| (sum_l |T_lk V_lj| + |b_k|)
      M (V T + b) and T^T (M V) + b (M 1) are sums of the same products a_ij T_lk V_lj and a_ij b_k; a product takes part in at most
      n_i + nin + 2 rounded operations on its way into y_ki in either order (nin fused steps and the offset in the transform, n_i
      fused steps and 6 wave-sum additions in the row, or those of the row first and then nin + 1 in the transform, the row sum M 1
      with its own n_i + 6), so the first-order forward error is within (n_i + nin + 12) u times the sum of their magnitudes.
  corrected apply                         |y1 - y0 TA/TB| <= ((ncol + 8) u SA/|TA| + (nlive + 8) u SB/|TB| + 4 u) |y0 TA/TB|
      the two dot products by the first bound, one division, one multiplication (test_gpu_apply_kernels.py's bound).
Exact cases: values and weights are powers of two in [2^-3, 2^3], fields small positive integers; every partial sum is a multiple of
2^-6 below 2^40, so every order of summation gives the same bits (test_apply_sidepath_cases.py proves it with math.fsum).

A CSR row holds a column once, so the 1025-entry row of the issue's list exists where ncol - 1 >= 1025 (the legacy matvec's matrices,
the longest-rows-first ones); in the transformed product's 255..400-column matrices it is the full row of ncol - 1 entries."""
import math

import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53

# the constants of spmm.hip that the cases turn on
TB_MAX = 384                       # doubles of T and b that travel in the kernarg segment
WD_MINLEN, WD_MAXCHUNK = 4096, 256
IBH_MAX_BATCH = 32
LPT_MAX_ROWS = 8192

LENGTHS = (0, 1, 63, 64, 65, 130, 1025)
FILL = -7.25
CANARY = 1234.5e-3


# ---- matrices ---------------------------------------------------------------------------------------------------------------
class Csr:
    """rowptr / colind / val, the weights, and where the special rows went (name -> row)."""

    def __init__(self, nrow, ncol, rowptr, colind, val, wM, Mw, where):
        self.nrow, self.ncol, self.rowptr, self.colind, self.val, self.wM, self.Mw, self.where = nrow, ncol, rowptr, colind, val, wM, Mw, where
        self.cnt = np.diff(rowptr)
        self.row = np.repeat(np.arange(nrow, dtype=np.int32), self.cnt)
        self.starts = rowptr[:-1].astype(np.int64)
        self.nnz = len(colind)

    def entries(self, r):
        return slice(int(self.rowptr[r]), int(self.rowptr[r + 1]))

    def row_sums(self, p):
        """per-row sums of the per-entry terms p[..., nnz] (long double, row order)"""
        out = np.zeros(p.shape[:-1] + (self.nrow,), LD)
        has = self.cnt > 0
        if self.nnz:
            out[..., has] = np.add.reduceat(p, self.starts[has], axis=-1)
        return out


def _row(seed, k, n, ncol, exact):
    """row k of a matrix: n columns below ncol - 1 and their values, from a generator of its own, so that the same row one entry
    longer is the same row plus that entry"""
    r = np.random.default_rng([seed, k])
    c = r.permutation(ncol - 1)[:n]
    u = r.uniform(size=(len(c), 2))
    v = 2.0 ** (np.floor(7 * u[:, 0]) - 3) if exact else (0.5 + 1.5 * u[:, 0]) * np.where(u[:, 1] < 0.5, -1.0, 1.0)
    o = np.argsort(c)
    return c[o], v[o]


def _finish(lens, names, ncol, seed, exact, dead):
    nrow = len(lens)
    rng = np.random.default_rng(seed)
    order = rng.permutation(nrow)
    rows = [_row(seed, int(k), int(lens[k]), ncol, exact) for k in order]
    where = {n: int(np.flatnonzero(order == k)[0]) for k, n in enumerate(names)}
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int32)
    colind = np.concatenate([c for c, _ in rows]).astype(np.int32)
    val = np.concatenate([v for _, v in rows])
    if exact:
        wM, Mw = 2.0 ** rng.integers(-3, 4, nrow), 2.0 ** rng.integers(-3, 4, ncol)
    else:
        wM, Mw = rng.uniform(0.5, 2.0, nrow), rng.uniform(0.5, 2.0, ncol)
    for n in dead:
        wM[where[n]] = 0.0
    Mw[ncol - 1] = 0.0                  # the column that no row names weighs nothing: its NaN stays out of Mw . X
    assert not np.any(val == 0.0) and colind.max(initial=0) < ncol - 1          # no stored zeros; the last column is never referenced
    return Csr(nrow, ncol, rowptr, colind, val, wM, Mw, where)


def side_matrix(nrow, ncol, seed, exact=False, short=None):
    """Rows of 0, 1, 63, 64, 65, 130 and min(1025, ncol - 1) entries, a dead row of min(66, ncol - 1) entries, a dead empty row, among
    short rows of 2-4 entries (or of the given lengths), shuffled.  Column ncol - 1 is never referenced."""
    names = ["len%d" % n for n in LENGTHS] + ["dead_entries", "dead_empty"]
    lens = [min(n, ncol - 1) for n in LENGTHS + (66, 0)]
    nshort = nrow - len(lens)
    short = np.random.default_rng([seed, nrow]).integers(2, 5, nshort) if short is None else np.asarray(short)
    assert len(short) == nshort and nshort > 0
    return _finish(lens + [int(n) for n in short], names, ncol, seed, exact, ("dead_entries", "dead_empty"))


def empty_matrix(n, seed, exact=False):
    """n x n without entries: only the weights matter.  A tenth of each weight vector is 0."""
    rng = np.random.default_rng(seed)
    if exact:
        wM, Mw = 2.0 ** rng.integers(-3, 4, n), 2.0 ** rng.integers(-3, 4, n)
    else:
        wM, Mw = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n), rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
    if n >= 10:
        wM[rng.choice(n, n // 10, replace=False)] = 0.0
        Mw[rng.choice(n, n // 10, replace=False)] = 0.0
    return Csr(n, n, np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0), wM, Mw, {})


def random_coo(nrow, ncol, per, seed):
    """The non-conservative matrices of the correction: `per` random entries a row (duplicates add up), a fiftieth of the rows dead,
    Mw == 0 on a third of the columns that no entry names."""
    rng = np.random.default_rng(seed)
    row = np.repeat(np.arange(nrow), per)
    col = rng.integers(0, ncol - 1, nrow * per)
    val = rng.uniform(0.5, 2.0, nrow * per)
    wM = rng.uniform(0.5, 2.0, nrow)
    wM[::50] = 0.0
    Mw = rng.uniform(0.5, 2.0, ncol)
    free = np.setdiff1d(np.arange(ncol), col)
    Mw[free[::3]] = 0.0
    return row, col, val, wM, Mw, free[::3]


# ---- gates --------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def holds(a, fill):
    return bool(np.all(np.isnan(a)) if np.isnan(fill) else np.all(a == fill))


def gate(y, ref, tol, what):
    """Every element: NaN exactly where the reference has it, |y - ref| <= tol elsewhere.  Returns the largest err / tol."""
    y = np.asarray(y)
    assert y.shape == ref.shape, "%s: shape %s, reference %s" % (what, y.shape, ref.shape)
    nan_ref = np.isnan(ref)
    bad = np.isnan(y) != nan_ref
    assert not bad.any(), "%s: NaN pattern differs at %s" % (what, np.argwhere(bad)[:5].tolist())
    ok = ~nan_ref
    err = np.where(ok, np.abs(np.where(ok, y, 0.0).astype(LD) - np.where(ok, ref, 0.0)), 0.0)
    tol = np.where(ok, tol, 0.0)
    viol = ~(err <= tol)
    if viol.any():
        i = tuple(np.argwhere(viol)[0])
        raise AssertionError("%s: %d values outside the bound; first at %s: y=%r ref=%r err=%.3e tol=%.3e"
                             % (what, viol.sum(), i, float(y[i]), float(ref[i]), float(err[i]), float(tol[i])))
    pos = tol > 0
    return float(np.max(err[pos] / tol[pos])) if pos.any() else 0.0


# ---- plain product --------------------------------------------------------------------------------------------------------------
def product_ref(m, X):
    """(ref, tol): y = M X row by row in long double with the dot bound (n_i + 8) u sum|a x|.  Dead rows are the caller's."""
    p = m.val.astype(LD) * X[:, m.colind].astype(LD)
    return m.row_sums(p), (m.cnt + 8) * U * m.row_sums(np.abs(p))


def check_product(m, y, X, fill, what):
    """a plain apply: dead rows hold fill exactly, live empty rows 0 exactly (tol == 0 there), the rest within the dot bound"""
    ref, tol = product_ref(m, X)
    dead = m.wM == 0.0
    assert holds(y[:, dead], fill), "%s: dead rows do not hold fill" % what
    return gate(y[:, ~dead], ref[:, ~dead], tol[:, ~dead], what)


# ---- A: transformed product ---------------------------------------------------------------------------------------------------
SHAPES_A = ((400, 255), (400, 256), (400, 257), (256, 256), (255, 400), (256, 400), (257, 400))
SIZES_A = ((1, 1), (5, 3), (23, 16), (31, 12), (24, 16))


def transforms_inputs_side(nrow, ncol):
    return ncol <= nrow


def coefficient_count(nin, nout):
    return nin * nout + nout


def transform(nin, nout, seed):
    """T [nin, nout] in +-[0.5, 2], b distinct and non-zero in every component.  (5, 3) is sparse: row 2 is all zero (its input
    variable is all NaN in transform_inputs) and every column keeps two entries."""
    rng = np.random.default_rng(1000 * nin + nout + 7919 * seed)
    T = rng.uniform(0.5, 2.0, (nin, nout)) * rng.choice([-1.0, 1.0], (nin, nout))
    if (nin, nout) == (5, 3):
        T[2, :] = 0.0
        T[0, 1] = T[1, 2] = T[3, 0] = T[3, 2] = T[4, 0] = T[4, 1] = 0.0
    b = (0.37 + seed) * (np.arange(nout) + 1.0) * np.where(np.arange(nout) % 2, -1.0, 1.0)
    return T, b


def nan_column(m):
    """the column whose NaN must reach exactly the rows that store it: the first entry of the 63-entry row"""
    return int(m.colind[m.rowptr[m.where["len63"]]])


def transform_inputs(m, nin, seed, T=None):
    """V [nin, ncol] in +-[0.5, 2]; NaN in the never-referenced column of every variable, in variable 0 at nan_column(m), and in the
    whole of every variable whose row of T is all zero."""
    rng = np.random.default_rng(seed)
    V = rng.uniform(0.5, 2.0, (nin, m.ncol)) * rng.choice([-1.0, 1.0], (nin, m.ncol))
    V[:, m.ncol - 1] = np.nan
    V[0, nan_column(m)] = np.nan
    if T is not None:
        V[~np.any(T != 0.0, axis=1), :] = np.nan
    return V


def transformed_ref(m, V, T, b, fill):
    """(ref, tol) of M (V T + b) in long double, skipping the entries of T that are exactly 0; dead rows hold fill with tol 0."""
    nin, nout = T.shape
    Vl = V.astype(LD)
    Xp = np.zeros((nout, m.ncol), LD)
    Xa = np.zeros((nout, m.ncol), LD)
    for k in range(nout):
        for l in range(nin):
            if T[l, k] != 0.0:
                t = LD(T[l, k]) * Vl[l]
                Xp[k] += t
                Xa[k] += np.abs(t)
        Xp[k] += LD(b[k])
        Xa[k] += abs(LD(b[k]))
    a = m.val.astype(LD)
    ref = m.row_sums(a * Xp[:, m.colind])
    tol = (m.cnt + nin + 12) * U * m.row_sums(np.abs(a) * Xa[:, m.colind])
    dead = m.wM == 0.0
    ref[:, dead], tol[:, dead] = fill, 0.0
    return ref, tol


def check_transformed(m, y, V, T, b, fill, what):
    ref, tol = transformed_ref(m, V, T, b, fill)
    dead = m.wM == 0.0
    assert holds(y[:, dead], fill), "%s: dead rows do not hold fill" % what
    assert np.all(y[:, m.where["len0"]] == 0.0), "%s: the live empty row is not 0" % what
    return gate(y[:, ~dead], ref[:, ~dead], tol[:, ~dead], what)


# ---- B: legacy matvec -----------------------------------------------------------------------------------------------------------
NROW_B, NCOL_B = 278, 1100


def matvec_matrices():
    """(thread, wave): 278 rows over 1100 columns with the same rows, except that the first short row has 3 entries in the first and
    the same 3 and one more in the second: nnz == 8 nrow - 1 = 2223 (one thread a row) and nnz == 8 nrow = 2224 (one wave a row)."""
    special = sum(LENGTHS) + 66
    nshort = NROW_B - len(LENGTHS) - 2
    out = []
    for extra in (0, 1):
        lens = np.full(nshort, 3)
        need = 8 * NROW_B - 1 - special - lens.sum()          # entries still missing of the thread form's count
        assert 0 <= need and need + 40 < nshort
        lens[1:1 + need + 20] = 4                              # 20 more rows of 4 ...
        lens[1 + need + 20:1 + need + 40] = 2                  # ... paid for by 20 rows of 2
        lens[0] += extra
        out.append(side_matrix(NROW_B, NCOL_B, 4242, short=lens))
    return tuple(out)


def _matvec_clean_columns(m):
    """the columns of the 63-, 64- and 65-entry rows: variable 0 is never NaN there, so that without ignore_nan these rows stay finite
    (a lane that drops entry 64 of the 65-entry row shows in both modes)"""
    return np.unique(np.concatenate([m.colind[m.entries(m.where[k])] for k in ("len63", "len64", "len65")]))


def matvec_all_nan_rows(m):
    """the rows whose every input is NaN in variable 0: the 1-entry row and the first short row clear of _matvec_clean_columns"""
    clean = _matvec_clean_columns(m)
    special = set(m.where.values())
    short = next(r for r in range(m.nrow) if r not in special and not np.isin(m.colind[m.entries(r)], clean).any())
    assert not np.isin(m.colind[m.entries(m.where["len1"])], clean).any()
    return [m.where["len1"], short]


def matvec_inputs(m, nvar, seed):
    """X [nvar, ncol]; the never-referenced column is NaN everywhere.  Variable 0: NaN in every input of matvec_all_nan_rows(m) and in
    the inputs of the 130-entry row but entries 3, 64, 129 and those in _matvec_clean_columns.  Variable 1 has no other NaN (the
    130- and 1025-entry rows stay finite without ignore_nan), variable 2 NaN in a random tenth of the columns."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.5, 2.0, (nvar, m.ncol)) * rng.choice([-1.0, 1.0], (nvar, m.ncol))
    X[:, m.ncol - 1] = np.nan
    for r in matvec_all_nan_rows(m):
        X[0, m.colind[m.entries(r)]] = np.nan
    c130 = np.delete(m.colind[m.entries(m.where["len130"])], [3, 64, 129])
    X[0, c130[~np.isin(c130, _matvec_clean_columns(m))]] = np.nan
    for f in range(2, nvar):
        X[f, rng.choice(m.ncol - 1, m.ncol // 10, replace=False)] = np.nan
    return X


def matvec_canaries(nvar, n):
    """a distinct value per element"""
    return 1000.0 + np.arange(nvar * n, dtype=np.float64).reshape(nvar, n)


def matvec_ref(m, X, Y0, ignore_nan):
    """The legacy contract: a row is written only if one of its terms survives; with ignore_nan the terms whose input is NaN are
    dropped.  Returns (ref, tol, written): ref holds Y0 with tol 0 where nothing is written."""
    x = X[:, m.colind].astype(LD)
    nanx = np.isnan(x)
    p = m.val.astype(LD) * x
    if ignore_nan:
        p = np.where(nanx, LD(0), p)
        n = m.row_sums((~nanx).astype(LD))
    else:
        n = np.broadcast_to(m.cnt.astype(LD), (X.shape[0], m.nrow))
    written = n > 0
    ref = np.where(written, m.row_sums(p), Y0.astype(LD))
    tol = np.where(written, (n + 8) * U * m.row_sums(np.abs(p)), LD(0))
    return ref, tol, written


# ---- C: weight dots --------------------------------------------------------------------------------------------------------------
SIZES_C = (1, 64, 1024, 1025, 4096, 4097, 8193, 1 << 20, (1 << 20) + 1)


def weight_dot_chunks(n):
    """(chunks, chunk length) of weight_dot_launch"""
    nchunk = 1 if n <= WD_MINLEN else min(WD_MAXCHUNK, -(-n // WD_MINLEN))
    return nchunk, -(-n // nchunk)


def weight_fields(w, nvar, seed, exact=False):
    """a different field per variable; NaN where the weight is 0"""
    rng = np.random.default_rng(seed)
    n = len(w)
    A = rng.integers(1, 9, (nvar, n)).astype(np.float64) if exact else rng.uniform(0.5, 2.0, (nvar, n)) * rng.choice([-1.0, 1.0], (nvar, n))
    A[:, w == 0.0] = np.nan
    return A


def weight_dot_ref(w, A):
    """(ref, tol) per variable: math.fsum of the float64 products over w != 0.  A product's own rounding is one of the bound's + 8."""
    live = w != 0.0
    ref, tol = [], []
    for a in A:
        t = w[live] * a[live]
        ref.append(LD(math.fsum(t)))
        tol.append((len(w) + 8) * U * LD(math.fsum(np.abs(t))))
    return np.array(ref, LD), np.array(tol, LD)


def sequential_sum(t):
    s = 0.0
    for v in np.asarray(t, np.float64).tolist():
        s += v
    return s


# ---- D: conservation correction ---------------------------------------------------------------------------------------------------
def correction_ref(y0, X, wM, Mw):
    """(exact, tol, factor64) of the corrected apply from the uncorrected result y0 AS COMPUTED: live rows times TA / TB with
    TA = Mw . X over Mw != 0 and TB = wM . y0 over wM != 0, in long double; factor64 is TA / TB evaluated in float64 from float64 sums
    (meaningful in the exact cases only).  Dead rows keep y0 (fill) with tol 0."""
    live, lc = wM != 0.0, Mw != 0.0
    Xl = X[:, lc].astype(LD)
    TA = (Xl * Mw[lc].astype(LD)).sum(axis=1)
    SA = (np.abs(Xl) * Mw[lc].astype(LD)).sum(axis=1)
    Y0 = y0[:, live].astype(LD)
    TB = (Y0 * wM[live].astype(LD)).sum(axis=1)
    SB = (np.abs(Y0) * np.abs(wM[live]).astype(LD)).sum(axis=1)
    rel = (len(Mw) + 8) * U * SA / np.abs(TA) + (live.sum() + 8) * U * SB / np.abs(TB) + 4 * U
    exact = y0.astype(LD)
    exact[:, live] = Y0 * (TA / TB)[:, None]
    tol = np.zeros(y0.shape, LD)
    tol[:, live] = rel[:, None] * np.abs(exact[:, live])
    return exact, tol, TA.astype(np.float64) / TB.astype(np.float64)


def correction_fields(nvar, ncol, nan_cols):
    """the fields of the random correction cases: NaN in variable 1 where Mw == 0 and no row reads"""
    X = np.random.default_rng(3).uniform(0.5, 2.0, (nvar, ncol))
    X[1, nan_cols] = np.nan
    return X


def batch_fields(X, nbatch):
    """X and nbatch - 1 more batches of its shape, a different random field with a scale of its own per batch and variable"""
    rng = np.random.default_rng(nbatch)
    return [X] + [rng.uniform(0.5, 2.0, X.shape) * rng.uniform(0.5, 3.0, (X.shape[0], 1)) for _ in range(nbatch - 1)]


def exact_fields(nvar, ncol, seed):
    X = np.random.default_rng(seed).integers(1, 9, (nvar, ncol)).astype(np.float64)
    X[:, ncol - 1] = np.nan
    return X


# ---- E: longest rows first ---------------------------------------------------------------------------------------------------------
def lpt_matrix(nrow, seed):
    """nrow rows over 2000 columns: most of 3 entries (ties resolve by index), every 97th of 2, every 101st of 5, and the lengths of
    LENGTHS where they fit."""
    if nrow == 1:
        return side_1row(seed)
    lens = np.full(nrow - len(LENGTHS) - 2, 3)
    lens[::97], lens[::101] = 2, 5
    return side_matrix(nrow, 2000, seed, short=lens)


def side_1row(seed):
    return _finish([130], ["len130"], 2000, seed, False, ())


# ---- triplets ----------------------------------------------------------------------------------------------------------------------
def csr_from_coo(nrow, ncol, row, col, val, wM, Mw):
    """triplets in any order, duplicates added up in the order given -> Csr (what from_coo loads)"""
    o = np.lexsort((col, row))
    row, col, val = np.asarray(row)[o], np.asarray(col)[o], np.asarray(val, np.float64)[o]
    first = np.ones(len(row), bool)
    first[1:] = (row[1:] != row[:-1]) | (col[1:] != col[:-1])
    start = np.flatnonzero(first)
    v = np.add.reduceat(val, start) if len(val) else val
    r = row[start]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=nrow))]).astype(np.int32)
    return Csr(nrow, ncol, rowptr, col[start].astype(np.int32), v, np.asarray(wM, np.float64), np.asarray(Mw, np.float64), {})


def shuffled_duplicate_triplets(m, seed):
    """the entries of m in a random order, every third one as two triplets of half the value (the halves add up to the value exactly)"""
    rng = np.random.default_rng(seed)
    split = np.arange(m.nnz) % 3 == 0
    row = np.concatenate([m.row, m.row[split]])
    col = np.concatenate([m.colind, m.colind[split]])
    val = np.concatenate([np.where(split, 0.5 * m.val, m.val), 0.5 * m.val[split]])
    o = rng.permutation(len(row))
    return row[o].astype(np.int32), col[o].astype(np.int32), val[o]
