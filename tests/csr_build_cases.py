"""The triplets -> CSR builder (csrbuild.hip build_csr_from_contributions and its helpers) and the CSR algebra (csrops.hip) at
their form edges: the table of selectors, the cases, and an exact restatement in plain Python / numpy float64.

A plain module (no test in it): tests/test_csr_build_cases.py checks on the CPU that every case lies where it claims, that the
restatement is the oracle, and that the values can tell a wrong kernel from a right one; tests/test_gpu_csr_build.py runs the
cases on the device, asserts the form that ran (ibh_selftest_triplets' info_out) and then the bits.

The restatement follows csrops.h and the comments of csrbuild.hip: triplets are ordered stably by (row, col); the terms of one
key are summed by an explicit sequential loop with the first term ASSIGNED (Eigen's setFromTriplets: a signed zero survives);
row sums run from 0.0 over ascending columns, column sums from 0.0 over ascending rows (spsparse sum); the product emits its
terms by row of L, k ascending, then the row of R; every product of a crop or scaling is rounded on its own."""
import numpy as np

SRB_MAX, CS_BIG = 32, 8192
INFO = ("order", "short_rows", "optimistic", "seg", "rowptr", "wM", "Mw", "nlong", "Mw_seg", "Mw_ptr")     # info_out of the hook
IN_ORDER, PIECES, RADIX = 0, 1, 2
NOT_TRIED, TAKEN, DECLINED = 0, 1, 2
HELD, FAILED = 1, 2
NONE, THREAD, WAVE = 0, 1, 2
SEARCH, HEADS_FILL = 1, 2
SLOTS, SORT = 1, 2
OPS = dict(transpose=0, crop_rows=1, crop_cols=2, scale_rows=3, scale_cols=4, scale_rows_recip=5, recip=6, mul=7, gather=8,
           expand_rows=9)

# selector -> (where it sits, what is measured (a key of measure()), the value on the first side, the value on the other side)
SELECTORS = {
    "seg_vals": ("seg_sums<false> in build_csr_from_contributions: n >= 8 * nnz", "n_minus_8nnz", 0, -1),
    "seg_wM": ("seg_sums<true> over the rows: nnz >= 8 * nrow", "nnz_minus_8nrow", 0, -1),
    "seg_Mw": ("seg_sums<true> in col_sums_by_sort: nnz >= 8 * ncol", "nnz_minus_8ncol", 0, -1),
    "chunk": ("k_seg_sums_wave: 64 values a chunk", "has_run_64_65", True, True),
    "rowptr": ("rowptr_from_rows: nrow < 65536", "nrow", 65535, 65536),
    "piece": ("order_and_chunk_sort: the longest piece <= 8192", "maxpiece", CS_BIG, CS_BIG + 1),
    "srb_try": ("build_csr_from_contributions: n <= 8 * nrow", "n_minus_8nrow", 0, 1),
    "srb_max": ("k_srb_unique: a row's contributions <= SRB_MAX", "maxrow_contrib", SRB_MAX, SRB_MAX + 1),
    "col_slots": ("the matrix builds: nnz <= 4 * ncol", "nnz_minus_4ncol", 0, 1),
    "col_pair": ("k_col_sums: a column of <= 2 entries in slot order", "has_col_2_3", True, True),
    "col_wave": ("k_col_sums / k_col_sums_long: a column of <= 64 entries", "has_col_64_65", True, True),
    "bits_row": ("bits_for(nrow): the row field of the sort keys", "nrow", 256, 257),
    "bits_col": ("bits_for(ncol): the column field of the sort keys", "ncol", 256, 257),
    "bits_row0": ("bits_for(1) == 0: no row field", "nrow", 1, 300),
    "bits_col0": ("bits_for(1) == 0: no column field", "ncol", 1, 300),
    "prod_emit": ("csr_product: total >= 8 * n", "total_minus_8n", 0, -1),
}


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def sum_assigned(v):
    """The terms of one key: the first assigned, the others added in order."""
    s = v[0]
    for x in v[1:]:
        s = s + x
    return s


def sum_from_zero(v):
    s = 0.0
    for x in v:
        s = s + x
    return s


def matrix(nrow, ncol, rowptr, colind, val):
    return dict(nrow=int(nrow), ncol=int(ncol), rowptr=np.asarray(rowptr, np.int32), colind=np.asarray(colind, np.int32),
                val=np.asarray(val, np.float64))


def runs_of(row, col):
    """The stable order by (row, col) and the [begin, end) of every key's run in it."""
    key = (np.asarray(row, np.int64) << 32) | np.asarray(col, np.int64)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]]) if len(ks) else np.zeros(0, np.int64)
    return order, ks, starts, np.r_[starts[1:], len(ks)].astype(np.int64)


def from_triplets(nrow, ncol, row, col, val):
    """Eigen setFromTriplets."""
    order, ks, starts, ends = runs_of(row, col)
    vs = np.asarray(val, np.float64)[order].tolist()
    out = [sum_assigned(vs[b:e]) for b, e in zip(starts.tolist(), ends.tolist())]
    uk = ks[starts]
    rowptr = np.searchsorted(uk >> 32, np.arange(nrow + 1))
    return matrix(nrow, ncol, rowptr, uk & 0xffffffff, out)


def weights(M):
    """(sum(M, 0, '+'), sum(M, 1, '+')): from 0.0, a row over ascending columns, a column over ascending rows."""
    v, rp = M["val"].tolist(), M["rowptr"].tolist()
    wM = [sum_from_zero(v[rp[r]:rp[r + 1]]) for r in range(M["nrow"])]
    Mw = [0.0] * M["ncol"]
    for c, x in zip(M["colind"].tolist(), v):               # CSR order: the rows of a column ascend
        Mw[c] = Mw[c] + x
    return np.asarray(wM, np.float64), np.asarray(Mw, np.float64)


def rows_of(M):
    return np.repeat(np.arange(M["nrow"], dtype=np.int32), np.diff(M["rowptr"]))


def product_terms(L, R):
    """The terms of L * R in emission order: by row of L, k ascending, then the row of R."""
    row, col, term = [], [], []
    Lp, Lc, Lv = L["rowptr"].tolist(), L["colind"].tolist(), L["val"].tolist()
    Rp, Rc, Rv = R["rowptr"].tolist(), R["colind"].tolist(), R["val"].tolist()
    for r in range(L["nrow"]):
        for e in range(Lp[r], Lp[r + 1]):
            k, l = Lc[e], Lv[e]
            for q in range(Rp[k], Rp[k + 1]):
                row.append(r); col.append(Rc[q]); term.append(l * Rv[q])
    return np.asarray(row, np.int32), np.asarray(col, np.int32), np.asarray(term, np.float64)


def product(L, R):
    row, col, term = product_terms(L, R)
    return from_triplets(L["nrow"], R["ncol"], row, col, term)


def transpose(M):
    return from_triplets(M["ncol"], M["nrow"], M["colind"], rows_of(M), M["val"])


def crop_rows(M, src, rs=None):
    """Row m of the result is row src[m] of M (-1: none), its values rs[src[m]] * v."""
    rp, ci, v = [0], [], []
    for p in np.asarray(src).tolist():
        if p >= 0:
            b, e = int(M["rowptr"][p]), int(M["rowptr"][p + 1])
            ci += M["colind"][b:e].tolist()
            v += [float(rs[p]) * x if rs is not None else x for x in M["val"][b:e].tolist()]
        rp.append(len(ci))
    return matrix(len(rp) - 1, M["ncol"], rp, ci, v)


def crop_cols(M, cmap, ncol_out, rs=None, cs=None):
    """Column k of M becomes cmap[k] (-1: dropped); the value is (rs[i] * v) * cs[cmap[k]], either factor optional."""
    rp, ci, v = [0], [], []
    for i in range(M["nrow"]):
        ent = []
        for e in range(int(M["rowptr"][i]), int(M["rowptr"][i + 1])):
            k = int(cmap[M["colind"][e]])
            if k < 0:
                continue
            x = float(M["val"][e])
            if rs is not None:
                x = float(rs[i]) * x
            if cs is not None:
                x = x * float(cs[k])
            ent.append((k, x))
        ent.sort()
        ci += [k for k, _ in ent]
        v += [x for _, x in ent]
        rp.append(len(ci))
    return matrix(M["nrow"], ncol_out, rp, ci, v)


def scale_rows(M, s):
    return dict(M, val=np.asarray(s, np.float64)[rows_of(M)] * M["val"])


def scale_cols(M, d):
    return dict(M, val=M["val"] * np.asarray(d, np.float64)[M["colind"]])


def scale_rows_recip(M, total):
    """val * (1 / total[row]): one reciprocal per row that has entries."""
    r = rows_of(M)
    inv = np.ones(M["nrow"])
    has = np.diff(M["rowptr"]) > 0
    inv[has] = 1. / np.asarray(total, np.float64)[has]
    return dict(M, val=M["val"] * inv[r])


# ---- values that tell a wrong sum from the right one -------------------------------------------------------------------------------
def chunked64(v, first_assigned):
    """A wrong wave form: every chunk of 64 summed on its own, the partial sums added."""
    parts = [sum_assigned(v[b:b + 64]) if first_assigned else sum_from_zero(v[b:b + 64]) for b in range(0, len(v), 64)]
    return sum_assigned(parts)


def wrong_sums(v, first_assigned):
    """name -> value of the ways a kernel could sum v wrongly (v: a list of floats, 3 or more of them)."""
    f = sum_assigned if first_assigned else sum_from_zero
    w = {"reversed": f(v[::-1]), "no_first": f(v[1:]), "no_last": f(v[:-1])}
    if len(v) >= 8:         # (np.sum adds fewer than 8 values one after the other: the sequential sum itself)
        w["pairwise"] = float(np.sum(np.asarray(v)))
    if len(v) > 65:         # (at 65 terms the second chunk is one term: the partial sums add up to the sequential sum, identically)
        w["chunked64"] = chunked64(v, first_assigned)
    for b in range(64, len(v), 64):                          # the terms on either side of every chunk boundary: dropped, swapped
        w["no_%d" % (b - 1)] = f(v[:b - 1] + v[b:])
        w["no_%d" % b] = f(v[:b] + v[b + 1:])
        w["swap_%d_%d" % (b - 1, b)] = f(v[:b - 1] + [v[b], v[b - 1]] + v[b + 1:])
    return w


def same_bits(a, b):
    return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


def is_sensitive(v, first_assigned=True):
    v = [float(x) for x in v]
    if len(v) < 3:
        return True
    right = sum_assigned(v) if first_assigned else sum_from_zero(v)
    return np.isfinite(right) and not any(same_bits(right, w) for w in wrong_sums(v, first_assigned).values())


def draw(rng, n, first_assigned=True):
    """n values N(0, 1) * 10**U(-2, 2), redrawn (the generator is seeded: the same every time) until every wrong sum differs.  (Over
    more decades a term next to a chunk boundary is too often absorbed whole by the running sum.)"""
    for _ in range(10000):
        v = rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 2, n)
        if is_sensitive(v, first_assigned):
            return v
    raise AssertionError("no sensitive values of length %d" % n)


NEG_ZEROS = "negative zeros"        # a run that opens with -0.0 and stays -0.0: the sum started at 0.0 is +0.0
ZERO_PAIR = "[-0.0, +0.0]"          # the second term turns the assigned -0.0 into +0.0: the first term alone is -0.0


# ---- input orders that keep every key's emission order ------------------------------------------------------------------------------
def interleave(rng, labels):
    """A random order of the multiset `labels` (one label per term); term j of a label stays before term j + 1: returns, for
    every output position, the index of the input term (terms are listed label by label in emission order)."""
    labels = np.asarray(labels)
    perm = rng.permutation(len(labels))
    shuffled = labels[perm]
    # the positions that hold label x, ascending, receive x's terms in their input order
    out = np.empty(len(labels), np.int64)
    src = np.argsort(labels, kind="stable")
    dst = np.argsort(shuffled, kind="stable")
    out[dst] = src
    return out


def shuffle_block(rng, key, lo, hi, whole_piece):
    """Positions [lo, hi) of a sorted sequence of keys reordered as interleave does; whole_piece: the block's largest key comes
    first and its smallest last, so the block is ONE piece of the order analysis (no cut inside)."""
    idx = np.arange(lo, hi)
    p = interleave(rng, key[idx])
    if whole_piece:
        k = key[idx][p]
        assert k.max() > k.min()
        a, b = int(np.flatnonzero(k == k.max())[0]), int(np.flatnonzero(k == k.min())[-1])
        order = [a] + [i for i in range(len(k)) if i not in (a, b)] + [b]
        p = p[order]
    return idx[p]


class Case:
    """Triplets for ibh_selftest_triplets: name, shape, triplets in input order, the modes to run, per mode the forms the case is
    about (a subset of INFO), and the selectors it sits at (selector -> the measured value)."""

    def __init__(self, name, nrow, ncol, row, col, val, forms, at=(), special=()):
        self.name, self.nrow, self.ncol = name, int(nrow), int(ncol)
        self.row, self.col = np.ascontiguousarray(row, np.int32), np.ascontiguousarray(col, np.int32)
        self.val = np.ascontiguousarray(val, np.float64)
        self.forms, self.at, self.special = forms, dict(at), dict(special)      # special: (row, col) -> NEG_ZEROS | ZERO_PAIR
        self.weight_groups = None           # "rows" / "cols": the weights' sums are held to the sensitivity conditions as well

    @property
    def n(self):
        return len(self.val)


def terms_case(name, nrow, ncol, keyed, rng, order="interleave", **kw):
    """keyed: [((row, col), values)] -- the terms of every key in emission order."""
    labels = np.repeat(np.arange(len(keyed)), [len(v) for _, v in keyed])
    row = np.repeat([k[0] for k, _ in keyed], [len(v) for _, v in keyed])
    col = np.repeat([k[1] for k, _ in keyed], [len(v) for _, v in keyed])
    val = np.concatenate([np.asarray(v, np.float64) for _, v in keyed]) if keyed else np.zeros(0)
    if order == "interleave":
        p = interleave(rng, labels)
    else:
        p = order(row, col)
    return Case(name, nrow, ncol, row[p], col[p], val[p], **kw)


def distinct_keys(rng, nrow, ncol, n, taken=()):
    free = np.setdiff1d(np.arange(nrow * ncol), [r * ncol + c for r, c in taken])
    k = rng.choice(free, n, replace=False)
    return [(int(q // ncol), int(q % ncol)) for q in k]


RUN_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 192, 193)


def run_length_keyed(rng, nrow, ncol):
    """The ten runs (964 terms): 2 is [-0.0, +0.0], 127 opens with -0.0 and stays -0.0 (a full first chunk and a tail of 63: a
    padding lane added as +0.0 would show), the others drawn."""
    keys = distinct_keys(rng, nrow, ncol, len(RUN_LENGTHS))
    keyed, special = [], {}
    for k, n in zip(keys, RUN_LENGTHS):
        if n == 2:
            v, special[k] = np.asarray([-0.0, 0.0]), ZERO_PAIR
        elif n == 127:
            v, special[k] = np.full(n, -0.0), NEG_ZEROS
        else:
            v = draw(rng, n)
        keyed.append((k, v))
    return keyed, special


def solve_pad(terms, units, mult):
    """(s, p): s units of one term and p of two bring `terms` over `units` to terms == mult * units exactly."""
    for p in range(0, 64):
        rest = terms - mult * units - (mult - 2) * p         # = (mult - 1) * s
        if rest >= 0 and rest % (mult - 1) == 0:
            return rest // (mult - 1), p
    raise AssertionError((terms, units, mult))


def run_length_cases():
    out = []
    nrow, ncol = 12, 13
    for name, pad in (("runs_alone", None), ("runs_thread", "thread"), ("runs_8nnz", 0), ("runs_8nnz_minus_1", -1)):
        rng = np.random.default_rng(101)
        keyed, special = run_length_keyed(rng, nrow, ncol)
        if pad == "thread":
            singles, pairs = 127, 0
        elif pad is not None:
            singles, pairs = solve_pad(964, 10, 8)
        else:
            singles, pairs = 0, 0
        extra = distinct_keys(rng, nrow, ncol, singles + pairs, [k for k, _ in keyed])
        for j, k in enumerate(extra):
            keyed.append((k, draw(rng, 2 if j < pairs else 1)))
        if pad == -1:                           # one term fewer: a pair becomes a single
            i = next(i for i, (_, v) in enumerate(keyed) if len(v) == 2 and keyed[i][0] not in special)
            keyed[i] = (keyed[i][0], keyed[i][1][:1])
        wave = pad in (None, 0)
        forms = {m: dict(seg=WAVE if wave else THREAD, short_rows=NOT_TRIED, rowptr=SEARCH) for m in (0, 1)}
        at = {"chunk": True}
        if pad in (0, -1):
            at["seg_vals"] = pad
        c = terms_case(name, nrow, ncol, keyed, rng, forms=forms, at=at, special=special)
        out.append(c)
    return out


def order_cases():
    """The same triplets in input orders that keep every key's emission order (mode 0): sorted, disordered inside short pieces, one
    piece of 8192 (sorted in LDS) and one of 8193 (radix)."""
    rng = np.random.default_rng(202)
    nrow, ncol, nkey = 100, 200, 3000
    keys = distinct_keys(rng, nrow, ncol, nkey)
    counts = 1 + rng.multinomial(9000 - nkey, np.ones(nkey) / nkey)
    keyed = [(k, draw(rng, int(n))) for k, n in zip(keys, counts)]

    def order_of(kind):
        def f(row, col):
            key = (row.astype(np.int64) << 32) | col
            p = np.argsort(key, kind="stable")
            ks = key[p]
            r = np.random.default_rng(7)
            if kind == "short_pieces":
                q = np.concatenate([shuffle_block(r, ks, b, min(b + 37, len(ks)), False) for b in range(0, len(ks), 37)])
            elif kind == "sorted":
                q = np.arange(len(ks))
            else:
                L = int(kind)
                starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
                ends_at = set(starts.tolist()) | {len(ks)}
                lo = next(int(b) for b in starts[40:] if int(b) + L in ends_at)     # the block begins and ends where a key does
                hi = lo + L
                q = np.r_[np.arange(lo), shuffle_block(r, ks, lo, hi, True), np.arange(hi, len(ks))]
            return p[q]
        return f

    out = []
    for kind, order in (("sorted", IN_ORDER), ("short_pieces", PIECES), (str(CS_BIG), PIECES), (str(CS_BIG + 1), RADIX)):
        at = {"piece": int(kind)} if kind.isdigit() else {}
        c = terms_case("order_" + kind, nrow, ncol, keyed, rng, order=order_of(kind), forms={0: dict(order=order)}, at=at)
        out.append(c)
    return out


def optimistic_cases():
    """Mode 1, past the per-row slots (n > 8 * nrow): row blocks in shuffled order with the columns ascending inside each (the
    row-only sort is the full order), and with one row's columns descending (its check fails, the full sort runs)."""
    out = []
    for name, want in (("optimistic_held", HELD), ("optimistic_failed", FAILED)):
        rng = np.random.default_rng(303)
        nrow, ncol = 50, 64
        row, col, val = [], [], []
        for r in rng.permutation(nrow).tolist():
            cols = np.sort(rng.choice(ncol, 12, replace=False))
            cols = np.repeat(cols, rng.integers(1, 4, len(cols)))            # duplicates, adjacent
            if want == FAILED and r == 17:
                cols = cols[::-1]
            row += [r] * len(cols); col += cols.tolist()
        row, col = np.asarray(row), np.asarray(col)
        val = np.zeros(len(row))
        order, ks, starts, ends = runs_of(row, col)
        for b, e in zip(starts, ends):
            val[order[b:e]] = draw(rng, int(e - b))
        out.append(Case(name, nrow, ncol, row, col, val, forms={1: dict(short_rows=NOT_TRIED, order=RADIX, optimistic=want)}))
    return out


def short_row_cases():
    """Mode 1: the longest row has 32 contributions (slots taken) or 33 (declined, then sorted); duplicate columns inside the short
    rows; n == 8 * nrow against 8 * nrow + 1 (slots not tried)."""
    out = []
    nrow, ncol = 40, 12
    for name, n, longest, want in (("srb_taken_32", 8 * nrow, SRB_MAX, TAKEN), ("srb_declined_33", 8 * nrow, SRB_MAX + 1, DECLINED),
                                   ("srb_not_tried", 8 * nrow + 1, SRB_MAX, NOT_TRIED)):
        rng = np.random.default_rng(404)
        cnt = np.zeros(nrow, np.int64)
        cnt[23] = longest
        others = np.setdiff1d(np.arange(nrow), [23, 5])                      # (row 5 stays empty)
        for _ in range(n - longest):
            while True:
                r = int(rng.choice(others))
                if cnt[r] < 12:
                    cnt[r] += 1
                    break
        row = np.repeat(np.arange(nrow), cnt)
        col = rng.integers(0, ncol, len(row))                                # 12 columns: a row of 32 repeats them
        p = rng.permutation(len(row))
        row, col = row[p], col[p]
        val = np.zeros(len(row))
        order, ks, starts, ends = runs_of(row, col)
        for b, e in zip(starts, ends):
            val[order[b:e]] = draw(rng, int(e - b))
        # the duplicates of one column of a short row are all -0.0: the per-row selection assigns its first term as well
        b, e = next((b, e) for b, e in zip(starts, ends) if e - b >= 2 and ks[b] >> 32 != 23)
        val[order[b:e]] = -0.0
        special = {(int(ks[b] >> 32), int(ks[b] & 0xffffffff)): NEG_ZEROS}
        forms = dict(short_rows=want)
        if want == TAKEN:
            forms.update(seg=NONE, rowptr=NONE, order=IN_ORDER)
        at = {"srb_try": n - 8 * nrow, "srb_max": longest}
        out.append(Case(name, nrow, ncol, row, col, val, forms={1: forms}, at=at, special=special))
    return out


def extent_cases():
    """Extents of 1 (a key field of 0 bits), 256 / 257 (8 / 9 bits) and 65535 / 65536 (the two row-pointer forms), with entries in
    the last row and the last column; the tall ones with empty leading and trailing rows and a gap of more than 256 rows, only
    the first row, only the last row; no triplets at all."""
    out = []

    def filled(name, nrow, ncol, n, rows, rng, at, forms=None, modes=(0, 1)):
        row = rng.choice(rows, n) if len(rows) else np.zeros(0, np.int64)
        col = rng.integers(0, ncol, n)
        if n and rows[-1] == nrow - 1:
            row[n // 2], col[n // 2] = nrow - 1, ncol - 1                    # the last row and the last column
        val = np.zeros(n)
        order, ks, starts, ends = runs_of(row, col)
        for b, e in zip(starts, ends):
            val[order[b:e]] = draw(rng, int(e - b))
        f = {m: dict(forms or {}) for m in modes}
        if nrow >= 65535 and 0 in f and n:
            f[0]["rowptr"] = SEARCH if nrow < 65536 else HEADS_FILL
        out.append(Case(name, nrow, ncol, row, col, val, forms=f, at=at))

    rng = np.random.default_rng(505)
    for nrow, ncol, n in ((1, 1, 70), (1, 300, 500), (300, 1, 500), (256, 256, 700), (257, 257, 700), (3, 65536, 3000)):
        at = {}
        if nrow in (256, 257):
            at.update(bits_row=nrow, bits_col=ncol)
        if nrow == 1 or (nrow, ncol) == (300, 1):
            at["bits_row0"] = nrow
        if ncol == 1 or (nrow, ncol) == (1, 300):
            at["bits_col0"] = ncol
        filled("extent_%dx%d" % (nrow, ncol), nrow, ncol, n, np.arange(nrow), rng, at)
    for nrow in (65535, 65536):
        some = np.r_[np.arange(1000, 30000), np.arange(30300, 60000)]        # leading, trailing and 300 middle rows empty
        filled("tall_%d_gaps" % nrow, nrow, 3, 3000, some, rng, {"rowptr": nrow})
        filled("tall_%d_dense" % nrow, nrow, 3, 3000, np.arange(nrow), rng, {"rowptr": nrow})
        filled("tall_%d_first_row" % nrow, nrow, 3, 40, np.asarray([0]), rng, {"rowptr": nrow})
        filled("tall_%d_last_row" % nrow, nrow, 3, 40, np.asarray([nrow - 1]), rng, {"rowptr": nrow})
        filled("tall_%d_empty" % nrow, nrow, 3, 0, np.zeros(0, np.int64), rng, {"rowptr": nrow})
    filled("empty_0x0", 0, 0, 0, np.zeros(0, np.int64), rng, {})
    filled("empty_5x7", 5, 7, 0, np.zeros(0, np.int64), rng, {})
    return out


ROW_LENGTHS = (0, 1, 63, 64, 65, 128, 129)
COL_LENGTHS = (0, 1, 2, 3, 64, 65, 130)


def weight_row_cases():
    """One term per key; rows of 0, 1, 63, 64, 65, 128 and 129 entries and one that holds only -0.0 (its sum from 0.0 is +0.0), on
    both sides of nnz >= 8 * nrow: the eight rows alone (wave), with 60 single-entry rows (thread), and at the two edge values."""
    out = []
    base = sum(ROW_LENGTHS) + 2
    for name, pad in (("wM_wave", None), ("wM_thread", "thread"), ("wM_8nrow", 0), ("wM_8nrow_minus_1", -1)):
        rng = np.random.default_rng(606)
        lengths = list(ROW_LENGTHS) + [2]
        if pad == "thread":
            lengths += [1] * 60
        elif pad is not None:
            s, p = solve_pad(base, len(lengths), 8)
            lengths += [2] * p + [1] * s
            if pad == -1:
                lengths[lengths.index(2, len(ROW_LENGTHS) + 1)] = 1
        ncol = 150
        row, col, val = [], [], []
        for r, n in enumerate(lengths):
            row += [r] * n
            col += np.sort(rng.choice(ncol - 1, n, replace=False)).tolist()
            val += (np.full(n, -0.0) if r == len(ROW_LENGTHS) else draw(rng, n, False)).tolist()
        row, col, val = np.asarray(row), np.asarray(col), np.asarray(val)
        col[-1] = ncol - 1 if lengths[-1] else col[-1]
        p = rng.permutation(len(row))
        wave = pad in (None, 0)
        at = {"seg_wM": pad} if pad in (0, -1) else {}
        c = Case(name, len(lengths), ncol, row[p], col[p], val[p], forms={0: dict(wM=WAVE if wave else THREAD)}, at=at)
        c.weight_groups, c.neg_zero_row = "rows", len(ROW_LENGTHS)
        out.append(c)
    return out


def weight_col_cases():
    """One term per key; columns of 0, 1, 2, 3, 64, 65 and 130 entries: with nnz == 4 * ncol (slots: two columns go to a wave each),
    at nnz == 4 * ncol + 1 (the sort, a thread per column), the seven columns alone (the sort, a wave per column, at nnz >= 8 * ncol
    and one below), and over 65 600 columns (slots)."""
    out = []
    nrow = 140
    base = sum(COL_LENGTHS)
    slots, sort_thread, sort_wave = dict(Mw=SLOTS, nlong=2), dict(Mw=SORT, Mw_seg=THREAD, Mw_ptr=SEARCH), dict(Mw=SORT, Mw_seg=WAVE, Mw_ptr=SEARCH)
    for name, singles, empties, forms in (("Mw_slots_4ncol", 3, 57, slots), ("Mw_sort_4ncol_plus_1", 4, 56, sort_thread),
                                          ("Mw_sort_wave", 0, 0, sort_wave), ("Mw_sort_8ncol", 0, 0, sort_wave),
                                          ("Mw_sort_8ncol_minus_1", 0, 0, sort_thread), ("Mw_slots_wide", 5, 65600, slots)):
        rng = np.random.default_rng(707)
        lengths = list(COL_LENGTHS) + [1] * singles
        if name.startswith("Mw_sort_8ncol"):
            s, p = solve_pad(base, len(COL_LENGTHS), 8)
            lengths += [2] * p + [1] * s
            if name.endswith("minus_1"):
                lengths[lengths.index(2, len(COL_LENGTHS))] = 1
        ncol = len(lengths) + empties
        cols = np.insert(rng.permutation(ncol - 1)[:len(lengths) - 1], COL_LENGTHS.index(130), ncol - 1)    # the longest is the last column
        row, col, val = [], [], []
        for c, n in zip(cols.tolist(), lengths):
            rows = np.sort(rng.choice(nrow, n, replace=False))
            row += rows.tolist(); col += [c] * n
            val += draw(rng, n, False).tolist()
        row, col, val = np.asarray(row), np.asarray(col), np.asarray(val)
        p = rng.permutation(len(row))
        nnz = len(row)
        at = {"col_pair": True, "col_wave": True}
        if name in ("Mw_slots_4ncol", "Mw_sort_4ncol_plus_1"):
            at["col_slots"] = nnz - 4 * ncol
        if name.startswith("Mw_sort_8ncol"):
            at["seg_Mw"] = nnz - 8 * ncol
        c = Case(name, nrow, ncol, row[p], col[p], val[p], forms={0: dict(forms)}, at=at)
        c.weight_groups = "cols"
        out.append(c)
    return out


def measure(c):
    """Every quantity a SELECTORS row or predict() speaks of, from the triplets alone."""
    row, col = c.row.astype(np.int64), c.col.astype(np.int64)
    n = len(row)
    key = (row << 32) | col
    order, ks, starts, ends = runs_of(row, col)
    nnz = len(starts)
    urow, ucol = ks[starts] >> 32, ks[starts] & 0xffffffff
    col_len = np.bincount(ucol, minlength=c.ncol) if nnz else np.zeros(c.ncol, np.int64)
    m = dict(n=n, nnz=nnz, nrow=c.nrow, ncol=c.ncol, n_minus_8nnz=n - 8 * nnz, nnz_minus_8nrow=nnz - 8 * c.nrow,
             nnz_minus_8ncol=nnz - 8 * c.ncol, n_minus_8nrow=n - 8 * c.nrow, nnz_minus_4ncol=nnz - 4 * c.ncol,
             maxrun=int((ends - starts).max()) if nnz else 0, runs=set((ends - starts).tolist()),
             maxrow_contrib=int(np.bincount(row).max()) if n else 0,
             row_lengths=set(np.bincount(urow, minlength=c.nrow).tolist()) if c.nrow else set(), col_lengths=set(col_len.tolist()),
             nlong=int(np.count_nonzero(col_len > 64)))
    m["has_run_64_65"] = {64, 65} <= m["runs"]
    m["has_col_2_3"] = {2, 3} <= m["col_lengths"]
    m["has_col_64_65"] = {64, 65} <= m["col_lengths"]
    m["full_dec"] = bool(n >= 2 and np.any(key[1:] < key[:-1]))
    m["lo_dec"] = bool(n >= 2 and np.any(col[1:] < col[:-1]))
    if n >= 2:
        before = np.r_[0, np.maximum.accumulate(key)[:-1]]                   # max(keys[0..k))
        after = np.minimum.accumulate(key[::-1])[::-1]                       # min(keys[k..n))
        cut = np.flatnonzero(np.r_[True, before[1:] <= after[1:]])
        m["maxpiece"] = int(np.diff(np.r_[cut, n]).max())
    else:
        m["maxpiece"] = n
    by_row = key[np.argsort(row, kind="stable")]
    m["row_sort_is_full"] = bool(np.all(by_row[1:] >= by_row[:-1]))
    return m


def bits_for(n):
    b = 0
    while n > (1 << b):
        b += 1
    return b


def predict(m, mode):
    """The forms ibh_selftest_triplets reports for a case that measures m: the selectors of SELECTORS, restated."""
    f = dict.fromkeys(INFO, 0)
    n, nnz, nrow, ncol = m["n"], m["nnz"], m["nrow"], m["ncol"]
    built = n == 0
    if n and mode == 1 and nrow > 0 and n <= 8 * nrow:
        f["short_rows"] = TAKEN if m["maxrow_contrib"] <= SRB_MAX else DECLINED
        built = f["short_rows"] == TAKEN
    if not built:
        if mode == 0:
            f["order"] = IN_ORDER if not m["full_dec"] else PIECES if m["maxpiece"] <= CS_BIG else RADIX
        else:
            f["order"] = RADIX if m["full_dec"] else IN_ORDER
            if m["full_dec"] and m["lo_dec"] and bits_for(nrow) > 0:
                f["optimistic"] = HELD if m["row_sort_is_full"] else FAILED
        f["seg"] = WAVE if n >= 8 * nnz else THREAD
        f["rowptr"] = SEARCH if nrow < 65536 else HEADS_FILL
    f["wM"] = NONE if nrow == 0 else WAVE if nnz >= 8 * nrow else THREAD
    if nnz and nnz <= 4 * ncol:
        f["Mw"], f["nlong"] = SLOTS, m["nlong"]
    elif nnz:
        f["Mw"], f["Mw_seg"], f["Mw_ptr"] = SORT, WAVE if nnz >= 8 * ncol else THREAD, SEARCH if ncol < 65536 else HEADS_FILL
    return f


def reference(c):
    """The matrix and its weights by the restatement."""
    M = from_triplets(c.nrow, c.ncol, c.row, c.col, c.val)
    wM, Mw = weights(M)
    return M, wM, Mw


_cases = []


def cases():
    if not _cases:
        _cases.extend(run_length_cases() + order_cases() + optimistic_cases() + short_row_cases() + extent_cases() + weight_row_cases()
                      + weight_col_cases())
        assert len({c.name for c in _cases}) == len(_cases)
    return _cases


def case(name):
    return next(c for c in cases() if c.name == name)


# ---- matrices for the product and the algebra ------------------------------------------------------------------------------------
def random_matrix(rng, nrow, ncol, lengths, values=None):
    """Row r has lengths[r] entries at random columns (ascending); values(n) draws a row's values."""
    rp, ci, v = [0], [], []
    for n in lengths:
        ci += np.sort(rng.choice(ncol, int(n), replace=False)).tolist()
        v += (values(int(n)) if values else rng.uniform(-1., 1., int(n))).tolist()
        rp.append(len(ci))
    assert len(lengths) == nrow
    return matrix(nrow, ncol, rp, ci, v)


def controlled_product(rng, Llen, Rlen, ncol, shared_col=None):
    """L (rows of Llen entries) and R (rows of Rlen entries over ncol columns) whose product terms are drawn values: row r of L
    takes the next Llen[r] rows of R, so every entry of R feeds one (r, c) alone and is set to (the drawn term) / L(r, k); the
    terms as the product rounds them are what draw()'s conditions are asked of.  shared_col: a column every row of R holds."""
    nk = int(sum(Llen))
    assert len(Rlen) == nk
    L = matrix(len(Llen), nk, np.r_[0, np.cumsum(Llen)], np.arange(nk), rng.uniform(0.5, 2., nk) * rng.choice([-1., 1.], nk))
    cols = []
    for n in Rlen:
        c = rng.choice(ncol, int(n), replace=False)
        if shared_col is not None and n and shared_col not in c:
            c[0] = shared_col
        cols.append(np.sort(c))
    Rp = np.r_[0, np.cumsum(Rlen)].astype(np.int64)
    Rc = np.concatenate(cols) if nk else np.zeros(0, np.int64)
    Rv = np.zeros(len(Rc))
    for r in range(len(Llen)):
        ks = np.arange(L["rowptr"][r], L["rowptr"][r + 1])
        for c in range(ncol):
            ent = [(k, int(Rp[k] + np.searchsorted(cols[k], c))) for k in ks if c in cols[k]]      # k ascending: the emission order
            if not ent:
                continue
            l = np.asarray([L["val"][k] for k, _ in ent])
            at = [e for _, e in ent]
            for _ in range(1000):
                Rv[at] = draw(rng, len(ent)) / l
                if is_sensitive(l * Rv[at]):
                    break
            else:
                raise AssertionError("no sensitive terms for (%d, %d)" % (r, c))
    return L, matrix(nk, ncol, Rp, Rc, Rv)


def build_product_cases():
    """name -> (L, R, the emit form: 64 lanes or 1).  long: rows of R with 63, 64, 65 and 129 entries (and none) under the 64-lane
    emit, an (r, c) reached by 65 and more terms (every row of R holds column 0), an empty first and last row of L; edge /
    edge_minus_1: total == 8 * n and one below."""
    out = {}
    rng = np.random.default_rng(808)
    Llen = [0, 80, 1, 2, 66, 0, 3, 0]
    L, R = controlled_product(rng, Llen, [(63, 64, 65, 129, 0, 5)[k % 6] for k in range(sum(Llen))], 130, shared_col=0)
    out["long"] = (L, R, 64)
    Llen = [0, 4, 4, 4, 4, 4, 4, 4, 4, 8]                                    # 40 rows of R with 2 entries: 80 terms == 8 * 10
    out["edge"] = controlled_product(rng, Llen, [2] * 40, 6) + (64,)
    out["edge_minus_1"] = controlled_product(rng, Llen, [2] * 17 + [1] + [2] * 22, 6) + (1,)
    return out


_products = {}


def product_cases():        # (built once: the values are drawn until they are sensitive)
    if not _products:
        _products.update(build_product_cases())
    return _products


def product_total(L, R):
    return int(sum(int(R["rowptr"][k + 1] - R["rowptr"][k]) for k in L["colind"].tolist()))


def algebra_matrix(rng=None):
    """A 12 x 150 matrix with rows of 0, 1, 63, 64, 65 and 129 entries (twice), empty rows and empty columns (70 to 74 and the
    last five)."""
    rng = rng or np.random.default_rng(909)
    M = random_matrix(rng, 12, 140, [0, 1, 63, 64, 65, 129, 0, 129, 65, 64, 63, 1])
    return matrix(12, 150, M["rowptr"], M["colind"] + 5 * (M["colind"] >= 70), M["val"])


def short_matrix(rng=None):
    """A 30 x 40 matrix with rows of 1 to 12 entries and some of none (crop_cols: a thread per row, insertion into place)."""
    rng = rng or np.random.default_rng(910)
    return random_matrix(rng, 30, 40, [(r % 13) for r in range(30)])


def wide_matrix(rng=None):
    """3 x 70 000, for the transpose (70 000 rows, the heads + fill row pointer)."""
    rng = rng or np.random.default_rng(911)
    return random_matrix(rng, 3, 70000, [2000, 0, 1500])


# ---- kernel -> the test that runs it (tests/test_capi_symbols.py checks both tables against the code objects: every kernel of
# csrops.o is a key of CSROPS_KERNELS, every kernel of csrbuild.o a key of LAYER_KERNELS, and the other way round) ------------------
G = "test_gpu_csr_build.py::"
# E1vE0 and I2vX against the oracle, bit for bit (E1vE0's two-sheet, own-X-dims cases reach k_csr_to_contrib and k_scatter_rowmap)
E1VE0 = "test_gpu_parity.py::test_e1ve0_bit_exact_against_oracle"
I2VX = "test_gpu_global_ec.py::test_make_I2vX_bitwise"
CSROPS_KERNELS = {
    "k_prod_count": G + "test_product", "k_prod_emit<64>": G + "test_product", "k_prod_emit<1>": G + "test_product",
    "k_crop_rows_count": G + "test_crop_rows", "k_crop_rows_fill": G + "test_crop_rows",
    "k_crop_cols_count": G + "test_crop_cols", "k_crop_cols_fill": G + "test_crop_cols",
    "k_recip": G + "test_vector_ops", "k_mul": G + "test_vector_ops", "k_gather": G + "test_vector_ops",
    "k_scale_rows": G + "test_scalings", "k_scale_cols": G + "test_scalings", "k_scale_rows_recip": G + "test_scale_rows_recip_skips_empty_rows",
    "k_expand_rows": G + "test_transpose_and_expand_rows",
    "k_e1ve0<0>": E1VE0, "k_e1ve0<1>": E1VE0, "k_scatter_rowmap": E1VE0, "k_add_by_sparse": E1VE0, "k_csr_to_contrib": E1VE0,
    "k_fill_f64": E1VE0,
    "k_i2vx_count": I2VX, "k_i2vx_terms": I2VX, "k_i2vx_wM": I2VX,
}
LAYER_KERNELS = {
    "k_head_flags": G + "test_run_lengths", "k_segment_heads": G + "test_run_lengths",
    "k_rowptr_heads": G + "test_extents", "k_rowptr_fill": G + "test_extents", "k_rowptr_search": G + "test_extents",
    "k_seg_sums_thread<false>": G + "test_run_lengths", "k_seg_sums_wave<false>": G + "test_run_lengths",
    "k_seg_sums_thread<true>": G + "test_weights", "k_seg_sums_wave<true>": G + "test_weights",
    "k_col_keys": G + "test_weights", "k_col_count": G + "test_weights", "k_col_scatter": G + "test_weights",
    "k_col_sums": G + "test_weights", "k_col_sums_long": G + "test_weights", "k_keys_to_i32": G + "test_weights",
    "k_srb_count": G + "test_short_rows", "k_srb_scatter": G + "test_short_rows", "k_srb_unique": G + "test_short_rows",
    "k_srb_emit": G + "test_short_rows", "k_coo_keys": G + "test_run_lengths",
}
