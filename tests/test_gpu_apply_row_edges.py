"""The row kernels' tail batch at every slot edge, one apply per launch and batched.

A row's tail batch issues only the 64-entry slots that hold entries of it (spmm.hip tail_slots / with_slot_count), each slot
count through a body of its own.  That may not change a bit of a result.  The matrices have rows on every slot edge (n = 0, 1,
63..65, 127..129, 831..833), on the 14 * 64 batch edge (895..897: a full batch plus a tail), on the staged segment's edge (1023,
1024) and two rows of two segments (1025, 1921).

Expected values are computed on the host in the kernels' own order: entry e of a row goes to wave (e / 64) % WK, lane e % 64, in
the order of e with one fma each; a wave's 64 lanes are summed as a binary tree of neighbours (wave_sum); the WK waves in order.
Values and inputs carry 26 significant bits, so every product is exact in double and fma(v, x, acc) is the double sum v * x + acc
rounded once -- plain numpy arithmetic -- while the sums still round, so the order is pinned.  Results are compared as bit
patterns, and against the exact row-by-row reference of tests/test_gpu_apply_kernels.py."""
import os
import sys

import numpy as np
import pytest

from icebin_amd.linear import linear_Weighted

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_apply_kernels import Reference  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = -7.25
SENTINEL = 1234.5e-3
NQ, NF = 32, 64
LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129, 831, 832, 833, 895, 896, 897, 1023, 1024]
LENGTHS2 = [1025, 1921]

INSTS = {
    "spmm_rowblock_kernel<1, 1, 14, 8, false>": dict(wk=1, options=dict(rowblock_fpw=1, rowblock_many_fpw=1, rowblock_wk=1, rowblock_waves=8,
                                                                        rowblock_unroll=14, rowone=0)),
    "spmm_rowblock_kernel<1, 1, 8, 8, false>": dict(wk=1, options=dict(rowblock_fpw=1, rowblock_many_fpw=1, rowblock_wk=1, rowblock_waves=8,
                                                                       rowblock_unroll=8, rowone=0)),
    "spmm_rowblock_kernel<4, 2, 4, 4, false>": dict(wk=2, options=dict(rowblock_fpw=4, rowblock_many_fpw=4, rowblock_wk=2, rowblock_waves=4,
                                                                       rowblock_unroll=4, rowone=0)),
    "spmm_rowone_kernel<8, 14>": dict(wk=1, options=dict(rowone=1, rowone_waves=8, rowone_unroll=14, rowblock_fpw=1, rowblock_wk=1)),
}


def bits26(rng, shape):
    """+-[1, 2) with 26 significant bits: the product of two is exact in double"""
    return rng.integers(1 << 25, 1 << 26, shape).astype(np.float64) * 2.0 ** -25 * rng.choice([-1.0, 1.0], shape)


class Matrix:
    """rows of the given lengths: random columns with repeats between rows, the last entry of every row in a column of its own
    (ncol - 1 - nrow + i), column ncol - 1 in no row; values of 26 bits times a power of two per row"""

    def __init__(self, lengths, ncol, seed):
        rng = np.random.default_rng(seed)
        self.nrow, self.ncol = len(lengths), ncol
        shared = ncol - 1 - self.nrow
        cols = []
        for i, n in enumerate(lengths):
            c = rng.permutation(shared)[:n]
            if n:
                c[-1] = shared + i
            cols.append(c)
        self.rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
        self.colind = np.concatenate(cols).astype(np.int32)
        self.val = bits26(rng, len(self.colind)) * np.repeat(2.0 ** rng.integers(-20, 21, self.nrow), lengths)
        self.last_col = [shared + i if n else None for i, n in enumerate(lengths)]
        self.X = bits26(rng, (NQ, NF, ncol))        # a different input per batch
        self._exp = {}

    def weighted(self, name, dead=()):
        wM = np.ones(self.nrow)
        wM[list(dead)] = 0.0
        w = linear_Weighted.from_csr((self.nrow, self.ncol), self.rowptr, self.colind, self.val, wM, np.ones(self.ncol))
        for k, v in INSTS[name]["options"].items():
            w.set_option(k, v)
        w.set_kernel("rowblock")
        rowptr, col, val = w.csr_dense()
        assert np.array_equal(rowptr, self.rowptr) and np.array_equal(col, self.colind) and np.array_equal(val.view(np.uint64), self.val.view(np.uint64))
        return w

    def expected(self, wk, X=None):
        """[NQ, NF, nrow] in the kernels' order (computed once per WK for the matrix's own inputs)"""
        if X is None:
            if wk not in self._exp:
                self._exp[wk] = self.expected(wk, self.X)
                self._exp[wk].setflags(write=False)
            return self._exp[wk]
        nq, nf = X.shape[:2]
        Y = np.zeros((nq, nf, self.nrow))
        XT = np.ascontiguousarray(X.transpose(2, 0, 1))            # [col, q, f]
        step = 64 * wk
        with np.errstate(invalid="ignore"):
            for r in range(self.nrow):
                b, e = self.rowptr[r], self.rowptr[r + 1]
                acc = np.zeros((step, nq, nf))                     # [wave * 64 + lane]
                for k in range(b, e, step):
                    m = min(step, e - k)
                    acc[:m] = self.val[k:k + m, None, None] * XT[self.colind[k:k + m]] + acc[:m]      # exact product: one rounding
                t = acc.reshape(wk, 64, nq, nf)
                while t.shape[1] > 1:                              # wave_sum: neighbours, then neighbouring pairs, ...
                    t = t[:, 0::2] + t[:, 1::2]
                s = t[0, 0]
                for w in range(1, wk):
                    s = s + t[w, 0]
                Y[:, :, r] = s
        return Y


@pytest.fixture(scope="module")
def mats():
    return [Matrix(LENGTHS, 1100, 11), Matrix(LENGTHS2, 2100, 12)]


@pytest.fixture(scope="module")
def dev_inputs(mats):
    import torch
    return [torch.from_numpy(m.X).cuda() for m in mats]


class Outputs:
    """nb result planes [nf, nrow] inside sentinel-filled buffers: leading dimension nrow + 5, one more plane beyond nf"""

    def __init__(self, torch, nb, nf, nrow):
        self.nf, self.nrow, self.ld = nf, nrow, nrow + 5
        self.buf = torch.full((nb, nf + 1, self.ld), SENTINEL, dtype=torch.float64, device="cuda")
        self.views = [self.buf[q, :nf, :nrow] for q in range(nb)]

    def result(self, what):
        b = self.buf.cpu().numpy()
        assert np.all(b[:, self.nf:, :] == SENTINEL) and np.all(b[:, :, self.nrow:] == SENTINEL), "%s: wrote outside its result planes" % what
        y = b[:, :self.nf, :self.nrow]
        assert not np.any(y == SENTINEL), "%s: result elements left unwritten" % what
        return y


def run(torch, w, name, x, nb, nf, nrow, what):
    """nb batches of nf fields through ONE launch (rowone: one launch each, its only form); [nb, nf, nrow]"""
    out = Outputs(torch, nb, nf, nrow)
    xs = [x[q, :nf] for q in range(nb)]
    if name.startswith("spmm_rowone") or nb == 1:
        for q in range(nb):
            w.apply_device(xs[q], out=out.views[q], fill=FILL, force_conservation=False)
            assert w.last_launch() == name, "%s: launched %r" % (what, w.last_launch())
    else:
        w.apply_many_device(xs, outs=out.views, fill=FILL, force_conservation=False)
        assert w.last_launch() == name, "%s: launched %r" % (what, w.last_launch())
    torch.cuda.synchronize()
    return out.result(what)


def same_bits(y, exp, what):
    bad = y.view(np.uint64) != np.ascontiguousarray(exp).view(np.uint64)
    assert not bad.any(), "%s: %d values differ from the kernel-order sums; first (batch, field, row) %s" % (
        what, bad.sum(), np.argwhere(bad)[0].tolist())


@pytest.mark.parametrize("nf", [8, 9, 64])
@pytest.mark.parametrize("name", list(INSTS))
def test_row_edges_bitwise(mats, dev_inputs, name, nf):
    import torch
    for m, x in zip(mats, dev_inputs):
        w = m.weighted(name)
        exp = m.expected(INSTS[name]["wk"])
        for nb in (1, 2, 5, 32):
            what = "%s rows %s nf=%d nbatch=%d" % (name, m.nrow, nf, nb)
            y = run(torch, w, name, x, nb, nf, m.nrow, what)
            same_bits(y, exp[:nb, :nf], what)
        Reference(w).check(y[0], m.X[0, :nf], FILL, name + " against exact rows")


@pytest.mark.parametrize("name", [n for n in INSTS if n.startswith("spmm_rowblock")])
def test_batched_launch_is_bitwise_single_applies(mats, dev_inputs, name):
    """32 batches in one launch (16 batch groups of 2, then 11 groups of 3 with a tail of 2) against 32 separate applies: every
    (row, chunk, batch) is written, with the bits of its own apply, and nothing else is touched."""
    import torch
    for m, x in zip(mats, dev_inputs):
        w = m.weighted(name)
        for nf in (9, 64):
            sep = np.stack([run(torch, w, name, x[q:q + 1], 1, nf, m.nrow, "%s single apply %d" % (name, q))[0] for q in range(NQ)])
            for qi in (None, 3):
                w.set_option("rowblock_many_qi", qi)
                try:
                    what = "%s rows %d nf=%d nbatch=32 qi=%s" % (name, m.nrow, nf, qi)
                    y = run(torch, w, name, x, NQ, nf, m.nrow, what)
                finally:
                    w.set_option("rowblock_many_qi", None)
                assert np.array_equal(y.view(np.uint64), sep.view(np.uint64)), "%s: differs from the separate applies" % what


@pytest.mark.parametrize("name", list(INSTS))
def test_nan_stays_in_its_row(mats, name):
    """NaN in a column no row uses reaches no result; NaN in the column of a row's last entry (a column of that row alone)
    reaches that row and no other."""
    import torch
    m = mats[0]
    w = m.weighted(name)
    nf, nb = 9, 5
    hit = [LENGTHS.index(n) for n in (1, 64, 65, 833, 896, 897, 1024)]
    X = m.X[:nb, :nf].copy()
    X[:, :, m.ncol - 1] = np.nan
    X[:, 0::2, [m.last_col[r] for r in hit]] = np.nan
    y = run(torch, w, name, torch.from_numpy(X).cuda(), nb, nf, m.nrow, name + " NaN")
    want = np.zeros(y.shape, bool)
    want[:, 0::2, hit] = True
    assert np.array_equal(np.isnan(y), want), "%s: NaN at %s" % (name, np.argwhere(np.isnan(y) != want)[:5].tolist())
    ok = ~want
    assert np.array_equal(y[ok].view(np.uint64), m.expected(INSTS[name]["wk"])[:nb, :nf][ok].view(np.uint64))


@pytest.mark.parametrize("name", list(INSTS))
def test_dead_rows_receive_fill(mats, name):
    import torch
    m = mats[0]
    dead = [LENGTHS.index(n) for n in (0, 65, 897)]
    w = m.weighted(name, dead=dead)
    nf, nb = 9, 5
    y = run(torch, w, name, torch.from_numpy(m.X).cuda(), nb, nf, m.nrow, name + " dead rows")
    exp = m.expected(INSTS[name]["wk"])[:nb, :nf].copy()
    exp[:, :, dead] = FILL
    same_bits(y, exp, name + " dead rows")
