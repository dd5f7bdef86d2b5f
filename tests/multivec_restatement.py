"""The loops around icebin::VectorMultivec, restated as plain sequential Python over numpy float64 scalars: one product, then
one add, in entry order.  What the device code must reproduce bit for bit.

  add / concatenate       multivec.cpp:8-33
  append_weighted         IceCoupler.cpp:447-458 (one entry per dense row, field-major product -> entry-major vals)
  to_dense_scale          multivec.cpp:35-50
  to_dense                multivec.cpp:55-81 (with its NaN rule)
  update_dense            modele/GCMCoupler_ModelE.cpp:864-892 (without ModelE's index arithmetic)
  add_dense / densify     IceCoupler.cpp:294-314
"""
import numpy as np


class Multivec:
    def __init__(self, nvar):
        if nvar < 1:
            raise ValueError("nvar=%d" % nvar)
        self.nvar = nvar
        self.index, self.weights, self.vals = [], [], []

    def size(self):
        return len(self.index)

    def add(self, ix, val, weight):
        assert len(val) == self.nvar
        self.index.append(int(ix))
        self.weights.append(np.float64(weight))
        for v in val:
            self.vals.append(np.float64(v))

    def val(self, ivar, ix):
        return self.vals[ix * self.nvar + ivar]

    def arrays(self):
        return (np.array(self.index, np.int64), np.array(self.weights, np.float64),
                np.array(self.vals, np.float64).reshape(len(self.index), self.nvar))


def concatenate(vecs):
    if len(vecs) == 0:
        raise ValueError("Must concatenate at least one vector")
    ret = Multivec(vecs[0].nvar)
    for v in vecs:
        if v.nvar != ret.nvar:
            raise ValueError("Inconsistant nvar: %d vs %d" % (ret.nvar, v.nvar))
        ret.index += v.index
        ret.weights += v.weights
        ret.vals += v.vals
    return ret


def append_weighted(mv, to_sparse, wM, B):
    """B[nvar, nrow]: the field-major product; every dense row becomes an entry, rows ascending."""
    B = np.asarray(B, np.float64)
    if B.shape[0] != mv.nvar:
        raise ValueError("Inconsistant nvar: %d vs %d" % (mv.nvar, B.shape[0]))
    for jj in range(B.shape[1]):
        mv.add(to_sparse[jj], [B[nn, jj] for nn in range(mv.nvar)], wM[jj])


def _check(iE, nE, i):
    if iE < 0 or iE >= nE:
        raise IndexError("entry %d: Index out of range: %d vs. %d" % (i, iE, nE))


def to_dense_scale(mv, nE):
    scale = np.zeros(nE, np.float64)
    for i in range(mv.size()):
        iE = mv.index[i]
        _check(iE, nE, i)
        scale[iE] = scale[iE] + mv.weights[i]
    with np.errstate(divide="ignore"):
        return np.float64(1.0) / scale          # every element on its own: no order to keep


def to_dense(mv, scale, fill):
    """[nvar, nE]; untouched = NaN, a NaN running value is REPLACED by the next term, a final NaN becomes fill."""
    nE = len(scale)
    out = np.full((mv.nvar, nE), np.nan, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for ivar in range(mv.nvar):
            for i in range(mv.size()):
                iE = mv.index[i]
                _check(iE, nE, i)
                p = mv.val(ivar, i) * scale[iE]
                if np.isnan(out[ivar, iE]):
                    out[ivar, iE] = p
                else:
                    out[ivar, iE] = out[ivar, iE] + p
    out[np.isnan(out)] = fill                   # every element on its own
    return out


def update_dense(mv, scale, out):
    """In place on out[nvar, nE]: named cells are cleared to 0.0, then += val * scale in entry order."""
    nE = len(scale)
    for i in range(mv.size()):
        _check(mv.index[i], nE, i)
    for i in range(mv.size()):
        for ivar in range(mv.nvar):
            out[ivar, mv.index[i]] = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(mv.size()):
            iE = mv.index[i]
            for ivar in range(mv.nvar):
                out[ivar, iE] = out[ivar, iE] + mv.val(ivar, i) * scale[iE]
    return out


def add_dense(to_sparse, mv):
    """The set (a list, dense -> sparse) after add_dense of every index in entry order: first-seen numbering."""
    table = [int(k) for k in to_sparse]
    inv = {k: d for d, k in enumerate(table)}
    for i in range(mv.size()):
        k = mv.index[i]
        if k not in inv:
            inv[k] = len(table)
            table.append(k)
    return table


def densify(mv, to_sparse):
    """[nvar, dense_extent]: zero, then += the values at to_dense(index), entry order; weights unused."""
    inv = {int(k): d for d, k in enumerate(to_sparse)}
    out = np.zeros((mv.nvar, len(to_sparse)), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(mv.size()):
            if mv.index[i] not in inv:
                raise KeyError("entry %d: index %d is not in the SparseSet" % (i, mv.index[i]))
            d = inv[mv.index[i]]
            for ivar in range(mv.nvar):
                out[ivar, d] = out[ivar, d] + mv.val(ivar, i)
    return out
