"""Numpy restatements for the global_ec tests: the masked overlap exchange grid (ExchAccum, global_ec.cpp:296-322) and
make_I2vX's products (global_ec.cpp:345-376) in Eigen's order."""
import numpy as np


def exgrid_ref(iB, iA, val, elevmaskI):
    """Stream-order overlap entries (WEIGHT over every term) filtered by the ice mask: indices [nX, 2], overlaps, dimA
    (ascending GCM cells with a kept entry), dimI (ice cells first-seen)."""
    keep = ~np.isnan(np.asarray(elevmaskI, np.float64)[iA])
    b, a, v = iB[keep], iA[keep], val[keep]
    dimA = np.unique(b)
    _, first = np.unique(a, return_index=True)
    dimI = a[np.sort(first)]
    return np.stack([b, a], axis=1).astype(np.int32), v, dimA.astype(np.int64), dimI.astype(np.int64)


def i2vx_ref(trip, dimI, dimI2_in, IvX_rows, IvX_cols, IvX_vals, IvX_wM, IvX_Mw, nX):
    """trip: (iI, iI2, v) of Hntr(hspecI as B, hspecI2 as A).overlap under ElevMaskClip, stream order.  dimI dense ids:
    TO_DENSE_IGNORE_MISSING; dimI2: ADD_DENSE first-seen onto dimI2_in.  Returns (row, col, val sorted by (row, col), wM, Mw,
    dimI2)."""
    tI = {int(s): d for d, s in enumerate(dimI)}
    d2 = list(int(x) for x in dimI2_in)
    t2 = {s: d for d, s in enumerate(d2)}
    cols = {}                                 # dense I -> {dense I2: value}, duplicates summed in stream order
    for i, i2, v in zip(*trip):
        di = tI.get(int(i))
        if di is None:
            continue
        if int(i2) not in t2:
            t2[int(i2)] = len(d2)
            d2.append(int(i2))
        c = cols.setdefault(di, {})
        k = t2[int(i2)]
        c[k] = c[k] + v if k in c else v
    nI2 = len(d2)
    rows_of = {}
    for r, c, v in zip(IvX_rows, IvX_cols, IvX_vals):
        rows_of.setdefault(int(r), []).append((int(c), float(v)))
    M, wM = {}, {}
    for di in sorted(cols):
        col = sorted(cols[di].items())
        cs = 0.
        for _, v in col:
            cs = cs + v
        sI = 1. / cs
        sX = 1. / IvX_wM[di]
        for i2, v in col:
            t = (v * sI) * IvX_wM[di]
            wM[i2] = wM[i2] + t if i2 in wM else t
            L = v * sX
            for x, m in rows_of.get(di, []):
                k = (i2, x)
                M[k] = M[k] + L * m if k in M else L * m
    keys = sorted(M)
    row = np.asarray([k[0] for k in keys], np.int32)
    col = np.asarray([k[1] for k in keys], np.int32)
    val = np.asarray([M[k] for k in keys], np.float64)
    wMo = np.asarray([wM.get(i, 0.) for i in range(nI2)], np.float64)
    return row, col, val, wMo, np.asarray(IvX_Mw, np.float64).copy(), np.asarray(d2, np.int64)
