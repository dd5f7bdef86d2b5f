"""Plain-loop numpy restatement of the chunked half of modele/global_ec.cpp (main(), :752-893) and of combine_chunks
(modele/combine_global_ec.cpp:94-262): the oracle of tests/test_gpu_global_ec_chunks.py, checked on its own by
tests/test_global_ec_chunks_restatement.py.  Loops in the reference's order, one statement per reference statement; nothing
here is vectorised, so that the order of every sum is the one written down."""
import math

import numpy as np


def nesting(imO, jmO, imI, jmI):
    """:752-760."""
    mult_i, mult_j = imI // imO, jmI // jmO
    if mult_i * imO != imI or mult_j * jmO != jmI:
        raise ValueError("Hntr grid (%dx%d) must be an even multiple of (%dx%d)" % (imI, jmI, imO, jmO))
    return mult_i, mult_j


def elev_range(fgiceI, elevI):
    """:805-813: int16 min / max of elevI over fgiceI != 0, from {10000, -10000}."""
    lo, hi = 10000, -10000
    jm, im = fgiceI.shape
    for j in range(jm):
        for i in range(im):
            if fgiceI[j, i]:
                lo = min(lo, int(elevI[j, i]))
                hi = max(hi, int(elevI[j, i]))
    return lo, hi


def ec_range(rng, ec_skip):
    """:815-816."""
    return ec_skip * math.floor(float(rng[0]) / ec_skip), ec_skip * math.ceil(float(rng[1]) / ec_skip)


def tile_counts(fgiceI, imO, jmO):
    """The inner count of :881-884 for every O cell, whatever fgiceO is."""
    mult_i, mult_j = nesting(imO, jmO, fgiceI.shape[1], fgiceI.shape[0])
    nice = np.zeros((jmO, imO), np.int32)
    for jO in range(jmO):
        for iO in range(imO):
            n = 0
            for jI in range(jO * mult_j, (jO + 1) * mult_j):
                for iI in range(iO * mult_i, (iO + 1) * mult_i):
                    if fgiceI[jI, iI]:
                        n += 1
            nice[jO, iO] = n
    return nice


def chunk_plan_counts(c, imO, jmO, chunk_size):
    """:863-893 with the tile count of each O cell with fgiceO != 0 given as c[jO, iO] (0 elsewhere): a cell with c == 0 adds
    nothing and cannot make `nice >= chunk_size` newly true, so skipping it is what `if (fgiceO(jO, iO) != 0)` does."""
    c = np.asarray(c).reshape(jmO, imO)
    chunks = []
    iO = jO = 0
    chunkno = 0
    while jO < jmO and iO < imO:
        nice = 0
        jO0, iO0 = jO, iO
        done = False
        while jO < jmO:
            while iO < imO:
                if c[jO, iO] != 0:
                    nice += int(c[jO, iO])
                    if nice >= chunk_size:
                        done = True         # goto endscan2: iO is not advanced
                        break
                iO += 1
            if done:
                break
            iO = 0
            jO += 1
        chunks.append(((chunkno, jO0, iO0, jO, iO), nice))
        chunkno += 1
    return chunks


def chunk_plan(fgiceI, fgiceO, chunk_size):
    """:863-893 as written: the tile is counted only where fgiceO != 0."""
    jmO, imO = fgiceO.shape
    nice = tile_counts(fgiceI, imO, jmO)
    c = np.zeros((jmO, imO), np.int64)
    for jO in range(jmO):
        for iO in range(imO):
            if fgiceO[jO, iO] != 0:
                c[jO, iO] = nice[jO, iO]
    return chunk_plan_counts(c, imO, jmO, chunk_size)


def chunk_mask(fgiceI, elevI, fgiceO, chunk):
    """:818-855: elevmaskI of the chunk (chunkno, jO0, iO0, jO1, iO1)."""
    jmO, imO = fgiceO.shape
    mult_i, mult_j = nesting(imO, jmO, fgiceI.shape[1], fgiceI.shape[0])
    em = np.full(fgiceI.shape, np.nan)
    _, jO, iO, jO1, iO1 = chunk
    ijO1 = jO1 * imO + iO1
    ijO = jO * imO + iO
    while True:
        ended = False
        while iO < imO:
            if ijO >= ijO1:
                ended = True
                break
            if fgiceO[jO, iO] != 0:
                for jI in range(jO * mult_j, (jO + 1) * mult_j):
                    for iI in range(iO * mult_i, (iO + 1) * mult_i):
                        if fgiceI[jI, iI]:
                            em[jI, iI] = float(elevI[jI, iI])
            iO += 1
            ijO += 1
        if ended or ijO >= ijO1:
            break
        iO = 0
        jO += 1
    return em


def combine(chunks, scale):
    """combine_chunks (:145-249).  chunks: dicts with dimB, dimA (int64), wM, Mw, row, col (dense, stored row-major order), val
    and extents (extB, extA).  Returns dict(iB, iA, val: the stream of M.add calls; dimB, dimA: the keys of the weight
    accumulators first-seen; wM, Mw: their sums; sM_s)."""
    extB = chunks[0]["extents"][0]
    sM_s = np.zeros(extB)
    for ch in chunks:                                   # :156-171
        for i in range(len(ch["wM"])):
            sM_s[ch["dimB"][i]] += ch["wM"][i]
    with np.errstate(divide="ignore"):
        for i in range(extB):                           # :174
            sM_s[i] = 1. / sM_s[i]
    wM, Mw = {}, {}                                     # accumulators: key -> sum, in first-seen order (python dicts keep it)
    iB, iA, val = [], [], []
    for ch in chunks:
        for i in range(len(ch["wM"])):                  # :199-200
            k = int(ch["dimB"][i])
            wM[k] = wM.get(k, 0.0) + ch["wM"][i]
        for e in range(len(ch["val"])):                 # :219-227
            b, a = int(ch["dimB"][ch["row"][e]]), int(ch["dimA"][ch["col"][e]])
            iB.append(b)
            iA.append(a)
            val.append(ch["val"][e] * sM_s[b] if scale else ch["val"][e])
        for i in range(len(ch["Mw"])):                  # :249
            k = int(ch["dimA"][i])
            Mw[k] = Mw.get(k, 0.0) + ch["Mw"][i]
    return dict(iB=np.asarray(iB, np.int64), iA=np.asarray(iA, np.int64), val=np.asarray(val, np.float64),
                dimB=np.asarray(list(wM), np.int64), dimA=np.asarray(list(Mw), np.int64),
                wM=np.asarray(list(wM.values()), np.float64), Mw=np.asarray(list(Mw.values()), np.float64), sM_s=sM_s)


def set_from_triplets(dimB, dimA, iB, iA, val):
    """Eigen's setFromTriplets of the stream over the dense ids of {dimB, dimA}: (row, col, val) sorted by (row, col), the
    duplicates summed in stream order with the first assigned."""
    dB = {int(k): d for d, k in enumerate(dimB)}
    dA = {int(k): d for d, k in enumerate(dimA)}
    acc = {}
    for e in range(len(val)):
        key = (dB[int(iB[e])], dA[int(iA[e])])
        acc[key] = acc[key] + val[e] if key in acc else val[e]
    keys = sorted(acc)
    return (np.asarray([k[0] for k in keys], np.int32), np.asarray([k[1] for k in keys], np.int32),
            np.asarray([acc[k] for k in keys], np.float64))
