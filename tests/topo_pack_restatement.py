"""The end of GCMCoupler_ModelE::update_topo and couple()'s unit conversion restated in plain Python, loop for loop: the
packing of the TOPOA planes into gcm_ivalss_s[ATOPO] / [ETOPO] (modele/GCMCoupler_ModelE.cpp:1118-1129, :1151-1163), the
mergemaskA0 rule (:1017, :1167), underice_d (:1090-1097) and val = val * mm + bb (:1216-1228).  Plain lists and scalars, no
vectorisation; planes are flat lists in (j, i) / (ihc, j, i) order.  Pinned by hand in tests/test_topo_pack_restatement.py."""


class VectorMultivec:
    """slib/icebin/multivec.hpp:25-31 with add() of multivec.cpp:8-13"""

    def __init__(self, nvar):
        self.nvar = nvar
        self.index, self.weights, self.vals = [], [], []

    def add(self, ix, val, weight):
        self.index.append(ix)
        for ivar in range(self.nvar):
            self.vals.append(val[ivar])
        self.weights.append(weight)

    def size(self):
        return len(self.index)


def pack_A(gcm_ivalsA_s, iarrays, mergemaskA, mergemaskA0, im, jm, indexingA):
    """:1118-1129.  iarrays: the contract's variables in order, each [jm * im]; indexingA(i, j) -> index."""
    val = [0.] * gcm_ivalsA_s.nvar
    for j in range(jm):
        for i in range(im):
            if mergemaskA[j * im + i] == 0 and mergemaskA0[j * im + i] == 0:
                continue
            for k in range(gcm_ivalsA_s.nvar):
                val[k] = iarrays[k][j * im + i]
            ij = indexingA(i, j)
            gcm_ivalsA_s.add(ij, val, 1.0)


def pack_E(gcm_ivalsE_s, iarrays, nhc, mergemaskA, mergemaskA0, im, jm, indexingE):
    """:1151-1163.  iarrays: each [>= nhc * jm * im]; indexingE(i, j, ihc) -> index."""
    val = [0.] * gcm_ivalsE_s.nvar
    for ihc in range(nhc):
        for j in range(jm):
            for i in range(im):
                if mergemaskA[j * im + i] == 0 and mergemaskA0[j * im + i] == 0:
                    continue
                for k in range(gcm_ivalsE_s.nvar):
                    val[k] = iarrays[k][(ihc * jm + j) * im + i]
                ij = indexingE(i, j, ihc)
                gcm_ivalsE_s.add(ij, val, 1.0)


def convert_units(gcm_ivals_s, mm, bb):
    """:1221-1227, one output vector"""
    nvar = gcm_ivals_s.nvar
    for ix in range(gcm_ivals_s.size()):
        for ivar in range(nvar):
            val = gcm_ivals_s.vals[ix * nvar + ivar]
            gcm_ivals_s.vals[ix * nvar + ivar] = val * mm[ivar] + bb[ivar]


def underice_d(underice_i):
    """:1090-1097: the int16 array assigned to a double one"""
    return [float(int(u)) for u in underice_i]


class Coupler:
    """The state update_topo keeps from one call to the next: mergemaskA0."""

    def __init__(self):
        self.mergemaskA0 = None

    def pack(self, run_ice, mergemaskA, arraysA, arraysE, nhc, im, jm, indexingA, indexingE, unitsA=None, unitsE=None):
        """arraysA: the ATOPO contract's planes; arraysE: the ETOPO contract's (underice_d already a double plane); units = (mm,
        bb) or None: no conversion -> (gcm_ivalsA_s, gcm_ivalsE_s)."""
        if not run_ice:
            self.mergemaskA0 = mergemaskA           # :1017: no mergemask on initialisation
        A, E = VectorMultivec(len(arraysA)), VectorMultivec(len(arraysE))
        pack_A(A, arraysA, mergemaskA, self.mergemaskA0, im, jm, indexingA)
        pack_E(E, arraysE, nhc, mergemaskA, self.mergemaskA0, im, jm, indexingE)
        self.mergemaskA0 = mergemaskA               # :1167
        if unitsA is not None:
            convert_units(A, *unitsA)
        if unitsE is not None:
            convert_units(E, *unitsE)
        return A, E
