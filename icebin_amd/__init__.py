"""icebin_amd: MI355X-native implementation of IceBin's conservative-regridding hot path.

Python surface mirrors pylib/_icebin.pyx (GCMRegridder, RegridMatrices, HntrSpec, Hntr) and
ibmisc.linear_Weighted; all compute goes through libicebin_hip.so (include/icebin_hip.h).
"""
from ._capi import IcebinHipError, device_count  # noqa: F401
from .linear import SparseSet, compute_E1vE0c, coo_multiply, linear_Weighted, nc_read_weighted, set_tuning  # noqa: F401
from .regrid import GCMRegridder, RegridMatrices, from_synthetic  # noqa: F401
from .hntr import Hntr, HntrSpec  # noqa: F401
from .etopo1 import etopo1_ice  # noqa: F401
from .topoo import make_topoO  # noqa: F401
from .multivec import VectorMultivec, append_planes_many, concatenate  # noqa: F401
from .modele import (EOpvAOpResult, GCMRegridder_ModelE, RegridMatrices_ModelE, TopoPacker, UI_GLOBALICE, UI_LOCALICE,  # noqa: F401
                     compute_AAmvEAm, compute_EOpvAOp_merged, make_hntrA, make_topoA, merge_topoO)
