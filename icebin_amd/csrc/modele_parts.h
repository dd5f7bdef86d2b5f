// modele_parts.h -- the topo.cpp helpers (slib/icebin/modele/topo.cpp:50-240) that both ModelE matrix makers compose: the
// per-sheet matrices of modele.hip (GCMRegridder_ModelE::regrid_matrices) and the global AvE of globalave.hip
// (_compute_AAmvEAm_EIGEN).  Defined in modele.hip.  Each takes what it works on as arguments: the weights and the sets of
// a given EOpvAOp, the elevation-class count and the two indexingHC.  Where the work lives is DESIGN.md 15:
// the keys of the GCM-grid-sized sets on the host, every matrix entry and weight on the device.
#pragma once
#include <memory>
#include <vector>

#include "common.h"

namespace ibh {

// Hntr's overlap triplets (B cell, A cell, area) of the B cells in includeB, on the host: count, then fetch
struct HostTriplets { std::vector<int32_t> iB, iA; std::vector<double> v; };
HostTriplets hntr_overlap_triplets(const ibh_hntr *h, double eq_rad, const uint8_t *includeB);

// compute_wAOm (topo.cpp:84-109) with scaled_AOmvAOp (topo.cpp:50-81).  d_wAOp: device, dense over dimAOp, whose keys index
// the two ocean fractions [nO] (the caller has checked that they lie in [0, nO)).  dimAOm becomes the cells of dimAOp, in
// dense order, that ModelE calls land; aop2aom the dense AOp -> dense AOm map (-1: ocean for ModelE).  IBH_EINVAL for an
// fcont_m that is neither 0 nor 1.  Synchronises st: d_wAOp may go away when it returns.
void compute_wAOm(const double *foceanAOp, const double *foceanAOm, int64_t nO, const double *d_wAOp, const ibh_sparse_set &dimAOp,
                  ibh_sparse_set &dimAOm, std::vector<int32_t> &aop2aom, DevBuf<double> &wAOm, hipStream_t st);

// compute_EOmvAOm_unscaled (topo.cpp:211-240) on a given EOpvAOp over {dimEOp, dimAOp}: visited by columns, rows ascending
// inside; kept where the column is a cell of dimAOm; dimEOm (sparse extent extentEOm) numbered first-seen.  Then
// EOmvAOms = sum(EOmvAOm, 1, '-') and wEOm = EOmvAOm * diag(EOmvAOms) * wAOm (:226-228), on the device and, for raw_EOvEA's
// "weight != 0" test, on the host.  EOmvAOm / EOmvAOms: where to leave the matrix and its inverted column sums (null: a
// caller that wants the weights alone).  Synchronises st.
void compute_EOmvAOm_unscaled(const ibh_weighted &EOpvAOp, const ibh_sparse_set &dimEOp, const ibh_sparse_set &dimAOp,
                              const ibh_sparse_set &dimAOm, const DevBuf<double> &wAOm, int64_t extentEOm, ibh_sparse_set &dimEOm,
                              ibh_weighted *EOmvAOm, DevBuf<double> *EOmvAOms, DevBuf<double> &wEOm, std::vector<double> &wEOm_h,
                              hipStream_t st);

// raw_EOvEA (topo.cpp:112-204), by its columns: Hntr's O -> A overlap clipped by includeO (DimClip(dimAOm)), every entry
// expanded over nhc elevation classes through indexingHCO / indexingHCA; numbers dimEAm.  IBH_EINVAL for an
// overlap below 1e-8 in magnitude.  Synchronises st.
std::unique_ptr<ibh_weighted> raw_EOvEA(const ibh_hntr *hntr, double eq_rad, const std::vector<uint8_t> &includeO,
                                        const ibh_sparse_set &dimEOm, const DevBuf<double> &wEOm, const std::vector<double> &wEOm_h,
                                        int32_t nhc, HcIndexing hcO, HcIndexing hcA, ibh_sparse_set &dimEAm, hipStream_t st);

// y = (M * diag(d)) * w: y[r] = sum over the row's columns k ascending, from 0, of (M(r, k) * d[k]) * w[k]
void scaled_matvec(const ibh_weighted &M, const double *d, const double *w, double *y, hipStream_t st);

}  // namespace ibh
