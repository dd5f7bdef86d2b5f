// smooth.h -- entry points of the smoother (smooth.hip): M <- smoothI * M for a finished CSR.
#pragma once
#include "common.h"

namespace ibh {
// what a smoothed build needs of its arguments (the ice grid's centroids, three positive sigmas), for a caller that wants the
// failure before it has built anything; smooth_matrix checks the same
void smooth_check(const ibh_regrid_matrices *rm, const double sigma[3]);
// row_s: the sparse index of every row of w (device).
// comm (world > 1): every rank of the communicator calls this with the same matrix; the tile form is shared (w->built_fast = 3),
// the direct form and the triplet pipeline run on every rank.  The result is the same bits on every rank and for every world.
void smooth_matrix(ibh_weighted *w, const ibh_regrid_matrices *rm, const int64_t *row_s, const double sigma[3], hipStream_t st,
                   ibh_comm *comm = nullptr);
}  // namespace ibh
