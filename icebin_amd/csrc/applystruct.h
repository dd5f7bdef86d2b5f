// applystruct.h -- the builders of a matrix's apply structures (applystruct.hip; the types: common.h, the decision which one an
// apply wants: apply_plan.h).
#pragma once
#include "common.h"

namespace ibh {
// The apply structures of a matrix from its CSR; an unbuilt value: the matrix is not eligible or the structure not
// representable.  The handle is only read: the caller keeps what it gets.
Bands build_bands_from_csr(const ibh_weighted *w, hipStream_t st);      // (same result as building them with the matrix)
Sweep build_sweep_from_csr(const ibh_weighted *w, hipStream_t st);
RowGroups build_groups_from_csr(const ibh_weighted *w, hipStream_t st); // (with their tiles, where those fit)
// The bands at build time, from what the assembly already has: hc: how the row keys row_s decode into (GCM cell, class); row: the row
// of every entry; colptr/lrow/lidx: the per-column slots built for the column sums (csrbuild.h ColSlots).  Enqueued on st, arena.
// *d_total receives the number of band entries: the caller reads it back into Bands::n.
Bands build_bands(const ibh_weighted *w, HcIndexing hc, const int64_t *row_s, const int32_t *row, const uint32_t *colptr,
                  const int32_t *lrow, const uint32_t *lidx, uint32_t *d_total, hipStream_t st);
}  // namespace ibh
