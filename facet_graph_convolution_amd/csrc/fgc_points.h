// What the two sampled losses share (fgc_points.hip: fgc_point_loss; fgc_surface.hip: fgc_surface_loss): ONE copy of the
// sample gather and of the single-workgroup launch that sums the loss and reduces the terms that share a row.
#pragma once
#include "fgc_common.h"

namespace fgc {

// q[i] = p[ind[i]], a NaN row for an index outside [0, np)
void point_gather(const float* p, int np, const int* ind, int n, float* q, hipStream_t st);

// rows [nt0 + nt1], terms [nt0 + nt1] = (gradient on the row, value): loss[0] = 1000 (sum of the first nt0 values / n0 + sum of
// the other nt1 values / n1); g (may be NULL, zero on entry) [.,3]: every row >= 0 gets the sum of its terms in term order.
void point_loss_finish(const int* rows, const float4* terms, int nt0, int nt1, int n0, int n1, float* loss, float* g,
                       hipStream_t st);

}  // namespace fgc
