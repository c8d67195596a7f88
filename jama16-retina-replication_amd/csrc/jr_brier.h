// jr_brier.h — the Brier sum's arithmetic, one device function shared by
// jr_brier_accumulate (jr_misc.hip) and jr_metrics_accumulate
// (jr_metrics.hip): the two agree bit for bit.  The order is stated in jr.h.
#pragma once
#include "jr_common.h"

namespace jr {

// One block of 256 threads.  p and y widen to fp64 (exact); d = p - y, d * d
// and the running sum are one fp64 operation each (no FMA, whatever the
// file's contraction mode); thread t adds elements t, t + 256, ... in
// ascending order; block_sum256 then folds the 256 partials as a tree.
__device__ __forceinline__ double brier_sum256(const float* __restrict__ p, const float* __restrict__ y, int n,
                                               double* red) {
#pragma clang fp contract(off)
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double d = (double)p[i] - (double)y[i];
    const double q = d * d;
    s = s + q;
  }
  return block_sum256(s, red);
}

// Thread 0 of that block: acc[0] += sum, acc[1] += n.
__device__ __forceinline__ void brier_add(double* acc, double sum, int n) {
  acc[0] += sum;
  acc[1] += (double)n;
}

}  // namespace jr
