// jr_metrics.hip — streaming metrics and the per-step log in device memory:
// confusion counts at thresholds, the Brier sums, a ring of step records.
// All state is the caller's; no call synchronises the host, none uses an
// atomic, and only pointers and element counts are bound into a launch.
//
// Compiled with -ffp-contract=off (Makefile), like jr_misc.hip: the Brier
// arithmetic is jr_brier.h's, bit for bit jr_brier_accumulate's.
#include "jr_brier.h"
#include "jr_common.h"

namespace jr {

constexpr int kChunk = JR_METRICS_CHUNK;

// One thread owns threshold blockIdx.x * 256 + threadIdx.x.  The n samples
// pass through LDS in chunks of kChunk: the block loads a chunk together,
// every thread then walks it (all lanes read one address: a broadcast).  The
// owner adds its four counts by read-add-store, so the grid never shows.
// Block 0 also owns the Brier sums (which bit 1).
__global__ void __launch_bounds__(256) k_metrics(const float* __restrict__ p, const float* __restrict__ y, int n,
                                                 const float* __restrict__ thr, int T, uint32_t* counts,
                                                 double* brier, int which) {
  __shared__ float s_p[kChunk];
  __shared__ uint8_t s_y[kChunk];
  __shared__ double red[256];
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (which & 1) {
    const bool own = t < T;
    const float th = own ? thr[t] : 0.f;
    uint32_t tp = 0, fp = 0, ny = 0;
    for (int64_t base = 0; base < n; base += kChunk) {
      const int len = (int)min((int64_t)kChunk, n - base);
      __syncthreads();   // the previous chunk is read
      for (int i = threadIdx.x; i < len; i += 256) {
        s_p[i] = p[base + i];
        s_y[i] = y[base + i] != 0.f;
      }
      __syncthreads();
      for (int i = 0; i < len; ++i) {
        const uint32_t pos = s_p[i] > th, lab = s_y[i];   // NaN > th is false: negative
        tp += pos & lab;
        fp += pos & (lab ^ 1u);
        ny += lab;
      }
    }
    if (own) {
      counts[t] += tp;
      counts[T + t] += fp;
      counts[2 * T + t] += ny - tp;
      counts[3 * T + t] += ((uint32_t)n - ny) - fp;
    }
  }
  if ((which & 2) && blockIdx.x == 0) {
    __syncthreads();
    const double sum = brier_sum256(p, y, n, red);
    if (threadIdx.x == 0) brier_add(brier, sum, n);
  }
}

__global__ void k_step_log_append(jr_step_rec* ring, uint32_t capacity, uint32_t* cursor,
                                  const float* __restrict__ loss, const jr_opt_step* __restrict__ step) {
  const uint32_t c = *cursor;
  jr_step_rec r;
  r.loss = *loss;
  r.grad_norm = step ? step->grad_norm : 0.f;
  r.scale = step ? step->scale : 0.f;
  r.flags = step ? (1u | (step->skipped ? 2u : 0u)) : 0u;
  ring[c % capacity] = r;
  *cursor = c + 1u;
}

}  // namespace jr

using namespace jr;

JR_API int jr_metrics_accumulate(const float* probs, const float* labels, int32_t n, const float* thr, int32_t T,
                                 uint32_t* counts, double* brier, int32_t which, void* stream) {
  if (which < 1 || which > 3) return fail(JR_ERR_INVALID, "metrics_accumulate: which outside 1..3");
  if (!probs || !labels || n <= 0) return fail(JR_ERR_INVALID, "metrics_accumulate: bad arguments");
  if ((which & 1) && (!thr || !counts)) return fail(JR_ERR_INVALID, "metrics_accumulate: counts need thr and counts");
  if ((which & 2) && (!brier || ((uintptr_t)brier & 7)))
    return fail(JR_ERR_INVALID, "metrics_accumulate: null or misaligned brier");
  if (T < 1 || T > 1024) return fail(JR_ERR_INVALID, "metrics_accumulate: T outside 1..1024");
  const int blocks = (which & 1) ? (T + 255) / 256 : 1;
  hipLaunchKernelGGL(k_metrics, dim3(blocks), dim3(256), 0, as_stream(stream), probs, labels, (int)n, thr, (int)T,
                     counts, brier, (int)which);
  return check_launch("metrics_accumulate");
}

JR_API int jr_metrics_reset(uint32_t* counts, int32_t T, double* brier, void* stream) {
  if (counts && (T < 1 || T > 1024)) return fail(JR_ERR_INVALID, "metrics_reset: T outside 1..1024");
  hipStream_t s = as_stream(stream);
  if (counts && hipMemsetAsync(counts, 0, (size_t)4 * T * sizeof(uint32_t), s) != hipSuccess)
    return fail(JR_ERR_HIP, "metrics_reset: memset failed");
  if (brier && hipMemsetAsync(brier, 0, 2 * sizeof(double), s) != hipSuccess)
    return fail(JR_ERR_HIP, "metrics_reset: memset failed");
  return JR_OK;
}

JR_API int jr_step_log_append(jr_step_rec* ring, uint32_t capacity, uint32_t* cursor, const float* loss,
                              const jr_opt_step* step, void* stream) {
  if (!ring || !cursor || !loss || capacity == 0) return fail(JR_ERR_INVALID, "step_log_append: bad arguments");
  if (((uintptr_t)ring & 3) || ((uintptr_t)cursor & 3) || ((uintptr_t)loss & 3) || ((uintptr_t)step & 3))
    return fail(JR_ERR_INVALID, "step_log_append: misaligned pointer");
  hipLaunchKernelGGL(k_step_log_append, dim3(1), dim3(1), 0, as_stream(stream), ring, capacity, cursor, loss, step);
  return check_launch("step_log_append");
}
