// jr_dropout.hip — dropout between the global average pool and the dense
// layer (the published Inception-v3 recipe: rate 0.2; not in the reference),
// with its key, counter, threshold and scale in DEVICE memory (jr.h
// jr_dropout_state).  No mask is stored: element i keeps iff word i & 3 of
// philox4x32_10((lo32(i >> 2), hi32(i >> 2), step, 0), key) >= threshold, so
// the backward recomputes the forward's mask and a captured step draws a new
// one on every replay (jr_dropout_advance bumps the counter on the stream).
// One thread handles one quad: one Philox block, one 16-byte load and store;
// the last n % 4 elements go singly through the thread behind the last quad.
// tests/loss_ref.py restates the generator and the mask in numpy, bit for bit
// (compiled with -ffp-contract=off: the one multiply stays a multiply).
#include <cmath>

#include "jr_common.h"

namespace jr {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

struct Quad32 {
  uint32_t w[4];
};

__device__ __forceinline__ Quad32 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return Quad32{{c0, c1, c2, c3}};
}

__global__ void k_dropout_set(jr_dropout_state* st, uint32_t key0, uint32_t key1, uint32_t step, uint32_t threshold,
                              float scale) {
  st->key[0] = key0;
  st->key[1] = key1;
  st->step = step;
  st->threshold = threshold;
  st->scale = scale;
  st->pad[0] = st->pad[1] = st->pad[2] = 0u;
}

__global__ void k_dropout_advance(jr_dropout_state* st) { st->step = st->step + 1u; }

// y = keep ? x * scale : 0 over n elements (the backward: x == y); thread q < n / 4
// takes quad q, thread n / 4 the n % 4 elements behind the last quad
__global__ void __launch_bounds__(256) k_dropout(const float* x, float* y, int64_t n,
                                                 const jr_dropout_state* __restrict__ st) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x, nq = n >> 2;
  if (q > nq) return;
  const int tail = (int)(n & 3);
  if (q == nq && tail == 0) return;
  const uint32_t threshold = st->threshold;
  const float scale = st->scale;
  const Quad32 r = philox4x32_10((uint32_t)q, (uint32_t)((uint64_t)q >> 32), st->step, 0u, st->key[0], st->key[1]);
  if (q < nq) {
    float4 v = reinterpret_cast<const float4*>(x)[q];
    v.x = r.w[0] >= threshold ? v.x * scale : 0.0f;
    v.y = r.w[1] >= threshold ? v.y * scale : 0.0f;
    v.z = r.w[2] >= threshold ? v.z * scale : 0.0f;
    v.w = r.w[3] >= threshold ? v.w * scale : 0.0f;
    reinterpret_cast<float4*>(y)[q] = v;
  } else {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (j < tail) y[4 * nq + j] = r.w[j] >= threshold ? x[4 * nq + j] * scale : 0.0f;
  }
}

static int dropout_launch(const char* what, const float* x, float* y, int64_t n, const jr_dropout_state* state,
                          void* stream) {
  if (!x || !y || !state) return fail(JR_ERR_INVALID, std::string(what) + ": null pointer");
  if (n <= 0) return fail(JR_ERR_INVALID, std::string(what) + ": n must be positive");
  if ((((uintptr_t)x | (uintptr_t)y) & 15) || ((uintptr_t)state & 3))
    return fail(JR_ERR_INVALID, std::string(what) + ": buffers must be 16-byte aligned (the state 4-byte)");
  const int64_t threads = (n >> 2) + ((n & 3) ? 1 : 0);
  const int64_t blocks = ceil_div(threads, 256);
  if (blocks > 0x7fffffff) return fail(JR_ERR_INVALID, std::string(what) + ": n too large");
  hipLaunchKernelGGL(k_dropout, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, y, n, state);
  return check_launch(what);
}

}  // namespace jr

using namespace jr;

JR_API int jr_dropout_set(jr_dropout_state* state, uint32_t key0, uint32_t key1, float rate, uint32_t step,
                          void* stream) {
  if (!state || ((uintptr_t)state & 3)) return fail(JR_ERR_INVALID, "dropout_set: null or misaligned state");
  if (!(rate >= 0.f && rate < 1.f)) return fail(JR_ERR_INVALID, "dropout_set: rate outside [0, 1)");
  const double two32 = 4294967296.0;
  const uint32_t threshold = (uint32_t)std::floor((double)rate * two32);
  const float scale = (float)(1.0 / (1.0 - (double)threshold / two32));
  hipLaunchKernelGGL(k_dropout_set, dim3(1), dim3(1), 0, as_stream(stream), state, key0, key1, step, threshold, scale);
  return check_launch("dropout_set");
}

JR_API int jr_dropout_fwd(const float* x, float* y, int64_t n, const jr_dropout_state* state, void* stream) {
  return dropout_launch("dropout_fwd", x, y, n, state, stream);
}

JR_API int jr_dropout_bwd(float* dx, int64_t n, const jr_dropout_state* state, void* stream) {
  return dropout_launch("dropout_bwd", dx, dx, n, state, stream);
}

JR_API int jr_dropout_advance(jr_dropout_state* state, void* stream) {
  if (!state || ((uintptr_t)state & 3)) return fail(JR_ERR_INVALID, "dropout_advance: null or misaligned state");
  hipLaunchKernelGGL(k_dropout_advance, dim3(1), dim3(1), 0, as_stream(stream), state);
  return check_launch("dropout_advance");
}
