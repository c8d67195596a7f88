// jr_common.h — shared helpers for the libjr.so HIP sources (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <cstdlib>
#include <string>

#include "jr_bn_plan.h"   // kStatsLanes, kFoldMaxP: the host-only BN planner sizes with them too
#include "jr_error.h"

namespace jr {

// Map the last HIP launch error (if any) to JR_ERR_HIP.
int check_launch(const char* what);

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Device words the library owns per (device, stream, kind) (jr_api.cpp):
// zeroed once when allocated (in order on that stream) and used only by
// launches on that stream, which run in order -- so a kernel that leaves its
// words zero again (the stream-K hand-off flags, kind 0) needs no memset
// before each launch.  A capturing stream gets a fresh private region per
// call: graph replays may run on any stream.  nullptr if allocation failed.
unsigned* stream_scratch(hipStream_t s, int kind, size_t words);

// The current device's error word (jr_api.cpp): kernels count device-side
// failures into it (vector atomics); jr_device_check() reads, reports and
// clears it.  Allocated by jr_init (or on first use outside a capture).
unsigned* device_error_word(hipStream_t s);

// The *_guard entry points (jr.h): each checks its limit (finite, > 0) before
// anything else, then shares the unguarded call's validation and launcher,
// which takes limit = 0 for "no guard" and fetches the error word last, as
// jr_absmax_prep does.
inline bool guard_limit(float limit) { return limit > 0.f && limit < __builtin_inff(); }
struct Guard {
  float limit = 0.f;
  unsigned* err = nullptr;   // non-NULL: launch the GUARD kernel
};
inline int guard_word(const char* what, float limit, hipStream_t s, Guard& g) {
  g = Guard{};
  if (!(limit > 0.f)) return JR_OK;
  g.limit = limit;
  g.err = device_error_word(s);
  if (!g.err) return fail(JR_ERR_HIP, std::string(what) + ": no device error word (call jr_init before capturing)");
  return JR_OK;
}

// Bijective XCD-aware remap of a flat workgroup id (cdna_hip_programming.md
// §5 "XCD swizzle must be bijective"): blocks b, b+8, b+16 ... are dealt to one
// XCD by the dispatcher, so consecutive remapped ids land on one XCD's L2.
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
  const int xcd = orig & 7;
  const int q = nwg >> 3, r = nwg & 7;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (orig >> 3);
}

__device__ __forceinline__ float bf2f(uint16_t v) {
  return __uint_as_float(static_cast<uint32_t>(v) << 16);
}
// round-to-nearest-even f32 -> bf16 (NaN kept NaN by the cast path)
__device__ __forceinline__ uint16_t f2bf(float f) {
  __hip_bfloat16 h = __float2bfloat16(f);
  return *reinterpret_cast<uint16_t*>(&h);
}

// Sum of a block's 256 doubles in a fixed tree (the same pairs in every run);
// red: 256 doubles of LDS.  Every thread returns the sum.
__device__ __forceinline__ double block_sum256(double s, double* red) {
  const int t = threadIdx.x;
  red[t] = s;
  __syncthreads();
#pragma unroll
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  return red[0];
}

// BatchNormalization(scale=False) pre-activation, in one fixed rounding
// order: every kernel that applies or differentiates it (jr_bn.hip, the
// fused BN + max-pool of jr_pool.hip) sees bit-identical values and ReLU masks.
__device__ __forceinline__ float bn_xhat(float x, float mean, float invstd) {
  return __fmul_rn(__fsub_rn(x, mean), invstd);
}
__device__ __forceinline__ float bn_pre(float x, float mean, float invstd, float beta) {
  return __fadd_rn(bn_xhat(x, mean, invstd), beta);
}

// Canonical combine of ONE channel's fused BN-statistics partials (the conv
// epilogue's / split-K reduce's per-row-group (mean, M2) of R rows each; the
// last group holds the rest of the M rows) into (mean, invstd): an aligned
// group of 8 lanes, lane j summing partials j, j+8, ... in order, shifted by
// the first partial's mean K, in fp64; an xor butterfly over the 8 lanes.
// k_stats_finalize8 (jr_conv.hip) and jr_bn_relu_apply_stats (jr_bn.hip, the
// finalize folded into the BN apply) both call this, so they give bitwise the
// same statistics.  Every lane of the group returns the result.
// (kStatsLanes lanes, at most kFoldMaxP partials per channel: jr_bn_plan.h)
__device__ __forceinline__ void stats_combine8(const float* __restrict__ pm, const float* __restrict__ pq, int P,
                                               int R, int M, float eps, int j, float* mean, float* invstd) {
  const double K = pm[0];
  double sn = 0, sd = 0, sq = 0;
  constexpr int U = 16;   // loads in flight per lane and array
  for (int i0 = j; i0 < P; i0 += kStatsLanes * U) {
    float vm[U], vq[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {   // clamped unconditional loads, all issued before any use
      const int ic = min(i0 + kStatsLanes * u, P - 1);
      vm[u] = pm[ic];
      vq[u] = pq[ic];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + kStatsLanes * u;
      if (i < P) {
        const double c = (double)min(max(M - i * R, 0), R);
        const double d = (double)vm[u] - K;
        sn += c;
        sd += c * d;
        sq += (double)vq[u] + c * d * d;
      }
    }
  }
#pragma unroll
  for (int o = kStatsLanes / 2; o > 0; o >>= 1) {
    sn += __shfl_xor(sn, o, kStatsLanes);
    sd += __shfl_xor(sd, o, kStatsLanes);
    sq += __shfl_xor(sq, o, kStatsLanes);
  }
  const double dm = sn > 0 ? sd / sn : 0.0;
  const double m2 = fmax(sq - sn * dm * dm, 0.0);
  *mean = (float)(K + dm);
  *invstd = (float)(1.0 / sqrt(m2 / (double)M + (double)eps));
}

// One launch expression for both path dtypes: calls f with a value of the
// element type, uint16_t (the bf16 bits) for JR_BF16 and float for every
// other dtype (JR_F32 and the fp32-tensor conv dtypes) -- in f,
// `using T = decltype(t);`.  A caller that takes only JR_F32 / JR_BF16
// rejects the rest before.  The call written first is instantiated first,
// and a translation unit's kernels sit in its code object in that order:
// kBf16First keeps the order of the conv sites, which always named bf16 first.
template <bool kBf16First = false, typename F>
inline void by_dtype(int dtype, F&& f) {
  if constexpr (kBf16First) {
    if (dtype == JR_BF16)
      f(uint16_t{});
    else
      f(float{});
  } else {
    if (dtype != JR_BF16)
      f(float{});
    else
      f(uint16_t{});
  }
}

// Element load/store of an activation in the path dtype.
template <typename T> struct Elt;
template <> struct Elt<float> {
  __device__ static float ld(const float* p) { return *p; }
  __device__ static void st(float* p, float v) { *p = v; }
};
template <> struct Elt<uint16_t> {
  __device__ static float ld(const uint16_t* p) { return bf2f(*p); }
  __device__ static void st(uint16_t* p, float v) { *p = f2bf(v); }
};

}  // namespace jr
