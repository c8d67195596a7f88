// jr_opt_expr.h — the per-element optimizer expressions shared by the
// by-value updates (jr_misc.hip) and the device-scalar updates (jr_opt.hip).
// Both files are compiled with -ffp-contract=off: every multiply and add
// rounds on its own (see jr_misc.hip).
#pragma once
#include "jr_common.h"

namespace jr {

__device__ __forceinline__ float nest1(float& w, float g, float& a, float lr, float m) {
  a = __fadd_rn(__fmul_rn(a, m), g);
  w = __fsub_rn(w, __fadd_rn(__fmul_rn(g, lr), __fmul_rn(__fmul_rn(a, m), lr)));
  return w;
}

// Correctly rounded sqrt (IEEE, as Eigen's sqrt on the CPU): v_sqrt_f32 is
// within 1 ulp, so check its neighbours with exact fma residuals and step
// once (denormal inputs are scaled by 2^32 first).
__device__ __forceinline__ float sqrt_cr(float x) {
  const bool tiny = x < 0x1.0p-96f;
  const float xs = tiny ? x * 0x1.0p+32f : x;
  float s = __builtin_amdgcn_sqrtf(xs);
  const float dn = __uint_as_float(__float_as_uint(s) - 1), up = __uint_as_float(__float_as_uint(s) + 1);
  if (__builtin_fmaf(-dn, s, xs) <= 0.f) s = dn;
  else if (__builtin_fmaf(-up, s, xs) > 0.f) s = up;
  s = tiny ? s * 0x1.0p-16f : s;
  return (xs == 0.f || !(xs < __builtin_inff())) ? __builtin_sqrtf(x) : s;
}

}  // namespace jr
