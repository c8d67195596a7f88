// jr_opt.hip — the optimizer recipe with its step scalars in device memory:
// the global gradient norm, the clip factor and the non-finite guard, and the
// four updates reading (lr, weight_decay) and (scale, skipped) from there, so a
// captured step replays under a changing learning rate (contracts: jr.h).
//
// Compiled with -ffp-contract=off like jr_misc.hip (Makefile): every fp32
// operation below is one correctly rounded op in the written order, which
// tests/opt_ref.py restates in numpy float32 bit for bit.
#include "jr_common.h"
#include "jr_opt_expr.h"

namespace jr {

constexpr int kNormBlocks = 1024;   // the norm's fixed grid: at most this many blocks of 256
constexpr int kTileQuads = 256;     // an update block's unit of work: one quad per thread, as jr_nesterov_update

static int norm_blocks(int64_t n) {
  return (int)std::min<int64_t>(std::max<int64_t>(ceil_div(n >> 2, 256), 1), kNormBlocks);
}

__global__ void k_set_hyper(jr_opt_hyper* h, float lr, float wd, float clip, float gs) {
  h->lr = lr;
  h->weight_decay = wd;
  h->clip_norm = clip;
  h->grad_scale = gs;
}

// Sum of 256 doubles in a fixed tree (the same pairs in every run).
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

// Each thread adds the squares of its quads in stride order (x, y, z, w of a
// quad in that order; the product of two fp32 values is exact in fp64), thread
// t < n % 4 of block 0 then the tail element n - n % 4 + t; one partial per block.
__global__ void __launch_bounds__(256) k_grad_sqnorm(const float* __restrict__ g, int64_t n, double* __restrict__ partials) {
  __shared__ double red[256];
  const int64_t n4 = n >> 2;
  double s = 0.0;
#pragma unroll 4
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 v = reinterpret_cast<const float4*>(g)[i];
    s += (double)v.x * (double)v.x;
    s += (double)v.y * (double)v.y;
    s += (double)v.z * (double)v.z;
    s += (double)v.w * (double)v.w;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const double x = g[n4 * 4 + threadIdx.x];
    s += x * x;
  }
  const double b = block_sum256(s, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = b;
}

__global__ void __launch_bounds__(256) k_opt_prepare(const double* __restrict__ partials, int nb,
                                                     const jr_opt_hyper* __restrict__ hyper, jr_opt_step* step) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) s += partials[i];
  const double S = block_sum256(s, red);
  if (threadIdx.x != 0) return;
  const float gs = hyper->grad_scale, clip = hyper->clip_norm;
  const float n32 = (float)sqrt(S);
  const float gn = __fmul_rn(n32, gs);
  const float factor = (clip > 0.f && gn > clip) ? __fdiv_rn(clip, gn) : 1.0f;
  float scale = __fmul_rn(gs, factor);
  const bool finite = fabsf(gn) < __builtin_inff();   // false for NaN too
  if (!finite) {
    scale = 0.f;
    step->skipped_total = step->skipped_total + 1u;
  }
  step->scale = scale;
  step->grad_norm = gn;
  step->skipped = finite ? 0u : 1u;
}

// The first range whose end lies past element e (nr if none).
__device__ __forceinline__ int range_after(const jr_opt_range* __restrict__ R, int nr, int64_t e) {
  int lo = 0, hi = nr;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (R[mid].end > e) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// Bit j: element e + j (j < 4) lies in a range; r: a range index at or before
// the first range that ends past e.
__device__ __forceinline__ unsigned decay_mask4(const jr_opt_range* __restrict__ R, int nr, int r, int64_t e) {
  while (r < nr && R[r].end <= e) ++r;
  if (r == nr || R[r].begin >= e + 4) return 0u;
  if (R[r].begin <= e && R[r].end >= e + 4) return 15u;
  unsigned m = 0u;   // a range boundary inside the quad
  for (int j = 0; j < 4; ++j) {
    while (r < nr && R[r].end <= e + j) ++r;
    if (r < nr && R[r].begin <= e + j) m |= 1u << j;
  }
  return m;
}

enum { kNesterov = 0, kMomentum = 1, kSgd = 2, kAdam = 3 };

// One element: g' = g*scale (+ wd*w inside a decay range), then the
// by-value kernel's expression of jr_misc.hip with lr from device memory.
// p0: momentum, or Adam's beta1 (p1: beta2, p2: epsilon).
template <int OPT>
__device__ __forceinline__ void update1(float& w, float g, float& a, float& v, bool decay, float scale, float wd,
                                        float lr, float p0, float p1, float p2) {
  g = __fmul_rn(g, scale);
  if (decay) g = __fadd_rn(g, __fmul_rn(wd, w));
  if constexpr (OPT == kNesterov) {
    nest1(w, g, a, lr, p0);
  } else if constexpr (OPT == kMomentum) {
    a = __fadd_rn(__fmul_rn(a, p0), g);
    w = __fsub_rn(w, __fmul_rn(a, lr));
  } else if constexpr (OPT == kSgd) {
    w = __fsub_rn(w, __fmul_rn(g, lr));
  } else {
    const float one_b1 = __fsub_rn(1.f, p0), one_b2 = __fsub_rn(1.f, p1);
    a = __fadd_rn(a, __fmul_rn(__fsub_rn(g, a), one_b1));
    v = __fadd_rn(v, __fmul_rn(__fsub_rn(__fmul_rn(g, g), v), one_b2));
    w = __fsub_rn(w, __fdiv_rn(__fmul_rn(a, lr), __fadd_rn(sqrt_cr(v), p2)));
  }
}

// A block takes tiles of kTileQuads quads in grid-stride order, the loop of
// the by-value kernels.  The range search runs once per tile on block-uniform
// values and classes the tile: outside every range, inside one range, or
// mixed -- only a mixed tile's quads walk the table themselves.  Every quad
// moves as 16 bytes; the decay only picks the arithmetic per element.
template <int OPT>
__global__ void __launch_bounds__(256) k_update_ex(float* __restrict__ w, const float* __restrict__ grad,
                                                   float* __restrict__ s1, float* __restrict__ s2, int64_t n, float p0,
                                                   float p1, float p2, const jr_opt_range* __restrict__ R, int nr,
                                                   const jr_opt_hyper* __restrict__ hyper,
                                                   const jr_opt_step* __restrict__ step) {
  if (step->skipped) return;   // a non-finite norm: nothing is written
  const float scale = step->scale, lr = hyper->lr, wd = hyper->weight_decay;
  if (wd == 0.f) nr = 0;
  constexpr bool kS1 = OPT != kSgd, kS2 = OPT == kAdam;
  constexpr unsigned kMixed = 16u;
  const int64_t n4 = n >> 2;
  const int64_t tiles = (n4 + kTileQuads - 1) / kTileQuads;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t i = t * kTileQuads + threadIdx.x;
    float4 wv, gv, av, vv;
    if (i < n4) {
      wv = reinterpret_cast<const float4*>(w)[i];
      gv = reinterpret_cast<const float4*>(grad)[i];
      if constexpr (kS1) av = reinterpret_cast<const float4*>(s1)[i];
      if constexpr (kS2) vv = reinterpret_cast<const float4*>(s2)[i];
    }
    unsigned cls = 0u;   // block-uniform: 0, 15 (every element decays) or kMixed
    int r0 = 0;
    if (nr) {
      const int64_t e0 = t * kTileQuads * 4, e1 = e0 + kTileQuads * 4;
      r0 = range_after(R, nr, e0);
      if (r0 < nr && R[r0].begin < e1) cls = (R[r0].begin <= e0 && R[r0].end >= e1) ? 15u : kMixed;
    }
    if (i < n4) {
      const unsigned d = cls == kMixed ? decay_mask4(R, nr, r0, i * 4) : cls;
      float za = 0.f, zv = 0.f;   // unused state of the optimizer
      update1<OPT>(wv.x, gv.x, kS1 ? av.x : za, kS2 ? vv.x : zv, d & 1u, scale, wd, lr, p0, p1, p2);
      update1<OPT>(wv.y, gv.y, kS1 ? av.y : za, kS2 ? vv.y : zv, d & 2u, scale, wd, lr, p0, p1, p2);
      update1<OPT>(wv.z, gv.z, kS1 ? av.z : za, kS2 ? vv.z : zv, d & 4u, scale, wd, lr, p0, p1, p2);
      update1<OPT>(wv.w, gv.w, kS1 ? av.w : za, kS2 ? vv.w : zv, d & 8u, scale, wd, lr, p0, p1, p2);
      reinterpret_cast<float4*>(w)[i] = wv;
      if constexpr (kS1) reinterpret_cast<float4*>(s1)[i] = av;
      if constexpr (kS2) reinterpret_cast<float4*>(s2)[i] = vv;
    }
  }
  // tail: the last n % 4 elements, one thread each
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t e = n4 * 4 + threadIdx.x;
    bool d = false;
    if (nr) {
      const int r = range_after(R, nr, e);
      d = r < nr && R[r].begin <= e;
    }
    float za = 0.f, zv = 0.f;
    update1<OPT>(w[e], grad[e], kS1 ? s1[e] : za, kS2 ? s2[e] : zv, d, scale, wd, lr, p0, p1, p2);
  }
}

template <int OPT>
static int launch_update_ex(const char* what, float* w, const float* grad, float* s1, float* s2, int64_t n, float p0,
                            float p1, float p2, const jr_opt_range* ranges, int32_t nranges,
                            const jr_opt_hyper* hyper, const jr_opt_step* step, void* stream) {
  const bool state_ok = (OPT == kSgd || s1) && (OPT != kAdam || s2);
  if (!w || !grad || !state_ok || !hyper || !step || n < 0 || nranges < 0 || (nranges > 0 && !ranges))
    return fail(JR_ERR_INVALID, std::string(what) + ": bad arguments");
  if (((uintptr_t)w | (uintptr_t)grad | (uintptr_t)s1 | (uintptr_t)s2) & 15)
    return fail(JR_ERR_INVALID, std::string(what) + ": buffers must be 16-byte aligned");
  if (((uintptr_t)ranges & 7) || ((uintptr_t)hyper & 3) || ((uintptr_t)step & 3))
    return fail(JR_ERR_INVALID, std::string(what) + ": misaligned range table, hyper or step struct");
  if (n == 0) return JR_OK;
  const int64_t tiles = std::max<int64_t>(ceil_div(n >> 2, kTileQuads), 1);
  hipLaunchKernelGGL(k_update_ex<OPT>, dim3((unsigned)std::min<int64_t>(tiles, 256 * 32)), dim3(256), 0,
                     as_stream(stream), w, grad, s1, s2, n, p0, p1, p2, ranges, (int)nranges, hyper, step);
  return check_launch(what);
}

}  // namespace jr

using namespace jr;

JR_API int jr_opt_set_hyper(jr_opt_hyper* hyper, float lr, float weight_decay, float clip_norm, float grad_scale,
                            void* stream) {
  if (!hyper || ((uintptr_t)hyper & 3)) return fail(JR_ERR_INVALID, "opt_set_hyper: bad arguments");
  hipLaunchKernelGGL(k_set_hyper, dim3(1), dim3(1), 0, as_stream(stream), hyper, lr, weight_decay, clip_norm,
                     grad_scale);
  return check_launch("opt_set_hyper");
}

JR_API size_t jr_grad_sqnorm_workspace_size(int64_t n) {
  if (n < 0) return 0;
  return (size_t)norm_blocks(n) * sizeof(double);
}

JR_API int jr_grad_sqnorm(const float* grad, int64_t n, void* partials, size_t ws_bytes, void* stream) {
  if (!grad || !partials || n < 0) return fail(JR_ERR_INVALID, "grad_sqnorm: bad arguments");
  if (((uintptr_t)grad & 15) || ((uintptr_t)partials & 7))
    return fail(JR_ERR_INVALID, "grad_sqnorm: grad must be 16-byte, partials 8-byte aligned");
  if (ws_bytes < jr_grad_sqnorm_workspace_size(n)) return fail(JR_ERR_INVALID, "grad_sqnorm: workspace too small");
  hipLaunchKernelGGL(k_grad_sqnorm, dim3(norm_blocks(n)), dim3(256), 0, as_stream(stream), grad, n, (double*)partials);
  return check_launch("grad_sqnorm");
}

JR_API int jr_opt_prepare(const void* partials, int64_t n, const jr_opt_hyper* hyper, jr_opt_step* step, void* stream) {
  if (!partials || !hyper || !step || n < 0) return fail(JR_ERR_INVALID, "opt_prepare: bad arguments");
  if (((uintptr_t)partials & 7) || ((uintptr_t)hyper & 3) || ((uintptr_t)step & 3))
    return fail(JR_ERR_INVALID, "opt_prepare: misaligned partials, hyper or step struct");
  hipLaunchKernelGGL(k_opt_prepare, dim3(1), dim3(256), 0, as_stream(stream), (const double*)partials, norm_blocks(n),
                     hyper, step);
  return check_launch("opt_prepare");
}

JR_API int jr_nesterov_update_ex(float* w, const float* grad, float* accum, int64_t n, float momentum,
                                 const jr_opt_range* ranges, int32_t nranges, const jr_opt_hyper* hyper,
                                 const jr_opt_step* step, void* stream) {
  return launch_update_ex<kNesterov>("nesterov_ex", w, grad, accum, nullptr, n, momentum, 0.f, 0.f, ranges, nranges,
                                     hyper, step, stream);
}

JR_API int jr_momentum_update_ex(float* w, const float* grad, float* accum, int64_t n, float momentum,
                                 const jr_opt_range* ranges, int32_t nranges, const jr_opt_hyper* hyper,
                                 const jr_opt_step* step, void* stream) {
  return launch_update_ex<kMomentum>("momentum_ex", w, grad, accum, nullptr, n, momentum, 0.f, 0.f, ranges, nranges,
                                     hyper, step, stream);
}

JR_API int jr_sgd_update_ex(float* w, const float* grad, int64_t n, const jr_opt_range* ranges, int32_t nranges,
                            const jr_opt_hyper* hyper, const jr_opt_step* step, void* stream) {
  return launch_update_ex<kSgd>("sgd_ex", w, grad, nullptr, nullptr, n, 0.f, 0.f, 0.f, ranges, nranges, hyper, step,
                                stream);
}

JR_API int jr_adam_update_ex(float* w, const float* grad, float* m, float* v, int64_t n, float beta1, float beta2,
                             float eps, const jr_opt_range* ranges, int32_t nranges, const jr_opt_hyper* hyper,
                             const jr_opt_step* step, void* stream) {
  return launch_update_ex<kAdam>("adam_ex", w, grad, m, v, n, beta1, beta2, eps, ranges, nranges, hyper, step, stream);
}
