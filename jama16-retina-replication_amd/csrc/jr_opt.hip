// jr_opt.hip — the optimizers: one update body behind the by-value calls
// (lr and grad_scale as launch arguments) and the device-scalar recipe (the
// global gradient norm, the clip factor and the non-finite guard, and the five
// updates reading (lr, weight_decay) and (scale, skipped) from device memory,
// so a captured step replays under a changing learning rate; contracts: jr.h),
// the moving average of the weights with its counter in device memory, and the
// add that accumulates K micro-batches' gradients per update.
//
// The updates replace the TF ApplyMomentum / ApplyGradientDescent / ApplyAdam
// ops that .minimize adds at train.py:147-153; ApplyRMSProp
// and ExponentialMovingAverage are the two parts of the published Inception-v3
// recipe the reference does not use [TF-3P, from reading, version unpinned].  One launch
// updates the whole flat parameter buffer (21,770,401 fp32 values); each lane
// moves 16-byte vectors and the arithmetic is the unfused TF expression order.
// NOTE: hipcc contracts a*b+c into an FMA by default (-ffp-contract=fast),
// and without OCML_BASIC_ROUNDED_OPERATIONS __fmul_rn / __fadd_rn are the
// plain operators, so this file is compiled with -ffp-contract=off
// (Makefile): every fp32 operation below is one correctly rounded op in the
// written order, the IEEE fp32 evaluation of TF's (Eigen, non-fused)
// expressions, which tests/opt_ref.py restates in numpy float32 bit for bit.
#include "jr_common.h"

namespace jr {

constexpr int kNormBlocks = 1024;   // the norm's fixed grid: at most this many blocks of 256
constexpr int kTile = 256;          // an update block's unit of work: one vector (a quad or an element) per thread

static int norm_blocks(int64_t n) {
  return (int)std::min<int64_t>(std::max<int64_t>(ceil_div(n >> 2, 256), 1), kNormBlocks);
}

__global__ void k_set_hyper(jr_opt_hyper* h, float lr, float wd, float clip, float gs) {
  h->lr = lr;
  h->weight_decay = wd;
  h->clip_norm = clip;
  h->grad_scale = gs;
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

enum { kNesterov = 0, kMomentum = 1, kSgd = 2, kAdam = 3, kRmsprop = 4 };

// One element: g' = g*scale (+ wd*w inside a decay range), then
//   ApplyMomentum(use_nesterov): accum = accum*m + g'; var -= g'*lr + accum*m*lr
//   ApplyMomentum:               accum = accum*m + g'; var -= accum*lr
//   ApplyGradientDescent:        var -= g'*lr
//   ApplyAdam (training_ops.cc ApplyAdamNonCuda):
//     m += (g' - m) * (1 - beta1);  v += (g'*g' - v) * (1 - beta2);
//     var -= (m * alpha) / (sqrt(v) + epsilon); lr is the step's alpha =
//     rate * sqrt(1 - beta2^t) / (1 - beta1^t) (lr_t, computed on the host).
//   ApplyRMSProp (training_ops.cc, the CPU functor; a: mom, v: ms):
//     ms += (g'*g' - ms) * (1 - rho);  mom = mom*momentum + (g'*lr) / sqrt(ms + epsilon);
//     var -= mom
// p0: momentum, or Adam's beta1 (p1: beta2, p2: epsilon), or RMSProp's rho
// (p1: momentum, p2: epsilon).
template <int OPT>
__device__ __forceinline__ void update1(float& w, float g, float& a, float& v, bool decay, float scale, float wd,
                                        float lr, float p0, float p1, float p2) {
  g = __fmul_rn(g, scale);
  if (decay) g = __fadd_rn(g, __fmul_rn(wd, w));
  if constexpr (OPT == kNesterov) {
    a = __fadd_rn(__fmul_rn(a, p0), g);
    w = __fsub_rn(w, __fadd_rn(__fmul_rn(g, lr), __fmul_rn(__fmul_rn(a, p0), lr)));
  } else if constexpr (OPT == kMomentum) {
    a = __fadd_rn(__fmul_rn(a, p0), g);
    w = __fsub_rn(w, __fmul_rn(a, lr));
  } else if constexpr (OPT == kSgd) {
    w = __fsub_rn(w, __fmul_rn(g, lr));
  } else if constexpr (OPT == kRmsprop) {
    v = __fadd_rn(v, __fmul_rn(__fsub_rn(__fmul_rn(g, g), v), __fsub_rn(1.f, p0)));
    a = __fadd_rn(__fmul_rn(a, p1), __fdiv_rn(__fmul_rn(g, lr), sqrt_cr(__fadd_rn(v, p2))));
    w = __fsub_rn(w, a);
  } else {
    const float one_b1 = __fsub_rn(1.f, p0), one_b2 = __fsub_rn(1.f, p1);
    a = __fadd_rn(a, __fmul_rn(__fsub_rn(g, a), one_b1));
    v = __fadd_rn(v, __fmul_rn(__fsub_rn(__fmul_rn(g, g), v), one_b2));
    w = __fsub_rn(w, __fdiv_rn(__fmul_rn(a, lr), __fadd_rn(sqrt_cr(v), p2)));
  }
}

// Where an update takes its step scalars from.  ByValue: launch arguments;
// weight decay 0, no range table, never skipped -- all three known when the
// body is compiled.  FromDevice: jr_opt_hyper / jr_opt_step, read at the start
// of every block, and weight decay inside the ranges of the table.
struct ByValue {
  float lr, scale;
};
struct FromDevice {
  const jr_opt_range* R;
  int nr;
  const jr_opt_hyper* hyper;
  const jr_opt_step* step;
};

template <int W>
struct alignas(4 * W) Vec {
  float e[W];
};

// Every update kernel.  A block takes tiles of kTile vectors of W elements in
// grid-stride order, thread i of tile t the vector t * kTile + i; W = 4 moves
// every quad as 16 bytes and leaves the last n % 4 elements to block 0, W = 1
// is for buffers that are not 16-byte aligned.  FromDevice: the range search
// runs once per tile on block-uniform values and classes the tile: outside
// every range, inside one range, or mixed -- only a mixed tile's quads walk
// the table themselves; the decay only picks the arithmetic per element.
template <int OPT, int W, class SRC>
__device__ __forceinline__ void update_body(float* __restrict__ w, const float* __restrict__ grad,
                                            float* __restrict__ s1, float* __restrict__ s2, int64_t n, float p0, float p1,
                                            float p2, const SRC src) {
  constexpr bool kDev = std::is_same<SRC, FromDevice>::value;
  static_assert(W == 4 || (W == 1 && !kDev), "the decay classes are per quad");
  constexpr bool kS1 = OPT != kSgd, kS2 = OPT == kAdam || OPT == kRmsprop;
  constexpr unsigned kMixed = 16u;
  using V = Vec<W>;
  float scale, lr, wd = 0.f, za = 0.f, zv = 0.f;   // za, zv: the state an optimizer does not have
  int nr = 0;
  if constexpr (kDev) {
    if (src.step->skipped) return;   // a non-finite norm: nothing is written
    scale = src.step->scale, lr = src.hyper->lr, wd = src.hyper->weight_decay;
    nr = wd == 0.f ? 0 : src.nr;
  } else {
    scale = src.scale, lr = src.lr;
  }
  const int64_t nv = W == 4 ? n >> 2 : n;
  int64_t t = blockIdx.x;   // the tile of i: block-uniform
  for (int64_t i = t * kTile + threadIdx.x; i < nv; i += (int64_t)gridDim.x * kTile, t += gridDim.x) {
    V wv = reinterpret_cast<const V*>(w)[i], av, vv;
    const V gv = reinterpret_cast<const V*>(grad)[i];
    if constexpr (kS1) av = reinterpret_cast<const V*>(s1)[i];
    if constexpr (kS2) vv = reinterpret_cast<const V*>(s2)[i];
    unsigned d = 0u;   // bit j: element j of the vector decays
    if constexpr (kDev) {
      if (nr) {
        const int64_t e0 = t * kTile * 4, e1 = e0 + kTile * 4;
        const int r0 = range_after(src.R, nr, e0);
        unsigned cls = 0u;   // block-uniform: 0, 15 (every element decays) or kMixed
        if (r0 < nr && src.R[r0].begin < e1) cls = (src.R[r0].begin <= e0 && src.R[r0].end >= e1) ? 15u : kMixed;
        d = cls == kMixed ? decay_mask4(src.R, nr, r0, i * 4) : cls;
      }
    }
#pragma unroll
    for (int j = 0; j < W; ++j)
      update1<OPT>(wv.e[j], gv.e[j], kS1 ? av.e[j] : za, kS2 ? vv.e[j] : zv, d >> j & 1u, scale, wd, lr, p0, p1, p2);
    reinterpret_cast<V*>(w)[i] = wv;
    if constexpr (kS1) reinterpret_cast<V*>(s1)[i] = av;
    if constexpr (kS2) reinterpret_cast<V*>(s2)[i] = vv;
  }
  // tail: the last n % W elements, one thread each
  if (blockIdx.x == 0 && threadIdx.x < (n & (W - 1))) {
    const int64_t e = nv * W + threadIdx.x;
    bool d = false;
    if constexpr (kDev) {
      if (nr) {
        const int r = range_after(src.R, nr, e);
        d = r < nr && src.R[r].begin <= e;
      }
    }
    update1<OPT>(w[e], grad[e], kS1 ? s1[e] : za, kS2 ? s2[e] : zv, d, scale, wd, lr, p0, p1, p2);
  }
}

__host__ __device__ static inline bool aligned16(const void* a, const void* b, const void* c = nullptr,
                                                 const void* d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

// The by-value updates that take any 4-byte alignment: quads when every buffer is
// 16-byte aligned (the host sizes the grid by the same test), else single elements.
template <int OPT>
__device__ __forceinline__ void update_by_alignment(float* __restrict__ w, const float* __restrict__ grad,
                                                    float* __restrict__ s1, float* __restrict__ s2, int64_t n, float p0,
                                                    float p1, float p2, const ByValue src) {
  if (aligned16(w, grad, s1, s2))
    update_body<OPT, 4>(w, grad, s1, s2, n, p0, p1, p2, src);
  else
    update_body<OPT, 1>(w, grad, s1, s2, n, p0, p1, p2, src);
}

// The kernels keep one name per optimizer and scalar source: traces and the
// tools that read them find the step's end by it.
__global__ void __launch_bounds__(256) k_nesterov(float* __restrict__ w, const float* __restrict__ grad,
                                                  float* __restrict__ accum, int64_t n, float lr, float m, float gs) {
  update_body<kNesterov, 4>(w, grad, accum, nullptr, n, m, 0.f, 0.f, ByValue{lr, gs});
}

__global__ void __launch_bounds__(256) k_momentum(float* __restrict__ w, const float* __restrict__ grad,
                                                  float* __restrict__ accum, int64_t n, float lr, float m, float gs) {
  update_by_alignment<kMomentum>(w, grad, accum, nullptr, n, m, 0.f, 0.f, ByValue{lr, gs});
}

__global__ void __launch_bounds__(256) k_sgd(float* __restrict__ w, const float* __restrict__ grad, int64_t n,
                                             float lr, float gs) {
  update_by_alignment<kSgd>(w, grad, nullptr, nullptr, n, 0.f, 0.f, 0.f, ByValue{lr, gs});
}

__global__ void __launch_bounds__(256) k_adam(float* __restrict__ w, const float* __restrict__ grad,
                                              float* __restrict__ mm, float* __restrict__ vv, int64_t n, float lr_t,
                                              float b1, float b2, float eps, float gs) {
  update_by_alignment<kAdam>(w, grad, mm, vv, n, b1, b2, eps, ByValue{lr_t, gs});
}

__global__ void __launch_bounds__(256) k_rmsprop(float* __restrict__ w, const float* __restrict__ grad,
                                                 float* __restrict__ mom, float* __restrict__ ms, int64_t n, float lr,
                                                 float rho, float m, float eps, float gs) {
  update_by_alignment<kRmsprop>(w, grad, mom, ms, n, rho, m, eps, ByValue{lr, gs});
}

#define JR_UPDATE_EX_KERNEL(NAME, OPT)                                                                               \
  __global__ void __launch_bounds__(256) NAME(                                                                       \
      float* __restrict__ w, const float* __restrict__ grad, float* __restrict__ s1, float* __restrict__ s2, int64_t n, \
      float p0, float p1, float p2, const jr_opt_range* __restrict__ R, int nr, const jr_opt_hyper* __restrict__ hyper, \
      const jr_opt_step* __restrict__ step) {                                                                        \
    update_body<OPT, 4>(w, grad, s1, s2, n, p0, p1, p2, FromDevice{R, nr, hyper, step});                             \
  }
JR_UPDATE_EX_KERNEL(k_nesterov_ex, kNesterov)
JR_UPDATE_EX_KERNEL(k_momentum_ex, kMomentum)
JR_UPDATE_EX_KERNEL(k_sgd_ex, kSgd)
JR_UPDATE_EX_KERNEL(k_adam_ex, kAdam)
JR_UPDATE_EX_KERNEL(k_rmsprop_ex, kRmsprop)
#undef JR_UPDATE_EX_KERNEL

static dim3 update_grid(int64_t vectors) {
  return dim3((unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(vectors, kTile), 1), 256 * 32));
}

static int launch_update_ex(const char* what, int opt, float* w, const float* grad, float* s1, float* s2, int64_t n,
                            float p0, float p1, float p2, const jr_opt_range* ranges, int32_t nranges,
                            const jr_opt_hyper* hyper, const jr_opt_step* step, void* stream) {
  static constexpr decltype(&k_nesterov_ex) kernels[] = {k_nesterov_ex, k_momentum_ex, k_sgd_ex, k_adam_ex,
                                                        k_rmsprop_ex};
  const bool state_ok = (opt == kSgd || s1) && ((opt != kAdam && opt != kRmsprop) || s2);
  if (!w || !grad || !state_ok || !hyper || !step || n < 0 || nranges < 0 || (nranges > 0 && !ranges))
    return fail(JR_ERR_INVALID, std::string(what) + ": bad arguments");
  if (!aligned16(w, grad, s1, s2))
    return fail(JR_ERR_INVALID, std::string(what) + ": buffers must be 16-byte aligned");
  if (((uintptr_t)ranges & 7) || ((uintptr_t)hyper & 3) || ((uintptr_t)step & 3))
    return fail(JR_ERR_INVALID, std::string(what) + ": misaligned range table, hyper or step struct");
  if (n == 0) return JR_OK;
  hipLaunchKernelGGL(kernels[opt], update_grid(n >> 2), dim3(256), 0, as_stream(stream), w, grad, s1, s2, n, p0, p1,
                     p2, ranges, (int)nranges, hyper, step);
  return check_launch(what);
}

// ---- the moving average of the weights (contracts: jr.h) ----
__global__ void k_ema_set(jr_ema_state* st, float decay, uint32_t warm, uint32_t updates) {
  st->decay = decay;
  st->one_minus_decay = __fsub_rn(1.f, decay);
  st->updates = updates;
  st->warm = warm;
}

__global__ void k_ema_prepare(jr_ema_state* st, const jr_opt_step* __restrict__ step) {
  if (step && step->skipped) {
    st->one_minus_decay = 0.f;
    return;
  }
  const float decay = st->decay;
  const uint32_t updates = st->updates;
  const float t = (float)updates;
  const float d = st->warm ? fminf(decay, __fdiv_rn(__fadd_rn(1.f, t), __fadd_rn(10.f, t))) : decay;
  st->one_minus_decay = __fsub_rn(1.f, d);
  st->updates = updates + 1u;
}

__device__ __forceinline__ float ema1(float s, float w, float omd) {
  return __fsub_rn(s, __fmul_rn(__fsub_rn(s, w), omd));
}

// The loop of update_body at W = 4: tiles of kTile quads in grid-stride order,
// the last n % 4 elements on block 0.
__global__ void __launch_bounds__(256) k_ema_update(float* __restrict__ shadow, const float* __restrict__ w, int64_t n,
                                                    const jr_ema_state* __restrict__ st,
                                                    const jr_opt_step* __restrict__ step) {
  if (step && step->skipped) return;   // a skipped step: nothing is written
  using V = Vec<4>;
  const float omd = st->one_minus_decay;
  const int64_t nv = n >> 2;
  for (int64_t i = (int64_t)blockIdx.x * kTile + threadIdx.x; i < nv; i += (int64_t)gridDim.x * kTile) {
    V sv = reinterpret_cast<const V*>(shadow)[i];
    const V wv = reinterpret_cast<const V*>(w)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) sv.e[j] = ema1(sv.e[j], wv.e[j], omd);
    reinterpret_cast<V*>(shadow)[i] = sv;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t e = nv * 4 + threadIdx.x;
    shadow[e] = ema1(shadow[e], w[e], omd);
  }
}

// ---- gradient accumulation (contract: jr.h) ----
// k_ema_update's loop at W = 4 (W = 1: buffers that are not 16-byte aligned,
// no tail).  FIRST: a copy -- dst is not read.
template <int W, bool FIRST>
__device__ __forceinline__ void accumulate_body(float* __restrict__ dst, const float* __restrict__ src, int64_t n) {
  using V = Vec<W>;
  const int64_t nv = W == 4 ? n >> 2 : n;
  for (int64_t i = (int64_t)blockIdx.x * kTile + threadIdx.x; i < nv; i += (int64_t)gridDim.x * kTile) {
    V sv = reinterpret_cast<const V*>(src)[i];
    if constexpr (!FIRST) {
      const V dv = reinterpret_cast<const V*>(dst)[i];
#pragma unroll
      for (int j = 0; j < W; ++j) sv.e[j] = __fadd_rn(dv.e[j], sv.e[j]);
    }
    reinterpret_cast<V*>(dst)[i] = sv;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & (W - 1))) {
    const int64_t e = nv * W + threadIdx.x;
    dst[e] = FIRST ? src[e] : __fadd_rn(dst[e], src[e]);
  }
}

__global__ void __launch_bounds__(256) k_grad_accumulate(float* __restrict__ dst, const float* __restrict__ src,
                                                         int64_t n, int first) {
  if (aligned16(dst, src)) {   // (the host sizes the grid by the same test)
    if (first) accumulate_body<4, true>(dst, src, n);
    else accumulate_body<4, false>(dst, src, n);
  } else {
    if (first) accumulate_body<1, true>(dst, src, n);
    else accumulate_body<1, false>(dst, src, n);
  }
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

JR_API int jr_nesterov_update(float* w, const float* grad, float* accum, int64_t n, float lr, float momentum,
                              float grad_scale, void* stream) {
  if (!w || !grad || !accum || n < 0) return fail(JR_ERR_INVALID, "nesterov: bad arguments");
  if (!aligned16(w, grad, accum)) return fail(JR_ERR_INVALID, "nesterov: buffers must be 16-byte aligned");
  if (n == 0) return JR_OK;
  hipLaunchKernelGGL(k_nesterov, update_grid(n >> 2), dim3(256), 0, as_stream(stream), w, grad, accum, n, lr,
                     momentum, grad_scale);
  return check_launch("nesterov");
}

JR_API int jr_momentum_update(float* w, const float* grad, float* accum, int64_t n, float lr, float momentum,
                              float grad_scale, void* stream) {
  if (!w || !grad || !accum || n < 0) return fail(JR_ERR_INVALID, "momentum: bad arguments");
  if (n == 0) return JR_OK;
  hipLaunchKernelGGL(k_momentum, update_grid(aligned16(w, grad, accum) ? n >> 2 : n), dim3(256), 0, as_stream(stream),
                     w, grad, accum, n, lr, momentum, grad_scale);
  return check_launch("momentum");
}

JR_API int jr_sgd_update(float* w, const float* grad, int64_t n, float lr, float grad_scale, void* stream) {
  if (!w || !grad || n < 0) return fail(JR_ERR_INVALID, "sgd: bad arguments");
  if (n == 0) return JR_OK;
  hipLaunchKernelGGL(k_sgd, update_grid(aligned16(w, grad) ? n >> 2 : n), dim3(256), 0, as_stream(stream), w, grad, n,
                     lr, grad_scale);
  return check_launch("sgd");
}

JR_API int jr_adam_update(float* w, const float* grad, float* m, float* v, int64_t n, float lr_t, float beta1,
                          float beta2, float eps, float grad_scale, void* stream) {
  if (!w || !grad || !m || !v || n < 0) return fail(JR_ERR_INVALID, "adam: bad arguments");
  if (n == 0) return JR_OK;
  hipLaunchKernelGGL(k_adam, update_grid(aligned16(w, grad, m, v) ? n >> 2 : n), dim3(256), 0, as_stream(stream), w,
                     grad, m, v, n, lr_t, beta1, beta2, eps, grad_scale);
  return check_launch("adam");
}

JR_API int jr_nesterov_update_ex(float* w, const float* grad, float* accum, int64_t n, float momentum,
                                 const jr_opt_range* ranges, int32_t nranges, const jr_opt_hyper* hyper,
                                 const jr_opt_step* step, void* stream) {
  return launch_update_ex("nesterov_ex", kNesterov, w, grad, accum, nullptr, n, momentum, 0.f, 0.f, ranges, nranges,
                          hyper, step, stream);
}

JR_API int jr_momentum_update_ex(float* w, const float* grad, float* accum, int64_t n, float momentum,
                                 const jr_opt_range* ranges, int32_t nranges, const jr_opt_hyper* hyper,
                                 const jr_opt_step* step, void* stream) {
  return launch_update_ex("momentum_ex", kMomentum, w, grad, accum, nullptr, n, momentum, 0.f, 0.f, ranges, nranges,
                          hyper, step, stream);
}

JR_API int jr_sgd_update_ex(float* w, const float* grad, int64_t n, const jr_opt_range* ranges, int32_t nranges,
                            const jr_opt_hyper* hyper, const jr_opt_step* step, void* stream) {
  return launch_update_ex("sgd_ex", kSgd, w, grad, nullptr, nullptr, n, 0.f, 0.f, 0.f, ranges, nranges, hyper, step,
                          stream);
}

JR_API int jr_adam_update_ex(float* w, const float* grad, float* m, float* v, int64_t n, float beta1, float beta2,
                             float eps, const jr_opt_range* ranges, int32_t nranges, const jr_opt_hyper* hyper,
                             const jr_opt_step* step, void* stream) {
  return launch_update_ex("adam_ex", kAdam, w, grad, m, v, n, beta1, beta2, eps, ranges, nranges, hyper, step, stream);
}

JR_API int jr_rmsprop_update(float* w, const float* grad, float* mom, float* ms, int64_t n, float lr, float rho,
                             float momentum, float eps, float grad_scale, void* stream) {
  if (!w || !grad || !mom || !ms || n < 0) return fail(JR_ERR_INVALID, "rmsprop: bad arguments");
  if (n == 0) return JR_OK;
  hipLaunchKernelGGL(k_rmsprop, update_grid(aligned16(w, grad, mom, ms) ? n >> 2 : n), dim3(256), 0,
                     as_stream(stream), w, grad, mom, ms, n, lr, rho, momentum, eps, grad_scale);
  return check_launch("rmsprop");
}

JR_API int jr_rmsprop_update_ex(float* w, const float* grad, float* mom, float* ms, int64_t n, float rho,
                                float momentum, float eps, const jr_opt_range* ranges, int32_t nranges,
                                const jr_opt_hyper* hyper, const jr_opt_step* step, void* stream) {
  return launch_update_ex("rmsprop_ex", kRmsprop, w, grad, mom, ms, n, rho, momentum, eps, ranges, nranges, hyper,
                          step, stream);
}

JR_API int jr_ema_set(jr_ema_state* state, float decay, uint32_t warm, uint32_t updates, void* stream) {
  if (!state || ((uintptr_t)state & 3) || !(decay >= 0.f && decay < 1.f))
    return fail(JR_ERR_INVALID, "ema_set: bad arguments");
  hipLaunchKernelGGL(k_ema_set, dim3(1), dim3(1), 0, as_stream(stream), state, decay, warm ? 1u : 0u, updates);
  return check_launch("ema_set");
}

JR_API int jr_ema_prepare(jr_ema_state* state, const jr_opt_step* step, void* stream) {
  if (!state || ((uintptr_t)state & 3) || ((uintptr_t)step & 3))
    return fail(JR_ERR_INVALID, "ema_prepare: bad arguments");
  hipLaunchKernelGGL(k_ema_prepare, dim3(1), dim3(1), 0, as_stream(stream), state, step);
  return check_launch("ema_prepare");
}

JR_API int jr_ema_update(float* shadow, const float* w, int64_t n, const jr_ema_state* state, const jr_opt_step* step,
                         void* stream) {
  if (!shadow || !w || !state || n < 0) return fail(JR_ERR_INVALID, "ema_update: bad arguments");
  if (!aligned16(shadow, w)) return fail(JR_ERR_INVALID, "ema_update: buffers must be 16-byte aligned");
  if (((uintptr_t)state & 3) || ((uintptr_t)step & 3))
    return fail(JR_ERR_INVALID, "ema_update: misaligned state or step struct");
  if (n == 0) return JR_OK;
  hipLaunchKernelGGL(k_ema_update, update_grid(n >> 2), dim3(256), 0, as_stream(stream), shadow, w, n, state, step);
  return check_launch("ema_update");
}

JR_API int jr_grad_accumulate(float* dst, const float* src, int64_t n, int first, void* stream) {
  if (!dst || !src || n <= 0) return fail(JR_ERR_INVALID, "grad_accumulate: bad arguments");
  if (((uintptr_t)dst | (uintptr_t)src) & 3) return fail(JR_ERR_INVALID, "grad_accumulate: misaligned buffers");
  const uintptr_t d0 = (uintptr_t)dst, s0 = (uintptr_t)src, bytes = (uintptr_t)n * 4;
  if (d0 < s0 + bytes && s0 < d0 + bytes) return fail(JR_ERR_INVALID, "grad_accumulate: dst and src overlap");
  hipLaunchKernelGGL(k_grad_accumulate, update_grid(aligned16(dst, src) ? n >> 2 : n), dim3(256), 0, as_stream(stream),
                     dst, src, n, first ? 1 : 0);
  return check_launch("grad_accumulate");
}
