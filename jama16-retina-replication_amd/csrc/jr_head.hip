// jr_head.hip — the classification head and the loss.
//
//   logits = feat . W + b          tf.layers.dense(units)        train.py:133
//   probs  = sigmoid(logits)       tf.sigmoid(name='predictions') train.py:136
//   loss   = mean(max(z,0) - z*y + log1p(exp(-|z|)))             train.py:140-141
//            (tf.nn.sigmoid_cross_entropy_with_logits + reduce_mean)
// Softmax mode (north-star extra): probs = softmax(logits), loss =
// mean_b(-sum_u y log p).  Everything here is a few kB: one workgroup per
// sample for the dense layer, one workgroup for the loss reduction, fixed
// reduction order (deterministic).
//
// The loss recipe (jr.h jr_loss_spec: label smoothing, class weights, a focal
// term) is the kRecipe = true instantiation of the same loss and gradient
// kernels; jr_head_fwd / jr_head_bwd and a neutral spec launch kRecipe = false,
// whose expressions are the ones above, bit for bit.
#include <cmath>

#include "jr_common.h"

namespace jr {

constexpr int kMaxUnits = 16;

__device__ __forceinline__ float warp_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one block (256 threads) per sample b: logits[b][u], probs[b][u]
__global__ void __launch_bounds__(256) k_head_logits(int mode, const float* __restrict__ feat,
                                                     const float* __restrict__ w, const float* __restrict__ bias,
                                                     int c, int units, float* logits, float* probs) {
  __shared__ float red[4][kMaxUnits];
  __shared__ float z[kMaxUnits];
  const int b = blockIdx.x, t = threadIdx.x;
  float acc[kMaxUnits];
#pragma unroll
  for (int u = 0; u < kMaxUnits; ++u) acc[u] = 0.f;
  for (int k = t; k < c; k += 256) {
    const float f = feat[(int64_t)b * c + k];
#pragma unroll
    for (int u = 0; u < kMaxUnits; ++u)
      if (u < units) acc[u] = fmaf(f, w[(int64_t)k * units + u], acc[u]);
  }
#pragma unroll
  for (int u = 0; u < kMaxUnits; ++u) {
    if (u < units) {
      const float s = warp_sum(acc[u]);
      if ((t & 63) == 0) red[t >> 6][u] = s;
    }
  }
  __syncthreads();
  if (t < units) {
    const float s = ((red[0][t] + red[1][t]) + (red[2][t] + red[3][t])) + bias[t];
    z[t] = s;
    logits[(int64_t)b * units + t] = s;
  }
  __syncthreads();
  if (t == 0) {
    if (mode == JR_HEAD_SIGMOID) {
      for (int u = 0; u < units; ++u) probs[(int64_t)b * units + u] = 1.f / (1.f + expf(-z[u]));
    } else {
      float mx = z[0];
      for (int u = 1; u < units; ++u) mx = fmaxf(mx, z[u]);
      float se = 0.f;
      for (int u = 0; u < units; ++u) se += expf(z[u] - mx);
      for (int u = 0; u < units; ++u) probs[(int64_t)b * units + u] = expf(z[u] - mx) / se;
    }
  }
}

// ---- the loss recipe (formulas: jr.h).  Every sigmoid term comes from z:
// e = exp(-|z|) never overflows, p and 1 - p are 1 / (1 + e) and e / (1 + e) by
// the sign of z, sp(z) and sp(-z) share log1p(e).
struct SigTerms {
  float p, q, spz, spn;   // sigmoid(z), sigmoid(-z), sp(z), sp(-z)
};
__device__ __forceinline__ SigTerms sig_terms(float z) {
  const float e = expf(-fabsf(z)), l = log1pf(e), r = 1.f / (1.f + e), er = e * r;
  SigTerms s;
  s.p = z >= 0.f ? r : er;
  s.q = z >= 0.f ? er : r;
  s.spz = fmaxf(z, 0.f) + l;
  s.spn = fmaxf(-z, 0.f) + l;
  return s;
}
__device__ __forceinline__ float focal_pow(float x, float g) { return g == 0.f ? 1.f : powf(x, g); }
__device__ __forceinline__ float smooth(float y, float eps, float share) { return y * (1.f - eps) + eps * share; }

__device__ __forceinline__ float sig_loss(const jr_loss_spec& sp, int u, float z, float y) {
  const SigTerms s = sig_terms(z);
  const float g = sp.focal_gamma, t = smooth(y, sp.label_smoothing, 0.5f);
  return sp.class_weight[u] * t * focal_pow(s.q, g) * s.spn + (1.f - t) * focal_pow(s.p, g) * s.spz;
}
__device__ __forceinline__ float sig_dz(const jr_loss_spec& sp, int u, float z, float y) {
  const SigTerms s = sig_terms(z);
  const float g = sp.focal_gamma, t = smooth(y, sp.label_smoothing, 0.5f);
  return -sp.class_weight[u] * t * focal_pow(s.q, g) * (g * s.p * s.spn + s.q) +
         (1.f - t) * focal_pow(s.p, g) * (g * s.q * s.spz + s.p);
}
// softmax: the sample weight s = sum_u c_u y_u and sum_v t_v of sample row yb
__device__ __forceinline__ void softmax_sums(const jr_loss_spec& sp, const float* yb, int units, float* s, float* st) {
  float a = 0.f, b = 0.f;
  const float share = 1.f / (float)units;
  for (int u = 0; u < units; ++u) {
    a += sp.class_weight[u] * yb[u];
    b += smooth(yb[u], sp.label_smoothing, share);
  }
  *s = a;
  *st = b;
}

// single block: loss = mean over elements (sigmoid) or samples (softmax)
template <bool kRecipe>
__global__ void __launch_bounds__(256) k_head_loss(int mode, const jr_loss_spec spec, const float* __restrict__ logits,
                                                   const float* __restrict__ labels, int n, int units,
                                                   float* loss) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  double s = 0.0;
  if (mode == JR_HEAD_SIGMOID) {
    for (int e = t; e < n * units; e += 256) {
      const float z = logits[e], y = labels[e];
      if constexpr (kRecipe)
        s += (double)sig_loss(spec, e % units, z, y);
      else
        s += (double)(fmaxf(z, 0.f) - z * y + log1pf(expf(-fabsf(z))));
    }
  } else {
    for (int b = t; b < n; b += 256) {
      const float* zb = logits + (int64_t)b * units;
      float mx = zb[0];
      for (int u = 1; u < units; ++u) mx = fmaxf(mx, zb[u]);
      float se = 0.f;
      for (int u = 0; u < units; ++u) se += expf(zb[u] - mx);
      const float lse = mx + logf(se);
      float l = 0.f;
      if constexpr (kRecipe) {
        const float* yb = labels + (int64_t)b * units;
        const float share = 1.f / (float)units;
        float sw, st;
        softmax_sums(spec, yb, units, &sw, &st);
        for (int u = 0; u < units; ++u) l += smooth(yb[u], spec.label_smoothing, share) * (lse - zb[u]);
        l *= sw;
      } else {
        for (int u = 0; u < units; ++u) l += labels[(int64_t)b * units + u] * (lse - zb[u]);
      }
      s += (double)l;
    }
  }
  const double sum = block_sum256(s, red);
  if (t == 0) {
    const double denom = mode == JR_HEAD_SIGMOID ? (double)n * units : (double)n;
    loss[0] = (float)(sum / denom);
  }
}

// dloss / dz[b][u]; kRecipe = false: (p - y) / denom, in that order
template <bool kRecipe>
__device__ __forceinline__ float head_dz(int mode, const jr_loss_spec& spec, const float* logits, const float* probs,
                                         const float* labels, int b, int u, int n, int units) {
  const float p = probs[(int64_t)b * units + u], y = labels[(int64_t)b * units + u];
  const float denom = mode == JR_HEAD_SIGMOID ? (float)n * (float)units : (float)n;
  if constexpr (kRecipe) {
    if (mode == JR_HEAD_SIGMOID) return sig_dz(spec, u, logits[(int64_t)b * units + u], y) / denom;
    float sw, st;
    softmax_sums(spec, labels + (int64_t)b * units, units, &sw, &st);
    return sw * (p * st - smooth(y, spec.label_smoothing, 1.f / (float)units)) / denom;
  }
  return (p - y) / denom;
}

// dfeat[b][k] = sum_u dz[b][u] * W[k][u]
template <bool kRecipe>
__global__ void k_head_dfeat(int mode, const jr_loss_spec spec, const float* __restrict__ logits,
                             const float* __restrict__ w, const float* __restrict__ probs,
                             const float* __restrict__ labels, int n, int c, int units, float* dfeat) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)n * c) return;
  const int b = (int)(e / c), k = (int)(e - (int64_t)b * c);
  float s = 0.f;
  for (int u = 0; u < units; ++u)
    s = fmaf(head_dz<kRecipe>(mode, spec, logits, probs, labels, b, u, n, units), w[(int64_t)k * units + u], s);
  dfeat[e] = s;
}

// dW[k][u] = sum_b feat[b][k] dz[b][u];  db[u] = sum_b dz[b][u]
template <bool kRecipe>
__global__ void k_head_dw(int mode, const jr_loss_spec spec, const float* __restrict__ logits,
                          const float* __restrict__ feat, const float* __restrict__ probs,
                          const float* __restrict__ labels, int n, int c, int units, float* dw, float* db) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < (int64_t)c * units) {
    const int k = (int)(e / units), u = (int)(e - (int64_t)k * units);
    float s = 0.f;
    for (int b = 0; b < n; ++b)
      s = fmaf(feat[(int64_t)b * c + k], head_dz<kRecipe>(mode, spec, logits, probs, labels, b, u, n, units), s);
    dw[e] = s;
  }
  if (e < units) {
    float s = 0.f;
    for (int b = 0; b < n; ++b) s += head_dz<kRecipe>(mode, spec, logits, probs, labels, b, (int)e, n, units);
    db[e] = s;
  }
}

// dfeat[b][k] = W[k][t_b]: the gradient of logit t_b of sample b (no loss, no
// 1/n); a target outside [0, units) gives a row of zeros and forms no address
__global__ void k_head_logit_bwd(const float* __restrict__ w, const int32_t* __restrict__ target, int n, int c,
                                 int units, float* dfeat) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)n * c) return;
  const int b = (int)(e / c), k = (int)(e - (int64_t)b * c);
  const int t = target ? target[b] : 0;
  dfeat[e] = (t >= 0 && t < units) ? w[(int64_t)k * units + t] : 0.f;
}

}  // namespace jr

using namespace jr;

JR_API int jr_head_logit_bwd(const float* w, const int32_t* target, int32_t n, int32_t c, int32_t units, float* dfeat,
                             void* stream) {
  if (!w || !dfeat) return fail(JR_ERR_INVALID, "head_logit_bwd: null pointer");
  if (n <= 0 || c <= 0 || units <= 0 || units > kMaxUnits) return fail(JR_ERR_INVALID, "head_logit_bwd: bad sizes");
  hipLaunchKernelGGL(k_head_logit_bwd, dim3((int)ceil_div((int64_t)n * c, 256)), dim3(256), 0, as_stream(stream), w,
                     target, n, c, units, dfeat);
  return check_launch("head_logit_bwd");
}

// The spec of a launch: *spec checked (jr.h), or the neutral one for NULL.
// recipe: false when it changes nothing (the kRecipe = false kernels).
static int loss_spec(const char* what, int mode, const jr_loss_spec* spec, int units, jr_loss_spec* out, bool* recipe) {
  *out = jr_loss_spec{};
  for (int u = 0; u < kMaxUnits; ++u) out->class_weight[u] = 1.f;
  *recipe = false;
  if (!spec) return JR_OK;
  const float e = spec->label_smoothing, g = spec->focal_gamma;
  if (!(e >= 0.f && e < 1.f)) return fail(JR_ERR_INVALID, std::string(what) + ": label_smoothing outside [0, 1)");
  if (!(g >= 0.f && std::isfinite(g))) return fail(JR_ERR_INVALID, std::string(what) + ": focal_gamma must be finite and >= 0");
  if (mode == JR_HEAD_SOFTMAX && g != 0.f) return fail(JR_ERR_INVALID, std::string(what) + ": focal_gamma is sigmoid-only");
  out->label_smoothing = e;
  out->focal_gamma = g;
  bool neutral = e == 0.f && g == 0.f;
  for (int u = 0; u < units; ++u) {
    const float c = spec->class_weight[u];
    if (!(c > 0.f && std::isfinite(c))) return fail(JR_ERR_INVALID, std::string(what) + ": class_weight must be finite and > 0");
    out->class_weight[u] = c;
    neutral = neutral && c == 1.f;
  }
  *recipe = !neutral;
  return JR_OK;
}

static int head_fwd(const char* what, int mode, const jr_loss_spec* spec, const float* feat, const float* w,
                    const float* b, const float* labels, int32_t n, int32_t c, int32_t units, float* logits,
                    float* probs, float* loss, void* stream) {
  const std::string W(what);
  if (mode != JR_HEAD_SIGMOID && mode != JR_HEAD_SOFTMAX) return fail(JR_ERR_INVALID, W + ": bad mode");
  if (!feat || !w || !b || !logits || !probs) return fail(JR_ERR_INVALID, W + ": null pointer");
  if (n <= 0 || c <= 0 || units <= 0 || units > kMaxUnits) return fail(JR_ERR_INVALID, W + ": bad sizes");
  jr_loss_spec sp;
  bool recipe;
  int rc = loss_spec(what, mode, spec, units, &sp, &recipe);
  if (rc) return rc;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(k_head_logits, dim3(n), dim3(256), 0, s, mode, feat, w, b, c, units, logits, probs);
  rc = check_launch((W + " logits").c_str());
  if (rc) return rc;
  if (labels && loss) {
    if (recipe)
      hipLaunchKernelGGL(k_head_loss<true>, dim3(1), dim3(256), 0, s, mode, sp, (const float*)logits, labels, n, units,
                         loss);
    else
      hipLaunchKernelGGL(k_head_loss<false>, dim3(1), dim3(256), 0, s, mode, sp, (const float*)logits, labels, n, units,
                         loss);
    rc = check_launch((W + " loss").c_str());
  }
  return rc;
}

// logits: read by the recipe alone (the plain call passes none)
static int head_bwd(const char* what, int mode, const jr_loss_spec* spec, const float* logits, const float* feat,
                    const float* w, const float* probs, const float* labels, int32_t n, int32_t c, int32_t units,
                    float* dfeat, float* dw, float* db, void* stream) {
  const std::string W(what);
  if (mode != JR_HEAD_SIGMOID && mode != JR_HEAD_SOFTMAX) return fail(JR_ERR_INVALID, W + ": bad mode");
  if (!feat || !w || !probs || !labels || !dfeat || !dw || !db) return fail(JR_ERR_INVALID, W + ": null pointer");
  if (n <= 0 || c <= 0 || units <= 0 || units > kMaxUnits) return fail(JR_ERR_INVALID, W + ": bad sizes");
  jr_loss_spec sp;
  bool recipe;
  int rc = loss_spec(what, mode, spec, units, &sp, &recipe);
  if (rc) return rc;
  hipStream_t s = as_stream(stream);
  const dim3 gf((int)ceil_div((int64_t)n * c, 256)), gw((int)ceil_div((int64_t)c * units, 256));
  if (recipe)
    hipLaunchKernelGGL(k_head_dfeat<true>, gf, dim3(256), 0, s, mode, sp, logits, w, probs, labels, n, c, units, dfeat);
  else
    hipLaunchKernelGGL(k_head_dfeat<false>, gf, dim3(256), 0, s, mode, sp, logits, w, probs, labels, n, c, units, dfeat);
  rc = check_launch((W + " dfeat").c_str());
  if (rc) return rc;
  if (recipe)
    hipLaunchKernelGGL(k_head_dw<true>, gw, dim3(256), 0, s, mode, sp, logits, feat, probs, labels, n, c, units, dw, db);
  else
    hipLaunchKernelGGL(k_head_dw<false>, gw, dim3(256), 0, s, mode, sp, logits, feat, probs, labels, n, c, units, dw, db);
  return check_launch((W + " dw").c_str());
}

JR_API int jr_head_fwd(int mode, const float* feat, const float* w, const float* b, const float* labels,
                       int32_t n, int32_t c, int32_t units, float* logits, float* probs, float* loss,
                       void* stream) {
  return head_fwd("head_fwd", mode, nullptr, feat, w, b, labels, n, c, units, logits, probs, loss, stream);
}

JR_API int jr_head_fwd_ex(int mode, const jr_loss_spec* spec, const float* feat, const float* w, const float* b,
                          const float* labels, int32_t n, int32_t c, int32_t units, float* logits, float* probs,
                          float* loss, void* stream) {
  return head_fwd("head_fwd_ex", mode, spec, feat, w, b, labels, n, c, units, logits, probs, loss, stream);
}

JR_API int jr_head_bwd(int mode, const float* feat, const float* w, const float* probs, const float* labels,
                       int32_t n, int32_t c, int32_t units, float* dfeat, float* dw, float* db, void* stream) {
  return head_bwd("head_bwd", mode, nullptr, nullptr, feat, w, probs, labels, n, c, units, dfeat, dw, db, stream);
}

JR_API int jr_head_bwd_ex(int mode, const jr_loss_spec* spec, const float* logits, const float* feat, const float* w,
                          const float* probs, const float* labels, int32_t n, int32_t c, int32_t units, float* dfeat,
                          float* dw, float* db, void* stream) {
  if (!logits) return fail(JR_ERR_INVALID, "head_bwd_ex: null pointer");
  return head_bwd("head_bwd_ex", mode, spec, logits, feat, w, probs, labels, n, c, units, dfeat, dw, db, stream);
}
