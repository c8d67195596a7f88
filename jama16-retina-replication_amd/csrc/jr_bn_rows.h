// jr_bn_rows.h — the device loops that the BN kernels (jr_bn.hip) and the
// max-pools (jr_pool.hip) share, each written once: the 16-byte channel vector
// and thread layout of the BN passes, the per-element BN + ReLU expressions
// (forward, ReLU-masked gradient, the two backwards), the elementwise row pass,
// the block maximum and bound guard, the 3x3 stride-2 window scan and the
// 2x2-cell backward gather.  The bits of
// everything built from them are pinned by tests/golden/bn_bits.json.
#pragma once
#include "jr_common.h"

namespace jr {

// Pins a loaded vector in registers at this point: hipcc otherwise sinks a
// load into the conditional block of its only use (one wait per row).
__device__ __forceinline__ void pin(uint4& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }

// One 16-byte vector of channels: 4 fp32 or 8 bf16, widened to fp32.
template <typename T> struct Vec;
template <> struct Vec<float> {
  static constexpr int N = 4;
  __device__ static void unpack(uint4 u, float* v) {
    v[0] = __uint_as_float(u.x); v[1] = __uint_as_float(u.y);
    v[2] = __uint_as_float(u.z); v[3] = __uint_as_float(u.w);
  }
  __device__ static void st(float* p, const float* v) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
};
template <> struct Vec<uint16_t> {
  static constexpr int N = 8;
  __device__ static void unpack(uint4 u, float* v) {
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = __uint_as_float(w[i] << 16);
      v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  }
  __device__ static void st(uint16_t* p, const float* v) {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (uint32_t)f2bf(v[2 * i]) | ((uint32_t)f2bf(v[2 * i + 1]) << 16);
    *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  }
};

// Four channels (the pools' vector) as a float4.
template <typename T> struct P4;
template <> struct P4<float> {
  __device__ static float4 ld(const float* p) { return *reinterpret_cast<const float4*>(p); }
  __device__ static void st(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
};
template <> struct P4<uint16_t> {
  __device__ static float4 ld(const uint16_t* p) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u),
                       __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
  }
  __device__ static void st(uint16_t* p, float4 v) {
    uint2 u;
    u.x = (uint32_t)f2bf(v.x) | ((uint32_t)f2bf(v.y) << 16);
    u.y = (uint32_t)f2bf(v.z) | ((uint32_t)f2bf(v.w) << 16);
    *reinterpret_cast<uint2*>(p) = u;
  }
};

// ---- per-element BN + ReLU (bn_xhat / bn_pre: jr_common.h) -----------------
// forward: relu(bn_pre)
__device__ __forceinline__ float bn_relu(float x, float mean, float invstd, float beta) {
  return fmaxf(bn_pre(x, mean, invstd, beta), 0.f);
}
// ReluGrad: dy where the forward's pre-activation xhat + beta (bn_pre's
// rounding, so the mask is the forward's bit for bit) is positive, else 0 -- a
// select, whatever dy holds.  Every backward kernel and both reduces use this.
__device__ __forceinline__ float relu_grad(float xhat, float beta, float dy) {
  return __fadd_rn(xhat, beta) > 0.f ? dy : 0.f;
}
// backward under batch statistics (k1 = mean dy', k2 = mean dy' xhat)
__device__ __forceinline__ float bn_bwd_batch(float xhat, float g, float invstd, float k1, float k2) {
  return invstd * (g - k1 - xhat * k2);
}
// backward under frozen statistics: BN is affine
__device__ __forceinline__ float bn_bwd_frozen(float g, float invstd) { return __fmul_rn(g, invstd); }

// ---- thread layout and per-channel constants of the BN passes --------------
// A row of c channels is tpr = c / VW threads (one vector group q each); a
// 256-thread block covers rpp = 256 / tpr rows per pass (row phase rr; threads
// with rr >= rpp idle).  No index division in the loops.
struct RowLane {
  int tpr, rpp, q, rr;
  // the thread's first row in block bx of an elementwise pass (kAppUnroll rows per thread)
  __device__ int64_t block_row(int bx) const { return (int64_t)bx * rpp * kAppUnroll + rr; }
};
template <typename T> __device__ __forceinline__ RowLane row_lane(int c) {
  RowLane l;
  l.tpr = c / Vec<T>::N;
  l.rpp = 256 / l.tpr;
  l.q = threadIdx.x % l.tpr;
  l.rr = threadIdx.x / l.tpr;
  return l;
}

// mean / invstd / beta of a thread's VW channels (pointers at its first one)
template <int VW> struct BnConst {
  float mu[VW], is[VW], be[VW];
};
template <int VW>
__device__ __forceinline__ BnConst<VW> bn_const(const float* mean, const float* invstd, const float* beta) {
  BnConst<VW> k;
#pragma unroll
  for (int j = 0; j < VW; ++j) {
    k.mu[j] = mean[j]; k.is[j] = invstd[j]; k.be[j] = beta[j];
  }
  return k;
}

// the segment (BnSegs / ApplySegs) that holds channel ch
template <typename Segs> __device__ __forceinline__ int seg_of(const Segs& sg, int ch) {
  int s = 0;
#pragma unroll
  for (int i = 1; i < kMaxSegs; ++i) s += (i < sg.n && ch >= sg.c0[i]) ? 1 : 0;
  return s;
}
// a backward thread's upstream gradient (at its first channel ch) and beta
template <typename T> struct SegGrad {
  const T* dy;
  int stride;
  const float* beta;
};
template <typename T> __device__ __forceinline__ SegGrad<T> seg_grad(const BnSegs& sg, int ch) {
  const int s = seg_of(sg, ch), lc = ch - sg.c0[s];
  return {static_cast<const T*>(sg.dy[s]) + sg.dy_off[s] + lc, sg.dy_stride[s], sg.beta[s] + lc};
}

// ---- the elementwise row pass ---------------------------------------------
// One thread's kAppUnroll rows rb, rb + rpp, ... below `end` of one operand
// (x) or two (x and g; TWO), pointers at the thread's first channel:
// o[j] = f(j, x[j], g[j]) stored at y; returns max |o| (unused: eliminated).
// A block kernel calls it once with rb = RowLane::block_row and end = m; a
// folded kernel steps rb by rpp * kAppUnroll over its rows [r0, r1).
//
// Every row's load is unconditional (rows past `end` re-read row end - 1), and
// all are pinned before the first unpack: a load under `if (r < end)` whose
// bf16 unpack sat in the same branch made hipcc wait for each row in turn, and
// without the pins it sinks each load to its use, behind a vmcnt(0) -- a
// memory round trip per row.
template <typename T, bool TWO, typename F>
__device__ __forceinline__ float row_pass(const T* __restrict__ x, int xs, const T* __restrict__ g, int gs, T* y,
                                          int ys, int64_t rb, int rpp, int64_t end, F f) {
  constexpr int VW = Vec<T>::N;
  uint4 xr[kAppUnroll], gr[kAppUnroll];
#pragma unroll
  for (int u = 0; u < kAppUnroll; ++u) {
    const int64_t r = min(rb + (int64_t)u * rpp, end - 1);
    xr[u] = *reinterpret_cast<const uint4*>(x + r * xs);
    if (TWO) gr[u] = *reinterpret_cast<const uint4*>(g + r * gs);
  }
#pragma unroll
  for (int u = 0; u < kAppUnroll; ++u) {
    pin(xr[u]);
    if (TWO) pin(gr[u]);
  }
  float amax = 0.f;
#pragma unroll
  for (int u = 0; u < kAppUnroll; ++u) {
    const int64_t r = rb + (int64_t)u * rpp;
    if (r >= end) break;
    float xv[VW], gv[VW], o[VW];
    Vec<T>::unpack(xr[u], xv);
    if (TWO) Vec<T>::unpack(gr[u], gv);
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      o[j] = f(j, xv[j], TWO ? gv[j] : 0.f);
      amax = fmaxf(amax, fabsf(o[j]));
    }
    Vec<T>::st(y + r * ys, o);
  }
  return amax;
}

// ---- block maximum and the bound guard -------------------------------------
// The block's max of v (every value >= 0; fmaxf drops a NaN), valid in thread
// 0.  Every thread of the block calls it, once per kernel.
__device__ __forceinline__ float block_max(float v) {
  __shared__ float s_max[4];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = v;
  __syncthreads();
  float b = 0.f;
  if (threadIdx.x == 0) {
    b = s_max[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) b = fmaxf(b, s_max[w]);
  }
  return b;
}
// The guard of the *_guard entry points (jr.h): v is the largest magnitude the
// thread stored; a block whose largest is not <= limit counts one failure into
// the device error word (the predicate of k_absmax_segs: +inf trips it, a NaN
// the fmaxf dropped does not).  Every thread of the block calls it.
__device__ __forceinline__ void block_guard(float v, float limit, unsigned* err) {
  const float b = block_max(v);
  if (threadIdx.x == 0 && !(b <= limit)) atomicAdd(err, 1u);
}

// ---- max-pool 3x3 stride 2 'valid' ------------------------------------------
// Forward: a grid-stride loop (elements first, first + step, ...: the kernel
// reads its own block and grid size) over (output pixel, channel quad); each
// window is scanned in (r, c) order and the first maximum wins (argmax 0..8).
// taps(b, q) returns the per-tap transform a = tap(j, v) of image b's channel
// quad q: the identity for the plain pool, BN + ReLU + rounding to the path
// dtype for the fused one.  Returns the largest |y| this thread stored (0 if
// none; unused: eliminated).
template <typename T, typename Taps>
__device__ __forceinline__ float maxpool_scan(const jr_pool_desc& d, const T* __restrict__ x, T* y, uint8_t* argmax,
                                             int first, int step, Taps taps) {
  const int c4 = d.c >> 2;
  const int total = d.n * d.ho * d.wo * c4;
  float amax = 0.f;
  for (int e = first; e < total; e += step) {
    const int q = e % c4;
    const int pix = e / c4;
    const int ow = pix % d.wo;
    const int t = pix / d.wo;
    const int oh = t % d.ho;
    const int b = t / d.ho;
    const auto tap = taps(b, q);
    float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int arg[4] = {0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int ih = oh * 2 + r, iw = ow * 2 + c;
        const float4 v = P4<T>::ld(x + ((int64_t)(b * d.h + ih) * d.w + iw) * d.x_c_stride + d.x_c_off + q * 4);
        const float va[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float a = tap(j, va[j]);
          if (a > best[j] || (r == 0 && c == 0)) { best[j] = a; arg[j] = r * 3 + c; }
        }
      }
    }
    P4<T>::st(y + (int64_t)pix * d.y_c_stride + d.y_c_off + q * 4, make_float4(best[0], best[1], best[2], best[3]));
#pragma unroll
    for (int j = 0; j < 4; ++j) amax = fmaxf(amax, fabsf(best[j]));
    if (argmax) {
      const uint32_t packed = (uint32_t)arg[0] | ((uint32_t)arg[1] << 8) | ((uint32_t)arg[2] << 16) |
                              ((uint32_t)arg[3] << 24);
      *reinterpret_cast<uint32_t*>(argmax + (int64_t)pix * d.c + q * 4) = packed;
    }
  }
  return amax;
}

// Backward as a gather over 2x2 input cells: input rows 2a, 2a+1 and columns
// 2b, 2b+1 are covered only by the windows oh in {a-1, a}, ow in {b-1, b}, so
// one thread loads those (at most) four windows' dy and argmax once and hands
// the gradient of each in-bounds input pixel of its cell to sink(b, ih, iw, g) --
// one dy/argmax load per output pixel instead of the 2.25 of a thread per
// input pixel.  Each input pixel sums its windows from +0 in (oh, ow)
// ascending order.  cell: flat (image, cell row, cell column); q: channel quad.
template <typename T, typename Sink>
__device__ __forceinline__ void maxpool_bwd_cell(const jr_pool_desc& d, const uint8_t* __restrict__ argmax,
                                                 const T* __restrict__ dy, int cell, int q, Sink sink) {
  const int hc = (d.h + 1) >> 1, wc = (d.w + 1) >> 1;
  const int cb = cell % wc;
  const int t = cell / wc;
  const int ca = t % hc;
  const int b = t / hc;
  uint32_t am[2][2];
  float4 g[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int oh = ca - 1 + i, ow = cb - 1 + j;
      am[i][j] = 0xffffffffu;                  // position 255: matches no tap
      g[i][j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (oh >= 0 && oh < d.ho && ow >= 0 && ow < d.wo) {
        const int64_t op = ((int64_t)b * d.ho + oh) * d.wo + ow;
        am[i][j] = *reinterpret_cast<const uint32_t*>(argmax + op * d.c + q * 4);
        g[i][j] = P4<T>::ld(dy + op * d.y_c_stride + d.y_c_off + q * 4);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int ih = 2 * ca + u, iw = 2 * cb + v;
      if (ih >= d.h || iw >= d.w) continue;
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int r = u + 2 - 2 * i, c = v + 2 - 2 * j;   // tap of (ih, iw) in window (ca-1+i, cb-1+j)
          if (r > 2 || c > 2) continue;                      // compile-time after unrolling
          const float ga[4] = {g[i][j].x, g[i][j].y, g[i][j].z, g[i][j].w};
#pragma unroll
          for (int l = 0; l < 4; ++l)
            if ((int)((am[i][j] >> (8 * l)) & 0xff) == r * 3 + c) acc[l] += ga[l];
        }
      }
      sink(b, ih, iw, make_float4(acc[0], acc[1], acc[2], acc[3]));
    }
  }
}

}  // namespace jr
