// jr_bn.hip — BatchNormalization(axis=-1, scale=False, eps) + ReLU in
// training mode, forward and backward.
//
// Replaces the FusedBatchNorm / Relu / FusedBatchNormGrad / ReluGrad TF ops of
// every Keras conv2d_bn block built at train.py:129-130.
// The reference graph is built with set_learning_phase(True) (train.py:101),
// so batch statistics are used in training AND evaluation (App. C Q1).
//
//   fwd:  mean = E[x], var = E[(x-mean)^2] (biased), invstd = 1/sqrt(var+eps)
//         y = max((x - mean) * invstd + beta, 0)
//   bwd:  dy' = dy * (y > 0)            (ReluGrad)
//         dbeta = sum dy'
//         dx = invstd * (dy' - mean(dy') - xhat * mean(dy' * xhat))
//
// All passes are HBM-streaming: every thread moves one 16-byte vector per
// row (4 fp32 or 8 bf16 channels) and keeps several rows in flight.
// Reductions are per-chunk partial sums in fp64 combined in a fixed chunk
// order (deterministic, no atomics).
//
// This file holds the kernels and their launchers.  Every launch decision --
// chunk geometry, grids, workspace layout, argument validation, the tunable
// constants and the kernel-argument structs -- is host-only code in
// jr_bn_plan.h / jr_bn_plan.cpp.
#include "jr_bn_rows.h"

namespace jr {

#ifndef JR_BN_BWD_ROWS
#define JR_BN_BWD_ROWS 8
#endif
#ifndef JR_BN_F32_SELECT
#define JR_BN_F32_SELECT 0
#endif
constexpr bool kF32Select = JR_BN_F32_SELECT;  // (diagnostic) fp32 reduce loads in the select form
// rows in flight per thread in the reductions (16 B per row and operand)
template <int MODE> constexpr int red_rows() { return MODE == 0 ? 16 : JR_BN_BWD_ROWS; }

// (pin, Vec, the thread layout, seg_of, the per-element expressions and the
// elementwise row pass: jr_bn_rows.h)

// Per-chunk column sums.  MODE 0: (sum x, sum x^2).  MODE 1 (bwd):
// (sum dy', sum dy'*xhat).  Per-thread fp64 sums over a fixed row set,
// fixed-order block combine: deterministic.  bf16 MODE 1 sums each batch of
// U rows in fp32 (fma for dy'*xhat) and adds the batch sums in fp64: the
// per-element fp64 conversions and adds of 8 channels per thread had made
// the bf16 reduce VALU-bound (bf16 step 11.22 -> 10.84 ms, interleaved A/B
// on one box; per-shape bnbench 2.65 -> 2.16 ms).  fp32 (4 channels per
// thread) gained 0.3 % from the same change and keeps per-element fp64 sums:
// its 100-step loss-curve fixture is a chaotic trajectory that any change
// of summation order moves past the per-step bar.  Loads stay packed (one uint4
// per row and operand) until used, so red_rows<MODE>() rows are in flight
// per thread: the loop is latency-bound, not bandwidth-bound, with fewer.
// Partials: part[2][c][nchunks] (fp64, chunk-contiguous for the finalize).
// (body: chunk bx of nch; k_bn_reduce runs chunk blockIdx.x of gridDim.x,
// k_bn_reduce_batch a layer's chunk of a batched launch)
template <int MODE, typename T>
__device__ __forceinline__ void bn_reduce_body(const T* __restrict__ x, int xs, const BnSegs& sg, int64_t m, int c,
                                               int rows_per_chunk, const float* __restrict__ mean,
                                               const float* __restrict__ invstd, double* part, int bx, int64_t nch) {
  constexpr int VW = Vec<T>::N;
  constexpr int U = red_rows<MODE>();
  __shared__ double red[256 * 2 * VW];
  const int tpr = c / VW;
  const int rpp = 256 / tpr;
  const int t = threadIdx.x;
  const int q = t % tpr, rr = t / tpr;
  const int64_t r0 = (int64_t)bx * rows_per_chunk;
  const int64_t r1 = min(m, r0 + rows_per_chunk);
  double s0[VW], s1[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) s0[j] = s1[j] = 0.0;
  constexpr bool kBatch32 = sizeof(T) == 2;   // bf16: fp32 sums of one batch of U rows
  float f0[VW], f1[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) f0[j] = f1[j] = 0.f;
  if (rr < rpp) {
    float mu[VW], is[VW], be[VW];
    const T* gp = nullptr;
    int dy_stride = 0;
    if (MODE == 1) {
      const int sgi = seg_of(sg, q * VW), lc = q * VW - sg.c0[sgi];
      gp = static_cast<const T*>(sg.dy[sgi]) + sg.dy_off[sgi] + lc;
      dy_stride = sg.dy_stride[sgi];
#pragma unroll
      for (int j = 0; j < VW; ++j) {
        mu[j] = mean[q * VW + j]; is[j] = invstd[q * VW + j]; be[j] = sg.beta[sgi][lc + j];
      }
    }
    const T* xp = x + q * VW;
    for (int64_t r = r0 + rr; r < r1; r += (int64_t)rpp * U) {
      uint4 xr[U], gr[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        // Rows past the chunk add zero bits (= 0.0 in both dtypes): load the
        // chunk's last row (always valid) and zero after the load.  The
        // select form (JR_BN_F32_SELECT, the fp32 default before the pins
        // below) compiles to a FLAT load from a select of the row address
        // and a scratch copy of the zero constant, a branch and a wait per row.
        const int64_t ri = r + (int64_t)u * rpp;
        const uint4 z = make_uint4(0, 0, 0, 0);
        if constexpr (sizeof(T) == 4 && kF32Select) {
          xr[u] = ri < r1 ? *reinterpret_cast<const uint4*>(xp + ri * xs) : z;
          if (MODE == 1) gr[u] = ri < r1 ? *reinterpret_cast<const uint4*>(gp + ri * dy_stride) : z;
        } else {
          const bool in = ri < r1;
          const int64_t rc = in ? ri : r1 - 1;
          const uint4 xv = *reinterpret_cast<const uint4*>(xp + rc * xs);
          xr[u] = in ? xv : z;
          if (MODE == 1) {
            const uint4 gv = *reinterpret_cast<const uint4*>(gp + rc * dy_stride);
            gr[u] = in ? gv : z;
          }
        }
      }
      // all 2U loads in flight before the first use: without the pins hipcc
      // issued half of them one at a time, each behind vmcnt(0) (a memory
      // round trip per row: the 17^2 / 8^2 reduces took 14-16 us)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        pin(xr[u]);
        if (MODE == 1) pin(gr[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float xv[VW];
        Vec<T>::unpack(xr[u], xv);
        if (MODE == 0) {
#pragma unroll
          for (int j = 0; j < VW; ++j) {
            const double d = xv[j];
            s0[j] += d;
            s1[j] += d * d;
          }
        } else {
          float gv[VW];
          Vec<T>::unpack(gr[u], gv);
#pragma unroll
          for (int j = 0; j < VW; ++j) {
            const float xh = bn_xhat(xv[j], mu[j], is[j]);
            const float g = relu_grad(xh, be[j], gv[j]);
            if constexpr (kBatch32) {
              f0[j] += g;
              f1[j] = fmaf(g, xh, f1[j]);
            } else {
              s0[j] += (double)g;
              s1[j] += (double)g * (double)xh;
            }
          }
        }
      }
      if (MODE == 1 && kBatch32) {
#pragma unroll
        for (int j = 0; j < VW; ++j) {
          s0[j] += (double)f0[j];
          s1[j] += (double)f1[j];
          f0[j] = f1[j] = 0.f;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < VW; ++j) {
    red[t * 2 * VW + j] = s0[j];
    red[t * 2 * VW + VW + j] = s1[j];
  }
  __syncthreads();
  // fixed-shape tree over the row phases (log2(rpp) steps, deterministic)
  int span = 1;
  while (span < rpp) span <<= 1;
  for (int s = span >> 1; s > 0; s >>= 1) {
    if (rr < s && rr + s < rpp) {
      double* a = red + t * 2 * VW;
      const double* b = red + (t + s * tpr) * 2 * VW;
#pragma unroll
      for (int j = 0; j < 2 * VW; ++j) a[j] += b[j];
    }
    __syncthreads();
  }
  if (t < tpr) {
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      part[(int64_t)(q * VW + j) * nch + bx] = red[t * 2 * VW + j];
      part[(int64_t)(c + q * VW + j) * nch + bx] = red[t * 2 * VW + VW + j];
    }
  }
}

template <int MODE, typename T>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2)))
k_bn_reduce(const T* __restrict__ x, int xs, BnSegs sg, int64_t m, int c, int rows_per_chunk,
            const float* __restrict__ mean, const float* __restrict__ invstd, double* part) {
  bn_reduce_body<MODE, T>(x, xs, sg, m, c, rows_per_chunk, mean, invstd, part, blockIdx.x, gridDim.x);
}

// Fixed-order combine of the chunk partials: one wave per channel; lane j
// sums chunks j, j+64, ... (coalesced, eight loads in flight), then a fixed
// xor-butterfly adds the 64 lane sums (deterministic, independent of timing).
// MODE 0: mean, invstd.   MODE 1: k1 = sum dy'/m, k2 = sum dy'xhat/m, dbeta.
template <int MODE>
__global__ void __launch_bounds__(256) k_bn_finalize(const double* __restrict__ part, int nchunks, int c,
                                                     int64_t m, float eps, float* out0, float* out1, BnSegs sg) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= c) return;   // wave-uniform
  const double* p0 = part + (int64_t)k * nchunks;
  const double* p1 = part + (int64_t)(c + k) * nchunks;
  double a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
  for (int i0 = 0; i0 < nchunks; i0 += 256) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * 64 + lane;
      if (i < nchunks) { a[u] += p0[i]; b[u] += p1[i]; }
    }
  }
  double s0 = (a[0] + a[1]) + (a[2] + a[3]), s1 = (b[0] + b[1]) + (b[2] + b[3]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s0 += __shfl_xor(s0, o, 64);
    s1 += __shfl_xor(s1, o, 64);
  }
  if (lane != 0) return;
  const double inv_m = 1.0 / (double)m;
  if (MODE == 0) {
    const double mu = s0 * inv_m;
    double var = s1 * inv_m - mu * mu;
    if (var < 0) var = 0;
    out0[k] = (float)mu;
    out1[k] = (float)(1.0 / sqrt(var + (double)eps));
  } else {
    out0[k] = (float)(s0 * inv_m);
    out1[k] = (float)(s1 * inv_m);
    const int sgi = seg_of(sg, k);
    sg.dbeta[sgi][k - sg.c0[sgi]] = (float)s0;
  }
}

// Elementwise passes: block b covers rows [b*rpp*U, (b+1)*rpp*U), thread
// (q, rr) rows rr, rr+rpp, ...; per-channel constants loaded once; the rows
// themselves: row_pass (jr_bn_rows.h).
// Grouped (ensemble members, blockIdx.y = member): x, y, the statistics and
// beta move by their member strides (bytes; all 0 for an ordinary launch).
// GUARD (the *_guard entry points): the same pass, then block_guard over the
// largest magnitude the block stored -- guarded_relu is the stored value, so
// y is bit for bit the unguarded kernel's; idle threads stay for the block
// reduction with 0.
template <typename T> __device__ __forceinline__ float guarded_relu(float a) {
  return sizeof(T) == 2 ? bf2f(f2bf(a)) : a;   // (bf16: what Vec::st stores; rounding it again is the identity)
}

template <typename T, bool GUARD>
__global__ void __launch_bounds__(256) k_bn_relu_apply(const T* __restrict__ x, int xs, int64_t m, int c,
                                                       const float* __restrict__ mean,
                                                       const float* __restrict__ invstd,
                                                       const float* __restrict__ beta, T* y, int y_off,
                                                       int y_stride, int64_t x_mb, int64_t y_mb, int64_t st_mb,
                                                       int64_t be_mb, float limit, unsigned* err) {
  if (gridDim.y > 1) {
    const int64_t mb = blockIdx.y;
    x = reinterpret_cast<const T*>(reinterpret_cast<const char*>(x) + mb * x_mb);
    y = reinterpret_cast<T*>(reinterpret_cast<char*>(y) + mb * y_mb);
    mean = reinterpret_cast<const float*>(reinterpret_cast<const char*>(mean) + mb * st_mb);
    invstd = reinterpret_cast<const float*>(reinterpret_cast<const char*>(invstd) + mb * st_mb);
    beta = reinterpret_cast<const float*>(reinterpret_cast<const char*>(beta) + mb * be_mb);
  }
  constexpr int VW = Vec<T>::N;
  const RowLane l = row_lane<T>(c);
  const bool idle = l.rr >= l.rpp;
  if (!GUARD && idle) return;
  float amax = 0.f;
  if (!idle) {
    const int ch = l.q * VW;
    const BnConst<VW> k = bn_const<VW>(mean + ch, invstd + ch, beta + ch);
    amax = row_pass<T, false>(x + ch, xs, nullptr, 0, y + y_off + ch, y_stride, l.block_row(blockIdx.x), l.rpp, m,
                              [=](int j, float xv, float) {
                                const float a = bn_relu(xv, k.mu[j], k.is[j], k.be[j]);
                                return GUARD ? guarded_relu<T>(a) : a;
                              });
  }
  if (GUARD) block_guard(amax, limit, err);
}

// The apply of a fused sibling launch's members in ONE launch
// (jr_bn_relu_apply_multi): the raw output's c channels, segment i its own
// output slice and beta; per element exactly k_bn_relu_apply's arithmetic
// (and its GUARD).
template <typename T, bool GUARD>
__global__ void __launch_bounds__(256) k_bn_relu_apply_multi(const T* __restrict__ x, int xs, int64_t m, int c,
                                                             const float* __restrict__ mean,
                                                             const float* __restrict__ invstd, ApplySegs sg,
                                                             float limit, unsigned* err) {
  constexpr int VW = Vec<T>::N;
  const RowLane l = row_lane<T>(c);
  const bool idle = l.rr >= l.rpp;
  if (!GUARD && idle) return;
  float amax = 0.f;
  if (!idle) {
    const int ch = l.q * VW;
    const int si = seg_of(sg, ch), lc = ch - sg.c0[si];
    const BnConst<VW> k = bn_const<VW>(mean + ch, invstd + ch, sg.beta[si] + lc);
    amax = row_pass<T, false>(x + ch, xs, nullptr, 0, static_cast<T*>(sg.y[si]) + sg.y_off[si] + lc, sg.y_stride[si],
                              l.block_row(blockIdx.x), l.rpp, m, [=](int j, float xv, float) {
                                const float a = bn_relu(xv, k.mu[j], k.is[j], k.be[j]);
                                return GUARD ? guarded_relu<T>(a) : a;
                              });
  }
  if (GUARD) block_guard(amax, limit, err);
}

// k_bn_relu_apply with the statistics finalize folded in: block (bx, by)
// first combines the conv's single-stage partials of the 32 channels of group
// by (stats_combine8: 8 lanes per channel, bitwise what k_stats_finalize8
// writes) into LDS -- blocks with bx == 0 also store them as the layer's
// mean / invstd -- then applies BN + ReLU to rows [bx*rpb, (bx+1)*rpb) of
// those channels, thread (q, rr) one 16-byte vector q of the group and rows
// rr, rr + rpp, ... (the arithmetic of k_bn_relu_apply).
template <typename T>
__global__ void __launch_bounds__(256) k_bn_relu_apply_stats(const T* __restrict__ x, int xs, int64_t m, int c,
                                                             const float* __restrict__ pm, const float* __restrict__ pq,
                                                             int P, int R, float eps, float* mean_out,
                                                             float* invstd_out, const float* __restrict__ beta, T* y,
                                                             int y_off, int y_stride, int rpb) {
  constexpr int VW = Vec<T>::N;
  __shared__ float s_mu[kFoldCh], s_is[kFoldCh];
  const int t = threadIdx.x;
  const int c0 = blockIdx.y * kFoldCh;
  const int cg = min(kFoldCh, c - c0);
  {
    const int slot = t / kStatsLanes, j = t % kStatsLanes;
    if (slot < cg) {
      const int ch = c0 + slot;
      float mu, is;
      stats_combine8(pm + (int64_t)ch * P, pq + (int64_t)ch * P, P, R, (int)m, eps, j, &mu, &is);
      if (j == 0) {
        s_mu[slot] = mu;
        s_is[slot] = is;
        if (blockIdx.x == 0) {
          mean_out[ch] = mu;
          invstd_out[ch] = is;
        }
      }
    }
  }
  __syncthreads();
  const RowLane l = row_lane<T>(cg);
  if (l.rr >= l.rpp) return;
  const int co = c0 + l.q * VW;
  const BnConst<VW> k = bn_const<VW>(s_mu + l.q * VW, s_is + l.q * VW, beta + co);
  const int64_t r0 = (int64_t)blockIdx.x * rpb, r1 = min(m, r0 + rpb);
  for (int64_t rb = r0 + l.rr; rb < r1; rb += (int64_t)l.rpp * kAppUnroll)
    row_pass<T, false>(x + co, xs, nullptr, 0, y + y_off + co, y_stride, rb, l.rpp, r1,
                       [=](int j, float xv, float) { return bn_relu(xv, k.mu[j], k.is[j], k.be[j]); });
}

// The backward's rows of one thread: dx = bn_bwd_batch over rows rb, ... below
// `end` of the channels at ch, k1 / k2 at the thread's first channel; one
// pass (a block kernel) or, FOLD, stepped by rpp * kAppUnroll up to `end`.
// Returns the largest |dx| this thread stored (0 if none).
template <typename T, bool FOLD>
__device__ __forceinline__ float bn_bwd_rows(const BnSegs& sg, const T* __restrict__ x, int xs, int ch,
                                             const float* __restrict__ mean, const float* __restrict__ invstd,
                                             const float* k1, const float* k2, T* dx, int64_t rb, int rpp,
                                             int64_t end) {
  constexpr int VW = Vec<T>::N;
  const SegGrad<T> sd = seg_grad<T>(sg, ch);
  const BnConst<VW> k = bn_const<VW>(mean + ch, invstd + ch, sd.beta);
  float c1[VW], c2[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) {
    c1[j] = k1[j]; c2[j] = k2[j];
  }
  const auto f = [=](int j, float xv, float dy) {
    const float xh = bn_xhat(xv, k.mu[j], k.is[j]);
    return bn_bwd_batch(xh, relu_grad(xh, k.be[j], dy), k.is[j], c1[j], c2[j]);
  };
  if constexpr (!FOLD) return row_pass<T, true>(x + ch, xs, sd.dy, sd.stride, dx + ch, xs, rb, rpp, end, f);
  for (; rb < end; rb += (int64_t)rpp * kAppUnroll)
    row_pass<T, true>(x + ch, xs, sd.dy, sd.stride, dx + ch, xs, rb, rpp, end, f);
  return 0.f;
}

template <typename T>
__device__ __forceinline__ float bn_bwd_apply_body(const BnSegs& sg, const T* __restrict__ x, int xs, int64_t m, int c,
                                                   const float* __restrict__ mean, const float* __restrict__ invstd,
                                                   const float* __restrict__ k1, const float* __restrict__ k2, T* dx,
                                                   int bx) {
  const RowLane l = row_lane<T>(c);
  if (l.rr >= l.rpp) return 0.f;
  const int ch = l.q * Vec<T>::N;
  return bn_bwd_rows<T, false>(sg, x, xs, ch, mean, invstd, k1 + ch, k2 + ch, dx, l.block_row(bx), l.rpp, m);
}

// The block's max of v into word blockIdx.x % 64 of out (atomicMax on the
// float bits: every value is >= 0).  Every thread of the block calls it.
__device__ __forceinline__ void block_absmax_to(float v, float* out) {
  const float b = block_max(v);   // (jr_bn_rows.h)
  if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned*>(out) + (blockIdx.x & 63), __float_as_uint(b));
}

template <typename T>
__global__ void __launch_bounds__(256) k_bn_relu_bwd_apply(BnSegs sg, const T* __restrict__ x, int xs, int64_t m,
                                                           int c, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd,
                                                           const float* __restrict__ k1,
                                                           const float* __restrict__ k2, T* dx) {
  const float amax = bn_bwd_apply_body<T>(sg, x, xs, m, c, mean, invstd, k1, k2, dx, blockIdx.x);
  if (sg.absmax) block_absmax_to(amax, sg.absmax);   // (uniform: a kernel argument)
}

// The backward under FROZEN statistics (jr_bn_relu_bwd_frozen): mean and
// invstd are constants, so BN is affine and its backward one elementwise
// pass, dx = T(g * invstd) with g = relu_grad(dy).  Thread layout and loads as
// k_bn_relu_bwd_apply, and its sg.absmax (jr_bn_relu_bwd_frozen_absmax).
template <typename T>
__global__ void __launch_bounds__(256) k_bn_relu_bwd_frozen(BnSegs sg, const T* __restrict__ x, int xs, int64_t m,
                                                            int c, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, T* dx) {
  constexpr int VW = Vec<T>::N;
  const RowLane l = row_lane<T>(c);
  float amax = 0.f;
  if (l.rr < l.rpp) {
    const int ch = l.q * VW;
    const SegGrad<T> sd = seg_grad<T>(sg, ch);
    const BnConst<VW> k = bn_const<VW>(mean + ch, invstd + ch, sd.beta);
    amax = row_pass<T, true>(x + ch, xs, sd.dy, sd.stride, dx + ch, xs, l.block_row(blockIdx.x), l.rpp, m,
                             [=](int j, float xv, float dy) {
                               return bn_bwd_frozen(relu_grad(bn_xhat(xv, k.mu[j], k.is[j]), k.be[j], dy), k.is[j]);
                             });
  }
  if (sg.absmax) block_absmax_to(amax, sg.absmax);   // (uniform: a kernel argument)
}

// Canonical combine of ONE channel's backward-reduce partials when there are
// at most kFoldMaxP of them (fp64 (sum dy', sum dy' xhat) per chunk): an
// aligned group of 8 lanes, lane j summing chunks j, j+8, ... in order, then
// an xor butterfly.  k_bn_finalize8 and k_bn_relu_bwd_apply_fold share it, so
// the folded backward is bitwise the three-launch one.
__device__ __forceinline__ void bwd_combine8(const double* __restrict__ p0, const double* __restrict__ p1, int nch,
                                             int j, double* s0, double* s1) {
  double a = 0, b = 0;
  constexpr int U = 8;
  for (int i0 = j; i0 < nch; i0 += kStatsLanes * U) {
    double va[U], vb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ic = min(i0 + kStatsLanes * u, nch - 1);
      va[u] = p0[ic];
      vb[u] = p1[ic];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i0 + kStatsLanes * u < nch) {
        a += va[u];
        b += vb[u];
      }
  }
#pragma unroll
  for (int o = kStatsLanes / 2; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, kStatsLanes);
    b += __shfl_xor(b, o, kStatsLanes);
  }
  *s0 = a;
  *s1 = b;
}

// k_bn_finalize<1> for at most kFoldMaxP chunks: 32 channels per block.
__device__ __forceinline__ void bn_finalize8_body(const double* __restrict__ part, int nchunks, int c, int64_t m,
                                                  float* k1, float* k2, const BnSegs& sg, int bx) {
  const int k = bx * (256 / kStatsLanes) + threadIdx.x / kStatsLanes, j = threadIdx.x % kStatsLanes;
  if (k >= c) return;   // (whole 8-lane groups)
  double s0, s1;
  bwd_combine8(part + (int64_t)k * nchunks, part + (int64_t)(c + k) * nchunks, nchunks, j, &s0, &s1);
  if (j != 0) return;
  const double inv_m = 1.0 / (double)m;
  k1[k] = (float)(s0 * inv_m);
  k2[k] = (float)(s1 * inv_m);
  const int sgi = seg_of(sg, k);
  sg.dbeta[sgi][k - sg.c0[sgi]] = (float)s0;
}

__global__ void __launch_bounds__(256) k_bn_finalize8(const double* __restrict__ part, int nchunks, int c, int64_t m,
                                                      float* k1, float* k2, BnSegs sg) {
  bn_finalize8_body(part, nchunks, c, m, k1, k2, sg, blockIdx.x);
}

// The backward's finalize folded into its apply: block (bx, by) combines the
// reduce's partials of the 32 channels of group by (bwd_combine8; bx == 0
// also stores dbeta), then applies the backward to rows [bx*rpb, (bx+1)*rpb)
// of those channels with the arithmetic of k_bn_relu_bwd_apply.
template <typename T>
__global__ void __launch_bounds__(256) k_bn_relu_bwd_apply_fold(BnSegs sg, const T* __restrict__ x, int xs, int64_t m,
                                                                int c, const float* __restrict__ mean,
                                                                const float* __restrict__ invstd,
                                                                const double* __restrict__ part, int nchunks, T* dx,
                                                                int rpb) {
  __shared__ float s_k1[kFoldCh], s_k2[kFoldCh];
  const int t = threadIdx.x;
  const int c0 = blockIdx.y * kFoldCh;
  const int cg = min(kFoldCh, c - c0);
  {
    const int slot = t / kStatsLanes, j = t % kStatsLanes;
    if (slot < cg) {
      const int k = c0 + slot;
      double s0, s1;
      bwd_combine8(part + (int64_t)k * nchunks, part + (int64_t)(c + k) * nchunks, nchunks, j, &s0, &s1);
      if (j == 0) {
        const double inv_m = 1.0 / (double)m;
        s_k1[slot] = (float)(s0 * inv_m);
        s_k2[slot] = (float)(s1 * inv_m);
        if (blockIdx.x == 0) {
          const int sgi = seg_of(sg, k);
          sg.dbeta[sgi][k - sg.c0[sgi]] = (float)s0;
        }
      }
    }
  }
  __syncthreads();
  const RowLane l = row_lane<T>(cg);
  if (l.rr >= l.rpp) return;
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int v0 = l.q * Vec<T>::N;
  bn_bwd_rows<T, true>(sg, x, xs, c0 + v0, mean, invstd, s_k1 + v0, s_k2 + v0, dx, r0 + l.rr, l.rpp, min(m, r0 + rpb));
}

// Several independent layers' backwards in ONE set of three launches
// (jr_bn_relu_bwd_batch): layer l owns blocks [b0, b0 + blocks) of each
// launch and runs exactly the single-layer bodies on them (same chunk
// geometry, same finalize arithmetic: bitwise jr_bn_relu_bwd_multi per layer).
// (BnBatch: jr_bn_plan.h)
// the layer owning block b of launch `which` (wave-uniform linear scan)
__device__ __forceinline__ int bn_batch_layer(const BnBatch& bt, int which, int b) {
  int l = 0;
  for (int i = 1; i < bt.n; ++i) l = b >= bt.L[i].b0[which] ? i : l;
  return l;
}

template <typename T>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) k_bn_reduce_batch(BnBatch bt) {
  const int l = bn_batch_layer(bt, 0, blockIdx.x);
  const BnBatchLayer& L = bt.L[l];
  bn_reduce_body<1, T>(static_cast<const T*>(L.x), L.xs, L.sg, L.m, L.c, L.rpc, L.mean, L.invstd, L.part,
                       blockIdx.x - L.b0[0], L.nchunks);
}

__global__ void __launch_bounds__(256) k_bn_finalize8_batch(BnBatch bt) {
  const int l = bn_batch_layer(bt, 1, blockIdx.x);
  const BnBatchLayer& L = bt.L[l];
  bn_finalize8_body(L.part, L.nchunks, L.c, L.m, L.k1, L.k2, L.sg, blockIdx.x - L.b0[1]);
}

template <typename T>
__global__ void __launch_bounds__(256) k_bn_relu_bwd_apply_batch(BnBatch bt) {
  const int l = bn_batch_layer(bt, 2, blockIdx.x);
  const BnBatchLayer& L = bt.L[l];
  bn_bwd_apply_body<T>(L.sg, static_cast<const T*>(L.x), L.xs, L.m, L.c, L.mean, L.invstd, L.k1, L.k2,
                       static_cast<T*>(L.dx), blockIdx.x - L.b0[2]);
}

}  // namespace jr

using namespace jr;

// x moved to the first channel of its slice
static const void* at_channel(int dtype, const void* x, int32_t c_off) {
  return static_cast<const char*>(x) + (size_t)c_off * elt_size(dtype);
}

JR_API int jr_bn_stats(int dtype, const void* x, int64_t m, int32_t c, float eps, float* mean,
                       float* invstd, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_common(dtype, m, c);
  if (rc) return rc;
  if (!x || !mean || !invstd) return fail(JR_ERR_INVALID, "bn_stats: null pointer");
  const jr_bn_launch_plan p = bn_plan(dtype, m, c);
  if (!ws || ws_bytes < (size_t)p.workspace_size) return fail(JR_ERR_WORKSPACE, "bn_stats: workspace too small");
  double* part = static_cast<double*>(ws);
  hipStream_t s = as_stream(stream);
  const BnSegs none{};
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_bn_reduce<0, T>), dim3(p.reduce_grid), dim3(256), 0, s, (const T*)x, c, none, m, c,
                       p.rows_per_chunk, nullptr, nullptr, part);
  });
  rc = check_launch("bn_stats reduce");
  if (rc) return rc;
  hipLaunchKernelGGL((k_bn_finalize<0>), dim3(p.stats_finalize_grid), dim3(256), 0, s, part, p.nchunks, c, m, eps,
                     mean, invstd, none);
  return check_launch("bn_stats finalize");
}

// (Guard, guard_limit, guard_word: jr_common.h)
static int bn_apply_launch(int dtype, int members, const void* x, int32_t x_c_stride, int64_t x_mb, int64_t m,
                           int32_t c, const float* mean, const float* invstd, int64_t st_mb, const float* beta,
                           int64_t be_mb, void* y, int32_t y_c_off, int32_t y_c_stride, int64_t y_mb, float limit,
                           hipStream_t s) {
  Guard g;
  const int rc = guard_word("bn_relu_apply", limit, s, g);
  if (rc) return rc;
  const dim3 grid(bn_plan(dtype, m, c).apply_grid, members);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    if (!g.err)
      hipLaunchKernelGGL((k_bn_relu_apply<T, false>), grid, dim3(256), 0, s, (const T*)x, x_c_stride, m, c, mean,
                         invstd, beta, (T*)y, y_c_off, y_c_stride, x_mb, y_mb, st_mb, be_mb, 0.f, nullptr);
    else
      hipLaunchKernelGGL((k_bn_relu_apply<T, true>), grid, dim3(256), 0, s, (const T*)x, x_c_stride, m, c, mean,
                         invstd, beta, (T*)y, y_c_off, y_c_stride, x_mb, y_mb, st_mb, be_mb, g.limit, g.err);
  });
  return check_launch("bn_relu_apply");
}

// (limit = 0: jr_bn_relu_apply; > 0: jr_bn_relu_apply_guard)
static int bn_relu_apply(int dtype, const void* x, int32_t x_c_off, int32_t x_c_stride, int64_t m, int32_t c,
                         const float* mean, const float* invstd, const float* beta, void* y, int32_t y_c_off,
                         int32_t y_c_stride, float limit, void* stream) {
  int rc = check_common(dtype, m, c);
  if (rc) return rc;
  if (!x || !mean || !invstd || !beta || !y) return fail(JR_ERR_INVALID, "bn_relu_apply: null pointer");
  if (!check_slice(dtype, x_c_off, x_c_stride, c)) return fail(JR_ERR_INVALID, "bn_relu_apply: bad input slice");
  if (!check_slice(dtype, y_c_off, y_c_stride, c)) return fail(JR_ERR_INVALID, "bn_relu_apply: bad output slice");
  return bn_apply_launch(dtype, 1, at_channel(dtype, x, x_c_off), x_c_stride, 0, m, c, mean, invstd, 0, beta, 0, y,
                         y_c_off, y_c_stride, 0, limit, as_stream(stream));
}

JR_API int jr_bn_relu_apply(int dtype, const void* x, int32_t x_c_off, int32_t x_c_stride, int64_t m, int32_t c,
                            const float* mean, const float* invstd, const float* beta, void* y, int32_t y_c_off,
                            int32_t y_c_stride, void* stream) {
  return bn_relu_apply(dtype, x, x_c_off, x_c_stride, m, c, mean, invstd, beta, y, y_c_off, y_c_stride, 0.f, stream);
}

JR_API int jr_bn_relu_apply_guard(int dtype, const void* x, int32_t x_c_off, int32_t x_c_stride, int64_t m, int32_t c,
                                  const float* mean, const float* invstd, const float* beta, void* y,
                                  int32_t y_c_off, int32_t y_c_stride, float limit, void* stream) {
  if (!guard_limit(limit)) return fail(JR_ERR_INVALID, "bn_relu_apply_guard: limit must be finite and > 0");
  return bn_relu_apply(dtype, x, x_c_off, x_c_stride, m, c, mean, invstd, beta, y, y_c_off, y_c_stride, limit, stream);
}

static int bn_relu_apply_multi(int dtype, int nseg, const jr_bn_apply_seg* segs, const void* x, int32_t x_c_off,
                               int32_t x_c_stride, int64_t m, int32_t c, const float* mean, const float* invstd,
                               float limit, void* stream) {
  int rc = check_common(dtype, m, c);
  if (rc) return rc;
  if (!segs || nseg < 1 || nseg > kMaxSegs) return fail(JR_ERR_INVALID, "bn_relu_apply_multi: 1..4 segments");
  if (!x || !mean || !invstd) return fail(JR_ERR_INVALID, "bn_relu_apply_multi: null pointer");
  if (!check_slice(dtype, x_c_off, x_c_stride, c)) return fail(JR_ERR_INVALID, "bn_relu_apply_multi: bad input slice");
  ApplySegs sg;
  rc = apply_segs(dtype, nseg, segs, c, sg);
  if (rc) return rc;
  x = at_channel(dtype, x, x_c_off);
  const dim3 grid(bn_plan(dtype, m, c).apply_grid);
  hipStream_t s = as_stream(stream);
  Guard g;
  rc = guard_word("bn_relu_apply_multi", limit, s, g);
  if (rc) return rc;
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    if (!g.err)
      hipLaunchKernelGGL((k_bn_relu_apply_multi<T, false>), grid, dim3(256), 0, s, (const T*)x, x_c_stride, m, c, mean,
                         invstd, sg, 0.f, nullptr);
    else
      hipLaunchKernelGGL((k_bn_relu_apply_multi<T, true>), grid, dim3(256), 0, s, (const T*)x, x_c_stride, m, c, mean,
                         invstd, sg, g.limit, g.err);
  });
  return check_launch("bn_relu_apply_multi");
}

JR_API int jr_bn_relu_apply_multi(int dtype, int nseg, const jr_bn_apply_seg* segs, const void* x, int32_t x_c_off,
                                  int32_t x_c_stride, int64_t m, int32_t c, const float* mean, const float* invstd,
                                  void* stream) {
  return bn_relu_apply_multi(dtype, nseg, segs, x, x_c_off, x_c_stride, m, c, mean, invstd, 0.f, stream);
}

JR_API int jr_bn_relu_apply_multi_guard(int dtype, int nseg, const jr_bn_apply_seg* segs, const void* x,
                                        int32_t x_c_off, int32_t x_c_stride, int64_t m, int32_t c, const float* mean,
                                        const float* invstd, float limit, void* stream) {
  if (!guard_limit(limit)) return fail(JR_ERR_INVALID, "bn_relu_apply_multi_guard: limit must be finite and > 0");
  return bn_relu_apply_multi(dtype, nseg, segs, x, x_c_off, x_c_stride, m, c, mean, invstd, limit, stream);
}

JR_API int jr_bn_relu_apply_stats(int dtype, const void* x, int32_t x_c_off, int32_t x_c_stride, int64_t m, int32_t c,
                                  const float* part, int32_t P, int32_t R, int32_t n_total, int32_t stat_c_off,
                                  float eps, float* mean, float* invstd, const float* beta, void* y, int32_t y_c_off,
                                  int32_t y_c_stride, void* stream) {
  int rc = check_common(dtype, m, c);
  if (rc) return rc;
  if (!x || !part || !mean || !invstd || !beta || !y) return fail(JR_ERR_INVALID, "bn_relu_apply_stats: null pointer");
  if (!check_slice(dtype, x_c_off, x_c_stride, c) || !check_slice(dtype, y_c_off, y_c_stride, c))
    return fail(JR_ERR_INVALID, "bn_relu_apply_stats: bad input / output slice");
  if (P < 1 || R < 1 || (int64_t)P * R < m || stat_c_off < 0 || stat_c_off + c > n_total || m >= (1LL << 31))
    return fail(JR_ERR_INVALID, "bn_relu_apply_stats: partials inconsistent with the slice");
  x = at_channel(dtype, x, x_c_off);
  const float* pm = part + (int64_t)stat_c_off * P;
  const float* pq = part + (int64_t)(n_total + stat_c_off) * P;
  const jr_bn_launch_plan p = bn_plan(dtype, m, c);
  const dim3 grid(p.fold_grid_x, p.fold_grid_y);
  hipStream_t s = as_stream(stream);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_bn_relu_apply_stats<T>, grid, dim3(256), 0, s, (const T*)x, x_c_stride, m, c, pm, pq, P, R,
                       eps, mean, invstd, beta, (T*)y, y_c_off, y_c_stride, p.fold_rows);
  });
  return check_launch("bn_relu_apply_stats");
}

static int bn_relu_apply_grouped(int dtype, int32_t members, const void* x, int32_t x_c_off, int32_t x_c_stride,
                                 int64_t x_member_stride, int64_t m, int32_t c, const float* mean,
                                 const float* invstd, int64_t stats_member_stride, const float* beta,
                                 int64_t beta_member_stride, void* y, int32_t y_c_off, int32_t y_c_stride,
                                 int64_t y_member_stride, float limit, void* stream) {
  int rc = check_common(dtype, m, c);
  if (rc) return rc;
  if (members < 1 || members > 65535) return fail(JR_ERR_INVALID, "bn_relu_apply_grouped: members must be 1..65535");
  if (!x || !mean || !invstd || !beta || !y) return fail(JR_ERR_INVALID, "bn_relu_apply_grouped: null pointer");
  if (x_member_stride < 0 || y_member_stride < 0 || stats_member_stride < 0 || beta_member_stride < 0)
    return fail(JR_ERR_INVALID, "bn_relu_apply_grouped: negative member stride");
  if (!check_slice(dtype, x_c_off, x_c_stride, c) || !check_slice(dtype, y_c_off, y_c_stride, c))
    return fail(JR_ERR_INVALID, "bn_relu_apply_grouped: bad input / output slice");
  const size_t esz = elt_size(dtype);
  if (((x_member_stride * esz) | (y_member_stride * esz)) & 15)
    return fail(JR_ERR_INVALID, "bn_relu_apply_grouped: member strides must be 16-byte multiples");
  return bn_apply_launch(dtype, members, at_channel(dtype, x, x_c_off), x_c_stride, x_member_stride * esz, m, c, mean,
                         invstd, stats_member_stride * 4, beta, beta_member_stride * 4, y, y_c_off, y_c_stride,
                         y_member_stride * esz, limit, as_stream(stream));
}

JR_API int jr_bn_relu_apply_grouped(int dtype, int32_t members, const void* x, int32_t x_c_off, int32_t x_c_stride,
                                    int64_t x_member_stride, int64_t m, int32_t c, const float* mean,
                                    const float* invstd, int64_t stats_member_stride, const float* beta,
                                    int64_t beta_member_stride, void* y, int32_t y_c_off, int32_t y_c_stride,
                                    int64_t y_member_stride, void* stream) {
  return bn_relu_apply_grouped(dtype, members, x, x_c_off, x_c_stride, x_member_stride, m, c, mean, invstd,
                               stats_member_stride, beta, beta_member_stride, y, y_c_off, y_c_stride, y_member_stride,
                               0.f, stream);
}

JR_API int jr_bn_relu_apply_grouped_guard(int dtype, int32_t members, const void* x, int32_t x_c_off,
                                          int32_t x_c_stride, int64_t x_member_stride, int64_t m, int32_t c,
                                          const float* mean, const float* invstd, int64_t stats_member_stride,
                                          const float* beta, int64_t beta_member_stride, void* y, int32_t y_c_off,
                                          int32_t y_c_stride, int64_t y_member_stride, float limit, void* stream) {
  if (!guard_limit(limit)) return fail(JR_ERR_INVALID, "bn_relu_apply_grouped_guard: limit must be finite and > 0");
  return bn_relu_apply_grouped(dtype, members, x, x_c_off, x_c_stride, x_member_stride, m, c, mean, invstd,
                               stats_member_stride, beta, beta_member_stride, y, y_c_off, y_c_stride, y_member_stride,
                               limit, stream);
}

// The apply pass of the backward (k1, k2 from a finalize).
static int bn_bwd_apply_launch(int dtype, const BnSegs& sg, const void* x, int32_t x_c_stride, int64_t m, int32_t c,
                               const float* mean, const float* invstd, const float* k1, const float* k2, void* dx,
                               hipStream_t s) {
  const dim3 grid(bn_plan(dtype, m, c).apply_grid);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_bn_relu_bwd_apply<T>, grid, dim3(256), 0, s, sg, (const T*)x, x_c_stride, m, c, mean, invstd,
                       k1, k2, (T*)dx);
  });
  return check_launch("bn_bwd apply");
}

// The three backward launches over segments (validated by the callers).
static int bn_bwd_launch(int dtype, const BnSegs& sg, const void* x, int32_t x_c_stride, int64_t m, int32_t c,
                         const float* mean, const float* invstd, void* dx, void* ws, size_t ws_bytes,
                         hipStream_t s) {
  const jr_bn_launch_plan p = bn_plan(dtype, m, c);
  if (!ws || ws_bytes < (size_t)p.workspace_size) return fail(JR_ERR_WORKSPACE, "bn_relu_bwd: workspace too small");
  double* part = static_cast<double*>(ws);
  float* k1 = reinterpret_cast<float*>(static_cast<char*>(ws) + p.k1_offset);
  float* k2 = k1 + c;
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_bn_reduce<1, T>), dim3(p.reduce_grid), dim3(256), 0, s, (const T*)x, x_c_stride, sg, m, c,
                       p.rows_per_chunk, mean, invstd, part);
  });
  int rc = check_launch("bn_bwd reduce");
  if (rc) return rc;
  if (p.single_stage) {
    if (fold_bwd() && !sg.absmax) {   // the finalize inside the apply: one kernel boundary fewer
      const dim3 grid(p.fold_grid_x, p.fold_grid_y);
      by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_bn_relu_bwd_apply_fold<T>, grid, dim3(256), 0, s, sg, (const T*)x, x_c_stride, m, c, mean,
                           invstd, (const double*)part, p.nchunks, (T*)dx, p.fold_rows);
      });
      return check_launch("bn_bwd apply (fold)");
    }
    hipLaunchKernelGGL(k_bn_finalize8, dim3(p.finalize_grid), dim3(256), 0, s, (const double*)part, p.nchunks, c, m,
                       k1, k2, sg);
  } else {
    hipLaunchKernelGGL((k_bn_finalize<1>), dim3(p.finalize_grid), dim3(256), 0, s, part, p.nchunks, c, m, 0.f, k1, k2,
                       sg);
  }
  rc = check_launch("bn_bwd finalize");
  if (rc) return rc;
  return bn_bwd_apply_launch(dtype, sg, x, x_c_stride, m, c, mean, invstd, k1, k2, dx, s);
}

JR_API int jr_bn_relu_bwd(int dtype, const void* dy, int32_t dy_c_off, int32_t dy_c_stride, const void* x,
                          int32_t x_c_off, int32_t x_c_stride, int64_t m, int32_t c, const float* mean,
                          const float* invstd, const float* beta, void* dx, float* dbeta, void* ws, size_t ws_bytes,
                          void* stream) {
  jr_bn_seg seg{dy, dy_c_off, dy_c_stride, c, beta, dbeta};
  return jr_bn_relu_bwd_multi(dtype, 1, &seg, x, x_c_off, x_c_stride, m, c, mean, invstd, dx, ws, ws_bytes, stream);
}

JR_API int jr_bn_relu_bwd_multi(int dtype, int nseg, const jr_bn_seg* segs, const void* x, int32_t x_c_off,
                                int32_t x_c_stride, int64_t m, int32_t c, const float* mean, const float* invstd,
                                void* dx, void* ws, size_t ws_bytes, void* stream) {
  return jr_bn_relu_bwd_multi_absmax(dtype, nseg, segs, x, x_c_off, x_c_stride, m, c, mean, invstd, dx, ws, ws_bytes,
                                     nullptr, stream);
}

JR_API int jr_bn_relu_bwd_multi_absmax(int dtype, int nseg, const jr_bn_seg* segs, const void* x, int32_t x_c_off,
                                       int32_t x_c_stride, int64_t m, int32_t c, const float* mean,
                                       const float* invstd, void* dx, void* ws, size_t ws_bytes, float* dx_absmax,
                                       void* stream) {
  BnSegs sg;
  const int rc = bwd_setup(dtype, nseg, segs, x, x_c_off, x_c_stride, m, c, mean, invstd, dx, sg);
  if (rc) return rc;
  sg.absmax = dx_absmax;
  return bn_bwd_launch(dtype, sg, x, x_c_stride, m, c, mean, invstd, dx, ws, ws_bytes, as_stream(stream));
}

JR_API int jr_bn_relu_bwd_frozen(int dtype, int nseg, const jr_bn_seg* segs, const void* x, int32_t x_c_off,
                                 int32_t x_c_stride, int64_t m, int32_t c, const float* mean, const float* invstd,
                                 void* dx, void* stream) {
  return jr_bn_relu_bwd_frozen_absmax(dtype, nseg, segs, x, x_c_off, x_c_stride, m, c, mean, invstd, dx, nullptr,
                                      stream);
}

JR_API int jr_bn_relu_bwd_frozen_absmax(int dtype, int nseg, const jr_bn_seg* segs, const void* x, int32_t x_c_off,
                                        int32_t x_c_stride, int64_t m, int32_t c, const float* mean,
                                        const float* invstd, void* dx, float* dx_absmax, void* stream) {
  BnSegs sg;
  const int rc = bwd_setup(dtype, nseg, segs, x, x_c_off, x_c_stride, m, c, mean, invstd, dx, sg, false);
  if (rc) return rc;
  sg.absmax = dx_absmax;
  const dim3 grid(bn_plan(dtype, m, c).apply_grid);
  hipStream_t s = as_stream(stream);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_bn_relu_bwd_frozen<T>, grid, dim3(256), 0, s, sg, (const T*)x, x_c_stride, m, c, mean, invstd,
                       (T*)dx);
  });
  return check_launch("bn_relu_bwd_frozen");
}

JR_API int jr_bn_relu_bwd_batch(int dtype, int32_t n, const jr_bn_bwd_layer* layers, void* ws, size_t ws_bytes,
                                void* stream) {
  BnBatch bt;
  int blocks[3];
  int rc = bwd_batch_setup(dtype, n, layers, ws, ws_bytes, bt, blocks);
  if (rc) return rc;
  hipStream_t s = as_stream(stream);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_bn_reduce_batch<T>, dim3(blocks[0]), dim3(256), 0, s, bt);
  });
  rc = check_launch("bn_bwd batch reduce");
  if (rc) return rc;
  hipLaunchKernelGGL(k_bn_finalize8_batch, dim3(blocks[1]), dim3(256), 0, s, bt);
  rc = check_launch("bn_bwd batch finalize");
  if (rc) return rc;
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_bn_relu_bwd_apply_batch<T>, dim3(blocks[2]), dim3(256), 0, s, bt);
  });
  return check_launch("bn_bwd batch apply");
}

// ---------------------------------------------------------------------------
// The backward of a conv2d_bn layer whose output only a 3x3/2 max-pool reads
// (the stem's conv2d_3 / conv2d_5; forward: jr_bn_relu_maxpool3x3s2_fwd).
// k_maxpool_bwd_bn routes the pooled gradient to the layer's output exactly
// as k_maxpool_bwd (2x2 input cells, windows summed from +0 in (oh, ow)
// order, stored in the path dtype) and, holding each dy in registers, adds
// the BN reduce's sums (sum dy', sum dy' xhat, fp64) of its channel quad
// over every cell it visits; one partial per block and channel ([2][c][grid],
// fixed order: deterministic) replaces k_bn_reduce's second read of dy.
// k_bn_finalize and k_bn_relu_bwd_apply then run as for any layer.
template <typename T>
__global__ void __launch_bounds__(256) k_maxpool_bwd_bn(jr_pool_desc d, const uint8_t* __restrict__ argmax,
                                                        const T* __restrict__ pdy, T* __restrict__ dy,
                                                        const T* __restrict__ x, int xs, const float* __restrict__ mean,
                                                        const float* __restrict__ invstd,
                                                        const float* __restrict__ beta, double* part) {
  __shared__ double red[256][8];
  const int c4 = d.c >> 2;
  const int total = d.n * ((d.h + 1) >> 1) * ((d.w + 1) >> 1) * c4;
  const int stride = gridDim.x * blockDim.x;
  const int q = (blockIdx.x * blockDim.x + threadIdx.x) % c4;   // fixed per thread: blockDim.x % c4 == 0
  const BnConst<4> k = bn_const<4>(mean + q * 4, invstd + q * 4, beta + q * 4);
  double s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride)
    maxpool_bwd_cell(d, argmax, pdy, e / c4, q, [&](int b, int ih, int iw, float4 o) {
      const int64_t pix = ((int64_t)b * d.h + ih) * d.w + iw;
      P4<T>::st(dy + pix * d.x_c_stride + d.x_c_off + q * 4, o);
      float acc[4] = {o.x, o.y, o.z, o.w};
      if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int l = 0; l < 4; ++l) acc[l] = bf2f(f2bf(acc[l]));   // the value k_bn_reduce would read
      }
      const float4 xq = P4<T>::ld(x + pix * xs + q * 4);
      const float xv[4] = {xq.x, xq.y, xq.z, xq.w};
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        const float xh = bn_xhat(xv[l], k.mu[l], k.is[l]);
        const float g2 = relu_grad(xh, k.be[l], acc[l]);
        s0[l] += (double)g2;
        s1[l] += (double)g2 * (double)xh;
      }
    });
  const int t = threadIdx.x;
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    red[t][l] = s0[l];
    red[t][4 + l] = s1[l];
  }
  __syncthreads();
  // threads t, t + c4, t + 2 c4, ... hold the same channel quad: fixed-order sum
  if (t < c4) {
    double a[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = red[t][k];
    for (int o = t + c4; o < (int)blockDim.x; o += c4)
#pragma unroll
      for (int k = 0; k < 8; ++k) a[k] += red[o][k];
    const int64_t nch = gridDim.x;
    const int qq = (blockIdx.x * blockDim.x + t) % c4;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      part[(int64_t)(qq * 4 + l) * nch + blockIdx.x] = a[l];
      part[(int64_t)(d.c + qq * 4 + l) * nch + blockIdx.x] = a[4 + l];
    }
  }
}

JR_API int jr_bn_relu_bwd_maxpool(int dtype, const jr_pool_desc* d, const uint8_t* argmax, const void* pooled_dy,
                                  void* dy, const void* x, int32_t x_c_stride, const float* mean,
                                  const float* invstd, const float* beta, void* dx, float* dbeta, void* ws,
                                  size_t ws_bytes, void* stream) {
  return jr_bn_relu_bwd_maxpool_absmax(dtype, d, argmax, pooled_dy, dy, x, x_c_stride, mean, invstd, beta, dx, dbeta,
                                       ws, ws_bytes, nullptr, stream);
}

JR_API int jr_bn_relu_bwd_maxpool_absmax(int dtype, const jr_pool_desc* d, const uint8_t* argmax,
                                         const void* pooled_dy, void* dy, const void* x, int32_t x_c_stride,
                                         const float* mean, const float* invstd, const float* beta, void* dx,
                                         float* dbeta, void* ws, size_t ws_bytes, float* dx_absmax, void* stream) {
  if (!d || !argmax || !pooled_dy || !dy || !x || !mean || !invstd || !beta || !dx || !dbeta)
    return fail(JR_ERR_INVALID, "bn_relu_bwd_maxpool: null pointer");
  const int32_t c = d->c;
  const int64_t m = (int64_t)d->n * d->h * d->w;
  int rc = check_common(dtype, m, c);
  if (rc) return rc;
  if (c % 4 || c / 4 > 256) return fail(JR_ERR_UNSUPPORTED, "bn_relu_bwd_maxpool: c must be a multiple of 4, <= 1024");
  if (d->h < 3 || d->w < 3 || d->ho != (d->h - 3) / 2 + 1 || d->wo != (d->w - 3) / 2 + 1)
    return fail(JR_ERR_INVALID, "bn_relu_bwd_maxpool: the pool must be 3x3 stride 2 valid");
  if (!check_slice(dtype, d->y_c_off, d->y_c_stride, c) || !check_slice(dtype, d->x_c_off, d->x_c_stride, c) ||
      !check_slice(dtype, 0, x_c_stride, c))
    return fail(JR_ERR_INVALID, "bn_relu_bwd_maxpool: bad slice");
  if (!ws || ws_bytes < pool_bwd_ws(c)) return fail(JR_ERR_WORKSPACE, "bn_relu_bwd_maxpool: workspace too small");
  // the finalize and the apply see the dy this call writes as one segment
  const jr_bn_seg seg{dy, d->x_c_off, d->x_c_stride, c, beta, dbeta};
  BnSegs sg;
  rc = bwd_segs(dtype, 1, &seg, c, sg);
  if (rc) return rc;
  sg.absmax = dx_absmax;
  hipStream_t s = as_stream(stream);
  const PoolBwdGeom g = pool_bwd_geom(d);
  const jr_bn_launch_plan p = bn_plan(dtype, m, c);
  double* part = static_cast<double*>(ws);
  float* k1 = reinterpret_cast<float*>(part + (size_t)g.grid * 2 * c);
  float* k2 = k1 + c;
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_maxpool_bwd_bn<T>, dim3(g.grid), dim3(g.block), 0, s, *d, argmax, (const T*)pooled_dy, (T*)dy,
                       (const T*)x, x_c_stride, mean, invstd, beta, part);
  });
  rc = check_launch("maxpool_bwd + bn reduce");
  if (rc) return rc;
  hipLaunchKernelGGL((k_bn_finalize<1>), dim3(p.stats_finalize_grid), dim3(256), 0, s, part, g.grid, c, m, 0.f, k1,
                     k2, sg);
  rc = check_launch("bn_bwd finalize");
  if (rc) return rc;
  return bn_bwd_apply_launch(dtype, sg, x, x_c_stride, m, c, mean, invstd, k1, k2, dx, s);
}
