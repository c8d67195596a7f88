// jr_attribution.hip — per-image saliency maps: the data gradient of the
// image layer and the elementwise passes of the attribution drivers
// (jr/attribution.py; formulas and rounding: include/jr.h).
//
//   jr_conv2d_bwd_image   d raw / d image of a convolution with c_in <= 4
//                         (conv2d_1: the layer jr_conv2d_bwd_data refuses)
//   jr_attr_scale_input   dst = T(f32(src) * alpha)       (integrated gradients' path)
//   jr_attr_accumulate    acc = (first ? 0 : acc) + dx * weight
//   jr_attr_map           per-pixel map of a 3-channel gradient
//
// Compiled with -ffp-contract=off: every multiply and add below is rounded
// on its own, so a numpy float32 restatement reproduces the results bit for
// bit (tests/attribution_ref.py).
//
// The image gradient is the feature's one bandwidth kernel (299^2, B = 32:
// 91 MB of fp32 dy in, 34 MB out; each dy pixel feeds 9 input pixels).  A
// block owns a T x T patch of input pixels of one image and stages in LDS,
// as fp32, the dy patch those pixels read (16-byte global loads; a pixel's
// c_out channels padded by 4 words, so the 16-byte LDS reads of 8 lanes at
// consecutive pixels fall into distinct banks) and the whole filter (read at
// a wave-uniform address: a broadcast).  Threads are numbered stride phase
// first: with stride 2 and T = 16 each of the four waves holds the 8 x 8
// pixels of one (row, column) parity, which all walk the same taps.
#include "jr_common.h"

namespace jr {

constexpr int kImgMaxK = 7;               // kh, kw at most
constexpr int kImgPad = 4;                // LDS words between the channel rows of two dy pixels
constexpr size_t kImgMaxLds = 48 * 1024;  // dynamic LDS per block

__host__ __device__ inline int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// rows (columns) of dy that T consecutive input rows can read
__host__ __device__ inline int img_patch(int T, int k, int s) { return (T + k - 2) / s + 1; }

inline size_t img_lds_bytes(const jr_conv_desc* d, int T) {
  const size_t ph = img_patch(T, d->kh, d->stride_h), pw = img_patch(T, d->kw, d->stride_w);
  return 4 * (ph * pw * (size_t)(d->c_out + kImgPad) + (size_t)d->kh * d->kw * d->c_in * d->c_out);
}

template <typename T> struct DyVec;
template <> struct DyVec<float> {
  static constexpr int N = 4;
  __device__ static void ld(const float* p, float* v) {
    const float4 u = *reinterpret_cast<const float4*>(p);
    v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
  }
};
template <> struct DyVec<uint16_t> {
  static constexpr int N = 8;
  __device__ static void ld(const uint16_t* p, float* v) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = __uint_as_float(w[i] << 16);
      v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  }
};

// grid (ceil(w / TILE), ceil(h / TILE), n), TILE * TILE threads
template <typename T, int TILE>
__global__ void __launch_bounds__(TILE * TILE) k_conv_bwd_image(jr_conv_desc d, const T* __restrict__ dy,
                                                                const float* __restrict__ w, float* __restrict__ dx,
                                                                int dxs) {
  extern __shared__ float4 lds4[];
  float* sdy = reinterpret_cast<float*>(lds4);
  constexpr int NT = TILE * TILE, VW = DyVec<T>::N;
  const int t = threadIdx.x, img = blockIdx.z;
  const int iy0 = blockIdx.y * TILE, ix0 = blockIdx.x * TILE;
  const int sh = d.stride_h, sw = d.stride_w, cout = d.c_out, cin = d.c_in;
  const int ph = img_patch(TILE, d.kh, sh), pw = img_patch(TILE, d.kw, sw);
  const int ps = cout + kImgPad;                      // words per staged dy pixel
  float* sw_ = sdy + (size_t)ph * pw * ps;              // the filter [kh][kw][c_in][c_out]
  // first output row / column any pixel of the patch reads (may be negative)
  const int oy_lo = floor_div(iy0 + d.pad_h - (d.kh - 1) + sh - 1, sh);
  const int ox_lo = floor_div(ix0 + d.pad_w - (d.kw - 1) + sw - 1, sw);

  const int vpp = cout / VW;                          // 16-byte vectors per dy pixel
  for (int i = t; i < ph * pw * vpp; i += NT) {
    const int v = i % vpp, pp = i / vpp;
    const int px = pp % pw, py = pp / pw;
    const int oy = oy_lo + py, ox = ox_lo + px;
    float f[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) f[j] = 0.f;
    if (oy >= 0 && oy < d.ho && ox >= 0 && ox < d.wo)
      DyVec<T>::ld(dy + (((int64_t)img * d.ho + oy) * d.wo + ox) * d.y_c_stride + d.y_c_off + v * VW, f);
    float* o = sdy + (size_t)pp * ps + v * VW;
#pragma unroll
    for (int j = 0; j < VW; j += 4) *reinterpret_cast<float4*>(o + j) = make_float4(f[j], f[j + 1], f[j + 2], f[j + 3]);
  }
  const int wn = d.kh * d.kw * cin * cout;
  for (int i = t; i < wn; i += NT) sw_[i] = w[i];
  __syncthreads();

  // stride phase first: the threads of a wave share their tap set
  const int nyp = TILE / sh, nxp = TILE / sw;
  const int phase = t / (nyp * nxp), in = t % (nyp * nxp);
  const int ly = (in / nxp) * sh + phase / sw, lx = (in % nxp) * sw + phase % sw;
  const int iy = iy0 + ly, ix = ix0 + lx;
  if (iy >= d.h || ix >= d.w) return;
  const int ty = iy + d.pad_h, tx = ix + d.pad_w;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int r = ty % sh; r < d.kh; r += sh) {
    const int oy = (ty - r) / sh;
    if (r > ty || oy >= d.ho) continue;
    for (int s = tx % sw; s < d.kw; s += sw) {
      const int ox = (tx - s) / sw;
      if (s > tx || ox >= d.wo) continue;
      const float* g = sdy + (size_t)((oy - oy_lo) * pw + (ox - ox_lo)) * ps;
      const float* wf = sw_ + (size_t)(r * d.kw + s) * cin * cout;
      float p[4] = {0.f, 0.f, 0.f, 0.f};
      for (int co = 0; co < cout; co += 4) {
        const float4 g4 = *reinterpret_cast<const float4*>(g + co);
        const float gv[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
          if (ci < cin) {
            const float4 w4 = *reinterpret_cast<const float4*>(wf + ci * cout + co);
            const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) p[ci] = __fadd_rn(p[ci], __fmul_rn(gv[j], wv[j]));
          }
        }
      }
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) acc[ci] = __fadd_rn(acc[ci], p[ci]);
    }
  }
  float* o = dx + (((int64_t)img * d.h + iy) * d.w + ix) * dxs;
  if (dxs == 4) {
    *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);   // (channels >= c_in stayed 0)
  } else {
    for (int ci = 0; ci < dxs; ++ci) o[ci] = ci < 4 ? acc[ci] : 0.f;
  }
}

template <typename T>
__global__ void __launch_bounds__(256) k_attr_scale(const T* __restrict__ src, T* __restrict__ dst, int64_t n,
                                                    float alpha) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) Elt<T>::st(dst + e, __fmul_rn(Elt<T>::ld(src + e), alpha));
}

__global__ void __launch_bounds__(256) k_attr_accumulate(const float* __restrict__ dx, float* acc, int64_t n,
                                                         float weight, int first) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const float a = first ? 0.f : acc[e];
  acc[e] = __fadd_rn(a, __fmul_rn(dx[e], weight));
}

template <typename T>
__global__ void __launch_bounds__(256) k_attr_map(int mode, const float* __restrict__ acc, int as,
                                                  const T* __restrict__ x, int xs, int64_t pixels, float* map) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= pixels) return;
  const float* a = acc + e * as;
  if (mode == JR_ATTR_ABSMAX) {
    map[e] = fmaxf(fmaxf(fabsf(a[0]), fabsf(a[1])), fabsf(a[2]));
    return;
  }
  const T* xv = x + e * xs;
  const float p0 = __fmul_rn(a[0], Elt<T>::ld(xv)), p1 = __fmul_rn(a[1], Elt<T>::ld(xv + 1)),
              p2 = __fmul_rn(a[2], Elt<T>::ld(xv + 2));
  map[e] = __fadd_rn(__fadd_rn(p0, p1), p2);
}

}  // namespace jr

using namespace jr;

JR_API int jr_conv2d_bwd_image(const jr_conv_desc* d, int dtype, const void* dy, const float* w, float* dx,
                               int32_t dx_c_stride, void* stream) {
  if (!d) return fail(JR_ERR_INVALID, "conv bwd_image: null descriptor");
  if (dtype != JR_F32 && dtype != JR_BF16)
    return fail(JR_ERR_INVALID, "conv bwd_image: dy is JR_F32 or JR_BF16 (the storage dtypes)");
  if (!dy || !w || !dx) return fail(JR_ERR_INVALID, "conv bwd_image: null pointer");
  if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->c_in <= 0 || d->c_out <= 0 || d->kh <= 0 || d->kw <= 0 ||
      d->stride_h <= 0 || d->stride_w <= 0 || d->pad_h < 0 || d->pad_w < 0)
    return fail(JR_ERR_INVALID, "conv bwd_image: non-positive dimension");
  const int ho = (d->h + 2 * d->pad_h - d->kh) / d->stride_h + 1;
  const int wo = (d->w + 2 * d->pad_w - d->kw) / d->stride_w + 1;
  if (ho != d->ho || wo != d->wo || ho <= 0 || wo <= 0)
    return fail(JR_ERR_INVALID, "conv bwd_image: ho/wo inconsistent with h,w,k,stride,pad");
  const int q = dtype == JR_BF16 ? 8 : 4;
  if (d->y_c_off < 0 || d->y_c_off + d->c_out > d->y_c_stride || d->y_c_off % q || d->y_c_stride % q)
    return fail(JR_ERR_INVALID, "conv bwd_image: dy channel slice out of range or not 16-byte aligned");
  if (dx_c_stride < d->c_in) return fail(JR_ERR_INVALID, "conv bwd_image: dx_c_stride below c_in");
  if (d->n > 65535 || d->h > (1 << 19) || d->w > (1 << 19))      // (grid limits; element offsets are 64-bit)
    return fail(JR_ERR_INVALID, "conv bwd_image: tensor too large");
  if (d->c_in > 4) return fail(JR_ERR_UNSUPPORTED, "conv bwd_image: c_in above 4 (use jr_conv2d_bwd_data)");
  if (d->kh > kImgMaxK || d->kw > kImgMaxK) return fail(JR_ERR_UNSUPPORTED, "conv bwd_image: kernel larger than 7x7");
  if ((d->stride_h != 1 && d->stride_h != 2) || (d->stride_w != 1 && d->stride_w != 2))
    return fail(JR_ERR_UNSUPPORTED, "conv bwd_image: stride must be 1 or 2");
  if (d->c_out % 16 != 0) return fail(JR_ERR_UNSUPPORTED, "conv bwd_image: c_out must be a multiple of 16");
  const int tile = img_lds_bytes(d, 16) <= kImgMaxLds ? 16 : 8;
  const size_t lds = img_lds_bytes(d, tile);
  if (lds > kImgMaxLds)
    return fail(JR_ERR_UNSUPPORTED, "conv bwd_image: the dy patch of 8x8 pixels and the filter exceed 48 KiB of LDS");
  hipStream_t s = as_stream(stream);
  const dim3 grid((d->w + tile - 1) / tile, (d->h + tile - 1) / tile, d->n);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    if (tile == 16)
      hipLaunchKernelGGL((k_conv_bwd_image<T, 16>), grid, dim3(256), lds, s, *d, (const T*)dy, w, dx, dx_c_stride);
    else
      hipLaunchKernelGGL((k_conv_bwd_image<T, 8>), grid, dim3(64), lds, s, *d, (const T*)dy, w, dx, dx_c_stride);
  });
  return check_launch("conv bwd_image");
}

JR_API int jr_attr_scale_input(int dtype, const void* src, void* dst, int64_t n, float alpha, void* stream) {
  if (dtype != JR_F32 && dtype != JR_BF16) return fail(JR_ERR_INVALID, "attr_scale_input: bad dtype");
  if (!src || !dst) return fail(JR_ERR_INVALID, "attr_scale_input: null pointer");
  if (n <= 0 || n >= (1LL << 39)) return fail(JR_ERR_INVALID, "attr_scale_input: bad element count");
  hipStream_t s = as_stream(stream);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_attr_scale<T>, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, (const T*)src, (T*)dst, n,
                       alpha);
  });
  return check_launch("attr_scale_input");
}

JR_API int jr_attr_accumulate(const float* dx, float* acc, int64_t n, float weight, int first, void* stream) {
  if (!dx || !acc) return fail(JR_ERR_INVALID, "attr_accumulate: null pointer");
  if (n <= 0 || n >= (1LL << 39)) return fail(JR_ERR_INVALID, "attr_accumulate: bad element count");
  hipLaunchKernelGGL(k_attr_accumulate, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, as_stream(stream), dx, acc, n,
                     weight, first ? 1 : 0);
  return check_launch("attr_accumulate");
}

JR_API int jr_attr_map(int mode, const float* acc, int32_t acc_c_stride, const void* x, int dtype,
                       int32_t x_c_stride, int64_t pixels, int32_t c, float* map, void* stream) {
  if (mode != JR_ATTR_ABSMAX && mode != JR_ATTR_DOT_INPUT) return fail(JR_ERR_INVALID, "attr_map: bad mode");
  if (dtype != JR_F32 && dtype != JR_BF16) return fail(JR_ERR_INVALID, "attr_map: bad dtype");
  if (!acc || !map || (mode == JR_ATTR_DOT_INPUT && !x)) return fail(JR_ERR_INVALID, "attr_map: null pointer");
  if (pixels <= 0 || pixels >= (1LL << 39) || c <= 0) return fail(JR_ERR_INVALID, "attr_map: bad sizes");
  if (c != 3) return fail(JR_ERR_UNSUPPORTED, "attr_map: c must be 3");
  if (acc_c_stride < c || (mode == JR_ATTR_DOT_INPUT && x_c_stride < c))
    return fail(JR_ERR_INVALID, "attr_map: channel stride below c");
  hipStream_t s = as_stream(stream);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_attr_map<T>, dim3((unsigned)ceil_div(pixels, 256)), dim3(256), 0, s, mode, acc, acc_c_stride,
                       (const T*)x, x_c_stride, pixels, map);
  });
  return check_launch("attr_map");
}
