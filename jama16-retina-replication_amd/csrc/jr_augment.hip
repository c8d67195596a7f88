// jr_augment.hip — on-device training augmentation of a uint8 batch
// (jr_image_u8_augment_nhwc): left-right / up-down flips, hue and saturation
// (one HSV round trip), contrast about the per-image channel mean, brightness,
// clamp to [0, 1]; per image from a device table of jr_augment_param.  The
// reference has no augmentation: jr.h states the transform.
//
// Two launches on the caller's stream, no host sync, no allocation:
//   k_aug_sums   per image with contrast_factor != 1: the per-channel sums of
//                the image after the HSV stage, one fp32 partial triple per
//                kChunk source pixels (thread -> wave shuffle -> LDS -> one
//                slot of the workspace).  The slot count depends on (h, w)
//                alone and no atomics are used, so a mean is bitwise the same
//                whatever the batch size or the image's slot.  The parameter
//                table lives on the device, so the launch is unconditional;
//                blocks of images with contrast_factor == 1 leave at once.
//   k_aug_apply  one lane per destination pixel: combines the image's partials
//                in slot order in fp64, re-reads the uint8 source (the flip is
//                a source-address transform), redoes the convert and the HSV
//                stage and applies contrast, brightness and the clamp; one
//                8- or 16-byte store per pixel when dst_stride is 4
//                (or 8 for bf16, the engine's input width).
// Every skipped stage leaves the value untouched, so the identity table gives
// jr_image_u8_to_nhwc's output bit for bit.  Compiled with -ffp-contract=off
// (Makefile): each multiply and add rounds on its own, the IEEE fp32
// evaluation of the formulas in jr.h.
#include "jr_common.h"

namespace jr {

constexpr int kAugChunk = 2048;        // source pixels per partial: 256 threads x 8
constexpr int kAugMaxBlocks = 2048;    // pass-2 grid cap (grid-stride beyond)

static int aug_partials(int32_t h, int32_t w) { return (int)ceil_div((int64_t)h * w, kAugChunk); }

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// x mod 6 in [0, 6): fmodf is exact; a tiny negative remainder plus 6 can round to 6
__device__ __forceinline__ float mod6(float x) {
  float r = fmodf(x, 6.f);
  if (r < 0.f) r = __fadd_rn(r, 6.f);
  if (r >= 6.f) r = __fsub_rn(r, 6.f);
  return r;
}

// f(n) of the HSV -> RGB step; h in [0, 6), n in {1, 3, 5}: h + n < 12, so one
// conditional subtraction is the exact mod 6
__device__ __forceinline__ float hsv_f(float h, float n, float v, float vs) {
  float k = __fadd_rn(h, n);
  if (k >= 6.f) k = __fsub_rn(k, 6.f);
  const float t = clamp01(fminf(k, __fsub_rn(4.f, k)));
  return __fsub_rn(v, __fmul_rn(vs, t));
}

// stage 2: hue shift by hd (turns) and saturation scale by sf, in place
__device__ __forceinline__ void hue_sat(float& r, float& g, float& b, float hd, float sf) {
  const float v = fmaxf(r, fmaxf(g, b)), m = fminf(r, fminf(g, b));
  const float c = __fsub_rn(v, m);
  const float s = v > 0.f ? __fdiv_rn(c, v) : 0.f;
  float h6;
  if (c == 0.f) h6 = 0.f;
  else if (v == r) h6 = __fdiv_rn(__fsub_rn(g, b), c);
  else if (v == g) h6 = __fadd_rn(__fdiv_rn(__fsub_rn(b, r), c), 2.f);
  else h6 = __fadd_rn(__fdiv_rn(__fsub_rn(r, g), c), 4.f);
  const float h = mod6(__fadd_rn(h6, __fmul_rn(6.f, hd)));
  const float vs = __fmul_rn(v, clamp01(__fmul_rn(s, sf)));
  r = hsv_f(h, 5.f, v, vs);
  g = hsv_f(h, 3.f, v, vs);
  b = hsv_f(h, 1.f, v, vs);
}

// stages 0 and 2 of one source pixel
__device__ __forceinline__ void load_pixel(const uint8_t* __restrict__ s, bool hsv, float hd, float sf, float& r,
                                           float& g, float& b) {
  const float scale = 1.0f / 255.0f;
  r = __fmul_rn((float)s[0], scale);
  g = __fmul_rn((float)s[1], scale);
  b = __fmul_rn((float)s[2], scale);
  if (hsv) hue_sat(r, g, b, hd, sf);
}

// grid (P, n): block (p, i) sums source pixels [p * kAugChunk, ...) of image i
__global__ void __launch_bounds__(256) k_aug_sums(const uint8_t* __restrict__ src,
                                                  const jr_augment_param* __restrict__ params, int hw,
                                                  float* __restrict__ part) {
  const int img = blockIdx.y, P = gridDim.x;
  const jr_augment_param pr = params[img];
  if (pr.contrast_factor == 1.f) return;
  const bool hsv = !(pr.hue_delta == 0.f && pr.sat_factor == 1.f);
  const uint8_t* s = src + (int64_t)img * hw * 3;
  const int p0 = blockIdx.x * kAugChunk;
  float sr = 0.f, sg = 0.f, sb = 0.f;
#pragma unroll
  for (int k = 0; k < kAugChunk / 256; ++k) {
    const int p = p0 + k * 256 + (int)threadIdx.x;
    if (p < hw) {
      float r, g, b;
      load_pixel(s + (int64_t)p * 3, hsv, pr.hue_delta, pr.sat_factor, r, g, b);
      sr = __fadd_rn(sr, r);
      sg = __fadd_rn(sg, g);
      sb = __fadd_rn(sb, b);
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    sr = __fadd_rn(sr, __shfl_xor(sr, o, 64));
    sg = __fadd_rn(sg, __shfl_xor(sg, o, 64));
    sb = __fadd_rn(sb, __shfl_xor(sb, o, 64));
  }
  __shared__ float red[4][3];
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = sr;
    red[threadIdx.x >> 6][1] = sg;
    red[threadIdx.x >> 6][2] = sb;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int c = threadIdx.x;
    part[((int64_t)img * P + blockIdx.x) * 4 + c] =
        __fadd_rn(__fadd_rn(red[0][c], red[1][c]), __fadd_rn(red[2][c], red[3][c]));
  }
}

// grid (blocks per image, n), grid-stride over the image's destination pixels
// VEC = dst_stride when one aligned vector store covers the pixel (4: fp32 16 B
// or bf16 8 B; 8: bf16 16 B, the engine's bf16 input), 0: element stores
template <typename T, int VEC>
__global__ void __launch_bounds__(256) k_aug_apply(const uint8_t* __restrict__ src, T* __restrict__ dst,
                                                   const jr_augment_param* __restrict__ params, int h, int w, int ds,
                                                   int P, const float* __restrict__ part) {
  const int img = blockIdx.y, hw = h * w;
  const jr_augment_param pr = params[img];
  const bool hsv = !(pr.hue_delta == 0.f && pr.sat_factor == 1.f);
  const bool contrast = pr.contrast_factor != 1.f, bright = pr.brightness_delta != 0.f;
  const bool flip_lr = pr.flags & 1u, flip_ud = pr.flags & 2u;
  __shared__ float s_mean[3];
  if (contrast) {   // block-uniform
    if (threadIdx.x < 3) {
      const float* q = part + (int64_t)img * P * 4 + threadIdx.x;
      double a = 0.0;
      for (int i = 0; i < P; ++i) a += (double)q[(int64_t)i * 4];
      s_mean[threadIdx.x] = (float)(a / (double)hw);
    }
    __syncthreads();
  }
  float mr = 0.f, mg = 0.f, mb = 0.f;
  if (contrast) {
    mr = s_mean[0];
    mg = s_mean[1];
    mb = s_mean[2];
  }
  const uint8_t* s = src + (int64_t)img * hw * 3;
  T* d = dst + (int64_t)img * hw * ds;
  for (int p = blockIdx.x * 256 + (int)threadIdx.x; p < hw; p += (int)gridDim.x * 256) {
    const int y = p / w, x = p - y * w;
    const int sy = flip_ud ? h - 1 - y : y, sx = flip_lr ? w - 1 - x : x;
    float v[3];
    load_pixel(s + ((int64_t)sy * w + sx) * 3, hsv, pr.hue_delta, pr.sat_factor, v[0], v[1], v[2]);
    if (contrast) {
      v[0] = __fadd_rn(__fmul_rn(__fsub_rn(v[0], mr), pr.contrast_factor), mr);
      v[1] = __fadd_rn(__fmul_rn(__fsub_rn(v[1], mg), pr.contrast_factor), mg);
      v[2] = __fadd_rn(__fmul_rn(__fsub_rn(v[2], mb), pr.contrast_factor), mb);
    }
    if (bright) {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = __fadd_rn(v[c], pr.brightness_delta);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = clamp01(v[c]);
    T* o = d + (int64_t)p * ds;
    if constexpr (VEC == 4 && sizeof(T) == 4) {
      *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], 0.f);
    } else if constexpr (VEC == 4) {
      *reinterpret_cast<uint2*>(o) = make_uint2(f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16), f2bf(v[2]));
    } else if constexpr (VEC == 8) {
      *reinterpret_cast<uint4*>(o) = make_uint4(f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16), f2bf(v[2]), 0u, 0u);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) Elt<T>::st(o + c, v[c]);
      for (int c = 3; c < ds; ++c) Elt<T>::st(o + c, 0.f);
    }
  }
}

template <typename T>
static void launch_apply(const uint8_t* src, void* dst, int n, int h, int w, int ds, const jr_augment_param* params,
                         int P, const float* part, hipStream_t s) {
  const int bpi = (int)std::min<int64_t>(ceil_div((int64_t)h * w, 256), std::max(1, kAugMaxBlocks / n));
  const dim3 grid(bpi, n);
  const bool aligned = ((uintptr_t)dst & ((size_t)ds * sizeof(T) - 1)) == 0;
  if (ds == 4 && aligned)
    hipLaunchKernelGGL((k_aug_apply<T, 4>), grid, dim3(256), 0, s, src, (T*)dst, params, h, w, ds, P, part);
  else if (ds == 8 && sizeof(T) == 2 && aligned)
    hipLaunchKernelGGL((k_aug_apply<T, 8>), grid, dim3(256), 0, s, src, (T*)dst, params, h, w, ds, P, part);
  else
    hipLaunchKernelGGL((k_aug_apply<T, 0>), grid, dim3(256), 0, s, src, (T*)dst, params, h, w, ds, P, part);
}

// geometry both entry points accept: the batch is the grid's y extent and an
// image's pixel count stays far inside int32
static bool aug_geometry_ok(int32_t n, int32_t h, int32_t w) {
  return n > 0 && n <= 65535 && h > 0 && w > 0 && (int64_t)h * w <= (int64_t)1 << 28;
}

}  // namespace jr

using namespace jr;

JR_API size_t jr_augment_workspace_size(int32_t n, int32_t h, int32_t w) {
  if (!aug_geometry_ok(n, h, w)) return 0;
  return (size_t)n * aug_partials(h, w) * 4 * sizeof(float);
}

JR_API int jr_image_u8_augment_nhwc(const uint8_t* src, void* dst, int dtype, int32_t n, int32_t h, int32_t w,
                                    int32_t c, int32_t dst_stride, const jr_augment_param* params, void* ws,
                                    size_t ws_bytes, void* stream) {
  if (!src || !dst || !params || !ws) return fail(JR_ERR_INVALID, "image_u8_augment: null pointer");
  if (c != 3) return fail(JR_ERR_INVALID, "image_u8_augment: c must be 3 (RGB)");
  if (dst_stride < 3) return fail(JR_ERR_INVALID, "image_u8_augment: dst_stride must be >= 3");
  if (dtype != JR_F32 && dtype != JR_BF16) return fail(JR_ERR_INVALID, "image_u8_augment: dtype must be JR_F32 or JR_BF16");
  if (n == 0) return JR_OK;
  if (!aug_geometry_ok(n, h, w)) return fail(JR_ERR_INVALID, "image_u8_augment: bad n / h / w");
  if (ws_bytes < jr_augment_workspace_size(n, h, w))
    return fail(JR_ERR_INVALID, "image_u8_augment: workspace smaller than jr_augment_workspace_size");
  if ((uintptr_t)ws & 3) return fail(JR_ERR_INVALID, "image_u8_augment: workspace must be 4-byte aligned");
  hipStream_t s = as_stream(stream);
  const int P = aug_partials(h, w);
  float* part = (float*)ws;
  hipLaunchKernelGGL(k_aug_sums, dim3(P, n), dim3(256), 0, s, src, params, h * w, part);
  if (int rc = check_launch("image_u8_augment sums")) return rc;
  by_dtype(dtype, [&](auto t) { launch_apply<decltype(t)>(src, dst, n, h, w, dst_stride, params, P, part, s); });
  return check_launch("image_u8_augment");
}
