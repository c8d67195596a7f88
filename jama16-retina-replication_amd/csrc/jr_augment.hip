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
//
// jr_image_u8_warp_augment_nhwc adds a per-image affine resampling (rotation,
// zoom, shift: a jr_warp_param per image) in front of the HSV stage.  It is a
// gather: a row of destination pixels reads a slanted line of the source.
//   k_warp_sums   k_aug_sums over DESTINATION pixels after the warp and the HSV
//                 stage (fill pixels count): the same slots, the same pixel
//                 order and lane assignment, so at the identity matrix the
//                 mean is k_aug_sums' bit for bit; a block's 2048 pixels are a
//                 band of a few rows, its source footprint a slanted band
//   k_warp_apply  walks 16 x 16 destination tiles, one pixel per lane, so a
//                 block's source footprint is a compact patch that L1 / L2
//                 serve (no LDS staging; timings in DESIGN.md): flip, source position, outside
//                 test, four guarded taps, the two lerps, then the stages and
//                 the stores of k_aug_apply
// With fx == fy == 0 the lerps return the first tap bit for bit, so a matrix
// that maps the pixel lattice onto itself is a pure permutation.
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

// one block's channel sums into its partial slot: thread -> wave shuffle -> LDS
// -> three stores (every thread of the 256 calls)
__device__ __forceinline__ void block_partial(float sr, float sg, float sb, float* __restrict__ slot) {
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
    slot[c] = __fadd_rn(__fadd_rn(red[0][c], red[1][c]), __fadd_rn(red[2][c], red[3][c]));
  }
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
  block_partial(sr, sg, sb, part + ((int64_t)img * P + blockIdx.x) * 4);
}

// the contrast mean of one image from its P partial triples, in slot order in
// fp64 (block-uniform `contrast`; every thread of the block calls)
__device__ __forceinline__ void image_mean(bool contrast, const float* __restrict__ part, int P, int hw,
                                           float (&mean)[3]) {
  __shared__ float s_mean[3];
  mean[0] = mean[1] = mean[2] = 0.f;
  if (!contrast) return;
  if (threadIdx.x < 3) {
    const float* q = part + threadIdx.x;
    double a = 0.0;
    for (int i = 0; i < P; ++i) a += (double)q[(int64_t)i * 4];
    s_mean[threadIdx.x] = (float)(a / (double)hw);
  }
  __syncthreads();
  mean[0] = s_mean[0];
  mean[1] = s_mean[1];
  mean[2] = s_mean[2];
}

// stages 3 - 5 of one pixel after stage 2 and its store at o
// VEC = dst_stride when one aligned vector store covers the pixel (4: fp32 16 B
// or bf16 8 B; 8: bf16 16 B, the engine's bf16 input), 0: element stores
template <typename T, int VEC>
__device__ __forceinline__ void finish_pixel(float (&v)[3], const jr_augment_param& pr, bool contrast, bool bright,
                                             const float (&mean)[3], T* __restrict__ o, int ds) {
  if (contrast) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = __fadd_rn(__fmul_rn(__fsub_rn(v[c], mean[c]), pr.contrast_factor), mean[c]);
  }
  if (bright) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = __fadd_rn(v[c], pr.brightness_delta);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = clamp01(v[c]);
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

// grid (blocks per image, n), grid-stride over the image's destination pixels
template <typename T, int VEC>
__global__ void __launch_bounds__(256) k_aug_apply(const uint8_t* __restrict__ src, T* __restrict__ dst,
                                                   const jr_augment_param* __restrict__ params, int h, int w, int ds,
                                                   int P, const float* __restrict__ part) {
  const int img = blockIdx.y, hw = h * w;
  const jr_augment_param pr = params[img];
  const bool hsv = !(pr.hue_delta == 0.f && pr.sat_factor == 1.f);
  const bool contrast = pr.contrast_factor != 1.f, bright = pr.brightness_delta != 0.f;
  const bool flip_lr = pr.flags & 1u, flip_ud = pr.flags & 2u;
  float mean[3];
  image_mean(contrast, part + (int64_t)img * P * 4, P, hw, mean);
  const uint8_t* s = src + (int64_t)img * hw * 3;
  T* d = dst + (int64_t)img * hw * ds;
  for (int p = blockIdx.x * 256 + (int)threadIdx.x; p < hw; p += (int)gridDim.x * 256) {
    const int y = p / w, x = p - y * w;
    const int sy = flip_ud ? h - 1 - y : y, sx = flip_lr ? w - 1 - x : x;
    float v[3];
    load_pixel(s + ((int64_t)sy * w + sx) * 3, hsv, pr.hue_delta, pr.sat_factor, v[0], v[1], v[2]);
    finish_pixel<T, VEC>(v, pr, contrast, bright, mean, d + (int64_t)p * ds, ds);
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

constexpr int kWarpTile = 16;          // destination tile edge: 16 x 16 pixels, one per lane

// tap (x, y) of the bilinear footprint: the stage-0 value of that source pixel,
// 0 outside the image (no address is formed there)
__device__ __forceinline__ void warp_tap(const uint8_t* __restrict__ s, int h, int w, int x, int y, float (&p)[3]) {
  const float scale = 1.0f / 255.0f;
  p[0] = p[1] = p[2] = 0.f;
  if ((unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h) {
    const uint8_t* q = s + ((int64_t)y * w + x) * 3;
    p[0] = __fmul_rn((float)q[0], scale);
    p[1] = __fmul_rn((float)q[1], scale);
    p[2] = __fmul_rn((float)q[2], scale);
  }
}

__device__ __forceinline__ float lerp_rn(float a, float b, float f) { return __fadd_rn(a, __fmul_rn(f, __fsub_rn(b, a))); }

// stages 0 - 2 of destination pixel (x, y) of the warp entry point (jr.h 1a - 1d, then hue / saturation)
__device__ __forceinline__ void warp_pixel(const uint8_t* __restrict__ s, int h, int w, const jr_augment_param& pr,
                                           const jr_warp_param& wp, bool hsv, int x, int y, float (&v)[3]) {
  const float xf = (float)((pr.flags & 1u) ? w - 1 - x : x), yf = (float)((pr.flags & 2u) ? h - 1 - y : y);
  const float u = __fadd_rn(__fadd_rn(__fmul_rn(wp.m[0], xf), __fmul_rn(wp.m[1], yf)), wp.m[2]);
  const float t = __fadd_rn(__fadd_rn(__fmul_rn(wp.m[3], xf), __fmul_rn(wp.m[4], yf)), wp.m[5]);
  v[0] = v[1] = v[2] = 0.f;
  if (u > -1.f && u < (float)w && t > -1.f && t < (float)h) {   // false for NaN and +-inf too
    const float x0f = floorf(u), y0f = floorf(t);
    const float fx = __fsub_rn(u, x0f), fy = __fsub_rn(t, y0f);
    const int x0 = (int)x0f, y0 = (int)y0f;                     // in [-1, w - 1] x [-1, h - 1]
    float p00[3], p10[3], p01[3], p11[3];
    warp_tap(s, h, w, x0, y0, p00);
    warp_tap(s, h, w, x0 + 1, y0, p10);
    warp_tap(s, h, w, x0, y0 + 1, p01);
    warp_tap(s, h, w, x0 + 1, y0 + 1, p11);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = lerp_rn(lerp_rn(p00[c], p10[c], fx), lerp_rn(p01[c], p11[c], fx), fy);
  }
  if (hsv) hue_sat(v[0], v[1], v[2], pr.hue_delta, pr.sat_factor);
}

// grid (P, n): block (p, i) sums destination pixels [p * kAugChunk, ...) of
// image i after stages 0 - 2, in the pixel order and lane assignment of
// k_aug_sums: at the identity matrix the partials, and so the mean, are its
// bits.  The flips permute the destination pixels and leave their sum's terms
// alone, so the walk is over (x', y') of jr.h 1a, whatever the flags.
__global__ void __launch_bounds__(256) k_warp_sums(const uint8_t* __restrict__ src,
                                                   const jr_augment_param* __restrict__ params,
                                                   const jr_warp_param* __restrict__ warps, int h, int w,
                                                   float* __restrict__ part) {
  const int img = blockIdx.y, P = gridDim.x, hw = h * w;
  jr_augment_param pr = params[img];
  if (pr.contrast_factor == 1.f) return;
  pr.flags = 0;
  const jr_warp_param wp = warps[img];
  const bool hsv = !(pr.hue_delta == 0.f && pr.sat_factor == 1.f);
  const uint8_t* s = src + (int64_t)img * hw * 3;
  const int p0 = blockIdx.x * kAugChunk;
  float sr = 0.f, sg = 0.f, sb = 0.f;
#pragma unroll 2
  for (int k = 0; k < kAugChunk / 256; ++k) {
    const int p = p0 + k * 256 + (int)threadIdx.x;
    if (p < hw) {
      const int y = p / w;
      float v[3];
      warp_pixel(s, h, w, pr, wp, hsv, p - y * w, y, v);
      sr = __fadd_rn(sr, v[0]);
      sg = __fadd_rn(sg, v[1]);
      sb = __fadd_rn(sb, v[2]);
    }
  }
  block_partial(sr, sg, sb, part + ((int64_t)img * P + blockIdx.x) * 4);
}

// grid (blocks per image, n), grid-stride over the image's T destination tiles
template <typename T_, int VEC>
__global__ void __launch_bounds__(256) k_warp_apply(const uint8_t* __restrict__ src, T_* __restrict__ dst,
                                                    const jr_augment_param* __restrict__ params,
                                                    const jr_warp_param* __restrict__ warps, int h, int w, int ds,
                                                    int tx, int T, int P, const float* __restrict__ part) {
  const int img = blockIdx.y, hw = h * w;
  const jr_augment_param pr = params[img];
  const jr_warp_param wp = warps[img];
  const bool hsv = !(pr.hue_delta == 0.f && pr.sat_factor == 1.f);
  const bool contrast = pr.contrast_factor != 1.f, bright = pr.brightness_delta != 0.f;
  float mean[3];
  image_mean(contrast, part + (int64_t)img * P * 4, P, hw, mean);
  const uint8_t* s = src + (int64_t)img * hw * 3;
  T_* d = dst + (int64_t)img * hw * ds;
  const int lx = threadIdx.x % kWarpTile, ly = threadIdx.x / kWarpTile;
  for (int t = blockIdx.x; t < T; t += (int)gridDim.x) {
    const int ty = t / tx, x = (t - ty * tx) * kWarpTile + lx, y = ty * kWarpTile + ly;
    if (x < w && y < h) {
      float v[3];
      warp_pixel(s, h, w, pr, wp, hsv, x, y, v);
      finish_pixel<T_, VEC>(v, pr, contrast, bright, mean, d + ((int64_t)y * w + x) * ds, ds);
    }
  }
}

template <typename T>
static void launch_warp_apply(const uint8_t* src, void* dst, int n, int h, int w, int ds,
                              const jr_augment_param* params, const jr_warp_param* warps, int tx, int tiles, int P,
                              const float* part, hipStream_t s) {
  const dim3 grid(std::min(tiles, std::max(1, kAugMaxBlocks / n)), n);
  const bool aligned = ((uintptr_t)dst & ((size_t)ds * sizeof(T) - 1)) == 0;
  if (ds == 4 && aligned)
    hipLaunchKernelGGL((k_warp_apply<T, 4>), grid, dim3(256), 0, s, src, (T*)dst, params, warps, h, w, ds, tx, tiles, P,
                       part);
  else if (ds == 8 && sizeof(T) == 2 && aligned)
    hipLaunchKernelGGL((k_warp_apply<T, 8>), grid, dim3(256), 0, s, src, (T*)dst, params, warps, h, w, ds, tx, tiles, P,
                       part);
  else
    hipLaunchKernelGGL((k_warp_apply<T, 0>), grid, dim3(256), 0, s, src, (T*)dst, params, warps, h, w, ds, tx, tiles, P,
                       part);
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

// what both entry points check before they launch (`null`: one of their
// pointers is); JR_OK to go on -- n == 0 passes and launches nothing
static int aug_check(const std::string& who, bool null, int dtype, int32_t n, int32_t h, int32_t w, int32_t c,
                     int32_t dst_stride, const void* ws, size_t ws_bytes) {
  if (null) return fail(JR_ERR_INVALID, who + ": null pointer");
  if (c != 3) return fail(JR_ERR_INVALID, who + ": c must be 3 (RGB)");
  if (dst_stride < 3) return fail(JR_ERR_INVALID, who + ": dst_stride must be >= 3");
  if (dtype != JR_F32 && dtype != JR_BF16) return fail(JR_ERR_INVALID, who + ": dtype must be JR_F32 or JR_BF16");
  if (n == 0) return JR_OK;
  if (!aug_geometry_ok(n, h, w)) return fail(JR_ERR_INVALID, who + ": bad n / h / w");
  if (ws_bytes < jr_augment_workspace_size(n, h, w))
    return fail(JR_ERR_INVALID, who + ": workspace smaller than jr_augment_workspace_size");
  if ((uintptr_t)ws & 3) return fail(JR_ERR_INVALID, who + ": workspace must be 4-byte aligned");
  return JR_OK;
}

JR_API int jr_image_u8_augment_nhwc(const uint8_t* src, void* dst, int dtype, int32_t n, int32_t h, int32_t w,
                                    int32_t c, int32_t dst_stride, const jr_augment_param* params, void* ws,
                                    size_t ws_bytes, void* stream) {
  if (int rc = aug_check("image_u8_augment", !src || !dst || !params || !ws, dtype, n, h, w, c, dst_stride, ws, ws_bytes))
    return rc;
  if (n == 0) return JR_OK;
  hipStream_t s = as_stream(stream);
  const int P = aug_partials(h, w);
  float* part = (float*)ws;
  hipLaunchKernelGGL(k_aug_sums, dim3(P, n), dim3(256), 0, s, src, params, h * w, part);
  if (int rc = check_launch("image_u8_augment sums")) return rc;
  by_dtype(dtype, [&](auto t) { launch_apply<decltype(t)>(src, dst, n, h, w, dst_stride, params, P, part, s); });
  return check_launch("image_u8_augment");
}

JR_API int jr_image_u8_warp_augment_nhwc(const uint8_t* src, void* dst, int dtype, int32_t n, int32_t h, int32_t w,
                                         int32_t c, int32_t dst_stride, const jr_augment_param* params,
                                         const jr_warp_param* warps, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = aug_check("image_u8_warp_augment", !src || !dst || !params || !warps || !ws, dtype, n, h, w, c,
                         dst_stride, ws, ws_bytes))
    return rc;
  if (n == 0) return JR_OK;
  hipStream_t s = as_stream(stream);
  const int P = aug_partials(h, w);
  // (h w <= 2^28: the tile count stays inside int32)
  const int tx = (int)ceil_div(w, kWarpTile), tiles = tx * (int)ceil_div(h, kWarpTile);
  float* part = (float*)ws;
  hipLaunchKernelGGL(k_warp_sums, dim3(P, n), dim3(256), 0, s, src, params, warps, h, w, part);
  if (int rc = check_launch("image_u8_warp_augment sums")) return rc;
  by_dtype(dtype, [&](auto t) {
    launch_warp_apply<decltype(t)>(src, dst, n, h, w, dst_stride, params, warps, tx, tiles, P, part, s);
  });
  return check_launch("image_u8_warp_augment");
}
