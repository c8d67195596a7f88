// jr_bn_moving.hip — moving averages of the BN batch statistics, and the
// frozen (mean, invstd) a batch-independent forward normalises with.
//
// The reference's Keras BatchNormalization layers own moving_mean /
// moving_variance variables that its graph never updates (SURVEY.md App. C
// Q1); these two launches maintain them beside the training step and turn
// them into the [mean | invstd] layout every BN apply already reads.
// One launch each over a device segment table (jr_absmax_prep's convention):
// grid (ceil(max_c / 256), nseg, members), one thread per channel, no
// atomics, no LDS, no host sync -- capturable.  The formulas are the
// contract stated in jr.h; the file is compiled with -ffp-contract=off
// (Makefile) so every fp32 multiply and subtract rounds on its own.
#include "jr_common.h"

namespace jr {

// mm = mm - (mm - mean_b) d, mv = mv - (mv - var_b) d   (TF assign_moving_average)
__global__ void __launch_bounds__(256) k_bn_moving_update(const jr_bn_moving_seg* __restrict__ segs,
                                                          const float* __restrict__ stats, int64_t stats_ms,
                                                          float* __restrict__ moving, int64_t moving_ms,
                                                          float momentum, float eps) {
  const jr_bn_moving_seg sg = segs[blockIdx.y];
  const int ch = blockIdx.x * 256 + threadIdx.x;
  if (ch >= sg.c || sg.rows < 2) return;      // rows < 2: no unbiased variance, the segment is left as it is
  const float* st = stats + (int64_t)blockIdx.z * stats_ms + sg.stats_off;
  float* mo = moving + (int64_t)blockIdx.z * moving_ms + sg.moving_off;
  const float mean_b = st[ch];
  const double is = (double)st[sg.c + ch];
  double v = 1.0 / (is * is) - (double)eps;
  v = v < 0.0 ? 0.0 : v;
  v *= (double)sg.rows / (double)(sg.rows - 1);
  const float var_b = (float)v;
  const float d = __fsub_rn(1.0f, momentum);
  const float mm = mo[ch], mv = mo[sg.c + ch];
  mo[ch] = __fsub_rn(mm, __fmul_rn(__fsub_rn(mm, mean_b), d));
  mo[sg.c + ch] = __fsub_rn(mv, __fmul_rn(__fsub_rn(mv, var_b), d));
}

__global__ void __launch_bounds__(256) k_bn_moving_freeze(const jr_bn_moving_seg* __restrict__ segs,
                                                          const float* __restrict__ moving, int64_t moving_ms,
                                                          float* __restrict__ frozen, int64_t frozen_ms, float eps) {
  const jr_bn_moving_seg sg = segs[blockIdx.y];
  const int ch = blockIdx.x * 256 + threadIdx.x;
  if (ch >= sg.c) return;
  const float* mo = moving + (int64_t)blockIdx.z * moving_ms + sg.moving_off;
  float* fr = frozen + (int64_t)blockIdx.z * frozen_ms + sg.stats_off;
  fr[ch] = mo[ch];
  fr[sg.c + ch] = (float)(1.0 / sqrt((double)mo[sg.c + ch] + (double)eps));
}

static const char* bad_table(const void* segs, int32_t nseg, int32_t max_c, int32_t members, const void* a,
                             int64_t a_ms, const void* b, int64_t b_ms, float eps) {
  if (!segs || !a || !b) return "null pointer";
  if (nseg < 1 || nseg > 65535) return "nseg outside 1..65535";
  if (max_c < 1) return "max_c < 1";
  if (members < 1 || members > 65535) return "members outside 1..65535";
  if (a_ms < 0 || b_ms < 0) return "negative member stride";
  if (!(eps > 0.f)) return "eps must be > 0";
  return nullptr;
}

}  // namespace jr

using namespace jr;

JR_API int jr_bn_moving_update(const jr_bn_moving_seg* segs, int32_t nseg, int32_t max_c, int32_t members,
                               const float* stats, int64_t stats_member_stride, float* moving,
                               int64_t moving_member_stride, float momentum, float eps, void* stream) {
  if (const char* why = bad_table(segs, nseg, max_c, members, stats, stats_member_stride, moving,
                                  moving_member_stride, eps))
    return fail(JR_ERR_INVALID, std::string("bn_moving_update: ") + why);
  if (!(momentum >= 0.f && momentum <= 1.f)) return fail(JR_ERR_INVALID, "bn_moving_update: momentum outside [0, 1]");
  hipLaunchKernelGGL(k_bn_moving_update, dim3((max_c + 255) / 256, nseg, members), dim3(256), 0, as_stream(stream),
                     segs, stats, stats_member_stride, moving, moving_member_stride, momentum, eps);
  return check_launch("bn_moving_update");
}

JR_API int jr_bn_moving_freeze(const jr_bn_moving_seg* segs, int32_t nseg, int32_t max_c, int32_t members,
                               const float* moving, int64_t moving_member_stride, float* frozen,
                               int64_t frozen_member_stride, float eps, void* stream) {
  if (const char* why = bad_table(segs, nseg, max_c, members, moving, moving_member_stride, frozen,
                                  frozen_member_stride, eps))
    return fail(JR_ERR_INVALID, std::string("bn_moving_freeze: ") + why);
  hipLaunchKernelGGL(k_bn_moving_freeze, dim3((max_c + 255) / 256, nseg, members), dim3(256), 0, as_stream(stream),
                     segs, moving, moving_member_stride, frozen, frozen_member_stride, eps);
  return check_launch("bn_moving_freeze");
}
