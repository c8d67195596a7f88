// jr_bn_plan.h — host-only launch planning of the BatchNormalization + ReLU
// passes: the tunable constants, the chunk geometry that fixes the fp64
// summation grouping, grids, workspace sizes and offsets, argument validation,
// the segment tables and the batched backward's layout that the kernels take
// by value, and the two environment knobs.  Plain C++ (jr_bn_plan.cpp): it
// compiles and is tested without a device (tests/test_bn_plan.py pins its
// output through the C ABI).  The launchers of the BN kernels validate through
// it, read a plan and launch.
#pragma once
#include <cstddef>

#include "jr_error.h"

namespace jr {

// (an override must reach the planner and the kernels alike)
#ifndef JR_BN_MAX_CHUNKS
#define JR_BN_MAX_CHUNKS 1024
#endif
constexpr int kMaxChunks = JR_BN_MAX_CHUNKS;  // partial sums per channel (finalize reads them)
#ifndef JR_BN_MIN_ROWS
#define JR_BN_MIN_ROWS 16
#endif
constexpr int kMinRows = JR_BN_MIN_ROWS;      // rows per thread and chunk at least (chunk_geom)
#ifndef JR_BN_APP_UNROLL
#define JR_BN_APP_UNROLL 4
#endif
constexpr int kAppUnroll = JR_BN_APP_UNROLL;  // rows per thread in the elementwise passes

// The 8-lane combines (stats_combine8 of jr_common.h, bwd_combine8): lanes per
// channel, and the partials per channel they take -- the single-stage finalize,
// the folds and a jr_bn_relu_bwd_batch layer need nchunks <= kFoldMaxP.
constexpr int kStatsLanes = 8;
constexpr int kFoldMaxP = 512;
constexpr int kFoldCh = 256 / kStatsLanes;   // channels per folded apply / finalize8 block (32)
// partials per channel of the fused max-pool + BN backward (its grid's cap)
constexpr int kPoolBwdMaxParts = 4096;

// Backward inputs of one launch over the c channels of a conv launch's raw
// output: up to kMaxSegs channel segments (the members of a fused sibling
// group, jr_bn_relu_bwd_multi), each with its own upstream gradient slice
// and its own beta / dbeta (the members' tensors are separate).  A thread's
// channel vector is fixed, so it resolves its segment once.
// (BnSegs, ApplySegs, BnBatchLayer and BnBatch are kernel arguments: member
// order and types are part of the kernels' interface)
constexpr int kMaxSegs = 4;
struct BnSegs {
  const void* dy[kMaxSegs];
  const float* beta[kMaxSegs];
  float* dbeta[kMaxSegs];
  int dy_off[kMaxSegs], dy_stride[kMaxSegs];
  int c0[kMaxSegs + 1];   // first channel of each segment; c0[n] = c
  int n;
  // backward apply: NULL, or 64 words that receive max |dx| (atomicMax on the
  // bits of each block's max into word blockIdx.x % 64; JR_F32_X6H scales)
  float* absmax;
};

// The apply of a fused sibling launch's members in ONE launch
// (jr_bn_relu_apply_multi): the raw output's c channels, segment i its own
// output slice and beta.
struct ApplySegs {
  void* y[kMaxSegs];
  const float* beta[kMaxSegs];
  int y_off[kMaxSegs], y_stride[kMaxSegs];
  int c0[kMaxSegs + 1];
  int n;
};

// Several independent layers' backwards in ONE set of three launches
// (jr_bn_relu_bwd_batch): layer l owns blocks [b0, b0 + blocks) of each
// launch.
constexpr int kBnBatchMax = 8;
struct BnBatchLayer {
  BnSegs sg;
  const void* x;
  void* dx;
  const float* mean;
  const float* invstd;
  double* part;
  float* k1;
  float* k2;
  int64_t m;
  int c, xs, rpc, nchunks;
  int b0[3];   // first block in the reduce / finalize / apply launch
};
struct BnBatch {
  BnBatchLayer L[kBnBatchMax];
  int n;
};

inline int vec_width(int dtype) { return dtype == JR_BF16 ? 8 : 4; }
inline size_t elt_size(int dtype) { return dtype == JR_BF16 ? 2 : 4; }

// dtype, m, c of any BN entry point (more than 256 vectors per row:
// JR_ERR_UNSUPPORTED), and a channel slice [off, off + c) of rows `stride` wide
int check_common(int dtype, int64_t m, int c);
bool check_slice(int dtype, int off, int stride, int c);

// What the launches over m rows of c channels use (check_common passed): the
// jr_bn_launch_plan of jr.h.  Thread layout shared by every BN kernel: a row
// of c channels is tpr = c / vec_width threads; a 256-thread block covers
// rpp = 256 / tpr rows per pass.
jr_bn_launch_plan bn_plan(int dtype, int64_t m, int c);

// JR_FOLD_BN_BWD=1 (read once): the backward's finalize inside its apply
bool fold_bwd();

// Validates the segments of a jr_bn_relu_apply_multi / backward launch
// (pointers, channel counts, slices, channels summing to c) and fills the
// kernel's table.  nseg is 1..kMaxSegs (the callers check it first).
int apply_segs(int dtype, int nseg, const jr_bn_apply_seg* segs, int c, ApplySegs& sg);
int bwd_segs(int dtype, int nseg, const jr_bn_seg* segs, int c, BnSegs& sg, bool need_dbeta = true);
// Validates the segments and slices of a backward launch set; on success
// fills sg and moves x / dx to the slice's first channel.  need_dbeta = false
// (jr_bn_relu_bwd_frozen, which writes none): a segment's dbeta may be NULL.
int bwd_setup(int dtype, int nseg, const jr_bn_seg* segs, const void*& x, int32_t x_c_off, int32_t x_c_stride,
              int64_t m, int32_t c, const float* mean, const float* invstd, void*& dx, BnSegs& sg,
              bool need_dbeta = true);

// A batched backward: validates every layer (each as bwd_setup, at most
// kFoldMaxP chunks) and the workspace, lays the layers' partials out in ws
// (each layer's workspace_size, 256-byte aligned) and their blocks in the
// three launches; blocks[] receives the three grid sizes.
int bwd_batch_setup(int dtype, int32_t n, const jr_bn_bwd_layer* layers, void* ws, size_t ws_bytes, BnBatch& bt,
                    int blocks[3]);

// The fused max-pool + BN backward: one thread per (2x2 input cell, channel
// quad), a whole number of channel-quad rows per block, at most
// kPoolBwdMaxParts blocks (= partials per channel, which sizes the workspace)
struct PoolBwdGeom {
  int block, grid;
};
PoolBwdGeom pool_bwd_geom(const jr_pool_desc* d);
size_t pool_bwd_ws(int c);

}  // namespace jr
