/*
 * jr.h — C-ABI of libjr.so, the MI355X (gfx950) compute library behind the
 * jama16-retina-replication hot path: the Inception-v3 training step and
 * ensemble inference of train.py / evaluate.py.
 *
 * The reference has no FFI: every op below replaces a TensorFlow op that the
 * reference graph instantiates.  Each entry point cites the
 * reference call site whose TF op it replaces.
 *
 * Conventions
 *  - Every function returns JR_OK (0) or a negative jr_status; the message of
 *    the last failure on the calling thread is returned by jr_last_error().
 *  - All tensor arguments are caller-owned DEVICE pointers (torch.Tensor
 *    .data_ptr() on the host side).  The library never allocates, except that
 *    multi-kernel ops take a caller-provided workspace sized by the matching
 *    *_workspace_size query.
 *  - Activations are NHWC (channels_last, lib/dataset.py:42-43); conv kernels
 *    are HWIO [kh][kw][cin][cout] (the Keras Conv2D layout).
 *  - A channel slice (c_off, c_stride) addresses channels
 *    [c_off, c_off + c) of a buffer whose pixel rows hold c_stride channels;
 *    this is how Inception-block outputs are written concat-free.
 *  - No host synchronisation inside any call; every call is enqueued on the
 *    given stream (hipStream_t passed as void*; NULL = the null stream), so a
 *    whole training step can be captured into a HIP graph.
 *  - dtype: JR_F32 = IEEE fp32 end to end (the reference's precision);
 *    JR_BF16 = bf16 activations/weights with fp32 accumulation;
 *    JR_F32_X8 (convolution entry points only) = fp32 tensors exactly as
 *    JR_F32, the GEMM products formed on the bf16 matrix cores: every fp32
 *    operand is split exactly into three bf16 terms (x = h + m + l) and eight
 *    bf16 MFMAs accumulate hh+hm+mh+mm+hl+lh+ml+lm in fp32; only l*l
 *    (< 2^-32 |a b|) is dropped, so every product is exact to far below
 *    fp32 rounding and the result differs from JR_F32 only in summation
 *    order (bf16x9-style fp32 emulation).  Non-finite inputs give NaN where
 *    JR_F32 could give +-inf.
 *    JR_F32_X8P (convolution entry points only) = the JR_F32_X8 arithmetic
 *    with the split done once, outside the GEMM: every operand arrives as its
 *    three bf16 planes h, m, l (x = h + m + l exactly; jr_split_x8p,
 *    jr_conv_weights_x8p*), stored back to back, each plane in the JR_BF16
 *    layout of that operand (channel radices padded to 8; fwd filter
 *    W^T [c_out][kh][kw][c8], bwd_data filter HWIO).  The plane stride is the
 *    plane's element count as the descriptor implies: n*h*w*x_c_stride (x),
 *    n*ho*wo*y_c_stride (dy), c_out*kh*kw*c8 (W^T), kh*kw*c_in*c_out (HWIO).
 *    Eight MFMAs per product in the JR_F32_X8 order; outputs (y, dx, dw) are
 *    fp32 exactly as for JR_F32.
 *    JR_F32_X6H (convolution entry points only) = fp32 tensors as JR_F32_X8,
 *    the products on the fp16 matrix cores: each operand is scaled by a
 *    power of two s that puts its largest magnitude (the descriptor's
 *    x/w/dy absmax or bound) in [2^14, 2^15) and split into three fp16 terms
 *    x s = h + m + l (11-bit significands: exact for |x s| >= 2^-1, i.e.
 *    down to 2^-15 of the tensor's max, and down to 2^-24 absolute through
 *    fp16 subnormals); six f16 MFMAs accumulate hh+hm+mh+mm+hl+lh in fp32
 *    (dropped: ml + lm < 2^-32 |a b| and l*l, the JR_F32_X8 class), and the
 *    result is scaled back exactly.  Same tiles, config ids, split-K and
 *    stream-K plans as JR_F32_X8; 3/4 of its MFMAs.  A magnitude above the
 *    stated bound saturates (wrong results): bounds must hold.  Where a
 *    host bound has no proof (activations under frozen BN statistics), the
 *    *_guard entry points check it on the device as the values are stored
 *    and report through jr_device_check instead of saturating in silence.
 */
#ifndef JR_H_
#define JR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum jr_status {
  JR_OK = 0,
  JR_ERR_INVALID = -1,     /* bad argument / unsupported geometry          */
  JR_ERR_HIP = -2,         /* a HIP runtime call failed                    */
  JR_ERR_UNSUPPORTED = -3, /* valid request this build does not implement  */
  JR_ERR_WORKSPACE = -4,   /* workspace smaller than *_workspace_size      */
  JR_ERR_DEVICE = -5       /* a kernel reported a device-side failure      */
} jr_status;

typedef enum jr_dtype { JR_F32 = 0, JR_BF16 = 1, JR_F32_X8 = 2, JR_F32_X8P = 3, JR_F32_X6H = 4 } jr_dtype;

typedef enum jr_conv_op { JR_CONV_FWD = 0, JR_CONV_BWD_DATA = 1, JR_CONV_BWD_FILTER = 2 } jr_conv_op;

typedef enum jr_head_mode { JR_HEAD_SIGMOID = 0, JR_HEAD_SOFTMAX = 1 } jr_head_mode;

/* One Conv2D(use_bias=False) layer of keras_applications inception_v3
 * conv2d_bn (instantiated at train.py:129-130).  pad_* are the top/left
 * paddings: 'same' at stride 1 => (k-1)/2, 'valid' => 0. */
typedef struct jr_conv_desc {
  int32_t n, h, w, c_in;          /* input  [n, h, w, c_in] (slice)        */
  int32_t c_out, kh, kw;          /* kernel [kh, kw, c_in, c_out]          */
  int32_t stride_h, stride_w;
  int32_t pad_h, pad_w;
  int32_t ho, wo;                 /* output [n, ho, wo, c_out] (slice)     */
  int32_t x_c_off, x_c_stride;    /* channel slice of the input buffer     */
  int32_t y_c_off, y_c_stride;    /* channel slice of the output buffer    */
  /* JR_F32_X6H only (ignored by every other dtype; zero-initialise): the
   * largest magnitude of x, of the filter block w and of dy, which set each
   * operand's power-of-two scale.  *_absmax: NULL, or 64 device floats whose
   * maximum is (an upper bound of) max |tensor| -- jr_absmax_prep for
   * filters, jr_bn_relu_bwd_multi_absmax / jr_bn_relu_bwd_maxpool_absmax for
   * a data gradient; when NULL, *_bound is a host upper bound.  A stated
   * magnitude m > 0 gives the scale s = 2^k with m s in [2^14, 2^15) (k <=
   * 100), exactly 2^14 when m is a power of two: values up to twice a
   * power-of-two bound still split exactly.  A bound (or a words' maximum) of
   * 0 -- or negative, inf or NaN -- gives s = 1: the operand is split as it
   * is, which is right for magnitudes below 2^15, exact from 2^-1 up and to
   * 2^-24 absolute below. */
  const float* x_absmax;
  const float* w_absmax;
  const float* dy_absmax;
  float x_bound, w_bound, dy_bound;
} jr_conv_desc;

/* 3x3 pooling window; max: stride 2 'valid', avg: stride 1 'same' with the
 * TF exclude-padding divisor. */
typedef struct jr_pool_desc {
  int32_t n, h, w, c;
  int32_t ho, wo;
  int32_t x_c_off, x_c_stride;
  int32_t y_c_off, y_c_stride;
} jr_pool_desc;

/* ---- library ---------------------------------------------------------- */
int jr_init(int device);
const char* jr_last_error(void);
const char* jr_version(void);
/* Device-side failures of the launches on the CURRENT device since the last
 * check (call it after synchronising the streams that ran them): JR_OK, or
 * JR_ERR_DEVICE when a stream-K hand-off word was not left zero: either a
 * kernel counted a count found past its tile's piece count into the
 * library's device error word, or a hand-off word of a stream with no work
 * in flight is non-zero (a stale count below the piece count, which makes a
 * tile complete early; the words of every idle stream are scanned here).
 * The same error word counts the magnitude guards: a jr_absmax_prep segment
 * above its limit, or a block of a *_guard entry point that stored an
 * activation above its limit.
 * The outputs of the launches since the last check are then invalid.
 * Stream-K blocks never wait for one another, so no timeout exists.  On
 * JR_ERR_DEVICE the call synchronises the device, re-zeroes every stream-K
 * hand-off word and the error word, so the NEXT launches are correct.
 * Host-synchronising (a 4-byte copy plus the used hand-off words of each
 * idle stream; the repair path a device sync). */
int jr_device_check(void);
/* Diagnostics (tests): set every stream-K hand-off word of `stream` (the
 * current device's) to `value`, in stream order -- the next stream-K launch
 * there then miscounts and must be reported by jr_device_check. */
int jr_debug_poison_sk_counts(void* stream, uint32_t value);


/* ---- convolution (train.py:129-130 -> Keras Conv2D -> TF Conv2D,
 *      Conv2DBackpropInput, Conv2DBackpropFilter created by .minimize at
 *      train.py:150-153) ----------------------------------------------- */
/* c_out must be a multiple of 16.  Channel offsets/strides are multiples
 * of q = 4 (JR_F32) or 8 (JR_BF16) elements (one 16 B DMA piece).  c_in % q
 * != 0 (the 3-channel image of conv1) is supported for fwd / bwd_filter by
 * virtual padding to cq = round_up(c_in, q): the input buffer must hold cq
 * channels per pixel (x_c_off + cq <= x_c_stride) and channels [c_in, cq)
 * must be finite (zero).
 * Filter layouts: JR_F32 fwd / bwd_data and JR_BF16 bwd_data take the HWIO
 * kernel [kh][kw][c_in][c_out]; JR_BF16 fwd takes it transposed and padded,
 * [c_out][kh][kw][cq] (jr_conv_weights_bf16 produces both bf16 layouts);
 * bwd_filter writes fp32 HWIO for both dtypes.  JR_BF16 activations,
 * outputs and dx are bf16 (accumulation in fp32 MFMA, rounded once). */
size_t jr_conv2d_workspace_size(const jr_conv_desc* d, int op, int dtype);
/* y[.., y_c_off + co] = sum x * w   (raw conv output, no bias) */
int jr_conv2d_fwd(const jr_conv_desc* d, int dtype, const void* x, const void* w, void* y,
                  void* ws, size_t ws_bytes, void* stream);
/* jr_conv2d_fwd fused with the training-mode BatchNormalization statistics
 * of its output (Keras conv2d_bn: Conv2D -> BatchNormalization, App. C Q1):
 * mean[co] = E[y], invstd[co] = 1/sqrt(biased var + eps) over n*ho*wo rows,
 * of y as stored (bf16-rounded for JR_BF16).  Partial (mean, M2) per group
 * of rows from the GEMM epilogue (or the split-K reduce), combined in fp64
 * in a fixed order: deterministic.  Replaces jr_conv2d_fwd + jr_bn_stats. */
int jr_conv2d_fwd_bn_stats(const jr_conv_desc* d, int dtype, const void* x, const void* w, void* y, float eps,
                           float* mean, float* invstd, void* ws, size_t ws_bytes, void* stream);
/* Grouped jr_conv2d_fwd_bn_stats for the members of an ensemble (evaluate.py
 * -lm: the same layer of `members` models over the same batch, replacing the
 * reference's per-model sess.run of evaluate.py:166-211): ONE launch per GEMM,
 * member i reading x + i*x_member_stride and w + i*w_member_stride and
 * writing y + i*y_member_stride, mean / invstd + i*stats_member_stride
 * (strides in elements of each tensor; w = the filter operand of that dtype:
 * fp32 HWIO, or the bf16 W^T copy for JR_BF16).  dtype JR_F32, JR_BF16,
 * JR_F32_X8 or JR_F32_X6H (member i's magnitude words at x_absmax / w_absmax
 * + 64 i floats).  Each member's plan (tile, split-K) is the per-member plan, so
 * its y, mean and invstd are bitwise those of jr_conv2d_fwd_bn_stats on its
 * own tensors.  Workspace: jr_conv2d_workspace_size_grouped. */
size_t jr_conv2d_workspace_size_grouped(const jr_conv_desc* d, int dtype, int members);
int jr_conv2d_fwd_bn_stats_grouped(const jr_conv_desc* d, int dtype, int members, const void* x,
                                   int64_t x_member_stride, const void* w, int64_t w_member_stride, void* y,
                                   int64_t y_member_stride, float eps, float* mean, float* invstd,
                                   int64_t stats_member_stride, void* ws, size_t ws_bytes, void* stream);
/* The statistics finalize folded into the BN apply (a kernel boundary fewer
 * per conv2d_bn layer): jr_conv2d_bn_partials_layout says where the planned
 * forward GEMM of this geometry leaves its BN-statistics partials in the
 * workspace -- [2][N][P] fp32 (mean, M2) of R rows each (the last group the
 * rest of the M rows) at ws + ws_offset -- and whether they are single-stage;
 * jr_conv2d_fwd_bn_partials is jr_conv2d_fwd_bn_stats without the finalize
 * (JR_ERR_UNSUPPORTED for two-stage partials); jr_bn_relu_apply_stats then
 * combines the partials of its channels (bitwise the statistics
 * jr_conv2d_fwd_bn_stats writes), applies BN + ReLU and writes mean / invstd
 * for the backward.  The partials stay valid until the next call that uses
 * the same workspace. */
typedef struct jr_bn_partials {
  int64_t ws_offset;
  int32_t P, R, M, N;
  int32_t single_stage;
} jr_bn_partials;
int jr_conv2d_bn_partials_layout(const jr_conv_desc* d, int dtype, jr_bn_partials* out);
int jr_conv2d_fwd_bn_partials(const jr_conv_desc* d, int dtype, const void* x, const void* w, void* y, void* ws,
                              size_t ws_bytes, void* stream);
/* dx[.., x_c_off + ci] (+)= sum dy * w ; accumulate != 0 adds into dx */
int jr_conv2d_bwd_data(const jr_conv_desc* d, int dtype, const void* dy, const void* w, void* dx,
                       int accumulate, void* ws, size_t ws_bytes, void* stream);
/* dw[kh][kw][ci][co] = sum x * dy  (fp32 output for both dtypes) */
int jr_conv2d_bwd_filter(const jr_conv_desc* d, int dtype, const void* x, const void* dy, float* dw,
                         void* ws, size_t ws_bytes, void* stream);

/* Deferred filter-gradient reduce (one launch for many layers).  When the
 * planned bwd_filter GEMM of a layer splits K (jr_conv2d_wgrad_seg: splits
 * > 1), jr_conv2d_bwd_filter_slabs writes its fp32 partial slabs
 * [splits][m][n] (splits * m * n * 4 bytes) into caller memory and returns;
 * jr_wgrad_reduce later sums the slabs of every listed layer into its dw in
 * ONE launch, bitwise equal to jr_conv2d_bwd_filter's own reduce.  segs is
 * a DEVICE array; each entry is filled by jr_conv2d_wgrad_seg (geometry,
 * lanes g, blocks) plus the caller's slabs / dw pointers and block0 = the
 * exclusive prefix sum of blocks (total_blocks = the sum).  slab_bytes must
 * EQUAL the segment's splits * m * n * 4: a plan whose split count changed
 * since the segment was filled (another set_config / autotune on the same
 * geometry) fails with JR_ERR_INVALID instead of leaving stale slabs in the
 * reduce. */
typedef struct jr_wgrad_seg {
  const float* slabs;
  float* dw;
  int32_t m, n, splits, c_in, c_pad, g, block0, blocks;
} jr_wgrad_seg;
int jr_conv2d_wgrad_seg(const jr_conv_desc* d, int dtype, jr_wgrad_seg* seg);
int jr_conv2d_bwd_filter_slabs(const jr_conv_desc* d, int dtype, const void* x, const void* dy, float* slabs,
                               size_t slab_bytes, void* stream);
int jr_wgrad_reduce(const jr_wgrad_seg* segs, int32_t nseg, int32_t total_blocks, void* stream);

/* Time every candidate tile configuration of this op on the given buffers
 * (the output buffer is overwritten; host-synchronising) and cache the
 * fastest for later calls with the same geometry in this process.  Call
 * once per layer at plan time, outside graph capture. */
int jr_conv2d_autotune(const jr_conv_desc* d, int op, int dtype, const void* a, const void* b, void* c,
                       void* ws, size_t ws_bytes, void* stream);
/* Tile configuration the next call would use (DGRAD: per stride phase),
 * and an explicit override (reproducibility, tests).  A config id is
 * tile | (splits << 8), splits = 0: planner's split-K factor (at most
 * 1024); set_config
 * with cfg = -1 drops the override (autotuned or set) for that GEMM. */
int jr_conv2d_get_config(const jr_conv_desc* d, int op, int dtype, int phase);
int jr_conv2d_set_config(const jr_conv_desc* d, int op, int dtype, int phase, int cfg);
int jr_conv2d_num_configs(int dtype);   /* tiles of that dtype's table */
/* Process-wide counter, bumped whenever set_config or autotune CHANGES an
 * override (re-setting an equal value does not): a caller that bound plans
 * (e.g. deferred filter-gradient segments) re-applies its own configs when
 * the generation moved since it did. */
unsigned long long jr_conv2d_config_generation(void);

/* ---- BatchNormalization(scale=False, eps) + ReLU, training-mode batch
 *      statistics (Keras conv2d_bn; App. C Q1: always batch stats) ----- */
size_t jr_bn_workspace_size(int64_t m, int32_t c);
/* What the BN launches over m rows of c channels use (host only, no device
 * call): 16-byte vectors of vec_width channels; the reductions sum nchunks
 * chunks of rows_per_chunk rows each (reduce_grid = nchunks; this grouping
 * fixes the fp64 summation order); single_stage = nchunks <= 512: the
 * backward's 8-lane finalize runs, and the layer may join a
 * jr_bn_relu_bwd_batch; finalize_grid of the backward, stats_finalize_grid of
 * jr_bn_stats, apply_grid of the elementwise passes; k1_offset: the byte
 * offset of the backward's k1 / k2 behind the partials in the workspace;
 * fold_rows x (fold_grid_x, fold_grid_y): rows per block and grid of
 * jr_bn_relu_apply_stats; workspace_size = jr_bn_workspace_size(m, c).
 * Returns the status every BN entry point gives these (dtype, m, c):
 * JR_ERR_INVALID for a bad dtype or channel count, JR_ERR_UNSUPPORTED for
 * more than 256 vectors per row. */
typedef struct jr_bn_launch_plan {
  int32_t vec_width, rows_per_chunk, nchunks, single_stage;
  int32_t reduce_grid, finalize_grid, stats_finalize_grid, apply_grid;
  int32_t fold_rows, fold_grid_x, fold_grid_y, reserved;
  int64_t k1_offset, workspace_size;
} jr_bn_launch_plan;
int jr_bn_plan(int dtype, int64_t m, int32_t c, jr_bn_launch_plan* out);
/* x: raw conv output [m][c] contiguous.  mean/invstd: [c] fp32 outputs.
 * invstd = 1/sqrt(biased_var + eps). */
int jr_bn_stats(int dtype, const void* x, int64_t m, int32_t c, float eps, float* mean, float* invstd,
                void* ws, size_t ws_bytes, void* stream);
/* y[.., y_c_off + k] = max((x[.., x_c_off + k] - mean) * invstd + beta, 0)
 * (x: a channel slice of the raw conv output, e.g. one member of a fused
 * sibling-conv group) */
int jr_bn_relu_apply(int dtype, const void* x, int32_t x_c_off, int32_t x_c_stride, int64_t m, int32_t c,
                     const float* mean, const float* invstd, const float* beta, void* y, int32_t y_c_off,
                     int32_t y_c_stride, void* stream);
/* BN + ReLU apply of a fused sibling launch's members in ONE launch: x
 * spans the launch's c channels; segment i (channels [sum_{j<i} c_j, ... +
 * c_i), sum c_i = c, each a multiple of 4 fp32 / 8 bf16) writes its own
 * output slice with its own beta.  Per element bitwise jr_bn_relu_apply.
 * 1 <= nseg <= 4. */
typedef struct jr_bn_apply_seg {
  void* y;
  int32_t y_c_off, y_c_stride, c;
  const float* beta;
} jr_bn_apply_seg;
int jr_bn_relu_apply_multi(int dtype, int nseg, const jr_bn_apply_seg* segs, const void* x, int32_t x_c_off,
                           int32_t x_c_stride, int64_t m, int32_t c, const float* mean, const float* invstd,
                           void* stream);
/* jr_bn_relu_apply with the statistics finalize folded in: mean / invstd of
 * the c channels come from the single-stage partials of the producing conv
 * (jr_conv2d_fwd_bn_partials): part = ws + ws_offset, layout [2][n_total][P]
 * of R rows each over m rows, this slice's channels starting at stat_c_off
 * of n_total; mean / invstd [c] are written too (for the backward). */
int jr_bn_relu_apply_stats(int dtype, const void* x, int32_t x_c_off, int32_t x_c_stride, int64_t m, int32_t c,
                           const float* part, int32_t P, int32_t R, int32_t n_total, int32_t stat_c_off, float eps,
                           float* mean, float* invstd, const float* beta, void* y, int32_t y_c_off,
                           int32_t y_c_stride, void* stream);
/* jr_bn_relu_apply for the members of an ensemble in one launch: member i
 * reads x + i*x_member_stride, mean / invstd + i*stats_member_stride, beta +
 * i*beta_member_stride and writes y + i*y_member_stride (elements). */
int jr_bn_relu_apply_grouped(int dtype, int32_t members, const void* x, int32_t x_c_off, int32_t x_c_stride,
                             int64_t x_member_stride, int64_t m, int32_t c, const float* mean, const float* invstd,
                             int64_t stats_member_stride, const float* beta, int64_t beta_member_stride, void* y,
                             int32_t y_c_off, int32_t y_c_stride, int64_t y_member_stride, void* stream);
/* The guarded forms: the entry point of the same name with `limit` before
 * `stream` (also jr_bn_relu_maxpool3x3s2_fwd_guard / _grouped_guard below).
 * They exist for forwards under FROZEN statistics that feed JR_F32_X6H convs:
 * there the activation bound of the batch-statistics forward (Samuelson's
 * inequality) does not hold, so the kernels that store the activations check
 * it instead.
 *  - Every stored output (and argmax) is bit for bit the unguarded entry
 *    point's: the same kernels, thread layout and per-element device function.
 *  - limit must be finite and > 0: anything else is JR_ERR_INVALID, checked
 *    first, before any HIP call; the rest of the validation is the unguarded
 *    call's.
 *  - Each block whose largest stored |y| is not <= limit counts one failure
 *    into the library's device error word (JR_ERR_HIP if there is none: call
 *    jr_init before capturing); jr_device_check then returns JR_ERR_DEVICE
 *    once and clears the word.  +inf trips the guard; a NaN need not (the
 *    maximum is taken with fmaxf, which drops it).  A negative pre-activation
 *    of any size stores 0 and never trips it.
 *  - Grouped forms: one error word for all members.  No host synchronisation,
 *    no atomics but the error count; capturable.
 * With a power-of-two bound m on the descriptor of the conv that reads y,
 * limit = 2 m keeps the JR_F32_X6H split exact (see jr_conv_desc); fp16
 * saturates only near 4 m.  The scales are then constants: a frozen forward
 * guarded this way is bitwise independent of the other images of the batch. */
int jr_bn_relu_apply_guard(int dtype, const void* x, int32_t x_c_off, int32_t x_c_stride, int64_t m, int32_t c,
                           const float* mean, const float* invstd, const float* beta, void* y, int32_t y_c_off,
                           int32_t y_c_stride, float limit, void* stream);
int jr_bn_relu_apply_multi_guard(int dtype, int nseg, const jr_bn_apply_seg* segs, const void* x, int32_t x_c_off,
                                 int32_t x_c_stride, int64_t m, int32_t c, const float* mean, const float* invstd,
                                 float limit, void* stream);
int jr_bn_relu_apply_grouped_guard(int dtype, int32_t members, const void* x, int32_t x_c_off, int32_t x_c_stride,
                                   int64_t x_member_stride, int64_t m, int32_t c, const float* mean,
                                   const float* invstd, int64_t stats_member_stride, const float* beta,
                                   int64_t beta_member_stride, void* y, int32_t y_c_off, int32_t y_c_stride,
                                   int64_t y_member_stride, float limit, void* stream);
/* Backward of apply+stats: dy is the gradient w.r.t. y (a channel slice),
 * dx receives the gradient w.r.t. the raw conv output in the same channel
 * slice geometry as x, dbeta [c] receives sum of the ReLU-masked dy. */
int jr_bn_relu_bwd(int dtype, const void* dy, int32_t dy_c_off, int32_t dy_c_stride, const void* x,
                   int32_t x_c_off, int32_t x_c_stride, int64_t m, int32_t c, const float* mean,
                   const float* invstd, const float* beta, void* dx, float* dbeta, void* ws, size_t ws_bytes,
                   void* stream);
/* The same backward for the members of a fused sibling launch in ONE set of
 * launches: x / dx / mean / invstd span the launch's c channels; segment i
 * (channels [sum_{j<i} c_j, ... + c_i), sum c_i = c, each c_i a multiple of
 * 4 fp32 / 8 bf16) brings its own upstream gradient slice and its own beta /
 * dbeta.  1 <= nseg <= 4.  jr_bn_relu_bwd is the one-segment case. */
typedef struct jr_bn_seg {
  const void* dy;
  int32_t dy_c_off, dy_c_stride, c;
  const float* beta;
  float* dbeta;
} jr_bn_seg;
int jr_bn_relu_bwd_multi(int dtype, int nseg, const jr_bn_seg* segs, const void* x, int32_t x_c_off,
                         int32_t x_c_stride, int64_t m, int32_t c, const float* mean, const float* invstd, void* dx,
                         void* ws, size_t ws_bytes, void* stream);
/* jr_bn_relu_bwd_multi that also raises dx_absmax (64 device floats the
 * caller zeroed before the first launch that feeds them) so that their max
 * is max |dx| of every launch that fed them: the dy_absmax of the
 * JR_F32_X6H data- / filter-gradient GEMMs reading dx. */
int jr_bn_relu_bwd_multi_absmax(int dtype, int nseg, const jr_bn_seg* segs, const void* x, int32_t x_c_off,
                                int32_t x_c_stride, int64_t m, int32_t c, const float* mean, const float* invstd,
                                void* dx, void* ws, size_t ws_bytes, float* dx_absmax, void* stream);
/* The backward under FROZEN statistics (a forward that normalised with fixed
 * mean / invstd: BN is then affine in x and nothing is differentiated through
 * the statistics).  Segments, slices and the dx geometry are those of
 * jr_bn_relu_bwd_multi; a segment's dbeta is ignored and may be NULL.  No
 * workspace, one launch.  Per element, with pre the pre-activation exactly as
 * jr_bn_relu_apply forms it from x, mean, invstd, beta (one shared device
 * function: the gate is the forward's bit for bit):
 *   g  = pre > 0 ? f32(dy) : 0      (a select: NaN / inf dy under a closed gate give 0)
 *   dx = T(g * invstd)              (one fp32 multiply; JR_BF16: rounded to nearest-even)
 * dtype: JR_F32 or JR_BF16, anything else JR_ERR_INVALID as jr_bn_relu_apply. */
int jr_bn_relu_bwd_frozen(int dtype, int nseg, const jr_bn_seg* segs, const void* x, int32_t x_c_off,
                          int32_t x_c_stride, int64_t m, int32_t c, const float* mean, const float* invstd, void* dx,
                          void* stream);
/* jr_bn_relu_bwd_frozen (dx bitwise unchanged) that also raises dx_absmax,
 * exactly as jr_bn_relu_bwd_multi_absmax does: 64 device floats, zeroed by the
 * caller (jr_absmax_reset) before the first launch that feeds them, whose
 * maximum is then max |dx| of every launch that fed them -- the dy_absmax of
 * the JR_F32_X6H data-gradient GEMM that reads dx.  That scale is measured
 * per batch (a gradient has no a-priori bound), so an x6h input gradient
 * under frozen statistics is independent of the other images of the batch
 * only to within the x6h error class, not bitwise as the guarded frozen
 * forward is.  dx_absmax NULL: jr_bn_relu_bwd_frozen. */
int jr_bn_relu_bwd_frozen_absmax(int dtype, int nseg, const jr_bn_seg* segs, const void* x, int32_t x_c_off,
                                 int32_t x_c_stride, int64_t m, int32_t c, const float* mean, const float* invstd,
                                 void* dx, float* dx_absmax, void* stream);
/* Up to 8 independent conv2d_bn backwards (the branch-final layers of one
 * Inception block, whose upstream gradients become final together) in ONE
 * set of three launches; layer l is exactly the jr_bn_relu_bwd_multi call
 * with its fields (bitwise the same results), each with at most 512 reduce
 * chunks (the 35^2 / 17^2 / 8^2 shapes at batch 64; larger ones:
 * JR_ERR_UNSUPPORTED).  ws: jr_bn_relu_bwd_batch_workspace_size bytes. */
typedef struct jr_bn_bwd_layer {
  int32_t nseg;
  jr_bn_seg segs[4];
  const void* x;
  int32_t x_c_off, x_c_stride;
  int64_t m;
  int32_t c;
  const float* mean;
  const float* invstd;
  void* dx;
} jr_bn_bwd_layer;
size_t jr_bn_relu_bwd_batch_workspace_size(int32_t n, const jr_bn_bwd_layer* layers);
int jr_bn_relu_bwd_batch(int dtype, int32_t n, const jr_bn_bwd_layer* layers, void* ws, size_t ws_bytes,
                         void* stream);
/* The backward of a conv2d_bn layer whose output only a 3x3/2 max-pool reads
 * (forward: jr_bn_relu_maxpool3x3s2_fwd): the max-pool backward writes dy
 * (d's x slice, from the pooled gradient at d's y slice and the argmax) and
 * adds the BN backward's reduction sums from the same registers, then the
 * finalize and the dx pass run as in jr_bn_relu_bwd -- one read of dy fewer.
 * x: the raw conv output [n*h*w] x x_c_stride (channels 0..d->c), dx: its
 * gradient in that geometry; d->c a multiple of 4, <= 1024.  ws: at least
 * jr_bn_relu_bwd_maxpool_workspace_size(d) bytes. */
size_t jr_bn_relu_bwd_maxpool_workspace_size(const jr_pool_desc* d);
int jr_bn_relu_bwd_maxpool(int dtype, const jr_pool_desc* d, const uint8_t* argmax, const void* pooled_dy, void* dy,
                           const void* x, int32_t x_c_stride, const float* mean, const float* invstd,
                           const float* beta, void* dx, float* dbeta, void* ws, size_t ws_bytes, void* stream);
/* ... raising dx_absmax as jr_bn_relu_bwd_multi_absmax does. */
int jr_bn_relu_bwd_maxpool_absmax(int dtype, const jr_pool_desc* d, const uint8_t* argmax, const void* pooled_dy,
                                  void* dy, const void* x, int32_t x_c_stride, const float* mean, const float* invstd,
                                  const float* beta, void* dx, float* dbeta, void* ws, size_t ws_bytes,
                                  float* dx_absmax, void* stream);

/* ---- pooling (Keras MaxPooling2D((3,3),(2,2)) / AveragePooling2D((3,3),
 *      (1,1),'same') inside InceptionV3, train.py:129-130) ------------ */
/* argmax [n][ho][wo][c] uint8 (window position 0..8, first max in scan
 * order) is written by fwd when non-NULL and routes the gradient in bwd. */
int jr_maxpool3x3s2_fwd(const jr_pool_desc* d, int dtype, const void* x, void* y, uint8_t* argmax,
                        void* stream);
int jr_maxpool3x3s2_bwd(const jr_pool_desc* d, int dtype, const uint8_t* argmax, const void* dy,
                        void* dx, int accumulate, void* stream);
/* The fused forward of a conv2d_bn layer whose only reader is a max-pool
 * (the stem's conv2d_3 / conv2d_5 outputs): raw is the conv output (the
 * descriptor's x slice), each tap is max(bn_pre(raw), 0) in the path dtype
 * (jr_bn_relu_apply's value), then the max-pool as jr_maxpool3x3s2_fwd --
 * y and argmax bitwise the two calls', without the full-resolution
 * activation.  mean / invstd / beta: [c] fp32. */
int jr_bn_relu_maxpool3x3s2_fwd(const jr_pool_desc* d, int dtype, const void* raw, const float* mean,
                                const float* invstd, const float* beta, void* y, uint8_t* argmax, void* stream);
/* The same over the members of an ensemble as one batch of d->n images:
 * image b belongs to member b / images_per_member, whose mean / invstd sit
 * stats_member_stride and beta beta_member_stride floats further. */
int jr_bn_relu_maxpool3x3s2_fwd_grouped(const jr_pool_desc* d, int dtype, int32_t images_per_member,
                                        const void* raw, const float* mean, const float* invstd,
                                        int64_t stats_member_stride, const float* beta, int64_t beta_member_stride,
                                        void* y, uint8_t* argmax, void* stream);
/* Their guarded forms (the contract: jr_bn_relu_apply_guard).  The guard is
 * over the POOLED values these calls store, which are what the next conv
 * reads: a raw value in a row or column that no 3x3/2 window covers, or one
 * that is not its window's maximum, never trips it. */
int jr_bn_relu_maxpool3x3s2_fwd_guard(const jr_pool_desc* d, int dtype, const void* raw, const float* mean,
                                      const float* invstd, const float* beta, void* y, uint8_t* argmax, float limit,
                                      void* stream);
int jr_bn_relu_maxpool3x3s2_fwd_grouped_guard(const jr_pool_desc* d, int dtype, int32_t images_per_member,
                                              const void* raw, const float* mean, const float* invstd,
                                              int64_t stats_member_stride, const float* beta,
                                              int64_t beta_member_stride, void* y, uint8_t* argmax, float limit,
                                              void* stream);
int jr_avgpool3x3s1_fwd(const jr_pool_desc* d, int dtype, const void* x, void* y, void* stream);
int jr_avgpool3x3s1_bwd(const jr_pool_desc* d, int dtype, const void* dy, void* dx, int accumulate,
                        void* stream);

/* ---- GlobalAveragePooling2D (pooling='avg', train.py:130) ------------ */
int jr_gap_fwd(int dtype, const void* x, int32_t n, int32_t hw, int32_t c, float* y, void* stream);
int jr_gap_bwd(int dtype, const float* dy, int32_t n, int32_t hw, int32_t c, void* dx, void* stream);

/* ---- head: tf.layers.dense(units) (train.py:133) + tf.sigmoid
 *      'predictions' (train.py:136) + reduce_mean(sigmoid xent)
 *      (train.py:140-141).  Softmax mode = softmax cross-entropy.
 *      labels may be NULL (inference: loss not computed). ----------- */
int jr_head_fwd(int mode, const float* feat, const float* w, const float* b, const float* labels,
                int32_t n, int32_t c, int32_t units, float* logits, float* probs, float* loss,
                void* stream);
int jr_head_bwd(int mode, const float* feat, const float* w, const float* probs, const float* labels,
                int32_t n, int32_t c, int32_t units, float* dfeat, float* dw, float* db, void* stream);
/* The gradient of ONE logit per sample with respect to its features (no loss,
 * no probabilities, no 1/n): dfeat[i][k] = w[k][t_i], t_i = target ? target[i]
 * : 0.  A t_i outside [0, units) writes a row of zeros; no address is formed
 * from it.  w: the dense kernel [c][units]. */
int jr_head_logit_bwd(const float* w, const int32_t* target, int32_t n, int32_t c, int32_t units, float* dfeat,
                      void* stream);

/* ---- the loss recipe: label smoothing, class weights, a focal term --------
 * (not in the reference: label smoothing is the published Inception-v3
 * recipe's, the positive-class weight and the focal term are what a strongly
 * imbalanced screening label asks for.)  jr_head_fwd / jr_head_bwd with a
 * jr_loss_spec; the kernels are the same, the plain calls are their neutral
 * case.  spec is a HOST pointer, copied by value into the launch (nothing for
 * the host to keep alive); NULL: the neutral spec.
 *
 * Notation: z logit, y the raw label, p = sigmoid(z) (softmax: p_u),
 *   e = label_smoothing in [0, 1), g = focal_gamma >= 0,
 *   c_u = class_weight[u] > 0 (u < units; the rest is ignored),
 *   sp(z) = max(z, 0) + log1p(exp(-|z|))   (softplus: -log(1 - p) = sp(z),
 *                                           -log p = sp(-z)),
 *   1 - p = sigmoid(-z).  Every term is formed from z in these stable forms,
 *   never from log(1 - p) of a stored p (p is exactly 1 in fp32 from z ~ 17).
 *
 * JR_HEAD_SIGMOID, per element (sample i, unit u):
 *   t     = y (1 - e) + e / 2                   (tf.losses.sigmoid_cross_entropy)
 *   L     = c_u t (1 - p)^g sp(-z) + (1 - t) p^g sp(z)
 *   dL/dz = -c_u t (1 - p)^g [g p sp(-z) + (1 - p)] + (1 - t) p^g [g (1 - p) sp(z) + p]
 *   loss  = sum L / (n units): the plain mean, NOT normalised by the weights;
 *   the gradient carries the same 1 / (n units).  g = 0: TF
 *   weighted_cross_entropy_with_logits(pos_weight = c_u) on the smoothed
 *   target; g = 0 and c = 1: jr_head_fwd's loss with t for y.  (x^0 = 1.)
 * JR_HEAD_SOFTMAX, per sample:
 *   t_u  = y_u (1 - e) + e / units              (tf.losses.softmax_cross_entropy)
 *   s    = sum_u c_u y_u                        (the sample weight, raw labels)
 *   L    = s sum_u t_u (lse(z) - z_u),  loss = sum L / n
 *   dz_u = s (p_u sum_v t_v - t_u) / n
 *   focal_gamma != 0: JR_ERR_INVALID.
 * A neutral spec (e = 0, g = 0, every used c_u = 1) and NULL give bitwise
 * what jr_head_fwd / jr_head_bwd give: (p - y) / denom in that order.
 * JR_ERR_INVALID, before any HIP call: e outside [0, 1), g < 0 or not
 * finite, a used c_u not finite or <= 0, and everything the plain calls
 * refuse.  jr_head_bwd_ex takes the logits jr_head_fwd(_ex) left, as well as
 * the probabilities. */
typedef struct jr_loss_spec { float label_smoothing, focal_gamma; float class_weight[16]; } jr_loss_spec;
int jr_head_fwd_ex(int mode, const jr_loss_spec* spec, const float* feat, const float* w, const float* b,
                   const float* labels, int32_t n, int32_t c, int32_t units, float* logits, float* probs,
                   float* loss, void* stream);
int jr_head_bwd_ex(int mode, const jr_loss_spec* spec, const float* logits, const float* feat, const float* w,
                   const float* probs, const float* labels, int32_t n, int32_t c, int32_t units, float* dfeat,
                   float* dw, float* db, void* stream);

/* ---- dropout with its state in DEVICE memory (the published Inception-v3
 *      recipe: rate 0.2 between the global average pool and the dense layer;
 *      not in the reference) -------------------------------------------------
 * Nothing stores a mask: it is a pure function of *state and the element
 * index, so the backward recomputes it, and a captured step draws the next
 * mask on every replay with no host work.  Per training step, on one stream:
 *   jr_dropout_fwd  ...  jr_dropout_bwd  ...  jr_dropout_advance
 * The mask of element i:
 *   (r0, r1, r2, r3) = philox4x32_10(counter = (lo32(i >> 2), hi32(i >> 2), step, 0), key)
 *   keep(i) = r[i & 3] >= threshold
 * Philox4x32-10 (Salmon et al., SC'11; the Random123 known answers hold): ten
 * rounds of
 *   (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))
 * with M0 = 0xD2511F53, M1 = 0xCD9E8D57 (32 x 32 -> 64-bit products), the key
 * bumped by (0x9E3779B9, 0xBB67AE85) mod 2^32 between rounds.
 *   forward:   y  = keep ? x  * scale : 0.0f      (one multiply)
 *   backward:  dx = keep ? dx * scale : 0.0f      (in place)
 * rate 0 (threshold 0, scale 1) gives y == x bitwise.  One thread handles one
 * quad (one Philox block, one 16-byte load and store), the last n % 4
 * elements singly.  x, y, dx 16-byte aligned and state 4-byte aligned (else
 * JR_ERR_INVALID, no launch); n <= 0 or a null pointer: JR_ERR_INVALID.
 * The engine advances the counter once per ENQUEUED training step: a step the
 * non-finite guard (jr_opt_prepare) skips is counted too -- it drew its mask. */
typedef struct jr_dropout_state { uint32_t key[2], step, threshold; float scale; uint32_t pad[3]; } jr_dropout_state; /* DEVICE memory */
/* One thread stores the state (it travels by value in the launch):
 *   threshold = (uint32_t)floor((double)rate * 2^32)
 *   scale     = (float)(1.0 / (1.0 - threshold / 2^32))     (both on the host)
 * rate in [0, 1), else JR_ERR_INVALID. */
int jr_dropout_set(jr_dropout_state* state, uint32_t key0, uint32_t key1, float rate, uint32_t step, void* stream);
int jr_dropout_fwd(const float* x, float* y, int64_t n, const jr_dropout_state* state, void* stream);
int jr_dropout_bwd(float* dx, int64_t n, const jr_dropout_state* state, void* stream);
/* One thread: step += 1 (mod 2^32). */
int jr_dropout_advance(jr_dropout_state* state, void* stream);

/* ---- optimizers (train.py:147-153: GradientDescentOptimizer /
 *      MomentumOptimizer(use_nesterov=True) -> TF ApplyMomentum) ------- */
/* accum = accum*momentum + g; w -= g*lr + accum*momentum*lr   (g = grad*grad_scale) */
int jr_nesterov_update(float* w, const float* grad, float* accum, int64_t n, float lr,
                       float momentum, float grad_scale, void* stream);
/* plain momentum (use_nesterov=False): accum = accum*m + g; w -= lr*accum */
int jr_momentum_update(float* w, const float* grad, float* accum, int64_t n, float lr,
                       float momentum, float grad_scale, void* stream);
int jr_sgd_update(float* w, const float* grad, int64_t n, float lr, float grad_scale, void* stream);
/* Adam (north-star extra, not in the reference): TF AdamOptimizer form */
int jr_adam_update(float* w, const float* grad, float* m, float* v, int64_t n, float lr_t,
                   float beta1, float beta2, float eps, float grad_scale, void* stream);

/* ---- the optimizer recipe with its step scalars in DEVICE memory --------
 * Weight decay, clipping of the global gradient norm, a guard against a
 * non-finite gradient and a learning rate that may change between replays of
 * a captured step (not in the reference: the engine uses these calls only
 * when asked to).  Per step, on one stream:
 *   jr_opt_set_hyper   (when a scalar changes; outside any captured graph)
 *   jr_grad_sqnorm  ->  jr_opt_prepare  ->  jr_<optimizer>_update_ex
 * Every fp32 operation is one correctly rounded op in the order written
 * here (no FMA contraction). */
typedef struct jr_opt_hyper { float lr, weight_decay, clip_norm, grad_scale; } jr_opt_hyper; /* written by jr_opt_set_hyper */
typedef struct jr_opt_step { float scale, grad_norm; uint32_t skipped, skipped_total; } jr_opt_step; /* written by jr_opt_prepare */
typedef struct jr_opt_range { int64_t begin, end; } jr_opt_range; /* decayed elements [begin, end) */
/* One thread stores the four scalars into *hyper (device memory, 4-byte
 * aligned).  They travel by value in the launch: no staging buffer the host
 * could reuse while a copy is in flight.  clip_norm <= 0: no clipping.  For
 * jr_adam_update_ex, lr carries the step's alpha (lr_t of jr_adam_update). */
int jr_opt_set_hyper(jr_opt_hyper* hyper, float lr, float weight_decay, float clip_norm, float grad_scale,
                     void* stream);
/* S = sum_i (double)grad[i]^2 over the raw gradient, left as per-block partials
 * (doubles; jr_grad_sqnorm_workspace_size(n) bytes, 8-byte aligned; grad
 * 16-byte aligned).  A fixed grid of min(1024, ceil(floor(n/4)/256)) >= 1
 * blocks of 256 threads; a thread adds its 16-byte quads in grid-stride order,
 * a block sums in a fixed tree; no atomics, no hand-off between blocks: the
 * same gradient gives bitwise the same partials in every run and on every
 * data-parallel replica. */
size_t jr_grad_sqnorm_workspace_size(int64_t n);
int jr_grad_sqnorm(const float* grad, int64_t n, void* partials, size_t ws_bytes, void* stream);
/* One block sums the partials of jr_grad_sqnorm(grad, n, ...) in a fixed
 * tree (fp64) into S and writes *step:
 *   n32       = (float)sqrt(S)
 *   grad_norm = n32 * grad_scale
 *   factor    = (clip_norm > 0 && grad_norm > clip_norm) ? clip_norm / grad_norm : 1
 *   scale     = grad_scale * factor
 * grad_norm not finite (inf or NaN, a norm that overflows fp32 included):
 * scale = 0, skipped = 1, skipped_total += 1; else skipped = 0 (skipped_total
 * is never reset by the library: zero *step once).  S == 0 gives factor 1. */
int jr_opt_prepare(const void* partials, int64_t n, const jr_opt_hyper* hyper, jr_opt_step* step, void* stream);
/* jr_nesterov_update / _momentum_ / _sgd_ / _adam_ with lr = hyper->lr and,
 * per element,  g = grad * step->scale;  inside a decay range and with
 * hyper->weight_decay != 0:  g = g + weight_decay * w  (a multiply, then an
 * add), then the by-value call's expression.  This is L2 decay in the loss
 * form: the decay term goes through the momentum / Adam moments (it is NOT
 * decoupled decay), and the clip factor in step->scale covers the data
 * gradient only, not the decay term.  step->skipped != 0: nothing at all is
 * written, neither weights nor optimizer state.  The skip is a device
 * decision the host does not wait for: a caller that counts steps on the
 * host (Adam's t in its alpha, moving averages) counts a skipped step too.
 * ranges: a DEVICE array of nranges element ranges, sorted, disjoint, at any
 * element offsets (NULL with nranges == 0: nothing decays).  w, grad and the
 * state buffers 16-byte aligned. */
int jr_nesterov_update_ex(float* w, const float* grad, float* accum, int64_t n, float momentum,
                          const jr_opt_range* ranges, int32_t nranges, const jr_opt_hyper* hyper,
                          const jr_opt_step* step, void* stream);
int jr_momentum_update_ex(float* w, const float* grad, float* accum, int64_t n, float momentum,
                          const jr_opt_range* ranges, int32_t nranges, const jr_opt_hyper* hyper,
                          const jr_opt_step* step, void* stream);
int jr_sgd_update_ex(float* w, const float* grad, int64_t n, const jr_opt_range* ranges, int32_t nranges,
                     const jr_opt_hyper* hyper, const jr_opt_step* step, void* stream);
int jr_adam_update_ex(float* w, const float* grad, float* m, float* v, int64_t n, float beta1, float beta2, float eps,
                      const jr_opt_range* ranges, int32_t nranges, const jr_opt_hyper* hyper, const jr_opt_step* step,
                      void* stream);

/* ---- RMSProp (TF ApplyRMSProp, the CPU functor [TF-3P, from reading,
 *      version unpinned]; not in the reference: the optimizer the published
 *      Inception-v3 recipe was tuned for, decay 0.9, momentum 0.9, epsilon 1) --
 * Per element, every fp32 operation one correctly rounded op in this order:
 *   g   = grad * grad_scale            (_ex: grad * step->scale, then
 *                                       g = g + weight_decay * w inside a range)
 *   ms  = ms + (g*g - ms) * (1 - rho)
 *   mom = mom*momentum + (g*lr) / sqrt(ms + eps)   (sqrt and / correctly rounded)
 *   w   = w - mom
 * TF starts ms at ones and mom at zeros; the library initialises neither.
 * jr_rmsprop_update takes any 4-byte alignment (16-byte moves when all four
 * buffers are 16-byte aligned); jr_rmsprop_update_ex follows every rule of
 * the _ex calls above (lr = hyper->lr, the skip, the ranges, the alignment). */
int jr_rmsprop_update(float* w, const float* grad, float* mom, float* ms, int64_t n, float lr, float rho,
                      float momentum, float eps, float grad_scale, void* stream);
int jr_rmsprop_update_ex(float* w, const float* grad, float* mom, float* ms, int64_t n, float rho, float momentum,
                         float eps, const jr_opt_range* ranges, int32_t nranges, const jr_opt_hyper* hyper,
                         const jr_opt_step* step, void* stream);

/* ---- the moving average of the weights (TF ExponentialMovingAverage
 *      [TF-3P, from reading, version unpinned]; not in the reference) -------
 * The counter and the step's decay live in DEVICE memory, so a captured step
 * replays correctly and a step the non-finite guard skipped is not counted.
 * Per step, on one stream, after the optimizer's update:
 *   jr_ema_prepare  ->  jr_ema_update
 * step: the jr_opt_step of this step's jr_opt_prepare, or NULL (never skipped). */
typedef struct jr_ema_state { float decay, one_minus_decay; uint32_t updates, warm; } jr_ema_state;
/* One thread stores decay, one_minus_decay = 1 - decay, updates and warm
 * (0 or 1) into *state (device memory, 4-byte aligned).  decay in [0, 1). */
int jr_ema_set(jr_ema_state* state, float decay, uint32_t warm, uint32_t updates, void* stream);
/* One thread.  step && step->skipped: one_minus_decay = 0, updates unchanged.
 * Otherwise, each operation rounded once:
 *   t = (float)updates
 *   d = warm ? min(decay, (1 + t) / (10 + t)) : decay
 *   one_minus_decay = 1 - d;  updates += 1 */
int jr_ema_prepare(jr_ema_state* state, const jr_opt_step* step, void* stream);
/* shadow = shadow - (shadow - w) * state->one_minus_decay, a subtract, a
 * multiply, a subtract, per element; step && step->skipped: nothing is
 * written.  shadow and w 16-byte aligned (else JR_ERR_INVALID, no launch). */
int jr_ema_update(float* shadow, const float* w, int64_t n, const jr_ema_state* state, const jr_opt_step* step,
                  void* stream);

/* ---- gradient accumulation (K micro-batches per optimizer update; not in
 *      the reference) ---------------------------------------------------------
 *   dst[i] = first ? src[i] : dst[i] + src[i],   i in [0, n)
 * one correctly rounded fp32 add per element, no atomics: the result does not
 * depend on the grid.  One call serves both directions of a group of
 * micro-batches: acc <- (first ? g : acc + g) on a micro-step that does not
 * close the group, g <- g + acc (first = 0) on the one that does; fp32 addition
 * commutes, so the closed gradient is bitwise ((g0 + g1) + g2) + ... in
 * micro-batch order.  first != 0 is a copy: dst is never read, so whatever an
 * abandoned group left there (a NaN included) is gone.
 * Any 4-byte alignment (16-byte moves when both pointers are 16-byte aligned,
 * single elements otherwise: the data-parallel path folds bucket sub-ranges of
 * the flat buffers).  JR_ERR_INVALID, before any HIP call: a null or
 * misaligned pointer, n <= 0, or [dst, dst + n) overlapping [src, src + n). */
int jr_grad_accumulate(float* dst, const float* src, int64_t n, int first, void* stream);

/* ---- bf16 filter copies (the bf16 conv path's weight operands) -------
 * From the fp32 master kernel [kh][kw][c_in][c_out] write
 *   w_hwio: bf16 [kh][kw][c_in][c_out]        (jr_conv2d_bwd_data, JR_BF16)
 *   w_t:    bf16 [c_out][kh][kw][c8], c8 = round_up(c_in, 8), zero padded
 *           (jr_conv2d_fwd, JR_BF16)
 * Either output may be NULL.  The _multi form does every layer of a model
 * in one launch from a DEVICE array of jr_wprep (offsets in elements from
 * the three bases; tile_start = exclusive prefix sum of
 * jr_conv_weights_bf16_tiles over the layers). */
typedef struct jr_wprep {
  int64_t src_off, hwio_off, wt_off;
  int32_t kh, kw, c_in, c_out;
  int32_t tile_start, reserved;
} jr_wprep;
int32_t jr_conv_weights_bf16_tiles(int32_t kh, int32_t kw, int32_t c_in, int32_t c_out);
int jr_conv_weights_bf16(const float* w, int32_t kh, int32_t kw, int32_t c_in, int32_t c_out, void* w_hwio,
                         void* w_t, void* stream);
int jr_conv_weights_bf16_multi(const jr_wprep* layers, int32_t n_layers, int32_t total_tiles, const float* src,
                               void* hwio, void* wt, void* stream);
/* JR_F32_X8P filter operands: the same two layouts as three bf16 planes
 * each (h, m, l of the exact split), plane stride = the layer's element
 * count (kh*kw*c_in*c_out for HWIO, c_out*kh*kw*c8 for W^T); in the _multi
 * form hwio_off / wt_off address each layer's first plane. */
int jr_conv_weights_x8p(const float* w, int32_t kh, int32_t kw, int32_t c_in, int32_t c_out, void* w_hwio,
                        void* w_t, void* stream);
int jr_conv_weights_x8p_multi(const jr_wprep* layers, int32_t n_layers, int32_t total_tiles, const float* src,
                              void* hwio, void* wt, void* stream);
/* Exact three-way bf16 split of an fp32 activation / gradient slice for
 * JR_F32_X8P: h = bf16_rn(x), m = bf16_rn(x - h), l = x - h - m (exact in
 * bf16).  src [rows][src_stride] channels [src_off, src_off + c) ->
 * dst + p * plane_stride (p = 0, 1, 2 for h, m, l), each [rows][dst_stride],
 * channels [dst_off, dst_off + c_pad); channels c..c_pad-1 are written as
 * zeros (the conv1 image: c = 3, c_pad = 8). */
int jr_split_x8p(const float* src, int64_t rows, int32_t c, int32_t src_off, int32_t src_stride, void* dst,
                 int32_t c_pad, int32_t dst_off, int32_t dst_stride, int64_t plane_stride, void* stream);

/* JR_F32_X6H operand magnitudes of parameter blocks (once per step, before
 * the forward): out[0 .. zero_floats) is zeroed (in stream order), then for
 * each segment the 64 floats out[seg.out * 64 ...] are raised so that their
 * max is max |src[off .. off + count)| (a conv launch's filter block: its
 * w_absmax).  limit > 0: a max above it counts a failure into the
 * device error word, which jr_device_check reports (JR_ERR_DEVICE) -- the
 * guard of a host bound that rests on these values (the BN betas bound the
 * activations: |relu(xhat + beta)| <= sqrt(N - 1) + max |beta|). */
typedef struct jr_absmax_seg {
  int64_t off, count;
  int32_t out;
  float limit;
} jr_absmax_seg;
int jr_absmax_prep(const float* src, const jr_absmax_seg* segs, int32_t nseg, float* out, int64_t zero_floats,
                   void* stream);
/* jr_absmax_prep's zeroing alone: rows[0 .. n_floats) = 0 in stream order (one
 * memset node: capturable), for absmax words that a launch list raises anew
 * on every run (jr_bn_relu_bwd_frozen_absmax).  JR_ERR_INVALID for a NULL
 * pointer or a negative count; n_floats == 0 does nothing. */
int jr_absmax_reset(float* rows, int64_t n_floats, void* stream);

/* ---- moving averages of the BN statistics, frozen inference ----------
 * The engines keep every conv launch's batch statistics in one flat fp32
 * "stats" buffer, [mean(c) | invstd(c)] per launch.  These two entry points
 * maintain Keras-style moving averages of them, layout [moving_mean(c) |
 * moving_var(c)] per launch, and turn the averages back into the stats layout
 * ("frozen") for a forward that does not depend on the batch.  Each is ONE
 * launch over a device table of segments, grid (ceil(max_c / 256), nseg,
 * members), member i at + i * its member stride (floats); no atomics, no host
 * sync, capturable.  max_c >= every segment's c.
 *
 * jr_bn_moving_update, per channel of a segment (mean_b, invstd from stats):
 *   1. v = 1.0 / ((double)invstd * (double)invstd) - (double)eps
 *   2. v = max(v, 0)
 *   3. v *= (double)rows / (double)(rows - 1)     (TF FusedBatchNorm feeds the
 *      running update the unbiased variance of the rows = n*ho*wo samples)
 *   4. var_b = (float)v
 *   5. fp32, every operation rounded on its own, d = 1.0f - momentum
 *      (TF assign_moving_average):
 *        mm = mm - (mm - mean_b) * d
 *        mv = mv - (mv - var_b) * d
 * A segment with rows < 2 has no unbiased variance: it is left untouched
 * (callers refuse to build such a table).
 *
 * jr_bn_moving_freeze, per channel:
 *   frozen_mean = mm
 *   frozen_invstd = (float)(1.0 / sqrt((double)mv + (double)eps))
 *
 * JR_ERR_INVALID (before any HIP call): a null pointer, nseg or members
 * outside 1..65535, max_c < 1, momentum outside [0, 1], eps <= 0, a negative
 * member stride. */
typedef struct jr_bn_moving_seg {
  int64_t stats_off;    /* the launch's [mean | invstd] in stats / frozen (floats) */
  int64_t moving_off;   /* the launch's [moving_mean | moving_var] in moving (floats) */
  int64_t rows;         /* n * ho * wo of the current batch */
  int32_t c;
  int32_t reserved;     /* must be 0 */
} jr_bn_moving_seg;
int jr_bn_moving_update(const jr_bn_moving_seg* segs, int32_t nseg, int32_t max_c, int32_t members,
                        const float* stats, int64_t stats_member_stride, float* moving,
                        int64_t moving_member_stride, float momentum, float eps, void* stream);
int jr_bn_moving_freeze(const jr_bn_moving_seg* segs, int32_t nseg, int32_t max_c, int32_t members,
                        const float* moving, int64_t moving_member_stride, float* frozen,
                        int64_t frozen_member_stride, float eps, void* stream);

/* ---- dtype helpers --------------------------------------------------- */
int jr_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
int jr_cast_bf16_to_f32(const void* src, float* dst, int64_t n, void* stream);
/* uint8 HWC images -> f32 * f32(1/255) (tf.image.convert_image_dtype,
 * lib/dataset.py:20-21) */
int jr_u8_to_f32_scaled(const uint8_t* src, void* dst, int dtype, int64_t n, void* stream);
/* uint8 [pixels][c] images -> dst [pixels][dst_stride] of f32(x) * f32(1/255),
 * channels [c, dst_stride) set to 0 (the conv1 input is kept 4 channels
 * wide, see jr_conv2d_fwd on c_in % 4 != 0). */
int jr_image_u8_to_nhwc(const uint8_t* src, void* dst, int dtype, int64_t pixels, int32_t c,
                        int32_t dst_stride, void* stream);
/* Training augmentation fused into the input conversion (not in the
 * reference, which trains unaugmented): uint8 [n][h][w][3] images -> dst
 * [n][h][w][dst_stride] of the path dtype (JR_F32 or JR_BF16), image i
 * transformed with params[i], in fp32, every operation rounded on its own:
 *  0. x = f32(u8) * f32(1/255)                      (jr_image_u8_to_nhwc)
 *  1. flags bit 0 mirrors left-right, bit 1 up-down (pure indexing)
 *  2. hue and saturation, skipped when hue_delta == 0 && sat_factor == 1:
 *     v = max(r,g,b), m = min(r,g,b), c = v - m, s = v > 0 ? c / v : 0,
 *     h6 = 0 if c == 0, else (g-b)/c if v == r, else (b-r)/c + 2 if v == g,
 *     else (r-g)/c + 4;  h6' = (h6 + 6 hue_delta) mod 6 in [0, 6),
 *     s' = clamp(s sat_factor, 0, 1);  k(n) = (h6' + n) mod 6,
 *     f(n) = v - v s' clamp(min(k, 4 - k), 0, 1), (r,g,b) = (f(5), f(3), f(1));
 *     IEEE divisions
 *  3. contrast, skipped when contrast_factor == 1:
 *     x = (x - mean_c) contrast_factor + mean_c, mean_c this image's mean of
 *     channel c over h*w after stage 2 (fp32 partials of 2048 pixels each,
 *     combined in fp64 in a fixed order, no atomics: bitwise reproducible
 *     and independent of n and of the image's slot in the batch)
 *  4. brightness, skipped when brightness_delta == 0: x += brightness_delta
 *  5. clamp to [0, 1]; channels [3, dst_stride) are written as 0.
 * The identity table (0, 1, 1, 0, flags 0) gives jr_image_u8_to_nhwc's
 * output bit for bit.  params: n entries in DEVICE memory.  Two launches on
 * the stream (the channel sums, then the transform); ws: at least
 * jr_augment_workspace_size(n, h, w) bytes, 4-byte aligned.  c must be 3,
 * dst_stride >= 3, n <= 65535. */
typedef struct jr_augment_param {   /* 32 bytes, one per image */
  float hue_delta, sat_factor, contrast_factor, brightness_delta;
  uint32_t flags;                   /* bit0 flip left-right, bit1 flip up-down */
  uint32_t reserved[3];             /* must be 0 */
} jr_augment_param;
size_t jr_augment_workspace_size(int32_t n, int32_t h, int32_t w);
int jr_image_u8_augment_nhwc(const uint8_t* src, void* dst, int dtype, int32_t n, int32_t h, int32_t w,
                             int32_t c, int32_t dst_stride, const jr_augment_param* params,
                             void* ws, size_t ws_bytes, void* stream);
/* The same transform with a per-image affine resampling (rotation, zoom,
 * shift) in stage 1; also the input kernel of test-time augmentation.  The
 * arguments, their validation and the workspace are jr_image_u8_augment_nhwc's,
 * plus warps: n entries in DEVICE memory.  Stages 0, 2, 3, 4 and the clamp are
 * unchanged; fp32, every operation rounded on its own.  Stage 1 of destination
 * pixel (x, y) of image i, m = warps[i].m:
 *  1a. x' = w-1-x if flags & 1, else x;  y' = h-1-y if flags & 2, else y
 *  1b. u = (m0 f32(x') + m1 f32(y')) + m2,  v = (m3 f32(x') + m4 f32(y')) + m5:
 *      the source position in pixel-index units
 *  1c. unless u > -1 && u < w && v > -1 && v < h (false for NaN and +-inf as
 *      well) the stage-1 value is (0, 0, 0); no address is formed from such a
 *      u or v
 *  1d. x0 = floor(u), fx = u - x0, y0 = floor(v), fy = v - y0; tap p(i, j) is
 *      the stage-0 value of source pixel (x0 + i, y0 + j) inside the image,
 *      else 0; per channel top = p00 + fx (p10 - p00), bot = p01 + fx (p11 -
 *      p01), out = top + fy (bot - top)
 * The contrast mean of stage 3 is taken over all h*w destination pixels after
 * stages 1 - 2 (fill pixels count): fp32 partials, their number a function of
 * (h, w) alone, combined in fp64 in a fixed order, no atomics -- an image's
 * result is bitwise reproducible and independent of n and of its slot.  The
 * partials take the pixels in the order of (x', y') (a flip permutes the terms
 * of the sum, not their values), 2048 to a partial as above: at the identity
 * matrix the mean is jr_image_u8_augment_nhwc's bit for bit.
 * With fx = fy = 0 the lerps return p00 bit for bit, so a matrix that maps the
 * pixel lattice onto itself is a pure permutation: the identity (1, 0, 0, 0,
 * 1, 0) gives jr_image_u8_augment_nhwc's output, (-1, 0, w-1, 0, 1, 0) the
 * left-right flip, the quarter turns of a square image its rotations. */
typedef struct jr_warp_param {   /* 32 bytes, one per image */
  float m[6];                    /* destination pixel (x, y) -> source position (u, v), pixel-index units */
  uint32_t reserved[2];          /* must be 0 */
} jr_warp_param;
int jr_image_u8_warp_augment_nhwc(const uint8_t* src, void* dst, int dtype, int32_t n, int32_t h, int32_t w,
                                  int32_t c, int32_t dst_stride, const jr_augment_param* params,
                                  const jr_warp_param* warps, void* ws, size_t ws_bytes, void* stream);
/* acc[0] += sum (p - y)^2, acc[1] += n   (tf.metrics.mean_squared_error,
 * train.py:175-177).  One block of 256 threads, in this order:
 *   d_i = (double)p[i] - (double)y[i]        (fp32 widened exactly; one fp64 subtract)
 *   q_i = d_i * d_i                          (one fp64 multiply, no FMA with the sum)
 *   s_t = ((0.0 + q_t) + q_{t+256}) + ...    (thread t: i = t, t + 256, ..., ascending; fp64 adds)
 *   r   = s;  for o = 128, 64, ..., 1:  r[t] = r[t] + r[t + o]  for every t < o
 *   acc[0] = acc[0] + r[0];  acc[1] = acc[1] + (double)n           (fp64)
 * Nothing runs in fp32.  n == 0 does nothing. */
int jr_brier_accumulate(const float* probs, const float* labels, int32_t n, double* acc, void* stream);

/* ---- streaming metrics and the step log in device memory ---------------
 * (jr/engine.py metrics_* and step_log_*; tests/metrics_ref.py restates the
 * three kernels in numpy).  All state is the caller's device memory; no call
 * synchronises the host, none uses an atomic, and a launch binds nothing but
 * pointers and element counts: every call may be captured into a graph.
 *
 * jr_metrics_accumulate: probs and labels are n fp32 values (batch * units,
 * flattened); thr holds T fp32 thresholds; counts is uint32 [4][T], rows tp,
 * fp, fn, tn; brier is double[2].  which bit 0: update counts; bit 1: update
 * brier.  Per sample and threshold, positive iff p > thr[t] as an fp32
 * comparison (a NaN p is negative), the label true iff y != 0 (0.5 and NaN
 * true, -0.0 false).  One thread owns one threshold (ceil(T / 256) blocks of
 * 256 threads), walks the samples through LDS in chunks of JR_METRICS_CHUNK
 * and adds its four counts by a plain read, add and store: the result does
 * not depend on the grid.  brier is jr_brier_accumulate(probs, labels, n,
 * brier), bit for bit (one shared device function, run by block 0).
 * JR_ERR_INVALID, before any HIP call: a null pointer that `which` needs
 * (probs and labels always; thr and counts for bit 0; brier, 8-byte aligned,
 * for bit 1), n <= 0, T outside 1..1024, which outside 1..3. */
#define JR_METRICS_CHUNK 1024
int jr_metrics_accumulate(const float* probs, const float* labels, int32_t n, const float* thr, int32_t T,
                          uint32_t* counts, double* brier, int32_t which, void* stream);
/* counts[0 .. 4 T) = 0 and brier[0 .. 2) = 0 in stream order (one memset node
 * each: capturable, as jr_absmax_reset).  Either pointer may be NULL;
 * JR_ERR_INVALID for counts with T outside 1..1024. */
int jr_metrics_reset(uint32_t* counts, int32_t T, double* brier, void* stream);
/* One record per training step, in a ring the host reads once in a while.
 * One thread:
 *   slot = *cursor % capacity
 *   ring[slot] = { *loss, step ? step->grad_norm : 0, step ? step->scale : 0, flags }
 *   *cursor += 1
 * flags bit 0: an update ran (step != NULL); bit 1: step->skipped != 0.
 * step: this step's jr_opt_step, or NULL -- the by-value optimizer path, and
 * a micro-batch that leaves its accumulation group open.
 * JR_ERR_INVALID: a null ring, cursor or loss, capacity == 0, a pointer that
 * is not 4-byte aligned. */
typedef struct jr_step_rec { float loss, grad_norm, scale; uint32_t flags; } jr_step_rec; /* DEVICE memory */
int jr_step_log_append(jr_step_rec* ring, uint32_t capacity, uint32_t* cursor, const float* loss,
                       const jr_opt_step* step, void* stream);

/* ---- attribution: per-image input gradients under frozen BN ------------
 * (jr/attribution.py; not in the reference).  Every multiply and add named
 * below is an fp32 operation rounded on its own (no fused multiply-add), so
 * a float32 restatement reproduces the results bit for bit. */
/* The data gradient of a convolution whose c_in <= 4 (the image layer, which
 * jr_conv2d_bwd_data refuses).  dy: the raw-output gradient in the
 * descriptor's y slice, fp32 (JR_F32) or bf16 (JR_BF16) -- the storage dtypes
 * only, anything else JR_ERR_INVALID; y_c_off and y_c_stride multiples of 4
 * fp32 / 8 bf16 channels.  w: the fp32 HWIO master filter, whatever dtype.
 * dx: fp32 [n][h][w][dx_c_stride], dx_c_stride >= c_in; channels [c_in,
 * dx_c_stride) are written as 0 and EVERY pixel is written (0 where no output
 * covers it).  The descriptor's x slice fields are not read.
 * Pixel (iy, ix), channel ci: the valid taps are the (r, s) with iy + pad_h -
 * r >= 0, divisible by stride_h, quotient oy < ho (and the same in x); per
 * tap p(r,s) = 0.0f, then for co = 0 .. c_out-1 ascending p = p + f32(dy[n,
 * oy,ox,co]) * w[r,s,ci,co]; dx = (((0.0f + p(first)) + p(next)) + ...) over
 * the valid taps in (r, s) ascending order.  No address is formed from an
 * invalid (oy, ox).
 * JR_ERR_UNSUPPORTED: c_in > 4, kh or kw > 7, a stride other than 1 or 2,
 * c_out % 16 != 0, or a filter that with the dy patch of 8x8 pixels exceeds
 * 48 KiB of LDS (c_out in the hundreds). */
int jr_conv2d_bwd_image(const jr_conv_desc* d, int dtype, const void* dy, const float* w, float* dx,
                        int32_t dx_c_stride, void* stream);
/* dst[i] = T(f32(src[i]) * alpha), i < n (T: JR_F32 or JR_BF16; in place allowed) */
int jr_attr_scale_input(int dtype, const void* src, void* dst, int64_t n, float alpha, void* stream);
/* acc[i] = (first ? 0.0f : acc[i]) + dx[i] * weight */
int jr_attr_accumulate(const float* dx, float* acc, int64_t n, float weight, int first, void* stream);
/* One value per pixel from its c = 3 (else JR_ERR_UNSUPPORTED) channels of acc
 * (fp32, acc_c_stride apart):
 *   JR_ATTR_ABSMAX:     map = max_c |acc_c|                      (x may be NULL)
 *   JR_ATTR_DOT_INPUT:  map = ((acc_0 x_0 + acc_1 x_1) + acc_2 x_2), x of dtype
 *                       JR_F32 / JR_BF16 widened to fp32, x_c_stride apart */
typedef enum jr_attr_mode { JR_ATTR_ABSMAX = 0, JR_ATTR_DOT_INPUT = 1 } jr_attr_mode;
int jr_attr_map(int mode, const float* acc, int32_t acc_c_stride, const void* x, int dtype, int32_t x_c_stride,
                int64_t pixels, int32_t c, float* map, void* stream);

/* ---- host (CPU) helpers: TFRecord container and Example records ----- */
uint32_t jr_crc32c(const uint8_t* data, size_t n, uint32_t crc);
/* TFRecord masked CRC32C: ((c >> 15) | (c << 17)) + 0xa282ead8 */
uint32_t jr_masked_crc32c(const uint8_t* data, size_t n);
/* Index the records of one TFRecord file image in memory (replaces the
 * record walk of tf.data.TFRecordDataset behind lib/dataset.py:5-8,44-47).
 * Writes the payload offset/length of each record; stops at the first damaged
 * record (truncated, or CRC mismatch when verify != 0) with *n_records = the
 * good records before it and JR_ERR_INVALID.  offsets == NULL only counts. */
int jr_tfrecord_index(const uint8_t* buf, size_t len, int verify, uint64_t* offsets, uint64_t* lengths,
                      size_t cap, size_t* n_records);
/* Locate the lib/dataset.py:12-16 FixedLenFeatures (image/encoded,
 * image/format, image/class/label, image/height, image/width) in n serialized
 * tf.train.Example records at base + offsets[i] (replaces the
 * tf.parse_single_example of lib/dataset.py:17).  status[i]: 0 ok; > 0 bitmask
 * of keys missing / not exactly one value / wrong list type (bit k = key k in
 * the order above); -1 malformed protobuf.  enc_off is relative to base. */
int jr_example_parse_image(const uint8_t* base, const uint64_t* offsets, const uint64_t* lengths, size_t n,
                           uint64_t* enc_off, uint64_t* enc_len, int64_t* label, int64_t* height,
                           int64_t* width, int32_t* status);

/* ---- collectives: data-parallel gradient exchange over RCCL / xGMI ----
 * Replaces the reference's only multi-GPU path, the external
 * tf_cnn_benchmarks parameter server (benchmarks.yaml.jinja.example:81-90;
 * SURVEY.md §2 row 14, §8b/§8e): one communicator per process (one process
 * per GPU), in-place sum of the flat gradient enqueued on the caller's
 * stream.  The 128-byte unique id comes from rank 0's jr_comm_unique_id and
 * reaches the other ranks through the caller's bootstrap, or through a file
 * (jr_comm_init_file: rank 0 writes it, tagged with run_id, with an atomic
 * rename; the others poll up to timeout_ms, < 0 = forever, for the file of
 * THEIR run_id, so an id an earlier job left at uid_path is never joined;
 * run_id: any non-empty string every rank of one job shares, e.g. the
 * launcher's rendezvous id). */
#define JR_COMM_ID_BYTES 128
typedef struct jr_comm jr_comm;
int jr_comm_unique_id(uint8_t* id);
int jr_comm_init(int rank, int world, const uint8_t* id, int device, jr_comm** comm);
int jr_comm_init_file(int rank, int world, const char* uid_path, const char* run_id, int device, int timeout_ms,
                      jr_comm** comm);
/* buf[0..n) = sum over the ranks of buf[0..n), dtype JR_F32 or JR_BF16 */
int jr_allreduce_sum(jr_comm* comm, void* buf, size_t n, int dtype, void* stream);
int jr_comm_rank(const jr_comm* comm);
int jr_comm_world(const jr_comm* comm);
int jr_comm_destroy(jr_comm* comm);

/* ---- HIP graph capture of a whole step ------------------------------ */
int jr_graph_begin(void* stream);
int jr_graph_end(void* stream, void** graph_exec);
int jr_graph_launch(void* graph_exec, void* stream);
int jr_graph_destroy(void* graph_exec);
/* Device regions the library allocated for a capture (stream-K hand-off
 * flags of captured conv GEMMs) and released by jr_graph_destroy (tests). */
int jr_graph_regions(void* graph_exec);

/* ---- Cross-stream ordering of the branch lanes ---------------------- */
/* Events for device-side ordering between the library's callers' streams
 * (jr.lanes: a consumer on one lane waits for its producer on another):
 * no timing and no system-scope fence -- device memory only, the only
 * thing the lanes order.  (A recorded DisableSystemFence event costs the
 * producer's queue ~1.1 us less than a default one: profiles/r05_sync_probe2.txt.) */
int jr_event_create(void** event);
int jr_event_record(void* event, void* stream);
int jr_stream_wait_event(void* stream, void* event);
int jr_event_destroy(void* event);

#ifdef __cplusplus
}
#endif
#endif /* JR_H_ */
