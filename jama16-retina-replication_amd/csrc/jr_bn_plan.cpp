// jr_bn_plan.cpp — host-only launch planning of the BN passes (jr_bn_plan.h).
#include "jr_bn_plan.h"

#include <algorithm>
#include <cstdlib>

namespace jr {

// rows per folded apply block (JR_BN_FOLD_ROWS, read once; A/B knob): each
// block re-combines its 32 channels' partials, so fewer rows per block means
// more parallel blocks and more redundant partial reads
static int fold_rows() {
  static const int v = [] {
    const char* e = std::getenv("JR_BN_FOLD_ROWS");
    const int r = e ? std::atoi(e) : 0;
    return r > 0 ? r : 256;
  }();
  return v;
}
// the backward's finalize folded into its apply: opt-in (JR_FOLD_BN_BWD=1,
// read once) -- measured +0.14 ms/step bf16 against k_bn_finalize8 + apply
// (profiles/r05_ab_rows_bf16.txt), same arithmetic either way
bool fold_bwd() {
  static const bool on = [] {
    const char* e = std::getenv("JR_FOLD_BN_BWD");
    return e && e[0] == '1';
  }();
  return on;
}

struct ChunkGeom {
  int rows_per_chunk;
  int nchunks;
};

static ChunkGeom chunk_geom(int64_t m, int c, int vw) {
  const int tpr = c / vw;
  const int rpp = std::max(1, 256 / tpr);
  // one unrolled batch of rows per thread at least; at most kMaxChunks chunks
  // (chunks of fewer rows -- more blocks for the 17x17 / 8x8 layers -- measured
  // slower: 1.47 -> 1.83 ms of reduce + 0.46 -> 0.65 ms of finalize per step)
  // (round 2: a smaller minimum for small m only -- 4 rows per thread below
  // 32,768 rows -- measured slower too: bf16 step 11.46 vs 11.35 ms)
  const int un = kMinRows;
  int64_t rpc = std::max<int64_t>(ceil_div(m, kMaxChunks), (int64_t)rpp * un);
  rpc = ceil_div(rpc, (int64_t)rpp * un) * rpp * un;
  ChunkGeom g;
  g.rows_per_chunk = (int)rpc;
  g.nchunks = (int)ceil_div(m, rpc);
  return g;
}

// Partials for either dtype's geometry (the query carries no dtype).
static size_t ws_need(int64_t m, int c) {
  size_t n = 0;
  for (int vw : {4, 8})
    if (c % vw == 0) n = std::max(n, (size_t)chunk_geom(m, c, vw).nchunks);
  return n * 2 * c * sizeof(double) + 2 * (size_t)c * sizeof(float);
}

// workspace of a batched backward: each layer's ws_need, 256-byte aligned
static size_t batch_ws(int n, const jr_bn_bwd_layer* layers) {
  size_t off = 0;
  for (int l = 0; l < n; ++l) off += (ws_need(layers[l].m, layers[l].c) + 255) / 256 * 256;
  return off;
}

static int apply_grid(int64_t m, int c, int vw) {
  const int rpp = 256 / (c / vw);
  return (int)ceil_div(m, (int64_t)rpp * kAppUnroll);
}

int check_common(int dtype, int64_t m, int c) {
  if (dtype != JR_F32 && dtype != JR_BF16) return fail(JR_ERR_INVALID, "bn: bad dtype");
  if (m <= 0 || c <= 0) return fail(JR_ERR_INVALID, "bn: empty tensor");
  if (c % vec_width(dtype) != 0)
    return fail(JR_ERR_INVALID, "bn: channel count must be a multiple of 4 (fp32) / 8 (bf16)");
  if (c / vec_width(dtype) > 256) return fail(JR_ERR_UNSUPPORTED, "bn: more than 256 vectors per row");
  return JR_OK;
}

bool check_slice(int dtype, int off, int stride, int c) {
  const int q = vec_width(dtype);
  return off >= 0 && off + c <= stride && off % q == 0 && stride % q == 0;
}

jr_bn_launch_plan bn_plan(int dtype, int64_t m, int c) {
  const int vw = vec_width(dtype);
  const ChunkGeom g = chunk_geom(m, c, vw);
  jr_bn_launch_plan p{};
  p.vec_width = vw;
  p.rows_per_chunk = g.rows_per_chunk;
  p.nchunks = p.reduce_grid = g.nchunks;
  p.single_stage = g.nchunks <= kFoldMaxP;
  // one wave per channel (k_bn_finalize), or 8 lanes per channel (k_bn_finalize8)
  p.stats_finalize_grid = (int)ceil_div(c, 4);
  p.finalize_grid = p.single_stage ? (int)ceil_div(c, kFoldCh) : p.stats_finalize_grid;
  p.apply_grid = apply_grid(m, c, vw);
  // rows per folded block: a multiple of one pass x unroll (the 32-channel
  // group's widest pass), about JR_BN_FOLD_ROWS (each block re-combines its
  // group's partials: fewer, longer blocks read them fewer times)
  const int step = 256 / (kFoldCh / vw) * kAppUnroll;
  p.fold_rows = (int)std::max<int64_t>(step, (int64_t)(fold_rows() + step - 1) / step * step);
  p.fold_grid_x = (int32_t)(unsigned)ceil_div(m, p.fold_rows);
  p.fold_grid_y = (int32_t)(unsigned)ceil_div(c, kFoldCh);
  p.k1_offset = (int64_t)((size_t)g.nchunks * 2 * c * sizeof(double));
  p.workspace_size = (int64_t)ws_need(m, c);
  return p;
}

// What the validation reads of one segment of either kind, and its messages.
struct SegView {
  bool ptrs;
  int off, stride, c;
};
struct SegMsgs {
  const char *null_ptr, *bad_c, *bad_slice, *bad_sum;
};

static int check_segs(int dtype, int nseg, const SegView* v, int c, const SegMsgs& msg, int* c0) {
  int sum = 0;
  for (int i = 0; i < nseg; ++i) {
    if (!v[i].ptrs) return fail(JR_ERR_INVALID, msg.null_ptr);
    if (v[i].c <= 0 || v[i].c % vec_width(dtype) != 0) return fail(JR_ERR_INVALID, msg.bad_c);
    if (!check_slice(dtype, v[i].off, v[i].stride, v[i].c)) return fail(JR_ERR_INVALID, msg.bad_slice);
    c0[i] = sum;
    sum += v[i].c;
  }
  if (sum != c) return fail(JR_ERR_INVALID, msg.bad_sum);
  c0[nseg] = c;
  return JR_OK;
}

int apply_segs(int dtype, int nseg, const jr_bn_apply_seg* segs, int c, ApplySegs& sg) {
  static const SegMsgs msg = {"bn_relu_apply_multi: null pointer in a segment", "bn_relu_apply_multi: bad output segment",
                              "bn_relu_apply_multi: bad output segment",
                              "bn_relu_apply_multi: segment channels must sum to c"};
  SegView v[kMaxSegs];
  for (int i = 0; i < nseg; ++i) v[i] = {segs[i].y && segs[i].beta, segs[i].y_c_off, segs[i].y_c_stride, segs[i].c};
  sg = ApplySegs{};
  sg.n = nseg;
  const int rc = check_segs(dtype, nseg, v, c, msg, sg.c0);
  if (rc) return rc;
  for (int i = 0; i < nseg; ++i) {
    sg.y[i] = segs[i].y;
    sg.beta[i] = segs[i].beta;
    sg.y_off[i] = segs[i].y_c_off;
    sg.y_stride[i] = segs[i].y_c_stride;
  }
  return JR_OK;
}

int bwd_segs(int dtype, int nseg, const jr_bn_seg* segs, int c, BnSegs& sg, bool need_dbeta) {
  static const SegMsgs msg = {
      "bn_relu_bwd: null pointer in a segment",
      "bn_relu_bwd: segment channels must be a positive multiple of 4 (fp32) / 8 (bf16)", "bn_relu_bwd: bad dy slice",
      "bn_relu_bwd: segment channels must sum to c"};
  SegView v[kMaxSegs];
  for (int i = 0; i < nseg; ++i)
    v[i] = {segs[i].dy && segs[i].beta && (segs[i].dbeta || !need_dbeta), segs[i].dy_c_off, segs[i].dy_c_stride,
            segs[i].c};
  sg = BnSegs{};
  sg.n = nseg;
  const int rc = check_segs(dtype, nseg, v, c, msg, sg.c0);
  if (rc) return rc;
  for (int i = 0; i < nseg; ++i) {
    sg.dy[i] = segs[i].dy;
    sg.dy_off[i] = segs[i].dy_c_off;
    sg.dy_stride[i] = segs[i].dy_c_stride;
    sg.beta[i] = segs[i].beta;
    sg.dbeta[i] = segs[i].dbeta;
  }
  return JR_OK;
}

int bwd_setup(int dtype, int nseg, const jr_bn_seg* segs, const void*& x, int32_t x_c_off, int32_t x_c_stride,
              int64_t m, int32_t c, const float* mean, const float* invstd, void*& dx, BnSegs& sg,
              bool need_dbeta) {
  int rc = check_common(dtype, m, c);
  if (rc) return rc;
  if (!segs || nseg < 1 || nseg > kMaxSegs) return fail(JR_ERR_INVALID, "bn_relu_bwd: 1..4 segments");
  if (!x || !mean || !invstd || !dx) return fail(JR_ERR_INVALID, "bn_relu_bwd: null pointer");
  if (!check_slice(dtype, x_c_off, x_c_stride, c)) return fail(JR_ERR_INVALID, "bn_relu_bwd: bad x / dx slice");
  rc = bwd_segs(dtype, nseg, segs, c, sg, need_dbeta);
  if (rc) return rc;
  x = static_cast<const char*>(x) + (size_t)x_c_off * elt_size(dtype);
  dx = static_cast<char*>(dx) + (size_t)x_c_off * elt_size(dtype);
  return JR_OK;
}

int bwd_batch_setup(int dtype, int32_t n, const jr_bn_bwd_layer* layers, void* ws, size_t ws_bytes, BnBatch& bt,
                    int blocks[3]) {
  if (n < 1 || n > kBnBatchMax || !layers) return fail(JR_ERR_INVALID, "bn_relu_bwd_batch: 1..8 layers");
  if (!ws || ws_bytes < batch_ws(n, layers)) return fail(JR_ERR_WORKSPACE, "bn_relu_bwd_batch: workspace too small");
  bt = BnBatch{};
  bt.n = n;
  blocks[0] = blocks[1] = blocks[2] = 0;
  size_t off = 0;
  for (int l = 0; l < n; ++l) {
    const jr_bn_bwd_layer& e = layers[l];
    BnBatchLayer& L = bt.L[l];
    const void* x = e.x;
    void* dx = e.dx;
    const int rc = bwd_setup(dtype, e.nseg, e.segs, x, e.x_c_off, e.x_c_stride, e.m, e.c, e.mean, e.invstd, dx, L.sg);
    if (rc) return rc;
    const jr_bn_launch_plan p = bn_plan(dtype, e.m, e.c);
    if (!p.single_stage)
      return fail(JR_ERR_UNSUPPORTED, "bn_relu_bwd_batch: a layer with more than 512 reduce chunks (use jr_bn_relu_bwd_multi)");
    L.x = x;
    L.dx = dx;
    L.mean = e.mean;
    L.invstd = e.invstd;
    L.part = reinterpret_cast<double*>(static_cast<char*>(ws) + off);
    L.k1 = reinterpret_cast<float*>(static_cast<char*>(ws) + off + p.k1_offset);
    L.k2 = L.k1 + e.c;
    L.m = e.m;
    L.c = e.c;
    L.xs = e.x_c_stride;
    L.rpc = p.rows_per_chunk;
    L.nchunks = p.nchunks;
    const int grids[3] = {p.reduce_grid, p.finalize_grid, p.apply_grid};
    for (int k = 0; k < 3; ++k) {
      L.b0[k] = blocks[k];
      blocks[k] += grids[k];
    }
    off += ((size_t)p.workspace_size + 255) / 256 * 256;
  }
  return JR_OK;
}

PoolBwdGeom pool_bwd_geom(const jr_pool_desc* d) {
  const int c4 = d->c / 4;
  const int64_t cells = (int64_t)d->n * ((d->h + 1) / 2) * ((d->w + 1) / 2) * c4;
  PoolBwdGeom g;
  g.block = 256 / c4 * c4;   // a whole number of channel-quad rows per block
  g.grid = (int)std::min<int64_t>(std::max<int64_t>(ceil_div(cells, g.block), 1), kPoolBwdMaxParts);
  return g;
}

size_t pool_bwd_ws(int c) {
  return (size_t)kPoolBwdMaxParts * 2 * c * sizeof(double) + 2 * (size_t)c * sizeof(float);
}

}  // namespace jr

using namespace jr;

JR_API int jr_bn_plan(int dtype, int64_t m, int32_t c, jr_bn_launch_plan* out) {
  if (!out) return fail(JR_ERR_INVALID, "bn_plan: null output");
  const int rc = check_common(dtype, m, c);
  if (rc) return rc;
  *out = bn_plan(dtype, m, c);
  return JR_OK;
}

JR_API size_t jr_bn_workspace_size(int64_t m, int32_t c) {
  if (m <= 0 || c <= 0 || c % 4) return 0;
  return ws_need(m, c);
}

JR_API size_t jr_bn_relu_bwd_batch_workspace_size(int32_t n, const jr_bn_bwd_layer* layers) {
  if (n < 1 || n > kBnBatchMax || !layers) return 0;
  return batch_ws(n, layers);
}

JR_API size_t jr_bn_relu_bwd_maxpool_workspace_size(const jr_pool_desc* d) {
  if (!d || d->c <= 0) return 0;
  return pool_bwd_ws(d->c);
}
