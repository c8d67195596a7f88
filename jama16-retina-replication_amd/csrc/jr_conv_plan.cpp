// jr_conv_plan.cpp — the host-only conv planner (jr_conv_plan.h).
#include "jr_conv_plan.h"

#include <algorithm>
#include <cstdlib>
#include <map>
#include <mutex>
#include <vector>

namespace jr {

// ------------------------------------------------------------- config ids
// The tile ids of one dtype, in id order.  Ids are APPEND-ONLY: the committed
// tile tables (jr/tiles_mi355x.json) and the tests name them, so a new kernel
// family or tile goes behind every existing range of its dtype.
struct CfgSpace {
  std::vector<CfgEntry> ids;
  int std;   // the leading standard tiles
};

static CfgSpace build_space(int dtype) {
  CfgSpace s;
  auto tiles = [&](Kernel k, const TileCfg* t, int n, bool sk) {
    for (int i = 0; i < n; ++i) s.ids.push_back(CfgEntry{k, i, sk, t + i, nullptr});
  };
  switch (dtype) {
    case JR_F32:
      tiles(Kernel::F32_MFMA, kCfgs, kNumCfgs, false);
      s.std = kNumCfgs;
      break;
    // JR_F32_X8 also selects the fp32-MFMA kernel of every fp32 tile: both
    // are fp32-accurate, and on the stem's N = 32 / 64 filter-gradient GEMMs,
    // whose per-wave split VALU outweighs the 8-product MFMA gain, the fp32
    // MFMA is the faster one -- autotuning and the pinned tables choose per
    // GEMM (the planner heuristic keeps x8).  JR_F32_X6H shares all of it.
    case JR_F32_X8:
    case JR_F32_X6H:
      tiles(Kernel::X8_SPLIT, kCfgs, kNumCfgs, false);   // 0-13
      tiles(Kernel::F32_MFMA, kCfgs, kNumCfgs, false);   // 14-27
      tiles(Kernel::X8_SPLIT, kCfgs, kNumCfgs, true);    // 28-41: stream-K grids (k_conv SK)
      s.std = kNumCfgs;
      break;
    case JR_BF16:
      tiles(Kernel::BF16, kCfgsBf16, kNumCfgsBf16, false);         // 0-16
      for (int i = 0; i < kNumHaloBf16; ++i)                       // 17-24
        s.ids.push_back(CfgEntry{Kernel::HALO, i, false, &kHaloBf16[i].t, &kHaloBf16[i]});
      tiles(Kernel::BF16_WIDE, kCfgsBf16W, kNumCfgsBf16W, false);  // 25-32
      tiles(Kernel::BF16, kCfgsBf16, kNumCfgsBf16, true);          // 33-49: stream-K grids (k_conv_bf16 SK)
      tiles(Kernel::BF16_WIDE, kCfgsBf16W, kNumCfgsBf16W, true);   // 50-57
      s.std = kNumCfgsBf16;
      break;
    default:   // JR_F32_X8P: the bf16 kernels on three operand planes
      tiles(Kernel::BF16, kCfgsX8P, kNumCfgsX8P, false);           // 0-16
      tiles(Kernel::BF16_WIDE, kCfgsX8PW, kNumCfgsX8PW, false);    // 17-23
      s.std = kNumCfgsX8P;
      break;
  }
  return s;
}

static bool known_dtype(int dtype) { return dtype >= JR_F32 && dtype <= JR_F32_X6H; }

static const CfgSpace& cfg_space(int dtype) {
  static const CfgSpace spaces[] = {build_space(JR_F32), build_space(JR_BF16), build_space(JR_F32_X8),
                                    build_space(JR_F32_X8P), build_space(JR_F32_X6H)};
  static_assert(JR_F32 == 0 && JR_BF16 == 1 && JR_F32_X8 == 2 && JR_F32_X8P == 3 && JR_F32_X6H == 4,
                "cfg_space indexes by dtype");
  return spaces[dtype];
}

const CfgEntry& cfg_entry(int dtype, int id) { return cfg_space(dtype).ids[id]; }
int cfg_count(int dtype) { return known_dtype(dtype) ? (int)cfg_space(dtype).ids.size() : 0; }
int std_count(int dtype) { return cfg_space(dtype).std; }

// ---------------------------------------------------------------- geometry
int chan_pad(int c, int dtype) {
  const int q = bf16_operands(dtype) ? 8 : 4;
  return (c + q - 1) / q * q;
}

OpPhases::OpPhases(const jr_conv_desc* d, int op) : ph{}, n(1) {
  if (op != OP_DGRAD) return;
  n = 0;
  for (int py = 0; py < d->stride_h; ++py) {
    for (int px = 0; px < d->stride_w; ++px) {
      Phase p{};
      p.py = py; p.px = px;
      p.hc = py < d->h ? (d->h - py + d->stride_h - 1) / d->stride_h : 0;
      p.wc = px < d->w ? (d->w - px + d->stride_w - 1) / d->stride_w : 0;
      p.r0 = (py + d->pad_h) % d->stride_h;
      p.c0 = (px + d->pad_w) % d->stride_w;
      p.na = p.r0 < d->kh ? (d->kh - p.r0 + d->stride_h - 1) / d->stride_h : 0;
      p.nb = p.c0 < d->kw ? (d->kw - p.c0 + d->stride_w - 1) / d->stride_w : 0;
      p.ey = (py + d->pad_h - p.r0) / d->stride_h;
      p.ex = (px + d->pad_w - p.c0) / d->stride_w;
      ph[n++] = p;
    }
  }
}

void gemm_dims(const jr_conv_desc* d, int op, int dtype, const Phase& ph, int* M, int* N, int* K) {
  const int cp = chan_pad(d->c_in, dtype);
  if (op == OP_FWD) { *M = d->n * d->ho * d->wo; *N = d->c_out; *K = d->kh * d->kw * cp; }
  else if (op == OP_WGRAD) { *M = d->kh * d->kw * cp; *N = d->c_out; *K = d->n * d->ho * d->wo; }
  else { *M = d->n * ph.hc * ph.wc; *N = d->c_in; *K = ph.na * ph.nb * d->c_out; }
}

// Halo rows a BM-row tile needs: output rows it spans (bound) + kh - 1.
static int halo_rows(const jr_conv_desc* d, int bm) { return (bm + d->wo - 2) / d->wo + 1 + d->kh - 1; }
bool halo_ok(const jr_conv_desc* d, int op, int dtype, int tile) {
  const HaloCfg* h = cfg_entry(dtype, tile).halo;
  if (!h || op != OP_FWD) return false;
  return d->kh == h->kh && d->kw == h->kw && d->stride_h == 1 && d->stride_w == 1 && d->ho == d->h &&
         d->wo == d->w && d->c_in % 32 == 0 && halo_rows(d, h->t.bm) * (d->w + d->kw - 1) < h->slots;
}

// ------------------------------------------------------------------- plans
constexpr int kSkBlocks = 512;     // stream-K grid: 2 x 256 CUs
constexpr int kSkMinIters = 4;     // K-tiles per stream-K block at least

// Blocks the planner's split-K factor aims for (>= 2.5 per CU). x8 filter
// gradients aim for 384: their slabs are summed per layer on the GEMM's lane
// (the fp32 engine default), and fewer slabs measured 0.12-0.14 ms per step
// faster on two boxes (profiles/r05_ab_wsplit*_f32.txt; 320 / 1,024 slower,
// bf16 at 384 slower). JR_WGRAD_SPLIT_TARGET overrides it (A/B knob, read once).
// JR_WGRAD_SPLIT_KMAX (A/B knob, read once): x8 filter gradients aim for 384
// only where K = B.Ho.Wo is at most this, 640 above it (round 5's
// K-bounded rule: faster at 299^2 and 587^2, moved the B=16 fp32 curve
// past the round-5 bar; re-judged against the calibrated bars).
static int split_target(int dtype, int op, long long K) {
  static const int wg = [] {
    const char* e = std::getenv("JR_WGRAD_SPLIT_TARGET");
    const int v = e ? std::atoi(e) : 0;
    return v > 0 ? v : 0;
  }();
  static const long long kmax = [] {
    const char* e = std::getenv("JR_WGRAD_SPLIT_KMAX");
    const long long v = e ? std::atoll(e) : 0;
    return v > 0 ? v : 0LL;
  }();
  if (op != OP_WGRAD) return 640;
  if (wg > 0) return wg;
  if (dtype == JR_F32_X8 || dtype == JR_F32_X6H || dtype == JR_F32_X8P) return kmax > 0 && K > kmax ? 640 : 384;
  return 640;
}

Plan plan_with(int dtype, int cfg, int M, int N, int K, int op) {
  Plan p{};
  p.M = M; p.N = N; p.K = K; p.cfg = cfg; p.tile = cfg_tile(cfg);
  const CfgEntry& e = cfg_entry(dtype, p.tile);
  const TileCfg& t = *e.t;
  p.mt = (int)ceil_div(M, t.bm);
  p.nt = (int)ceil_div(N, t.bn);
  p.ktiles = (int)ceil_div(K, t.bk);
  const int tiles = p.mt * p.nt;
  int splits = 1;
  const int target = split_target(dtype, op, K);
  if (tiles < target) {
    splits = (int)ceil_div(target, tiles);
    const int max_by_k = std::max(1, p.ktiles / 8);
    splits = std::min(std::min(splits, max_by_k), 256);
  }
  if (cfg_splits(cfg) > 0) splits = std::min(cfg_splits(cfg), std::max(p.ktiles, 1));
  if (e.sk) {
    // stream-K: a fixed grid (two blocks per CU at most resident; larger
    // tiles run it in two equal rounds), at least kSkMinIters K-tiles each
    // (the config's split field picks the grid instead: 128 x s blocks, s <= 8)
    const long long grid = cfg_splits(cfg) > 0 ? 128LL * std::min(cfg_splits(cfg), 8) : kSkBlocks;
    splits = 1;
    const long long W = (long long)tiles * std::max(p.ktiles, 1);
    const long long P = std::max(1LL, std::min<long long>(grid, W / kSkMinIters));
    p.sk = true;
    p.sk_ipb = ceil_div(W, P);
    p.sk_blocks = (int)ceil_div(W, p.sk_ipb);
    p.sk_slot = t.bm * t.bn;   // two per block: the first segment's piece and the owner's last
  }
  p.kt_per_split = (int)ceil_div(std::max(p.ktiles, 1), splits);
  p.splits = (int)ceil_div(std::max(p.ktiles, 1), p.kt_per_split);
  return p;
}

int heuristic_cfg(int dtype, int M, int N, int K) {
  double best = 1e300;
  int bc = 0;
  for (int c = 0; c < std_count(dtype); ++c) {
    const TileCfg& t = *cfg_entry(dtype, c).t;
    const double tiles = (double)ceil_div(M, t.bm) * ceil_div(N, t.bn);
    double work = tiles * t.bm * t.bn / t.eff;
    // grids that cannot fill the 256 CUs and cannot be split along K lose
    if (tiles < 256 && ceil_div(K, t.bk) < 32) work *= 256.0 / tiles;
    if (work < best * 0.999) { best = work; bc = c; }
  }
  return bc;
}

Plan plan_for(const jr_conv_desc* d, int op, int dtype, const Phase& ph, int force_cfg) {
  int M, N, K;
  gemm_dims(d, op, dtype, ph, &M, &N, &K);
  int cfg = force_cfg < 0 ? tune_lookup(tune_key(dtype, op, M, N, K, d)) : force_cfg;
  // a halo config (tuned, pinned or forced) only where its geometry holds
  if (cfg < 0 || (cfg_entry(dtype, cfg_tile(cfg)).halo && !halo_ok(d, op, dtype, cfg_tile(cfg))))
    cfg = heuristic_cfg(dtype, M, N, K);
  return plan_with(dtype, cfg, M, N, K, op);
}

Plan dgrad_phase_plan(const jr_conv_desc* d, int dtype, const Phase& p, int force_cfg, bool* ok) {
  *ok = p.hc > 0 && p.wc > 0;
  if (p.na == 0 || p.nb == 0) {
    const int M = d->n * p.hc * p.wc;
    Plan pl = plan_with(dtype, heuristic_cfg(dtype, M, d->c_in, 16), M, d->c_in, 16, OP_DGRAD);
    pl.K = 0; pl.ktiles = 0; pl.splits = 1; pl.kt_per_split = 1;
    return pl;
  }
  return plan_for(d, OP_DGRAD, dtype, p, force_cfg);
}

// -------------------------------------------------- reduce and workspace
int reduce_lanes(const Plan& p) {
  const long long total = (long long)p.M * p.N / 4;
  int G = 1;
  while (G < 64 && G * 4 <= p.splits && total * G < 128 * 1024) G *= 2;
  return G;
}

size_t plan_ws(const Plan& p) {
  if (p.sk) return 2 * (size_t)p.sk_blocks * p.sk_slot * sizeof(float);
  return p.splits > 1 ? (size_t)p.splits * (size_t)p.M * (size_t)p.N * sizeof(float) : 0;
}

void stats_geom(int dtype, const Plan& p, int* P, int* R) {
  const TileCfg& t = *cfg_entry(dtype, p.tile).t;
  if (p.splits <= 1) {
    *R = t.bm / t.wgm;
    *P = p.mt * t.wgm;
    return;
  }
  const int rpp = 256 / (std::min(p.N, 1024) / 4);
  int r = std::max<int>(rpp, (int)ceil_div(p.M, 512));
  r = (int)ceil_div(r, rpp) * rpp;
  *R = r;
  *P = (int)ceil_div(p.M, r);
}

size_t stats_ws(int dtype, const Plan& p) {
  int P, R;
  stats_geom(dtype, p, &P, &R);
  const size_t S = P > kStatsChunk ? (size_t)ceil_div(P, kStatsChunk) : 0;
  return (2 * (size_t)p.N * P + 3 * (size_t)p.N * S) * sizeof(float);
}

size_t member_ws(int dtype, const Plan& p, bool stats) {
  return align256(stats ? align256(plan_ws(p)) + stats_ws(dtype, p) : plan_ws(p));
}

size_t ws_bytes_for(const jr_conv_desc* d, int op, int dtype) {
  const OpPhases phases(d, op);
  size_t w = 0, sw = 0;
  for (int i = 0; i < phases.n; ++i) {
    if (!phase_live(op, phases.ph[i])) continue;
    for (int c = 0; c < cfg_count(dtype); ++c) {
      const Plan p = plan_for(d, op, dtype, phases.ph[i], c);
      w = std::max(w, plan_ws(p));
      if (op == OP_FWD) {   // fused BN statistics partials, split or not
        Plan p1 = p;
        p1.splits = 1;
        sw = std::max(sw, std::max(stats_ws(dtype, p), stats_ws(dtype, p1)));
      }
    }
  }
  // 2x: room for the autotuner's doubled split-K factors; FWD: the statistics
  // partials live behind the slabs (or, conv2d_1's direct kernel, at 0)
  if (op == OP_FWD && conv1_direct_ok(d, dtype)) sw = std::max(sw, conv1_direct_ws(d));
  return op == OP_FWD ? align256(2 * w) + sw : 2 * w;
}

int validate(const jr_conv_desc* d, int op, int dtype) {
  if (!known_dtype(dtype)) return fail(JR_ERR_INVALID, "conv: bad dtype");
  const int q = bf16_operands(dtype) ? 8 : 4;   // channels per 16 B piece
  if (!d) return fail(JR_ERR_INVALID, "conv: null descriptor");
  if (op < OP_FWD || op > OP_WGRAD) return fail(JR_ERR_INVALID, "conv: bad op");
  if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->c_in <= 0 || d->c_out <= 0 || d->kh <= 0 ||
      d->kw <= 0 || d->stride_h <= 0 || d->stride_w <= 0 || d->pad_h < 0 || d->pad_w < 0)
    return fail(JR_ERR_INVALID, "conv: non-positive dimension");
  const int ho = (d->h + 2 * d->pad_h - d->kh) / d->stride_h + 1;
  const int wo = (d->w + 2 * d->pad_w - d->kw) / d->stride_w + 1;
  if (ho != d->ho || wo != d->wo || ho <= 0 || wo <= 0)
    return fail(JR_ERR_INVALID, "conv: ho/wo inconsistent with h,w,k,stride,pad");
  if (d->pad_h >= d->kh || d->pad_w >= d->kw)
    return fail(JR_ERR_INVALID, "conv: padding must be smaller than the kernel");
  const int cp = chan_pad(d->c_in, dtype);
  if (d->x_c_off < 0 || d->x_c_off + cp > d->x_c_stride)
    return fail(JR_ERR_INVALID, "conv: input channel slice (padded to 4 fp32 / 8 bf16 channels) out of range");
  if (d->y_c_off < 0 || d->y_c_off + d->c_out > d->y_c_stride)
    return fail(JR_ERR_INVALID, "conv: output channel slice out of range");
  if (d->c_out % 16 != 0)
    return fail(JR_ERR_UNSUPPORTED, "conv: c_out must be a multiple of 16");
  if (d->x_c_off % q || d->x_c_stride % q || d->y_c_off % q || d->y_c_stride % q)
    return fail(JR_ERR_INVALID, "conv: channel offsets and strides must be multiples of 4 (fp32) / 8 (bf16)");
  if (op == OP_DGRAD && d->c_in % q != 0)
    return fail(JR_ERR_UNSUPPORTED, "conv bwd_data: c_in must be a multiple of 4 (fp32) / 8 (bf16)");
  if (d->stride_h * d->stride_w > 64) return fail(JR_ERR_UNSUPPORTED, "conv: stride too large");
  const long long xin = (long long)d->n * d->h * d->w * d->x_c_stride;
  const long long yout = (long long)d->n * d->ho * d->wo * d->y_c_stride;
  const long long wsz = (long long)d->kh * d->kw * d->c_in * d->c_out;
  if (xin >= (1LL << 31) || yout >= (1LL << 31) || wsz >= (1LL << 31))
    return fail(JR_ERR_INVALID, "conv: tensor too large for 32-bit element offsets");
  return JR_OK;
}

// ---------------------------------------------------- division-free decode
FastDiv fastdiv_for(unsigned long long d, unsigned long long nmax) {
  const FastDiv none{0u, 0u, 0u};
  if (d == 0 || d > 0x7fffffffULL || nmax > 0xffffffffULL) return none;
  if (d == 1) return nmax < 0xffffffffULL ? FastDiv{0xffffffffu, 0xffffffffu, 0u} : none;
  unsigned s = 0;
  while ((2ULL << s) <= d) ++s;                 // floor(log2 d)
  if ((1ULL << s) == d) return FastDiv{0x80000000u, 0u, s - 1};   // n >> k, every 32-bit n
  const unsigned long long two = 1ULL << (32 + s);
  const unsigned long long m = (two + d - 1) / d;   // < 2^32 (d > 2^s)
  const unsigned long long e = m * d - two;         // < d
  // exact while n e < 2^(32+s): e < 2^31 and nmax < 2^32, so the product fits 64 bits
  if (e != 0 && nmax > (two - 1) / e) return none;
  return FastDiv{(unsigned)m, 0u, s};
}

ConvDivs conv_divs(const jr_conv_desc* d, int dtype, const Phase& ph, const Plan& p, bool* exact,
                   unsigned long long* div, unsigned long long* nmax) {
  const TileCfg& t = *cfg_entry(dtype, p.tile).t;
  const unsigned long long cp = (unsigned long long)chan_pad(d->c_in, dtype);
  // the stream-K walk keeps its iteration indices in 32-bit ints where it multiplies
  const bool walk32 = (unsigned long long)std::max(p.mt * (long long)p.nt, 1LL) * std::max(p.ktiles, 1) + p.ktiles < (1ULL << 31);
  // the largest row and reduction index a block decodes: tiles are whole, and
  // a row past M may be decoded before it is dropped
  const unsigned long long rows = (unsigned long long)std::max(p.mt, 1) * t.bm - 1;
  const unsigned long long ks = (unsigned long long)std::max(p.ktiles, 1) * t.bk - 1;
  const unsigned long long both = std::max(rows, ks);
  const unsigned long long W = (unsigned long long)std::max(p.mt * p.nt, 1) * std::max(p.ktiles, 1);
  unsigned long long dd[DV_COUNT] = {}, nn[DV_COUNT] = {};
  dd[DV_HW] = (unsigned long long)d->ho * d->wo;   nn[DV_HW] = both;      // FWD rows, WGRAD pixels along k
  dd[DV_WO] = (unsigned long long)d->wo;           nn[DV_WO] = std::max<unsigned long long>(both, t.bk);   // (WGRAD: BK / wo)
  dd[DV_HCWC] = (unsigned long long)ph.hc * ph.wc; nn[DV_HCWC] = rows;    // DGRAD rows of the phase
  dd[DV_WC] = (unsigned long long)ph.wc;           nn[DV_WC] = rows;
  dd[DV_CP] = cp;                                  nn[DV_CP] = both;      // FWD k, WGRAD rows
  dd[DV_COUT] = (unsigned long long)d->c_out;      nn[DV_COUT] = ks;      // DGRAD k
  dd[DV_KW] = (unsigned long long)d->kw;           nn[DV_KW] = both;      // taps of FWD k / WGRAD rows
  dd[DV_NB] = (unsigned long long)ph.nb;           nn[DV_NB] = ks;        // taps of DGRAD k
  dd[DV_NTN] = (unsigned long long)p.nt;           nn[DV_NTN] = W;        // tile -> (mt, nt)
  dd[DV_KTILES] = p.sk && walk32 ? (unsigned long long)p.ktiles : 0; nn[DV_KTILES] = W + p.ktiles;   // stream-K walk
  dd[DV_IPB] = p.sk && walk32 ? (unsigned long long)p.sk_ipb : 0;    nn[DV_IPB] = W + p.ktiles;
  ConvDivs out{};
  // a divisor of 0 is one this launch never divides by (DV_HCWC outside DGRAD,
  // a DGRAD phase no tap reaches, the walk of a plain grid); a stream-K walk
  // past 32-bit iteration indices has no exact reciprocal either
  *exact = !p.sk || walk32;
  for (int i = 0; i < DV_COUNT; ++i) {
    out.f[i] = fastdiv_for(dd[i], nn[i]);
    if (dd[i] != 0 && out.f[i].m == 0) *exact = false;
    if (div) div[i] = dd[i];
    if (nmax) nmax[i] = nn[i];
  }
  return out;
}

// ------------------------------------------------------------ conv1 direct
bool conv1_direct_ok(const jr_conv_desc* d, int dtype) {
  // opt-in (JR_CONV1_DIRECT=1, read once), fp32 only: per kernel (rocprofv3,
  // tools/conv1_probe.py, profiles/r05_conv1_kernels.txt) the x8 GEMM + its
  // two-stage finalize take ~138 us and this kernel ~108 us, but the bf16 GEMM
  // 68.5 us against 91-103 us; and its summation order moves the chaotic
  // B=16 100-step fp32 loss curve past test_gpu_golden's 3x-envelope bar at
  // steps 38-45 (the GEMM path stays inside it) -- off by default
  static const bool on = [] {
    const char* e = std::getenv("JR_CONV1_DIRECT");
    return e && e[0] == '1';
  }();
  const int q = 4;
  return on && (dtype == JR_F32 || dtype == JR_F32_X8) && d->c_in <= 3 &&
         d->x_c_stride == q && d->x_c_off == 0 && d->c_out == kD1Cout && d->y_c_off == 0 &&
         d->y_c_stride == kD1Cout && d->kh == 3 && d->kw == 3 && d->stride_h == 2 && d->stride_w == 2 &&
         d->pad_h == 0 && d->pad_w == 0;
}

void conv1_direct_partials(const jr_conv_desc* d, int* P, int* R) {
  const long long M = (long long)d->n * d->ho * d->wo;
  *R = kD1Rows;
  *P = (int)ceil_div(M, kD1Rows);
}

size_t conv1_direct_ws(const jr_conv_desc* d) {
  int P, R;
  conv1_direct_partials(d, &P, &R);
  return align256((size_t)2 * d->c_out * P * sizeof(float));
}

// -------------------------------------------------------------- tune cache
namespace {
struct TuneCache {
  std::mutex mu;
  std::map<TuneKey, int> tuned;
  unsigned long long gen = 1;
};
TuneCache& tune_cache() {
  static TuneCache c;
  return c;
}
}  // namespace

TuneKey tune_key(int dtype, int op, int M, int N, int K, const jr_conv_desc* d) {
  return TuneKey{dtype, op, M, N, K, d->h, d->w, d->kh, d->kw, d->stride_h, d->c_in, d->c_out, d->n};
}

int tune_lookup(const TuneKey& k) {
  TuneCache& c = tune_cache();
  std::lock_guard<std::mutex> lk(c.mu);
  auto it = c.tuned.find(k);
  return it != c.tuned.end() ? it->second : -1;
}

void tune_set(const TuneKey& k, int cfg) {
  TuneCache& c = tune_cache();
  std::lock_guard<std::mutex> lk(c.mu);
  auto it = c.tuned.find(k);
  if (cfg < 0) {
    if (it != c.tuned.end()) { c.tuned.erase(it); ++c.gen; }
  } else if (it == c.tuned.end() || it->second != cfg) {
    c.tuned[k] = cfg;
    ++c.gen;
  }
}

unsigned long long tune_generation() {
  TuneCache& c = tune_cache();
  std::lock_guard<std::mutex> lk(c.mu);
  return c.gen;
}

}  // namespace jr
