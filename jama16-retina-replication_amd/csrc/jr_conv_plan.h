// jr_conv_plan.h — host-only planning of the implicit-GEMM convolutions: the
// tile tables the kernels are instantiated from, the config-id space of each
// dtype, the plan of one GEMM (tile, split-K or stream-K grid), the workspace
// and statistics-partials sizing, descriptor validation and the tune cache.
// Plain C++ (jr_conv_plan.cpp): it compiles and is tested without a device
// (tests/test_conv_plan.py pins its output through the C ABI).
#pragma once
#include <array>
#include <cstddef>

#include "jr_error.h"

namespace jr {

enum { OP_FWD = 0, OP_DGRAD = 1, OP_WGRAD = 2 };

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// (an override must reach the planner and the launcher alike)
#ifndef JR_STATS_CHUNK
#define JR_STATS_CHUNK 4096
#endif
constexpr int kStatsChunk = JR_STATS_CHUNK;   // partials one finalize block combines

// ------------------------------------------------------------------ tiles
struct TileCfg {
  int bm, bn, wgm, bk, nbuf;
  double eff;  // relative MFMA efficiency guess used to rank padded work
  int nw = 4;  // waves per block (256 or 512 threads)
};

// Candidate tiles (block BMxBN, WGM waves along M, K-tile BK).  The planner
// ranks them by padded work / eff; jr_conv2d_autotune times them instead.
// The fp32-family launcher's switch (launch_op) has one arm per entry.
static constexpr TileCfg kCfgs[] = {
    {128, 128, 2, 16, 3, 1.00},  // 0: wave 64x64, 48 KiB LDS
    {128, 128, 2, 32, 2, 1.00},  // 1: 64 KiB
    {256, 64, 4, 16, 3, 1.00},   // 2: wave 64x64, 60 KiB
    {128, 64, 2, 16, 4, 0.92},   // 3: wave 64x32, 48 KiB
    {128, 64, 2, 32, 2, 0.92},   // 4: 48 KiB
    {128, 96, 4, 16, 3, 0.90},   // 5: wave 32x96, 42 KiB
    {256, 32, 4, 16, 4, 0.85},   // 6: wave 64x32, 72 KiB
    {64, 64, 2, 32, 3, 0.75},    // 7: wave 32x32, 48 KiB
    {128, 32, 4, 32, 3, 0.75},   // 8: wave 32x32, 60 KiB
    {64, 128, 2, 32, 2, 0.80},   // 9: wave 32x64, 48 KiB
    {128, 64, 2, 16, 2, 0.90},   // 10: wave 64x32, 24 KiB
    {128, 192, 2, 16, 3, 1.02},  // 11: wave 64x96, 60 KiB (N = 192 layers)
    {256, 96, 4, 16, 3, 1.02},   // 12: wave 64x96, 66 KiB (N = 96 layers)
    {256, 128, 2, 16, 3, 1.04},  // 13: wave 128x64, 72 KiB
};
constexpr int kNumCfgs = sizeof(kCfgs) / sizeof(kCfgs[0]);

// bf16 tiles (BK in bf16 elements; MFMA v_mfma_f32_32x32x16_bf16).
static constexpr TileCfg kCfgsBf16[] = {
    {128, 128, 2, 32, 3, 1.00},  // 0: wave 64x64, 48 KiB LDS
    {128, 128, 2, 64, 2, 1.00},  // 1: 64 KiB
    {256, 128, 2, 32, 3, 1.05},  // 2: wave 128x64, 72 KiB
    {128, 64, 2, 32, 3, 0.92},   // 3: wave 64x32, 36 KiB
    {256, 64, 4, 32, 3, 1.00},   // 4: wave 64x64, 60 KiB
    {128, 192, 2, 32, 3, 1.02},  // 5: wave 64x96, 60 KiB
    {128, 96, 4, 32, 3, 0.90},   // 6: wave 32x96, 42 KiB
    {64, 64, 2, 64, 3, 0.75},    // 7: wave 32x32, 48 KiB
    // one block per CU, wave tiles of 128 x 128 / 128 x 96: 16 / 12 MFMAs per
    // k-step against 4 DMA pieces per wave (0.25-0.33 DMA per MFMA, where the
    // 64 x 64 wave tiles issue 0.5: the per-MFMA issue budget is the bound)
    {256, 256, 2, 32, 3, 1.10},  // 8: wave 128x128, 96 KiB
    {256, 192, 2, 32, 3, 1.08},  // 9: wave 128x96, 84 KiB
    // deeper rings for the short-K-loop 17x17 / 8x8 GEMMs, whose K-tiles
    // carry few MFMAs per wave: NBUF - 2 stages stay in flight under the
    // compute of one (eff just below the same-shape tile above: the untuned
    // planner keeps its choice, autotuning / the pinned tables decide)
    {128, 64, 2, 32, 5, 0.91},   // 10: 60 KiB, 3 stages in flight
    {128, 128, 2, 32, 4, 0.99},  // 11: 64 KiB, 2 in flight
    {128, 96, 4, 32, 5, 0.89},   // 12: 70 KiB
    {128, 64, 2, 64, 3, 0.91},   // 13: 72 KiB, twice the MFMAs per K-tile
    // N = 32 GEMMs (the stem: conv1 / conv2 fwd and wgrad, conv2 / conv3
    // dgrad with N = c_in = 32), which the BN >= 64 tiles pad to twice the
    // MFMA work: four waves stacked along M, wave tile 64 x 32 / 32 x 32
    {256, 32, 4, 32, 3, 0.85},   // 14: 54 KiB
    {128, 32, 4, 32, 4, 0.80},   // 15: 40 KiB
    {256, 32, 4, 64, 3, 0.85},   // 16: 108 KiB
};
constexpr int kNumCfgsBf16 = sizeof(kCfgsBf16) / sizeof(kCfgsBf16[0]);

// JR_F32_X8P tiles: the bf16 kernel with three operand planes (h, m, l) and
// eight MFMAs per k-step, so BK = 16 (one k-step) already gives a wave
// 8 * TM * TN MFMAs per K-tile; LDS = NBUF * 3 * (BM + BN) * BK * 2 B.
static constexpr TileCfg kCfgsX8P[] = {
    {128, 128, 2, 16, 3, 1.00},  // 0: wave 64x64, 72 KiB LDS
    {128, 128, 2, 16, 4, 1.00},  // 1: 96 KiB
    {256, 128, 2, 16, 3, 1.05},  // 2: wave 128x64, 108 KiB
    {128, 64, 2, 16, 3, 0.92},   // 3: wave 64x32, 54 KiB
    {256, 64, 4, 16, 3, 1.00},   // 4: wave 64x64, 81 KiB
    {128, 192, 2, 16, 3, 1.02},  // 5: wave 64x96, 90 KiB
    {128, 96, 4, 16, 3, 0.90},   // 6: wave 32x96, 63 KiB
    {64, 64, 2, 32, 3, 0.75},    // 7: wave 32x32, 72 KiB
    {256, 256, 2, 16, 2, 1.10},  // 8: wave 128x128, 96 KiB
    {256, 192, 2, 16, 3, 1.08},  // 9: wave 128x96, 126 KiB
    {128, 64, 2, 16, 5, 0.91},   // 10: 90 KiB (deeper rings, as kCfgsBf16 10-13)
    {128, 128, 2, 16, 5, 0.99},  // 11: 120 KiB
    {128, 96, 4, 16, 4, 0.89},   // 12: 84 KiB
    {128, 64, 2, 32, 3, 0.91},   // 13: 108 KiB
    {256, 32, 4, 16, 3, 0.85},   // 14: 81 KiB (N = 32, as kCfgsBf16 14-16)
    {128, 32, 4, 16, 4, 0.80},   // 15: 60 KiB
    {256, 32, 4, 32, 2, 0.85},   // 16: 108 KiB
};
constexpr int kNumCfgsX8P = sizeof(kCfgsX8P) / sizeof(kCfgsX8P[0]);

// Wide tiles (round 3): 8 waves (512 threads, two per SIMD) on 256-row
// blocks, one block per CU.  Per K-tile a block moves (BM + BN) * BK operand
// elements through L2 -> LDS-DMA for BM * BN * BK MACs: at 128 x 128 that
// ratio needs ~2x the L2 -> LDS rate a CU sustains (~70 GB/s: the bf16 GEMMs
// ran at 0.1-0.2 of the MFMA peak and x8p at 0.57 MFMA busy), at 256 x 256
// half of it.  Two waves per SIMD hide each other's DMA issue, LDS reads and
// barrier waits.
static constexpr TileCfg kCfgsBf16W[] = {
    {256, 256, 2, 32, 3, 1.20, 8},   // 0: wave 128x64, 96 KiB
    {256, 192, 4, 32, 3, 1.16, 8},   // 1: wave 64x96, 84 KiB
    {256, 128, 4, 64, 2, 1.12, 8},   // 2: wave 64x64, 96 KiB
    {128, 256, 2, 64, 2, 1.12, 8},   // 3: wave 64x64, 96 KiB
    {256, 256, 2, 64, 2, 1.20, 8},   // 4: wave 128x64, 128 KiB
    {256, 192, 4, 64, 2, 1.16, 8},   // 5: wave 64x96, 112 KiB
    {256, 96, 8, 64, 2, 1.00, 8},    // 6: wave 32x96, 88 KiB
    {256, 64, 8, 64, 3, 0.95, 8},    // 7: wave 32x64, 120 KiB
};
constexpr int kNumCfgsBf16W = sizeof(kCfgsBf16W) / sizeof(kCfgsBf16W[0]);
static constexpr TileCfg kCfgsX8PW[] = {
    {256, 256, 2, 16, 3, 1.20, 8},   // 0: wave 128x64, 144 KiB
    {256, 192, 4, 16, 3, 1.16, 8},   // 1: wave 64x96, 126 KiB
    {256, 128, 4, 16, 3, 1.12, 8},   // 2: wave 64x64, 108 KiB
    {128, 256, 2, 16, 3, 1.12, 8},   // 3: wave 64x64, 108 KiB
    {256, 96, 8, 16, 4, 1.00, 8},    // 4: wave 32x96, 132 KiB
    {256, 64, 8, 16, 4, 0.95, 8},    // 5: wave 32x64, 120 KiB
    {128, 192, 4, 16, 3, 1.05, 8},   // 6: wave 32x96, 90 KiB
};
constexpr int kNumCfgsX8PW = sizeof(kCfgsX8PW) / sizeof(kCfgsX8PW[0]);

// Halo-tiled bf16 FWD configurations (the jr_conv_halo kernel): for stride-1 'same'
// convs of exactly this kh x kw with c_in % 32 == 0 whose halo (output rows a
// BM tile spans + kh - 1) x (w + kw - 1) fits in slots - 1 (the last slot
// stays zero).  t.bk = kh*kw*32 (one K-tile = one 32-channel chunk of every
// tap), so the planner's ktiles is the chunk count.  LDS per stage: slots x
// 64 B + kh*kw x BN x 64 B.
struct HaloCfg {
  int kh, kw, slots;
  TileCfg t;
};
static constexpr HaloCfg kHaloBf16[] = {
    {1, 7, 224, {128, 64, 2, 7 * 32, 2, 1.0}},   // 0: 17^2 1x7: 9 x 23 = 207 slots; 2 x 42 KiB
    {7, 1, 256, {128, 64, 2, 7 * 32, 2, 1.0}},   // 1: 17^2 7x1: 15 x 17 = 255 slots; 2 x 44 KiB
    {3, 3, 272, {128, 96, 4, 9 * 32, 2, 1.0}},   // 2: 35^2 3x3, N = 96: 7 x 37 = 259 slots; 2 x 71 KiB
    {3, 3, 272, {128, 64, 2, 9 * 32, 2, 1.0}},   // 3: 3x3, N = 64 tiles (8^2: 19 x 10 = 190 slots); 2 x 53 KiB
    {1, 3, 176, {128, 64, 2, 3 * 32, 3, 1.0}},   // 4: 8^2 1x3: 17 x 10 = 170 slots; 3 x 23 KiB
    {3, 1, 160, {128, 64, 2, 3 * 32, 3, 1.0}},   // 5: 8^2 3x1: 19 x 8 = 152 slots; 3 x 22 KiB
    {1, 7, 224, {128, 64, 2, 7 * 32, 3, 1.0}},   // 6: as 0, three stages (126 KiB)
    {7, 1, 256, {128, 64, 2, 7 * 32, 3, 1.0}},   // 7: as 1, three stages (132 KiB)
};
constexpr int kNumHaloBf16 = sizeof(kHaloBf16) / sizeof(kHaloBf16[0]);

// ------------------------------------------------------------- config ids
// A config id is tile id | (splits << 8): splits == 0 lets the planner pick
// the split-K factor, otherwise it is forced (autotuning explores both; on a
// stream-K id the field picks the grid instead).
constexpr int kSplitShift = 8;
// split-K factors up to 1024: the stem filter gradients (3 tiles of M = 288,
// K = 1.4 M pixels) still gain from 256 to 512 slabs (more resident blocks)
constexpr int kMaxSplits = 1024;
inline int cfg_tile(int cfg) { return cfg & ((1 << kSplitShift) - 1); }
inline int cfg_splits(int cfg) { return cfg >> kSplitShift; }

// What one tile id of a dtype is: the kernel family that runs it, the index
// into that family's tile table (kCfgs for F32_MFMA and X8_SPLIT; kCfgsBf16 /
// kCfgsBf16W for JR_BF16, kCfgsX8P / kCfgsX8PW for JR_F32_X8P; kHaloBf16),
// and whether the id is the stream-K grid of that tile.
enum class Kernel { F32_MFMA, X8_SPLIT, BF16, BF16_WIDE, HALO };
struct CfgEntry {
  Kernel kernel;
  int index;
  bool sk;
  const TileCfg* t;
  const HaloCfg* halo;   // HALO only
};
// id < cfg_count(dtype); JR_F32_X6H shares JR_F32_X8's ids and plans (the
// fp16 six-product kernel is chosen by dtype at launch)
const CfgEntry& cfg_entry(int dtype, int id);
int cfg_count(int dtype);   // 0 for an unknown dtype
int std_count(int dtype);   // the first ids: the dtype's standard tiles, which the planner heuristic ranks

// ------------------------------------------------------------------ plans
inline bool bf16_operands(int dtype) { return dtype == JR_BF16 || dtype == JR_F32_X8P; }
// Channel padding of the reduction operand: 16 B DMA pieces hold 4 fp32 or
// 8 bf16 channels.
int chan_pad(int c, int dtype);

// DGRAD: one GEMM per stride phase (py, px) (the jr_conv file header)
struct Phase {
  int py, px, r0, c0, na, nb, ey, ex, hc, wc;
};
// The phases of an op: DGRAD's stride_h * stride_w (validate bounds them by
// 64), otherwise a single nameless one.
struct OpPhases {
  Phase ph[64];
  int n;
  OpPhases(const jr_conv_desc* d, int op);
  // the phase a (op, phase) pair of the C ABI names (non-DGRAD ops ignore
  // `phase`); nullptr when out of range
  const Phase* at(int op, int phase) const { return op != OP_DGRAD ? ph : phase >= 0 && phase < n ? ph + phase : nullptr; }
};
// false: a DGRAD phase that no tap reaches or that holds no input pixel (no
// GEMM to plan or time; run_conv still zero-fills the former)
inline bool phase_live(int op, const Phase& p) { return op != OP_DGRAD || (p.na > 0 && p.nb > 0 && p.hc > 0 && p.wc > 0); }

struct Plan {
  int cfg;   // encoded id
  int tile;
  int M, N, K;
  int mt, nt, ktiles, splits, kt_per_split;
  // stream-K (k_conv SK): blocks and iterations (tiles x K-tiles) per block
  bool sk;
  int sk_blocks;
  long long sk_ipb;
  int sk_slot;   // floats of one block's partial (BM x BN)
};

void gemm_dims(const jr_conv_desc* d, int op, int dtype, const Phase& ph, int* M, int* N, int* K);
Plan plan_with(int dtype, int cfg, int M, int N, int K, int op);
int heuristic_cfg(int dtype, int M, int N, int K);
// the halo config `tile` fits this op and geometry
bool halo_ok(const jr_conv_desc* d, int op, int dtype, int tile);
// The plan of one GEMM: force_cfg, else the tune cache's entry, else the
// heuristic (also instead of a halo config where its geometry does not hold).
Plan plan_for(const jr_conv_desc* d, int op, int dtype, const Phase& ph, int force_cfg = -1);
// DGRAD plan of one stride phase as run_conv launches it (a phase no tap
// reaches is a K = 0 GEMM that stores zeros).  ok = false: nothing to launch.
Plan dgrad_phase_plan(const jr_conv_desc* d, int dtype, const Phase& p, int force_cfg, bool* ok);

// z-lanes per float4 column of the split-K reduce (k_splitk_reduce and the
// deferred k_wgrad_reduce: the same G gives the same summation order)
int reduce_lanes(const Plan& p);
// split-K slabs, or stream-K's two BM x BN fp32 partial slots per block
size_t plan_ws(const Plan& p);
// Fused BN statistics (FWD): partials of R rows each, P per column.  Without
// split-K the GEMM epilogue writes one per wave row-group (R = WM); with it,
// k_splitk_reduce_stats one per block of R rows (~512 blocks).
void stats_geom(int dtype, const Plan& p, int* P, int* R);
size_t stats_ws(int dtype, const Plan& p);
// Workspace of one member of a grouped GEMM: split-K slabs, then the fused
// BN statistics partials (their two-stage combine space included).
size_t member_ws(int dtype, const Plan& p, bool stats);
// Workspace of an op: twice the max over every config's planned split-K, so
// any tuned choice fits.
size_t ws_bytes_for(const jr_conv_desc* d, int op, int dtype);

int validate(const jr_conv_desc* d, int op, int dtype);

// ------------------------------------------------- division-free decode
// n / d for 0 <= n <= nmax as one 32 x 32 -> 64 multiply-add and a shift:
//   q = (uint32)((n * m + a) >> 32) >> s
// round-up form (a = 0): m = ceil(2^(32+s) / d), s = floor(log2 d) (d = 2^k,
// k >= 1: m = 2^31, s = k - 1).  With e = m d - 2^(32+s) (0 <= e < d) the
// quotient is exact while n e < 2^(32+s); e < 2^(s+1), so every n < 2^31 is.
// d = 1 has no 32-bit round-up multiplier: m = a = 2^32 - 1, s = 0 gives
// (n + 1)(2^32 - 1) >> 32 = n for n < 2^32 - 1.
// m = 0: the form is not exact on [0, nmax] (or d = 0, or d >= 2^31): no reciprocal.
struct FastDiv {
  unsigned m, a, s;
};
FastDiv fastdiv_for(unsigned long long d, unsigned long long nmax);
inline unsigned fastdiv_apply(const FastDiv& f, unsigned n) {
  return (unsigned)(((unsigned long long)n * f.m + f.a) >> 32) >> f.s;
}

// The reciprocals of one GEMM launch (ConvArgs::dv): of every runtime divisor
// the kernels' row, tap and column decode, the output addressing and the
// stream-K walk divide by, each valid over the whole range its dividends
// take in that launch (DV_*: the order of div[] / nmax[] below).
enum { DV_HW, DV_WO, DV_HCWC, DV_WC, DV_CP, DV_COUT, DV_KW, DV_NB, DV_NTN, DV_KTILES, DV_IPB, DV_COUNT };
struct ConvDivs {
  FastDiv f[DV_COUNT];
};
// exact = false: some divisor of the launch has no exact reciprocal on its
// range (FastDiv m = 0) -- the kernels carry no division to fall back to, so
// the launcher refuses such a GEMM (row, reduction or stream-K iteration
// indices of 2^31 and up: beyond validate's 32-bit tensor sizes in practice).
// div / nmax (optional): the divisors (0: unused by this launch) and the
// largest dividend of each.
// (of d: ho, wo, kw, c_in, c_out; of ph: hc, wc, nb -- zeros outside DGRAD)
ConvDivs conv_divs(const jr_conv_desc* d, int dtype, const Phase& ph, const Plan& p, bool* exact,
                   unsigned long long* div = nullptr, unsigned long long* nmax = nullptr);

// conv2d_1 as a direct VALU convolution (the jr_conv_direct kernel): the geometry
// test, its statistics partials (P of R rows) and their workspace
constexpr int kD1Rows = 1024;   // output pixels per block (= R of the statistics partials)
constexpr int kD1Cout = 32;
bool conv1_direct_ok(const jr_conv_desc* d, int dtype);
void conv1_direct_partials(const jr_conv_desc* d, int* P, int* R);
size_t conv1_direct_ws(const jr_conv_desc* d);

// ------------------------------------------------------------- tune cache
// (op, GEMM dims, conv geometry) -> config id: jr_conv2d_set_config and
// jr_conv2d_autotune write it, every plan_for reads it.  Thread-safe.
typedef std::array<int, 13> TuneKey;
TuneKey tune_key(int dtype, int op, int M, int N, int K, const jr_conv_desc* d);
int tune_lookup(const TuneKey& k);            // -1: no entry
void tune_set(const TuneKey& k, int cfg);     // cfg < 0 erases
// bumped whenever an entry changes value: a caller that bound plans (split-K
// slab sizes) to the overrides it applied re-applies them when it moved
// (jr_conv2d_config_generation)
unsigned long long tune_generation();

}  // namespace jr
