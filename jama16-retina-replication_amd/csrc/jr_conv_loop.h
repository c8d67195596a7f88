// jr_conv_loop.h — what the three GEMM convolution kernels (k_conv in
// jr_conv.hip, k_conv_bf16 in jr_conv_bf16.hip, k_conv_halo in
// jr_conv_halo.hip) share of their device skeleton: the vector types and the
// tile geometry.  Their K-tile ring, stream-K walk and address generation are
// still written per kernel: every shared form tried so far moved the register
// budget or the wait counts of some instantiation (DESIGN.md §3 has the
// numbers; tools/kernel_meta.py old new is the check).
// Included by those three files only -- jr_conv_direct.hip shares
// jr_conv_impl.h, and its code object moves with what that header declares.
#pragma once
#include "jr_conv_impl.h"

namespace jr {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- geometry
// The wave tile: WGM x WGN waves over a BM x BN block tile, TM x TN 32x32
// MFMA accumulators per wave.
template <int BM, int BN, int WGM, int NW>
struct WaveTile {
  static constexpr int WGN = NW / WGM;
  static constexpr int WM = BM / WGM, WN = BN / WGN;
  static constexpr int TM = WM / 32, TN = WN / 32;
  static_assert(WM % 32 == 0 && WN % 32 == 0, "wave tile must be a multiple of 32x32");
};

// The operand images of one K-tile, staged by 16 B LDS-DMA pieces of EPQ
// elements (4 floats or 8 bf16); one wave-instruction moves 64 pieces.
template <int BM, int BN, int WGM, int NW, int BK, int EPQ>
struct TileGeom : WaveTile<BM, BN, WGM, NW> {
  static constexpr int QPR = BK / EPQ;                 // 16 B quads per KC row
  static constexpr int RPI = 64 / QPR;                 // KC rows per DMA instruction
  static constexpr int SWZ = 16 / QPR;                 // rows sharing one swizzle value
  static constexpr int ASZ = BM * BK, BSZ = BN * BK;   // elements per image
  static constexpr int IEL = 64 * EPQ;                 // elements per DMA instruction
  static constexpr int A_INSTR = ASZ / IEL, B_INSTR = BSZ / IEL;
  static constexpr int A_PW = (A_INSTR + NW - 1) / NW, B_PW = (B_INSTR + NW - 1) / NW;  // per wave
  static_assert(ASZ % IEL == 0 && BSZ % IEL == 0, "tile must be whole DMA instructions");
  static_assert(QPR >= 1 && QPR <= 16 && 64 % QPR == 0, "a KC row is 1..16 quads");
};

}  // namespace jr
