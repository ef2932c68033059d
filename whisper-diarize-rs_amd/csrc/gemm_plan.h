// Encoder GEMM dispatch (projections of more than 64 rows): which kernel of the tiled family in
// kernels/gemm.hip runs a shape, on what grid and with how much dynamic LDS.  A pure host
// function of the shape and the A/B knobs -- no HIP, no GPU -- so the rule can be tested on its
// own (tests/test_gemm_plan.py through wdr_dbg_gemm_plan); launch_proj / launch_proj_fp8 launch
// what it returns.
#pragma once

#include <cstdint>

namespace wdr {

// Epilogue selectors for the projection kernels (GEMM / GEMV).
enum Epi : int {
  EPI_F16 = 0,          // out16 = acc + bias
  EPI_F16_GELU = 1,     // out16 = gelu_tanh(acc + bias)
  EPI_F32_RESID = 2,    // out32 += acc + bias          (pre-LN residual stream update)
  EPI_F32 = 3,          // out32 = acc + bias
  EPI_F32_GELU_POS = 4, // out32 = gelu_tanh(acc + bias) + pos[row % pos_rows]  (conv2 + positional)
  EPI_QKV_CACHE = 5,    // cols [0,d) -> out16 (Q); [d,2d) / [2d,3d) -> K / V self-attention cache rows
  EPI_XKV = 6,          // cross K/V of all layers (N = L*2d) into head-major slots (XKV_* in common.h):
                        // row = window*1500 + key -> slot out + window*seq_stride
  EPI_F8_GELU = 7       // fp8 GEMM only: out8 = e4m3(gelu_tanh(acc + bias)) with MX scales o_sc
                        // (the encoder fc1 -> fc2 operand, Fp8Operand layout)
};

// tile shapes: k_gemm / k_gemm2 128 x 128 (BK 32 / 64), the ping-pong kernels 256 rows x 256
// (k_gemm4, k_gemm8) or 128 (k_gemm5, k_gemm8n) columns, a K-tile of 128 B per row (64 f16, 128 fp8)
constexpr int GB_M = 128, GB_N = 128, GB_K = 32;
constexpr int G2_BK = 64;
constexpr int G3_M = 256, G3_N = 256, G3_BK = 64;
constexpr int G8_BK = 128;
// dynamic LDS of the ping-pong kernels: two buffers of 16-KB half-tile images (4 per 256 x 256
// tile, 3 per 256 x 128 tile), fp8 plus 2-KB scale images (a double buffer / a ring of three)
constexpr uint32_t G4_LDS = 2u * 4u * 16384u;           // 128 KB
constexpr uint32_t G5_LDS = 2u * 3u * 16384u;           // 96 KB
constexpr uint32_t G8_LDS = G4_LDS + 2u * 2048u;        // 132 KB
constexpr uint32_t G8N_LDS = G5_LDS + 3u * 2048u;       // 102 KB

enum GemmKernel : int { K_GEMM = 0, K_GEMM2 = 1, K_GEMM4 = 2, K_GEMM5 = 3, K_GEMM8 = 4, K_GEMM8N = 5 };

// A/B knobs of the dispatch, read from the environment once per process (gemm_knobs_reload:
// tools/gemm_bench sets them per variant).  The values are the variables' own:
//   WDR_GEMM1=1       every projection on k_gemm
//   WDR_GEMM4=0|1     the ping-pong f16 kernels off (k_gemm2 / k_gemm take their shapes) / k_gemm4
//                     forced on every shape it takes (unset, -1: the measured rule)
//   WDR_GEMM4_GM      row tiles per group of the ping-pong kernels' tile order, f16 and fp8 (4)
//   WDR_GEMM5=1       the narrow projections (o, fc2) on k_gemm5's 256 x 128 tiles.  Off since
//                     round 4: on the encode-ahead streams' 224 CUs its 240 tiles of o / fc2 take
//                     two rounds where k_gemm4's 120 take one and leave ~100 CUs to the decode
//                     chain (1-h bench 737-739 vs 725-731 xRT, profiles/r04/ab_gemm5.txt)
//   WDR_GEMM5_WIDE=0  fc1 (N = 4d) off k_gemm5
//   WDR_GEMM8N=0      the narrow fp8 projections on k_gemm8's 256 x 256 tiles
//   WDR_GEMM_CUS      persistent k_gemm4 / k_gemm5 workgroups, rounded down to a multiple of 8
//                     (0: one per tile; the fp8 kernels do not honour it)
struct GemmKnobs {
  int gemm1 = 0, gemm4 = -1, tile_gm = 4, gemm5 = 0, gemm5_wide = 1, gemm8n = 1, cus = 0;
};
GemmKnobs gemm_knobs_env();        // the environment's values now
const GemmKnobs& gemm_knobs();     // the process's values (read once)
void gemm_knobs_reload();          // re-read them: tools/gemm_bench's per-variant A/B only

struct GemmShape {
  int M, N, K;      // M > 64; f16: N % 128, K % 32; fp8: what launch_proj_fp8 accepts
  int epi;          // Epi
  int ldo, d;       // output row stride; EPI_QKV_CACHE's model width
  bool gemm_ref;    // ProjArgs::gemm_ref: k_gemm whatever the rule picks (f16 only)
  bool fp8;         // launch_proj_fp8's operands
};
struct GemmPlan {
  GemmKernel kernel;
  int grid_x, grid_y;   // workgroups (grid_y > 1 on k_gemm only)
  uint32_t lds;         // dynamic LDS bytes
};
GemmPlan gemm_plan(const GemmShape& s, const GemmKnobs& k);

}  // namespace wdr
