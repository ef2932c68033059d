// Encoder GEMM dispatch rule (gemm_plan.h).  The measurements behind every threshold stand next
// to it; all are tools/gemm_bench on large-v3 shapes, alone on the GPU, unless a bench is named.
#include "gemm_plan.h"

#include "env.h"

namespace wdr {

GemmKnobs gemm_knobs_env() {
  const GemmKnobs def;
  GemmKnobs k;
  k.gemm1 = env_int("WDR_GEMM1", def.gemm1);
  k.gemm4 = env_int("WDR_GEMM4", def.gemm4);
  k.tile_gm = env_int("WDR_GEMM4_GM", def.tile_gm);
  k.gemm5 = env_int("WDR_GEMM5", def.gemm5);
  k.gemm5_wide = env_int("WDR_GEMM5_WIDE", def.gemm5_wide);
  k.gemm8n = env_int("WDR_GEMM8N", def.gemm8n);
  k.cus = env_int("WDR_GEMM_CUS", def.cus);
  return k;
}
static GemmKnobs& process_knobs() {
  static GemmKnobs k = gemm_knobs_env();
  return k;
}
const GemmKnobs& gemm_knobs() { return process_knobs(); }
void gemm_knobs_reload() { process_knobs() = gemm_knobs_env(); }

static int cdiv_i(int a, int b) { return (a + b - 1) / b; }

GemmPlan gemm_plan(const GemmShape& s, const GemmKnobs& k) {
  const int M = s.M, N = s.N, K = s.K;
  const int rows256 = cdiv_i(M, G3_M);
  if (s.fp8) {
    // the narrow projections (o, fc2: N = 1280) on 256 x 128 tiles: 240 at M = 6000 where 256 x 256
    // tiles fill 120 CUs.  N % 256 != 0 (tiny's qkv, N = 1152) has only the 256 x 128 tiling; fc1's
    // GELU -> fp8 epilogue only the 256 x 256 one
    if (s.epi != EPI_F8_GELU && ((k.gemm8n != 0 && N < 2048) || N % G3_N != 0))
      return {K_GEMM8N, (N / 128) * rows256, 1, G8N_LDS};
    return {K_GEMM8, (N / G3_N) * rows256, 1, G8_LDS};
  }
  const bool ref = k.gemm1 != 0 || s.gemm_ref;
  const bool vec4 = s.ldo % 4 == 0 && (s.epi != EPI_QKV_CACHE || s.d % 4 == 0);   // epi_store4
  const bool tiled = !ref && vec4;   // every kernel but k_gemm stores four columns at a time
  // persistent form of the ping-pong kernels: WDR_GEMM_CUS workgroups (a multiple of 8) walk the tiles
  const int cus = k.cus / 8 * 8;
  auto persistent = [&](int ntiles) { return cus > 0 && cus < ntiles ? cus : ntiles; };
  // fc1 (N = 4d) on k_gemm5's 256 x 128 tiles (WDR_GEMM5_WIDE, default on): on the encode-ahead
  // streams' 224 CUs k_gemm4's 480 tiles take 3 rounds where k_gemm5's 960 half-size tiles take
  // 5 (2.5 of the big ones); alone both run at the same per-tile rate (875 TFLOP/s)
  const bool wide5 = k.gemm5_wide != 0 && N >= 4096 && N < 16384 && M >= 4096;
  // WDR_GEMM5: the narrow encoder projections (o, fc2) where 256 x 256 tiles would leave CUs idle:
  // 256 x 128 tiles fill 240 of 256 CUs at M = 6000 (o 53 vs 62 us on k_gemm2, fc2 107 vs 126 us;
  // at M = 12000 k_gemm4's 235 tiles are faster: fc2 194 vs 216 us)
  const bool narrow5 = k.gemm5 != 0 && N < 2048 && (N / G3_N) * rows256 < 192;
  if (N % 128 == 0 && K % G3_BK == 0 && M >= 4096 && tiled && k.gemm4 != 0 && (wide5 || narrow5))
    return {K_GEMM5, persistent((N / 128) * rows256), 1, G5_LDS};
  // round 6, partial encode batches and on-demand windows (profiles/r06/gemm_bench_mid_m.txt,
  // bit-identical outputs): fc1 (N = 4d) at M = 1500 / 3000 39.7 / 44.4 us on k_gemm4 vs 45.0 /
  // 67.3 on k_gemm / the retired two-stage 256 x 256 k_gemm3; qkv (3d) at M = 3000 41.9 vs 50.2
  // (k_gemm2), at M = 1500 29.2 on k_gemm2 stays; o / fc2 (N = d) below M = 4096 stay on k_gemm2
  // (25.7 / 68.5 vs 43.3 / 110.4).
  // Ping-pong 256 x 256 tiles: M = 6000 qkv 600 vs 557 TFLOP/s (k_gemm2), fc1 616 and cross-K/V
  // 818 vs 509 / 641 on the 128 x 128 kernels (574 / 742 on k_gemm3); M = 12000 every shape (o 394
  // and fc2 811 vs 335 / 620, 382 / 743 on k_gemm3); M = 1500 cross-K/V 773 vs 616.  The N = 1280
  // shapes at M = 6000 fill only 120 of 256 CUs (alone: 209 / 478 vs 314 / 618 TFLOP/s on
  // k_gemm2), but inside the pipeline the CUs they leave run decode steps: 1-h bench 480 vs 476
  // xRT.
  if (N % G3_N == 0 && K % G3_BK == 0 && tiled &&
      (k.gemm4 == 1 || (k.gemm4 != 0 && (M >= 4096 || N >= 16384 || (N >= 4096 && M > 1024) || (N >= 3072 && M >= 2560)))))
    return {K_GEMM4, persistent((N / G3_N) * rows256), 1, G4_LDS};
  // LDS-DMA GEMM where it measured faster than k_gemm (M = 6000: qkv -5 %, o -11 %, fc2 -23 %;
  // fc1 and the 82k-column cross-K/V GEMM stay on k_gemm, +8 % / +7 % there)
  if (K % G2_BK == 0 && N <= 4096 && tiled) return {K_GEMM2, (N / GB_N) * cdiv_i(M, GB_M), 1, 0};
  return {K_GEMM, N / GB_N, cdiv_i(M, GB_M), 0};
}

}  // namespace wdr
