// Load-time dequantization of whisper.cpp's block-quantized tensors (ggml q4_0 / q4_1 / q5_0 /
// q5_1 / q8_0, layouts in ggml_file.h) into the f16 weight buffers the model runs from.
//
//  k_dequant<type>   raw blocks -> f16, bit-identical to the host definition ggml_dequant_f32 +
//                    one round-to-nearest-even: float(d) * q (+ float(m)) in f32, then f16.
//
// A block is 18 / 20 / 22 / 24 / 34 bytes, so blocks are only 2-byte aligned.  A workgroup owns
// DQ_WG_BLOCKS = 256 consecutive blocks: 256 * block bytes is a multiple of 512, so every
// workgroup's raw span starts 16-byte aligned in a 16-byte-aligned source.  The span is copied
// into LDS with aligned 16-byte global loads (dwords for the tail of the last, partial workgroup:
// at most the source rounded up to a dword is read, padding the caller provides), then every
// lane expands 8 consecutive elements of one block from LDS with 2-byte reads and stores one
// 16-byte f16 vector: lane t of pass k writes vector k * 256 + t, fully coalesced.
#include "../common.h"
#include "../ggml_file.h"
#include "../prof.h"
#include "kernels.h"

namespace wdr {

constexpr int DQ_WG_BLOCKS = 256;   // blocks per workgroup (tests/test_gpu_ggml_quant.py sizes follow it)
constexpr int DQ_THREADS = 256;

template <int TYPE>
__global__ __launch_bounds__(DQ_THREADS) void k_dequant(const uint8_t* __restrict__ src, long long n_blocks,
                                                        f16* __restrict__ dst) {
  constexpr int BS = TYPE == 2 ? 18 : TYPE == 3 ? 20 : TYPE == 6 ? 22 : TYPE == 7 ? 24 : 34;
  constexpr bool HAS_M = TYPE == 3 || TYPE == 7, HAS_QH = TYPE == 6 || TYPE == 7;
  constexpr int QS_OFF = BS - (TYPE == 8 ? 32 : 16);             // bytes in front of qs
  constexpr int SUB = TYPE == 2 ? 8 : TYPE == 6 ? 16 : 0;
  __shared__ __attribute__((aligned(16))) uint32_t raw[DQ_WG_BLOCKS * BS / 4];

  const long long b0 = (long long)blockIdx.x * DQ_WG_BLOCKS;
  const int nb = (int)(n_blocks - b0 < DQ_WG_BLOCKS ? n_blocks - b0 : DQ_WG_BLOCKS);   // >= 1 by the grid size
  const int bytes = nb * BS;
  const uint8_t* span = src + b0 * BS;   // 16-byte aligned: b0 * BS is a multiple of 512
  const int n16 = bytes / 16;
  for (int i = threadIdx.x; i < n16; i += DQ_THREADS) ((uint4*)raw)[i] = ((const uint4*)span)[i];
  const int ndw = (bytes + 3) / 4;       // the last dword may reach into the source's padding
  for (int i = n16 * 4 + threadIdx.x; i < ndw; i += DQ_THREADS) raw[i] = ((const uint32_t*)span)[i];
  __syncthreads();

  const uint16_t* h = (const uint16_t*)raw;   // block b starts at halfword b * BS / 2
  for (int v = threadIdx.x; v < nb * 4; v += DQ_THREADS) {
    const int b = v >> 2, p = v & 3;          // elements 8 p .. 8 p + 7 of block b
    const uint16_t* blk = h + b * (BS / 2);
    const float d = (float)__builtin_bit_cast(f16, blk[0]);
    float m = 0.f;
    if constexpr (HAS_M) m = (float)__builtin_bit_cast(f16, blk[1]);
    uint32_t qh = 0;
    if constexpr (HAS_QH) qh = ((uint32_t)blk[HAS_M ? 2 : 1] | (uint32_t)blk[HAS_M ? 3 : 2] << 16) >> (8 * p);
    // the 8 source bytes: q8_0 qs[8p..8p+7]; else qs[8 (p & 1) ..], low nibbles for p < 2, high after
    const uint16_t* qs = blk + QS_OFF / 2 + (TYPE == 8 ? 4 * p : 4 * (p & 1));
    const int shift = TYPE == 8 ? 0 : 4 * (p >> 1);
    f16x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t byte = (qs[i >> 1] >> (8 * (i & 1))) & 0xff;
      int q;
      if constexpr (TYPE == 8) q = (int)(int8_t)byte;
      else q = (int)(((byte >> shift) & 15) | ((qh >> i) & 1) << 4) - SUB;
      float x = d * (float)q;   // exact in f32
      if constexpr (HAS_M) x += m;
      // the f32 value is materialised: the f16 conversion must round the f32 sum, not fuse with
      // the multiply-add into one rounding (v_fma_mix), which would differ from the host's two
      asm("" : "+v"(x));
      o[i] = (f16)x;
    }
    *(f16x8*)(dst + (b0 * 4 + v) * 8) = o;
  }
}

void launch_dequant(int type, const void* blocks, long long n_blocks, f16* dst, hipStream_t s) {
  WDR_CHECK(ggml_block_bytes(type) != 0, "dequant: not a block-quantized ggml type");
  WDR_CHECK(((uintptr_t)blocks & 15) == 0 && ((uintptr_t)dst & 15) == 0, "dequant: buffers must be 16-byte aligned");
  if (n_blocks <= 0) return;
  const long long wgs = (n_blocks + DQ_WG_BLOCKS - 1) / DQ_WG_BLOCKS;
  WDR_CHECK(wgs <= 0x7fffffffLL, "dequant: tensor too large");
  const dim3 grid((unsigned)wgs), block(DQ_THREADS);
  const uint8_t* src = (const uint8_t*)blocks;
  switch (type) {
    case 2: WDR_KLAUNCH(k_dequant<2>, grid, block, 0, s, src, n_blocks, dst); break;
    case 3: WDR_KLAUNCH(k_dequant<3>, grid, block, 0, s, src, n_blocks, dst); break;
    case 6: WDR_KLAUNCH(k_dequant<6>, grid, block, 0, s, src, n_blocks, dst); break;
    case 7: WDR_KLAUNCH(k_dequant<7>, grid, block, 0, s, src, n_blocks, dst); break;
    default: WDR_KLAUNCH(k_dequant<8>, grid, block, 0, s, src, n_blocks, dst); break;
  }
  WDR_HIP(hipGetLastError());
}

}  // namespace wdr
