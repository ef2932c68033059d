// Audio ingest: interleaved PCM / float frames of any supported format, channel
// count and rate -> 16 kHz mono int16, bit-identical to the host definition audio_convert_host
// (audio_file.cpp): decode, f32 downmix in channel order, polyphase Kaiser-sinc FIR as one
// sequential fmaf chain per output in tap order, scale / clamp / round-to-nearest-even.
//
//  k_audio_convert<fmt>  a workgroup owns AC_WG_OUT = 256 consecutive outputs.  Their input span
//                        (floor(255 M / L) + 1 + T frames, at most AC_MAX_SPAN) is decoded and
//                        downmixed once into LDS as mono f32; then lane t runs the T taps of
//                        output t from LDS against row (k M) mod L of the coefficient table.
//
//  k_audio_convert<fmt, true>  the channel-keeping form: blockIdx.y is a channel;
//                        the workgroup stages the same raw span through the same tiles, decodes
//                        only sample y of each frame into LDS (no downmix, no invC: the mono
//                        definition's C == 1 branch), runs the same tap loop and writes plane y
//                        of a planar [C][out_stride] result.  One channel per workgroup keeps LDS
//                        at the downmix form's 38.6 KB; the raw bytes are read once per channel.
//
// Frames are 1 .. 32 bytes, so a frame is in general unaligned.  The raw bytes of the span are
// staged AC_RAW_TILE bytes at a time: the tile's byte range, widened to 16-byte boundaries, is
// copied into LDS with aligned 16-byte global loads (as k_dequant stages its blocks) and the
// frames are picked out of LDS.  Every load lies inside the staging buffer rounded up to 16
// bytes, padding the caller provides; frames outside [frame0, frame0 + n_stage) are never read
// and count as zero, which is both the definition's edge rule and the bound of every access.
#include "../audio_file.h"
#include "../common.h"
#include "../prof.h"
#include "kernels.h"

namespace wdr {

constexpr int AC_WG_OUT = 256;    // outputs per workgroup (tests/test_gpu_audio_convert.py sizes follow it)
constexpr int AC_THREADS = 256;
// 384 kHz in: M / L = 24, H = 768 -> 255 * 24 + 1 + 2 * 768 frames; no supported rate needs more
constexpr int AC_MAX_SPAN = 255 * 24 + 1 + 2 * 768;
constexpr int AC_RAW_TILE = 8192;   // raw bytes staged per pass (>= 256 frames of 32 bytes)

template <int FMT, bool SPLIT>
__global__ __launch_bounds__(AC_THREADS) void k_audio_convert(const uint8_t* __restrict__ raw, int C, float invC,
                                                              long long frame0, long long n_stage,
                                                              const float* __restrict__ tab, int L, int M, int H, int T,
                                                              int16_t* __restrict__ out, long long k0, long long n_k,
                                                              long long out_stride) {
#pragma clang fp contract(off)
  constexpr int SB = FMT == AUDIO_U8 ? 1 : FMT == AUDIO_I16 ? 2 : FMT == AUDIO_I24 ? 3 : 4;
  __shared__ float mono[AC_MAX_SPAN];
  __shared__ __attribute__((aligned(16))) uint8_t stage[AC_RAW_TILE + 32];

  const int tid = threadIdx.x;
  [[maybe_unused]] const int ch = SPLIT ? (int)blockIdx.y : 0;   // < C by the grid size
  const long long kb = (long long)blockIdx.x * AC_WG_OUT;            // first output of this workgroup, from k0
  const int nk = (int)(n_k - kb < AC_WG_OUT ? n_k - kb : AC_WG_OUT);   // >= 1 by the grid size
  const long long k_first = k0 + kb, k_last = k_first + nk - 1;
  // frames [jlo, jhi] feed these outputs (T == 0, the 16 kHz path: L = M = 1, H = 1, frame k alone)
  const long long jlo = k_first * M / L - H + 1, jhi = k_last * M / L + H - (T == 0 ? 1 : 0);
  const int span = (int)(jhi - jlo + 1);                             // <= AC_MAX_SPAN (checked by the launcher)
  const long long a = jlo > frame0 ? jlo : frame0;                   // staged frames of the span: [a, b)
  const long long b = jhi + 1 < frame0 + n_stage ? jhi + 1 : frame0 + n_stage;
  for (int i = tid; i < span; i += AC_THREADS) {
    const long long j = jlo + i;
    if (j < a || j >= b) mono[i] = 0.0f;
  }

  const int FB = C * SB;                 // bytes per frame
  const int TF = AC_RAW_TILE / FB;       // frames per staged tile
  for (long long f = a; f < b; f += TF) {
    const int nf = (int)(b - f < TF ? b - f : TF);
    const long long byte0 = (f - frame0) * FB, al0 = byte0 & ~15LL;
    const int off = (int)(byte0 - al0);
    const int n16 = (off + nf * FB + 15) / 16;   // <= (15 + AC_RAW_TILE + 15) / 16: inside stage[]
    for (int i = tid; i < n16; i += AC_THREADS) ((uint4*)stage)[i] = ((const uint4*)(raw + al0))[i];
    __syncthreads();
    for (int i = tid; i < nf; i += AC_THREADS) {
      const uint8_t* fr = stage + off + i * FB;   // 2- / 4-byte aligned for 2- / 4-byte samples
      auto sample = [&](int c) {
        uint32_t bits;
        if constexpr (SB == 1) bits = fr[c];
        else if constexpr (SB == 2) bits = ((const uint16_t*)fr)[c];
        else if constexpr (SB == 3) bits = (uint32_t)fr[3 * c] | (uint32_t)fr[3 * c + 1] << 8 | (uint32_t)fr[3 * c + 2] << 16;
        else bits = ((const uint32_t*)fr)[c];
        return audio_sample_f32(FMT, bits);
      };
      if constexpr (SPLIT) {
        mono[(int)(f - jlo) + i] = sample(ch);   // the mono definition's C == 1 branch: no invC
      } else {
        float sum = 0.0f;
        for (int c = 0; c < C; ++c) {
          const float x = sample(c);
          sum = c == 0 ? x : sum + x;
        }
        mono[(int)(f - jlo) + i] = C == 1 ? sum : sum * invC;
      }
    }
    __syncthreads();
  }
  __syncthreads();   // the zero fill, when no tile ran

  if (tid < nk) {
    const long long k = k_first + tid;
    float acc;
    if (T == 0) {
      acc = mono[tid];
    } else {
      const long long km = k * M;
      const int base = (int)(km / L - H + 1 - jlo);       // >= 0, base + T <= span
      const float* row = tab + (km % L) * T;
      acc = 0.0f;
      for (int i = 0; i < T; ++i) acc = __builtin_fmaf(mono[base + i], row[i], acc);
    }
    out[(SPLIT ? (long long)ch * out_stride : 0) + (k - k0)] = audio_quantize(acc);
  }
}

// split: C planes of out_stride samples, grid.y = C; else one plane
static void audio_launch(bool split, const void* raw, int fmt, int C, float invC, long long frame0, long long n_stage,
                         const float* tab, int L, int M, int H, int T, int16_t* out, long long out_stride, long long k0,
                         long long n_k, hipStream_t s) {
  WDR_CHECK(fmt >= 0 && fmt <= 4, "audio: sample format must be 0 (u8), 1 (i16), 2 (i24), 3 (i32) or 4 (f32)");
  WDR_CHECK(C >= 1 && C <= AUDIO_MAX_CHANNELS, "audio: 1 to 8 channels");
  WDR_CHECK(((uintptr_t)raw & 15) == 0, "audio: the staging buffer must be 16-byte aligned");
  WDR_CHECK(L >= 1 && M >= 1 && H >= 1 && (T == 0 ? (L == 1 && M == 1 && H == 1 && !tab) : (T == 2 * H && tab)),
            "audio: inconsistent resampling table");
  WDR_CHECK((long long)(AC_WG_OUT - 1) * M / L + 1 + 2 * H <= AC_MAX_SPAN, "audio: input span exceeds the workgroup's LDS");
  WDR_CHECK(frame0 >= 0 && n_stage >= 0 && k0 >= 0, "audio: negative index");
  // plane c holds out[c * out_stride .. c * out_stride + n_k): the planes must not overlap
  WDR_CHECK(!split || (out_stride >= 0 && out_stride >= n_k), "audio: channel stride shorter than the outputs of a launch");
  if (n_k <= 0) return;
  const long long wgs = (n_k + AC_WG_OUT - 1) / AC_WG_OUT;
  WDR_CHECK(wgs <= 0x7fffffffLL, "audio: too many outputs in one launch");
  const dim3 grid((unsigned)wgs, split ? (unsigned)C : 1u), block(AC_THREADS);
  const uint8_t* src = (const uint8_t*)raw;
#define WDR_AC_LAUNCH(F)                                                                                             \
  do {                                                                                                               \
    if (split)                                                                                                       \
      WDR_KLAUNCH((k_audio_convert<F, true>), grid, block, 0, s, src, C, invC, frame0, n_stage, tab, L, M, H, T, out, \
                  k0, n_k, out_stride);                                                                              \
    else                                                                                                             \
      WDR_KLAUNCH((k_audio_convert<F, false>), grid, block, 0, s, src, C, invC, frame0, n_stage, tab, L, M, H, T,    \
                  out, k0, n_k, 0LL);                                                                                \
  } while (0)
  switch (fmt) {
    case AUDIO_U8: WDR_AC_LAUNCH(AUDIO_U8); break;
    case AUDIO_I16: WDR_AC_LAUNCH(AUDIO_I16); break;
    case AUDIO_I24: WDR_AC_LAUNCH(AUDIO_I24); break;
    case AUDIO_I32: WDR_AC_LAUNCH(AUDIO_I32); break;
    default: WDR_AC_LAUNCH(AUDIO_F32); break;
  }
#undef WDR_AC_LAUNCH
  WDR_HIP(hipGetLastError());
}

void launch_audio_convert(const void* raw, int fmt, int C, float invC, long long frame0, long long n_stage,
                          const float* tab, int L, int M, int H, int T, int16_t* out, long long k0, long long n_k,
                          hipStream_t s) {
  audio_launch(false, raw, fmt, C, invC, frame0, n_stage, tab, L, M, H, T, out, 0, k0, n_k, s);
}

void launch_audio_split(const void* raw, int fmt, int C, long long frame0, long long n_stage, const float* tab, int L,
                        int M, int H, int T, int16_t* out, long long out_stride, long long k0, long long n_k,
                        hipStream_t s) {
  audio_launch(true, raw, fmt, C, 1.0f, frame0, n_stage, tab, L, M, H, T, out, out_stride, k0, n_k, s);
}

}  // namespace wdr
