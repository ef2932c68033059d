// Audio ingest, host side (no HIP dependency: this header and audio_file.cpp compile alone).
//
//  audio_parse         a general RIFF/WAVE header walk: PCM 8/16/24/32-bit and IEEE f32, 1..8
//                      channels, 1000..384000 Hz, plain or WAVE_FORMAT_EXTENSIBLE headers
//  resample_table      the polyphase Kaiser-windowed-sinc table of a source rate
//  audio_convert_host  the host definition of the conversion to 16 kHz mono int16: the meaning
//                      of the feature, which the kernels (kernels/audio.hip) equal bit for bit.
//                      Single-threaded; tests and documentation only, never a product fallback.
//  audio_split_host    the same per channel, no downmix: the mono definition
//                      applied to each channel's samples
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define WDR_AUDIO_HD __host__ __device__
#else
#define WDR_AUDIO_HD
#endif

namespace wdr {

enum AudioFmt : int { AUDIO_U8 = 0, AUDIO_I16 = 1, AUDIO_I24 = 2, AUDIO_I32 = 3, AUDIO_F32 = 4 };
constexpr int AUDIO_OUT_RATE = 16000;
constexpr int AUDIO_MAX_CHANNELS = 8, AUDIO_MIN_RATE = 1000, AUDIO_MAX_RATE = 384000;

inline int audio_sample_bytes(int fmt) { return fmt == AUDIO_U8 ? 1 : fmt == AUDIO_I16 ? 2 : fmt == AUDIO_I24 ? 3 : 4; }

struct AudioInfo {
  int fmt = 0, channels = 0, rate = 0, bits = 0, block_align = 0;
  uint64_t data_off = 0;    // byte offset of the first frame in the file
  uint64_t n_frames = 0;    // whole frames (a trailing partial frame is dropped)
};

// the bytes the parser may look at: it asks for every range it reads, and a range that is not
// wholly inside the source is refused, so no header field can make it read out of bounds
struct ByteSource {
  virtual ~ByteSource() {}
  virtual uint64_t size() const = 0;
  virtual bool read(uint64_t off, void* dst, size_t n) const = 0;   // false: not n bytes at off
};
struct MemSource : ByteSource {
  const uint8_t* p;
  size_t n;
  MemSource(const uint8_t* p_, size_t n_) : p(p_), n(n_) {}
  uint64_t size() const override { return n; }
  bool read(uint64_t off, void* dst, size_t len) const override;
};

// throws std::runtime_error with a message that names the problem
AudioInfo audio_parse(const ByteSource& src);
AudioInfo audio_parse(const char* path);
// n bytes of the file at off into dst (throws when the file is shorter)
void audio_read_bytes(const char* path, uint64_t off, void* dst, size_t n);

// L = 16000 / g, M = rate / g (g = gcd), H = taps per side, T = 2 H; tab[p * T + i] is the
// coefficient of tap i (input frame floor(k M / L) - H + 1 + i) for phase p = (k M) mod L,
// evaluated in double and rounded once to f32.  rate == 16000: L = M = 1, T = 0, no table.
struct ResampleTable {
  int L = 1, M = 1, H = 0, T = 0;
  std::vector<float> tab;
};
void resample_dims(int rate, int* L, int* M, int* H);
ResampleTable resample_table(int rate);
inline uint64_t audio_n_out(uint64_t n_in, int L, int M) { return (n_in * (uint64_t)L + (uint64_t)M - 1) / (uint64_t)M; }

// one sample's little-endian bits (zero-extended to 32) -> f32; every scale is a power of two
WDR_AUDIO_HD inline float audio_sample_f32(int fmt, uint32_t bits) {
#pragma clang fp contract(off)
  switch (fmt) {
    case AUDIO_U8: return (float)((int)bits - 128) * 0.0078125f;
    case AUDIO_I16: return (float)(int)(int16_t)bits * 0.000030517578125f;
    case AUDIO_I24: return (float)((int)(bits << 8) >> 8) * 1.1920928955078125e-07f;
    case AUDIO_I32: return (float)(int)bits * 4.656612873077392578125e-10f;   // int -> f32 rounds to nearest even
    default: {
      const float s = __builtin_bit_cast(float, bits);
      return s != s ? 0.0f : s < -1.0f ? -1.0f : s > 1.0f ? 1.0f : s;
    }
  }
}
// f32 -> int16: scale (exact), clamp, round to nearest even
WDR_AUDIO_HD inline int16_t audio_quantize(float acc) {
#pragma clang fp contract(off)
  float v = acc * 32768.0f;
  v = v < -32768.0f ? -32768.0f : v > 32767.0f ? 32767.0f : v;
  return (int16_t)__builtin_rintf(v);
}

// raw: n_frames interleaved frames of `channels` samples of format fmt
std::vector<int16_t> audio_convert_host(const uint8_t* raw, uint64_t n_frames, int fmt, int channels, int rate);
// one channel per speaker: planar [channels][n_out] int16, channel c being
// audio_convert_host of the mono stream made of sample c of every frame (no downmix, no invC)
std::vector<int16_t> audio_split_host(const uint8_t* raw, uint64_t n_frames, int fmt, int channels, int rate);

}  // namespace wdr
