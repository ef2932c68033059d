// Audio ingest, host side: the WAV parser, the resampling table and the host definition of the
// conversion to 16 kHz mono int16 (audio_file.h).  No HIP dependency.
#include "audio_file.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>

namespace wdr {

bool MemSource::read(uint64_t off, void* dst, size_t len) const {
  if (off > n || len > n - off) return false;
  if (len) memcpy(dst, p + off, len);
  return true;
}

namespace {

struct FileSource : ByteSource {
  FILE* f = nullptr;
  uint64_t n = 0;
  explicit FileSource(const char* path) {
    f = path ? fopen(path, "rb") : nullptr;
    if (!f) throw std::runtime_error("failed to read file");
    if (fseeko(f, 0, SEEK_END) != 0) { fclose(f); throw std::runtime_error("failed to read file"); }
    const off_t e = ftello(f);
    n = e < 0 ? 0 : (uint64_t)e;
  }
  ~FileSource() override { if (f) fclose(f); }
  FileSource(const FileSource&) = delete;
  FileSource& operator=(const FileSource&) = delete;
  uint64_t size() const override { return n; }
  bool read(uint64_t off, void* dst, size_t len) const override {
    if (off > n || len > n - off) return false;
    if (!len) return true;
    if (fseeko(f, (off_t)off, SEEK_SET) != 0) return false;
    return fread(dst, 1, len, f) == len;
  }
};

uint16_t le16(const uint8_t* p) { return (uint16_t)(p[0] | p[1] << 8); }
uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

[[noreturn]] void bad(const std::string& m) { throw std::runtime_error(m); }

// [pos, end of the source) is empty or a run of whole chunks with printable ids (the pad byte of
// the last one may be missing)
bool chunks_to_end(const ByteSource& src, uint64_t pos) {
  const uint64_t size = src.size();
  while (pos < size) {
    uint8_t ck[8];
    if (size - pos < 8 || !src.read(pos, ck, 8)) return false;
    for (int i = 0; i < 4; ++i)
      if (ck[i] < 0x20 || ck[i] > 0x7E) return false;
    const uint64_t sz = le32(ck + 4);
    if (sz > size - pos - 8) return false;
    pos += 8 + sz;
    if ((sz & 1) && pos < size) ++pos;
  }
  return true;
}

}  // namespace

AudioInfo audio_parse(const ByteSource& src) {
  const uint64_t size = src.size();
  uint8_t hd[12];
  if (!src.read(0, hd, 12)) bad("not a RIFF/WAVE file");
  if (!memcmp(hd, "RF64", 4) || !memcmp(hd, "BW64", 4)) bad("RF64 files are not supported");
  if (memcmp(hd, "RIFF", 4) || memcmp(hd + 8, "WAVE", 4)) bad("not a RIFF/WAVE file");
  bool have_fmt = false, have_data = false;
  uint32_t tag = 0, ch = 0, rate = 0, align = 0, bits = 0;
  uint64_t dpos = 0, dlen = 0;
  uint64_t pos = 12;
  while (!(have_fmt && have_data) && pos <= size && size - pos >= 8) {
    uint8_t ck[8];
    if (!src.read(pos, ck, 8)) break;
    const uint32_t sz = le32(ck + 4);
    if (!memcmp(ck, "fmt ", 4) && !have_fmt) {
      if (sz < 16) bad("fmt chunk too short (" + std::to_string(sz) + " bytes)");
      uint8_t f[26];
      if (!src.read(pos + 8, f, 16)) bad("fmt chunk truncated");
      tag = le16(f); ch = le16(f + 2); rate = le32(f + 4); align = le16(f + 12); bits = le16(f + 14);
      if (tag == 0xFFFE) {   // WAVE_FORMAT_EXTENSIBLE: the tag is the head of the SubFormat GUID
        if (sz < 26) bad("extensible fmt chunk too short (" + std::to_string(sz) + " bytes)");
        if (!src.read(pos + 8, f, 26)) bad("fmt chunk truncated");
        tag = le16(f + 24);
      }
      have_fmt = true;
    } else if (!memcmp(ck, "data", 4) && !have_data) {
      dpos = pos + 8;
      const uint64_t avail = size - dpos;
      // 0 / 0xFFFFFFFF: a writer that could not seek back (piped output) -- to the end of the file.
      // A size of 0 is taken at its word only where the rest of the file is a run of whole chunks
      // (an empty data chunk in front of LIST and the like), which samples never are
      const bool to_end = sz == 0xFFFFFFFFu || (sz == 0 && !chunks_to_end(src, dpos));
      dlen = to_end ? avail : (sz < avail ? sz : avail);
      have_data = true;
      if (to_end) break;
    }
    pos += 8 + (uint64_t)sz + (sz & 1);   // chunks are padded to an even size
  }
  if (!have_fmt) bad("no fmt chunk");
  switch (tag) {
    case 1: case 3: break;
    case 2: case 0x11: bad("ADPCM audio is not supported (format tag " + std::to_string(tag) + ")");
    case 6: bad("A-law audio is not supported (format tag 6)");
    case 7: bad("mu-law audio is not supported (format tag 7)");
    default: bad("unsupported WAV format tag " + std::to_string(tag));
  }
  if (ch < 1 || ch > (uint32_t)AUDIO_MAX_CHANNELS) bad("unsupported channel count " + std::to_string(ch) + " (1 to 8)");
  if (rate < (uint32_t)AUDIO_MIN_RATE || rate > (uint32_t)AUDIO_MAX_RATE)
    bad("unsupported sample rate " + std::to_string(rate) + " Hz (1000 to 384000)");
  if (tag == 3 && bits == 64) bad("64-bit float samples are not supported");
  if (tag == 3 && bits != 32) bad("float samples must be 32-bit, found " + std::to_string(bits) + " bits per sample");
  if (bits != 8 && bits != 16 && bits != 24 && bits != 32)
    bad("unsupported bits per sample: " + std::to_string(bits) + " (8, 16, 24 or 32)");
  if (align != ch * bits / 8)
    bad("block align " + std::to_string(align) + " does not match " + std::to_string(ch) + " channels of " +
        std::to_string(bits) + " bits");
  if (!have_data) bad("no data chunk");
  AudioInfo a;
  a.fmt = tag == 3 ? AUDIO_F32 : bits == 8 ? AUDIO_U8 : bits == 16 ? AUDIO_I16 : bits == 24 ? AUDIO_I24 : AUDIO_I32;
  a.channels = (int)ch;
  a.rate = (int)rate;
  a.bits = (int)bits;
  a.block_align = (int)align;
  a.data_off = dpos;
  a.n_frames = dlen / align;
  return a;
}

AudioInfo audio_parse(const char* path) { return audio_parse(FileSource(path)); }

void audio_read_bytes(const char* path, uint64_t off, void* dst, size_t n) {
  const FileSource f(path);
  if (!f.read(off, dst, n)) throw std::runtime_error("failed to read file");
}

// ------------------------------------------------------------------ the resampling filter
static uint64_t gcd_u64(uint64_t a, uint64_t b) {
  while (b) { const uint64_t t = a % b; a = b; b = t; }
  return a;
}

void resample_dims(int rate, int* L, int* M, int* H) {
  if (rate < AUDIO_MIN_RATE || rate > AUDIO_MAX_RATE)
    throw std::runtime_error("unsupported sample rate " + std::to_string(rate) + " Hz (1000 to 384000)");
  const int g = (int)gcd_u64(AUDIO_OUT_RATE, (uint64_t)rate);
  *L = AUDIO_OUT_RATE / g;
  *M = rate / g;
  // H = ceil(W), W = 32 / min(1, L / M): 32 zero crossings a side at the narrower of the two rates
  *H = *M > *L ? (32 * *M + *L - 1) / *L : 32;
}

// modified Bessel function I0 by its power series (x <= 9 here: converges in ~30 terms)
static double bessel_i0(double x) {
  const double q = x * x / 4.0;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < sum * 1e-18) break;
  }
  return sum;
}

ResampleTable resample_table(int rate) {
  // the last table is kept: a rate such as 47999 Hz has 16000 phases of 192 taps (3 M Bessel
  // series), and callers convert many inputs of one rate in a row
  ResampleTable t;
  resample_dims(rate, &t.L, &t.M, &t.H);   // rejects a bad rate before anything else
  static std::mutex mu;
  static int last_rate = -1;               // no valid rate: nothing cached yet
  static ResampleTable last;
  std::lock_guard<std::mutex> lock(mu);
  if (rate == last_rate) return last;
  if (rate == AUDIO_OUT_RATE) { t.H = 0; return t; }
  const int L = t.L, M = t.M, H = t.H;
  t.T = 2 * H;
  const double s = M > L ? (double)L / (double)M : 1.0;
  const double W = M > L ? 32.0 * (double)M / (double)L : 32.0;
  const double cut = 0.94 * s, beta = 9.0, pi = 3.14159265358979323846;
  const double i0b = bessel_i0(beta);
  t.tab.resize((size_t)L * t.T);
  for (int p = 0; p < L; ++p)
    for (int i = 0; i < t.T; ++i) {
      const double x = (double)p / (double)L - (double)(i - H + 1);
      double g = 0.0;
      if (std::fabs(x) < W) {
        const double u = cut * x, r = x / W;
        const double sinc = u == 0.0 ? 1.0 : std::sin(pi * u) / (pi * u);
        g = cut * sinc * bessel_i0(beta * std::sqrt(1.0 - r * r)) / i0b;
      }
      t.tab[(size_t)p * t.T + i] = (float)g;
    }
  last = t;
  last_rate = rate;
  return t;
}

// ------------------------------------------------------------------ the host definition
// Every f32 step is written out: the one fused operation is the explicit fmaf of the tap loop,
// and contraction is off so that no multiply and add elsewhere become one rounding.
std::vector<int16_t> audio_convert_host(const uint8_t* raw, uint64_t n_frames, int fmt, int channels, int rate) {
#pragma clang fp contract(off)
  if (fmt < 0 || fmt > 4) throw std::runtime_error("audio: sample format must be 0 (u8), 1 (i16), 2 (i24), 3 (i32) or 4 (f32)");
  if (channels < 1 || channels > AUDIO_MAX_CHANNELS) throw std::runtime_error("unsupported channel count " + std::to_string(channels) + " (1 to 8)");
  const ResampleTable t = resample_table(rate);
  const int sb = audio_sample_bytes(fmt);
  const float invC = 1.0f / (float)channels;
  std::vector<float> m(n_frames);
  for (uint64_t j = 0; j < n_frames; ++j) {
    const uint8_t* fr = raw + j * (uint64_t)(sb * channels);
    float sum = 0.0f;
    for (int c = 0; c < channels; ++c) {
      uint32_t bits = 0;
      for (int b = 0; b < sb; ++b) bits |= (uint32_t)fr[c * sb + b] << (8 * b);
      const float x = audio_sample_f32(fmt, bits);
      sum = c == 0 ? x : sum + x;
    }
    m[j] = channels == 1 ? sum : sum * invC;
  }
  const uint64_t n_out = audio_n_out(n_frames, t.L, t.M);
  std::vector<int16_t> out(n_out);
  if (t.T == 0) {
    for (uint64_t k = 0; k < n_out; ++k) out[k] = audio_quantize(m[k]);
    return out;
  }
  for (uint64_t k = 0; k < n_out; ++k) {
    const uint64_t km = k * (uint64_t)t.M;
    const int64_t j0 = (int64_t)(km / (uint64_t)t.L);
    const float* row = &t.tab[(size_t)(km % (uint64_t)t.L) * t.T];
    float acc = 0.0f;
    for (int i = 0; i < t.T; ++i) {
      const int64_t j = j0 - t.H + 1 + i;
      const float x = j >= 0 && (uint64_t)j < n_frames ? m[(size_t)j] : 0.0f;
      acc = __builtin_fmaf(x, row[i], acc);
    }
    out[k] = audio_quantize(acc);
  }
  return out;
}

// Channel c of the split is, by definition, audio_convert_host of the mono stream made of sample
// c of every frame: nothing is computed here that the mono definition does not compute.
std::vector<int16_t> audio_split_host(const uint8_t* raw, uint64_t n_frames, int fmt, int channels, int rate) {
  if (fmt < 0 || fmt > 4) throw std::runtime_error("audio: sample format must be 0 (u8), 1 (i16), 2 (i24), 3 (i32) or 4 (f32)");
  if (channels < 1 || channels > AUDIO_MAX_CHANNELS) throw std::runtime_error("unsupported channel count " + std::to_string(channels) + " (1 to 8)");
  int L, M, H;
  resample_dims(rate, &L, &M, &H);   // rejects a bad rate
  const size_t sb = (size_t)audio_sample_bytes(fmt);
  const uint64_t n_out = audio_n_out(n_frames, L, M);
  std::vector<int16_t> out((size_t)channels * n_out);
  std::vector<uint8_t> one((size_t)n_frames * sb);
  for (int c = 0; c < channels; ++c) {
    for (uint64_t j = 0; j < n_frames; ++j) memcpy(&one[j * sb], raw + (j * (uint64_t)channels + (uint64_t)c) * sb, sb);
    const std::vector<int16_t> ch = audio_convert_host(one.data(), n_frames, fmt, 1, rate);
    if (n_out) memcpy(&out[(size_t)c * n_out], ch.data(), (size_t)n_out * 2);
  }
  return out;
}

}  // namespace wdr
