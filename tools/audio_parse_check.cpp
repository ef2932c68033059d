// Stand-alone check of the WAV parser (csrc/audio_file.cpp) on truncated and corrupted headers,
// meant to be built with -fsanitize=address,undefined (make -C whisper-diarize-rs_amd
// audio-parse-check).  Host code only: no HIP, no GPU.
//
// Cases: every prefix of a valid 60-byte file (plain and data-before-fmt layouts) and of an
// extensible-header file; every header field (chunk sizes, tag, channels, rate, block align,
// bits) set to each of a list of corrupt values, alone and in pairs; every single byte of the
// header set to 0x00 / 0xFF / flipped.  Each case is parsed from memory (a buffer allocated at
// the exact size, so that a read past it is caught) and must return or throw std::runtime_error;
// an accepted header must describe frames that lie inside the buffer.  A few cases also go
// through the file reader.  The host definition is run on a small input per format as well.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../whisper-diarize-rs_amd/csrc/audio_file.h"

using namespace wdr;

static long g_cases = 0, g_ok = 0, g_rejected = 0;

static void put16(std::vector<uint8_t>& v, size_t o, uint32_t x) { v[o] = x & 255; v[o + 1] = x >> 8 & 255; }
static void put32(std::vector<uint8_t>& v, size_t o, uint32_t x) { put16(v, o, x & 0xFFFF); put16(v, o + 2, x >> 16); }

static std::vector<uint8_t> chunk(const char* id, const std::vector<uint8_t>& body) {
  std::vector<uint8_t> c(8 + body.size() + (body.size() & 1), 0);
  memcpy(c.data(), id, 4);
  put32(c, 4, (uint32_t)body.size());
  if (!body.empty()) memcpy(c.data() + 8, body.data(), body.size());
  return c;
}

static std::vector<uint8_t> fmt_body(int tag, int ch, int rate, int bits, bool ext) {
  std::vector<uint8_t> f(ext ? 40 : 16, 0);
  put16(f, 0, ext ? 0xFFFE : tag); put16(f, 2, ch); put32(f, 4, rate); put32(f, 8, rate * ch * bits / 8);
  put16(f, 12, ch * bits / 8); put16(f, 14, bits);
  if (ext) {
    put16(f, 16, 22); put16(f, 18, bits); put32(f, 20, 0); put16(f, 24, tag);
    const uint8_t tail[14] = {0, 0, 0, 0, 0x10, 0, 0x80, 0, 0, 0xAA, 0, 0x38, 0x9B, 0x71};
    memcpy(f.data() + 26, tail, 14);
  }
  return f;
}

static std::vector<uint8_t> riff(const std::vector<std::vector<uint8_t>>& chunks) {
  std::vector<uint8_t> v(12, 0);
  memcpy(v.data(), "RIFF", 4);
  memcpy(v.data() + 8, "WAVE", 4);
  for (auto& c : chunks) v.insert(v.end(), c.begin(), c.end());
  put32(v, 4, (uint32_t)v.size() - 8);
  return v;
}

// parse n bytes held in an allocation of exactly n bytes
static void parse_case(const uint8_t* p, size_t n) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[n ? n : 1]);
  if (n) memcpy(buf.get(), p, n);
  ++g_cases;
  try {
    const AudioInfo a = audio_parse(MemSource(buf.get(), n));
    if (a.block_align <= 0 || a.data_off > n || a.n_frames > (n - a.data_off) / (uint64_t)a.block_align) {
      fprintf(stderr, "accepted header describes frames outside the file (%zu bytes)\n", n);
      exit(1);
    }
    // touch every frame the header claims
    unsigned sum = 0;
    for (uint64_t i = 0; i < a.n_frames * (uint64_t)a.block_align; ++i) sum += buf[a.data_off + i];
    static volatile unsigned sink;
    sink = sum;
    (void)sink;
    ++g_ok;
  } catch (const std::runtime_error&) {
    ++g_rejected;
  }
}

static void mutate(const std::vector<uint8_t>& base, size_t hdr_bytes) {
  for (size_t n = 0; n <= base.size(); ++n) parse_case(base.data(), n);
  for (size_t o = 0; o < hdr_bytes; ++o)
    for (int m = 0; m < 3; ++m) {
      std::vector<uint8_t> v = base;
      v[o] = m == 0 ? 0x00 : m == 1 ? 0xFF : (uint8_t)~v[o];
      parse_case(v.data(), v.size());
    }
}

int main() {
  std::vector<uint8_t> pcm(16);
  for (size_t i = 0; i < pcm.size(); ++i) pcm[i] = (uint8_t)(i * 37 + 1);
  const std::vector<uint8_t> plain = riff({chunk("fmt ", fmt_body(1, 1, 16000, 16, false)), chunk("data", pcm)});
  const std::vector<uint8_t> swapped = riff({chunk("data", pcm), chunk("fmt ", fmt_body(1, 1, 16000, 16, false))});
  const std::vector<uint8_t> ext = riff({chunk("fmt ", fmt_body(3, 2, 48000, 32, true)),
                                         chunk("LIST", std::vector<uint8_t>(7, 'x')), chunk("data", pcm)});
  if (plain.size() != 60 || swapped.size() != 60) { fprintf(stderr, "the valid file is not 60 bytes\n"); return 1; }
  mutate(plain, 44);
  mutate(swapped, 60);
  mutate(ext, ext.size() - 16);

  // corrupt values per header field of the plain file, alone and in pairs
  const uint32_t bad32[] = {0, 1, 2, 7, 8, 15, 16, 17, 40, 0x7FFFFFFF, 0x80000000u, 0xFFFFFFF0u, 0xFFFFFFFEu, 0xFFFFFFFFu, 999, 384001};
  const uint32_t bad16[] = {0, 1, 2, 3, 6, 7, 8, 9, 12, 16, 17, 24, 32, 64, 0x11, 0x55, 0x7FFF, 0x8000, 0xFFFE, 0xFFFF};
  struct Field { size_t off; int width; };
  const Field fields[] = {{4, 4}, {16, 4}, {20, 2}, {22, 2}, {24, 4}, {28, 4}, {32, 2}, {34, 2}, {40, 4}};
  const int nf = (int)(sizeof(fields) / sizeof(fields[0]));
  auto set = [](std::vector<uint8_t>& v, const Field& f, uint32_t x) { f.width == 4 ? put32(v, f.off, x) : put16(v, f.off, x); };
  for (int a = 0; a < nf; ++a) {
    const uint32_t* va = fields[a].width == 4 ? bad32 : bad16;
    const int na = fields[a].width == 4 ? (int)(sizeof(bad32) / 4) : (int)(sizeof(bad16) / 4);
    for (int i = 0; i < na; ++i) {
      std::vector<uint8_t> v = plain;
      set(v, fields[a], va[i]);
      parse_case(v.data(), v.size());
      for (int b = a + 1; b < nf; ++b) {
        const uint32_t* vb = fields[b].width == 4 ? bad32 : bad16;
        const int nb = fields[b].width == 4 ? (int)(sizeof(bad32) / 4) : (int)(sizeof(bad16) / 4);
        for (int j = 0; j < nb; ++j) {
          std::vector<uint8_t> w = v;
          set(w, fields[b], vb[j]);
          parse_case(w.data(), w.size());
        }
      }
    }
  }
  // the extensible header's own fields: fmt chunk size, cbSize, SubFormat tag
  for (uint32_t x : bad32) { std::vector<uint8_t> v = ext; put32(v, 16, x); parse_case(v.data(), v.size()); }
  for (uint32_t x : bad16) { std::vector<uint8_t> v = ext; put16(v, 44, x); parse_case(v.data(), v.size()); }

  // the file reader: a valid file, a truncated one and a missing one
  const char* dir = getenv("TMPDIR");
  const std::string path = std::string(dir ? dir : "/tmp") + "/wdr_audio_parse_check.wav";
  for (size_t n : {plain.size(), (size_t)50, (size_t)30, (size_t)0}) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
    fwrite(plain.data(), 1, n, f);
    fclose(f);
    ++g_cases;
    try {
      const AudioInfo a = audio_parse(path.c_str());
      std::vector<uint8_t> d((size_t)a.n_frames * a.block_align + 1);
      audio_read_bytes(path.c_str(), a.data_off, d.data(), d.size() - 1);
      ++g_ok;
    } catch (const std::runtime_error&) { ++g_rejected; }
  }
  remove(path.c_str());
  try { audio_parse("/nonexistent/wdr.wav"); return 1; } catch (const std::runtime_error&) {}

  // the host definition on a few frames of every format (its indexing under the sanitizer too)
  for (int fmt = 0; fmt <= 4; ++fmt)
    for (int rate : {16000, 48000, 44100, 8000}) {
      const int ch = 1 + fmt % 3, n = 300;
      std::vector<uint8_t> raw((size_t)n * ch * audio_sample_bytes(fmt));
      for (size_t i = 0; i < raw.size(); ++i) raw[i] = (uint8_t)(i * 131 + fmt);
      const std::vector<int16_t> o = audio_convert_host(raw.data(), n, fmt, ch, rate);
      const ResampleTable t = resample_table(rate);
      if (o.size() != audio_n_out(n, t.L, t.M)) { fprintf(stderr, "wrong output length\n"); return 1; }
    }
  printf("audio_parse_check: %ld cases, %ld accepted, %ld rejected, no sanitizer report\n", g_cases, g_ok, g_rejected);
  return 0;
}
