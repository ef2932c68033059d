// Audio ingest, device side (audio_gpu.h).
//
// Chunking.  The input is cut into chunks of chunk_frames frames.  Output k belongs to the one
// chunk [a, b) that holds its centre frame floor(k M / L), i.e. k in [ceil(a L / M), ceil(b L / M)),
// and its taps reach frames a - H + 1 .. b - 1 + H, so a chunk is staged with a halo of H frames a
// side (clipped to the file: frames outside it are zero by definition).  Every output is computed
// by the same instruction sequence from the same values whatever the chunk size, so chunk seams
// cannot show.  Two slots of pinned + device staging alternate: chunk i is filled and copied on
// the copy stream while chunk i - 1 converts on the compute stream.
#include "audio_gpu.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>

#include "kernels/kernels.h"
#include "prof.h"

namespace wdr {

namespace {

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// makes `dev` current and restores the caller's device on scope exit
struct DeviceScope {
  int prev = -1;
  explicit DeviceScope(int dev) {
    int cur = -1;
    WDR_HIP(hipGetDevice(&cur));
    if (cur != dev) {
      WDR_HIP(hipSetDevice(dev));
      prev = cur;
    }
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

size_t up16(size_t n) { return (n + 15) & ~size_t(15); }

constexpr size_t kChunkBytes = size_t(32) << 20;      // default raw bytes per chunk
constexpr uint64_t kChunkOutputs = uint64_t(16) << 20;   // and at most this many outputs (upsampling)
constexpr size_t kMaxTables = 4;                       // cached rates (12 MB at 47,999 Hz; 98 MB at worst, 383,999 Hz)

}  // namespace

AudioConverter::AudioConverter(int device) : dev_(device) {
  DeviceScope ds(dev_);
  WDR_HIP(hipStreamCreateWithFlags(&s_copy_, hipStreamNonBlocking));
  stream_note("audio_copy", s_copy_);
  WDR_HIP(hipStreamCreateWithFlags(&s_comp_, hipStreamNonBlocking));
  stream_note("audio", s_comp_);
  for (int i = 0; i < 2; ++i) {
    WDR_HIP(hipEventCreateWithFlags(&ev_copied_[i], hipEventDisableTiming));
    WDR_HIP(hipEventCreateWithFlags(&ev_done_[i], hipEventDisableTiming));
  }
}

void AudioConverter::release_pinned() {
  std::lock_guard<std::recursive_mutex> g(hip_alloc_mutex());
  for (int i = 0; i < 2; ++i) {
    if (h_in_[i]) (void)hipHostFree(h_in_[i]);
    if (h_out_[i]) (void)hipHostFree(h_out_[i]);
    h_in_[i] = nullptr;
    h_out_[i] = nullptr;
  }
}

AudioConverter::~AudioConverter() {
  int cur = -1;
  const bool ok = hipGetDevice(&cur) == hipSuccess && hipSetDevice(dev_) == hipSuccess;
  if (s_copy_) (void)hipStreamSynchronize(s_copy_);
  if (s_comp_) (void)hipStreamSynchronize(s_comp_);
  release_pinned();
  for (int i = 0; i < 2; ++i) {
    if (ev_copied_[i]) (void)hipEventDestroy(ev_copied_[i]);
    if (ev_done_[i]) (void)hipEventDestroy(ev_done_[i]);
    d_in_[i] = DevMem();
    d_out_[i] = DevMem();
  }
  tabs_.clear();
  if (s_copy_) (void)hipStreamDestroy(s_copy_);
  if (s_comp_) (void)hipStreamDestroy(s_comp_);
  if (ok && cur >= 0) (void)hipSetDevice(cur);
}

const AudioConverter::DevTable& AudioConverter::table(int rate) {
  auto it = tabs_.find(rate);
  if (it != tabs_.end()) return it->second;
  const ResampleTable t = resample_table(rate);
  if (tabs_.size() >= kMaxTables) {
    WDR_HIP(hipStreamSynchronize(s_comp_));
    tabs_.clear();
  }
  DevTable d;
  d.L = t.L; d.M = t.M; d.T = t.T;
  d.H = t.T ? t.H : 1;
  if (t.T) {
    d.tab = DevMem(t.tab.size() * 4);
    WDR_HIP(hipMemcpy(d.tab.p, t.tab.data(), t.tab.size() * 4, hipMemcpyHostToDevice));
  }
  return tabs_.emplace(rate, std::move(d)).first->second;
}

// staging for chunks of up to in_bytes raw bytes / out_samples outputs.  The input slots are
// padded to 16 bytes past the chunk: the kernel's aligned loads read that far
void AudioConverter::reserve(size_t in_bytes, size_t out_samples) {
  const size_t need_in = up16(in_bytes) + 16, need_out = std::max<size_t>(out_samples, 1);
  if (need_in <= cap_in_ && need_out <= cap_out_) return;
  WDR_HIP(hipStreamSynchronize(s_copy_));
  WDR_HIP(hipStreamSynchronize(s_comp_));
  const size_t new_in = std::max(cap_in_, need_in), new_out = std::max(cap_out_, need_out);
  // no capacity is claimed while the buffers are gone: a failed allocation leaves the converter
  // empty, and the next call allocates again
  cap_in_ = cap_out_ = 0;
  release_pinned();
  for (int i = 0; i < 2; ++i) {
    d_in_[i] = DevMem();
    d_out_[i] = DevMem();
  }
  for (int i = 0; i < 2; ++i) {
    d_in_[i] = DevMem(new_in);
    d_out_[i] = DevMem(new_out * 2);
    std::lock_guard<std::recursive_mutex> g(hip_alloc_mutex());
    WDR_HIP(hipHostMalloc((void**)&h_in_[i], new_in, hipHostMallocDefault));
    WDR_HIP(hipHostMalloc((void**)&h_out_[i], new_out * 2, hipHostMallocDefault));
    memset(h_in_[i], 0, new_in);
  }
  cap_in_ = new_in;
  cap_out_ = new_out;
}

std::vector<int16_t> AudioConverter::convert(const Fill& fill, uint64_t n_frames, int fmt, int channels, int rate,
                                             uint64_t chunk_frames) {
  return run(fill, n_frames, fmt, channels, rate, chunk_frames, false);
}

std::vector<int16_t> AudioConverter::convert_channels(const Fill& fill, uint64_t n_frames, int fmt, int channels,
                                                      int rate, uint64_t chunk_frames) {
  return run(fill, n_frames, fmt, channels, rate, chunk_frames, true);
}

// split: one output plane per channel (planar [channels][n_out]); else the one downmixed plane.
// A slot's output staging holds a chunk's planes back to back, n outputs each
std::vector<int16_t> AudioConverter::run(const Fill& fill, uint64_t n_frames, int fmt, int channels, int rate,
                                         uint64_t chunk_frames, bool split) {
  WDR_CHECK(fmt >= 0 && fmt <= 4, "audio: sample format must be 0 (u8), 1 (i16), 2 (i24), 3 (i32) or 4 (f32)");
  WDR_CHECK(channels >= 1 && channels <= AUDIO_MAX_CHANNELS,
            "unsupported channel count " + std::to_string(channels) + " (1 to 8)");
  const double t_start = now_s();
  last = Times{};
  DeviceScope ds(dev_);
  const DevTable& tb = table(rate);
  const uint64_t L = tb.L, M = tb.M, H = tb.H;
  const size_t fb = (size_t)channels * audio_sample_bytes(fmt);
  const float invC = 1.0f / (float)channels;
  const uint64_t planes = split ? (uint64_t)channels : 1, n_out = audio_n_out(n_frames, tb.L, tb.M);
  std::vector<int16_t> out((size_t)(planes * n_out));
  if (out.empty()) return out;
  uint64_t cf = chunk_frames;
  if (cf == 0) {
    // the output cap counts every plane, so a slot's output staging is the same for 8 channels as for 1
    cf = std::max<uint64_t>(1, kChunkBytes / fb);
    cf = std::min(cf, std::max<uint64_t>(1, kChunkOutputs / planes * M / L));
  }
  cf = std::min(cf, n_frames);
  reserve((size_t)(cf + 2 * H) * fb, (size_t)(planes * (cf * L / M + 2)));

  last.setup = now_s() - t_start;   // table, staging (pinned allocation the first time)

  struct Pending { bool on = false; uint64_t k = 0, n = 0; } pend[2];
  auto drain = [&](int slot) {
    if (!pend[slot].on) return;
    const double t0 = now_s();
    WDR_HIP(hipEventSynchronize(ev_done_[slot]));
    last.wait += now_s() - t0;
    for (uint64_t c = 0; c < planes; ++c)
      memcpy(out.data() + c * n_out + pend[slot].k, h_out_[slot] + c * pend[slot].n, pend[slot].n * 2);
    pend[slot].on = false;
  };
  try {
    int slot = 0;
    for (uint64_t a = 0; a < n_frames; a += cf) {
      const uint64_t b = std::min(n_frames, a + cf);
      const uint64_t k_lo = (a * L + M - 1) / M, k_hi = (b * L + M - 1) / M;
      if (k_hi == k_lo) continue;   // a chunk shorter than an output period can own no output
      const uint64_t s0 = a > H ? a - H : 0, s1 = std::min(n_frames, b + H);
      const size_t bytes = (size_t)(s1 - s0) * fb;
      drain(slot);   // the slot's previous chunk (two back) has left its buffers
      const double t0 = now_s();
      fill(s0, s1 - s0, h_in_[slot]);
      last.fill += now_s() - t0;
      WDR_HIP(wdr_memcpy_async(d_in_[slot].p, h_in_[slot], up16(bytes), hipMemcpyHostToDevice, s_copy_));
      WDR_HIP(hipEventRecord(ev_copied_[slot], s_copy_));
      WDR_HIP(hipStreamWaitEvent(s_comp_, ev_copied_[slot], 0));
      if (split)
        launch_audio_split(d_in_[slot].p, fmt, channels, (long long)s0, (long long)(s1 - s0), tb.tab.as<float>(), tb.L,
                           tb.M, tb.H, tb.T, d_out_[slot].as<int16_t>(), (long long)(k_hi - k_lo), (long long)k_lo,
                           (long long)(k_hi - k_lo), s_comp_);
      else
        launch_audio_convert(d_in_[slot].p, fmt, channels, invC, (long long)s0, (long long)(s1 - s0),
                             tb.tab.as<float>(), tb.L, tb.M, tb.H, tb.T, d_out_[slot].as<int16_t>(), (long long)k_lo,
                             (long long)(k_hi - k_lo), s_comp_);
      WDR_HIP(wdr_memcpy_async(h_out_[slot], d_out_[slot].p, (size_t)(planes * (k_hi - k_lo)) * 2, hipMemcpyDeviceToHost,
                               s_comp_));
      WDR_HIP(hipEventRecord(ev_done_[slot], s_comp_));
      pend[slot] = {true, k_lo, k_hi - k_lo};
      ++last.chunks;
      slot ^= 1;
    }
    drain(slot);       // the older of the two chunks in flight first
    drain(slot ^ 1);
  } catch (...) {
    // nothing may still be reading or writing the staging when the caller sees the error
    (void)hipStreamSynchronize(s_copy_);
    (void)hipStreamSynchronize(s_comp_);
    throw;
  }
  last.total = now_s() - t_start;
  if (const char* v = env_str("WDR_AUDIO_LOG"))
    if (v[0] == '1')
      fprintf(stderr, "wdr audio: %llu frames in %lld chunks: total %.4f s = setup %.4f + fill %.4f + gpu wait %.4f + rest\n",
              (unsigned long long)n_frames, last.chunks, last.total, last.setup, last.fill, last.wait);
  return out;
}

double AudioConverter::time_kernels(const uint8_t* raw, uint64_t n_frames, int fmt, int channels, int rate, int reps,
                                    bool split) {
  WDR_CHECK(fmt >= 0 && fmt <= 4, "audio: sample format must be 0 (u8), 1 (i16), 2 (i24), 3 (i32) or 4 (f32)");
  WDR_CHECK(channels >= 1 && channels <= AUDIO_MAX_CHANNELS,
            "unsupported channel count " + std::to_string(channels) + " (1 to 8)");
  DeviceScope ds(dev_);
  const DevTable& tb = table(rate);
  const size_t bytes = (size_t)n_frames * channels * audio_sample_bytes(fmt);
  const uint64_t n_out = audio_n_out(n_frames, tb.L, tb.M);
  if (!n_out) return 0.0;
  DevMem in(up16(bytes) + 16), out((split ? (uint64_t)channels : 1) * n_out * 2);
  WDR_HIP(hipMemcpy(in.p, raw, bytes, hipMemcpyHostToDevice));
  const float invC = 1.0f / (float)channels;
  auto run = [&] {
    if (split)
      launch_audio_split(in.p, fmt, channels, 0, (long long)n_frames, tb.tab.as<float>(), tb.L, tb.M, tb.H, tb.T,
                         out.as<int16_t>(), (long long)n_out, 0, (long long)n_out, s_comp_);
    else
      launch_audio_convert(in.p, fmt, channels, invC, 0, (long long)n_frames, tb.tab.as<float>(), tb.L, tb.M, tb.H, tb.T,
                           out.as<int16_t>(), 0, (long long)n_out, s_comp_);
  };
  run();
  WDR_HIP(hipStreamSynchronize(s_comp_));
  hipEvent_t e0, e1;
  WDR_HIP(hipEventCreate(&e0));
  WDR_HIP(hipEventCreate(&e1));
  WDR_HIP(hipEventRecord(e0, s_comp_));
  for (int i = 0; i < reps; ++i) run();
  WDR_HIP(hipEventRecord(e1, s_comp_));
  WDR_HIP(hipEventSynchronize(e1));
  float t = 0.f;
  WDR_HIP(hipEventElapsedTime(&t, e0, e1));
  WDR_HIP(hipEventDestroy(e0));
  WDR_HIP(hipEventDestroy(e1));
  return (double)t / reps;
}

static std::vector<int16_t> read_audio_impl(const char* path, int device, std::unique_ptr<AudioConverter>* conv,
                                            int* channels) {
  const AudioInfo a = audio_parse(path);
  if (channels) *channels = a.channels;
  if (a.fmt == AUDIO_I16 && a.channels == 1 && a.rate == AUDIO_OUT_RATE) {
    std::vector<int16_t> out(a.n_frames);
    if (!out.empty()) audio_read_bytes(path, a.data_off, out.data(), out.size() * 2);
    return out;
  }
  struct File {
    FILE* f;
    ~File() { if (f) fclose(f); }
  } file{fopen(path, "rb")};
  if (!file.f) throw std::runtime_error("failed to read file");
  const size_t fb = (size_t)a.block_align;
  auto fill = [&](uint64_t frame, uint64_t n, uint8_t* dst) {
    if (fseeko(file.f, (off_t)(a.data_off + frame * fb), SEEK_SET) != 0 || fread(dst, 1, (size_t)n * fb, file.f) != (size_t)n * fb)
      throw std::runtime_error("failed to read file");
  };
  std::unique_ptr<AudioConverter> own;
  if (!conv) conv = &own;
  if (!*conv) conv->reset(new AudioConverter(device));
  return channels ? (*conv)->convert_channels(fill, a.n_frames, a.fmt, a.channels, a.rate, 0)
                  : (*conv)->convert(fill, a.n_frames, a.fmt, a.channels, a.rate, 0);
}

std::vector<int16_t> read_audio_file(const char* path, int device, std::unique_ptr<AudioConverter>* conv) {
  return read_audio_impl(path, device, conv, nullptr);
}

std::vector<int16_t> read_audio_file_channels(const char* path, int device, std::unique_ptr<AudioConverter>* conv,
                                              int* channels) {
  int c = 0;
  std::vector<int16_t> out = read_audio_impl(path, device, conv, &c);
  if (channels) *channels = c;
  return out;
}

}  // namespace wdr
