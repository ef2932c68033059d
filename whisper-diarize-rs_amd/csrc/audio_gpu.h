// Audio ingest, device side: streams raw frames through kernels/audio.hip in chunks
// (DESIGN.md §3c).  Device and pinned staging are bounded by the chunk size whatever the length
// of the input; the coefficient tables are cached per source rate.
#pragma once

#include <functional>
#include <map>
#include <memory>
#include <vector>

#include "audio_file.h"
#include "common.h"
#include "whisper.h"

namespace wdr {

class AudioConverter {
 public:
  // copies frames [frame, frame + n) of the source into dst (n * channels * sample bytes)
  using Fill = std::function<void(uint64_t frame, uint64_t n, uint8_t* dst)>;
  // host seconds of the last convert() (WDR_AUDIO_LOG=1 prints them): table and staging set-up,
  // inside Fill (file read / copy into pinned memory), blocked on the GPU (copies and kernels
  // the overlap did not hide), and in all
  struct Times { double setup = 0, fill = 0, wait = 0, total = 0; long long chunks = 0; };

  explicit AudioConverter(int device);
  ~AudioConverter();
  AudioConverter(const AudioConverter&) = delete;
  AudioConverter& operator=(const AudioConverter&) = delete;

  // chunk_frames 0: the default (about 32 MB of raw bytes, at most 16 Mi outputs).  The result
  // does not depend on chunk_frames.  The caller's current device is restored on return.
  std::vector<int16_t> convert(const Fill& fill, uint64_t n_frames, int fmt, int channels, int rate,
                               uint64_t chunk_frames);
  // one speaker per channel: planar [channels][n_out], channel c being the
  // conversion of the mono stream made of sample c of every frame.  The same pipeline, halo rule
  // and indexing as convert(); chunk_frames 0: about 32 MB of raw bytes, at most 16 Mi outputs
  // counted over all channels together
  std::vector<int16_t> convert_channels(const Fill& fill, uint64_t n_frames, int fmt, int channels, int rate,
                                        uint64_t chunk_frames);
  // mean GPU milliseconds of `reps` back-to-back runs of the kernels over the whole input,
  // resident on the device (one untimed run first); split: the channel-keeping kernels
  double time_kernels(const uint8_t* raw, uint64_t n_frames, int fmt, int channels, int rate, int reps,
                      bool split = false);
  Times last;

 private:
  struct DevTable { int L = 1, M = 1, H = 1, T = 0; DevMem tab; };
  const DevTable& table(int rate);
  std::vector<int16_t> run(const Fill& fill, uint64_t n_frames, int fmt, int channels, int rate, uint64_t chunk_frames,
                           bool split);
  void reserve(size_t in_bytes, size_t out_samples);
  void release_pinned();

  int dev_;
  hipStream_t s_copy_ = nullptr, s_comp_ = nullptr;
  hipEvent_t ev_copied_[2] = {nullptr, nullptr}, ev_done_[2] = {nullptr, nullptr};
  uint8_t* h_in_[2] = {nullptr, nullptr};
  int16_t* h_out_[2] = {nullptr, nullptr};
  DevMem d_in_[2], d_out_[2];
  size_t cap_in_ = 0, cap_out_ = 0;
  std::map<int, DevTable> tabs_;
};

// any supported WAV -> 16 kHz mono int16.  A 16 kHz mono 16-bit file is returned as it is, with
// no GPU work; everything else goes through *conv (created on `device` when null)
std::vector<int16_t> read_audio_file(const char* path, int device, std::unique_ptr<AudioConverter>* conv);
// any supported WAV -> 16 kHz int16 per channel, planar [*channels][n] (n = size / *channels).  A
// 16 kHz 16-bit file involves no filter, and a mono one is returned as it is with no GPU work
std::vector<int16_t> read_audio_file_channels(const char* path, int device, std::unique_ptr<AudioConverter>* conv,
                                              int* channels);

}  // namespace wdr
