// whisper.cpp ggml model file (the `ggml-<model>.bin` files the reference's model manager
// caches, src/model_manager.rs:148-299, loaded by whisper-rs at src/transcribe.rs:154):
//   magic 0x67676d6c, 11 int32 hparams (n_vocab, n_audio_ctx, n_audio_state, n_audio_head,
//   n_audio_layer, n_text_ctx, n_text_state, n_text_head, n_text_layer, n_mels, ftype),
//   mel filters (int32 n_mel, int32 n_fft, f32[n_mel][n_fft]), vocabulary (int32 n, then n x
//   (int32 len, bytes)), then tensors until EOF: int32 n_dims, int32 name_len, int32 type,
//   int32 ne[n_dims] (ne[0] innermost), name bytes, data (type 0 = f32, 1 = f16, or one of the
//   block-quantized types below).
// Quantized tensors (the files whisper.cpp's `quantize` tool writes; ftype = base + 1000 *
// qnt_version) are rows of blocks of 32 consecutive elements along ne[0]; d / m are f16, all
// fields little-endian, blocks only 2-byte aligned:
//   2 q4_0 18 B  d, qs[16]          element j / j+16 = ((qs[j] & 15) - 8) d / ((qs[j] >> 4) - 8) d
//   3 q4_1 20 B  d, m, qs[16]       (qs[j] & 15) d + m / (qs[j] >> 4) d + m
//   6 q5_0 22 B  d, qh u32, qs[16]  bit e of qh is the fifth bit of element e; (q - 16) d
//   7 q5_1 24 B  d, m, qh, qs[16]   q d + m
//   8 q8_0 34 B  d, int8 qs[32]     qs[i] d
// The value is float(d) * q (+ float(m)) in f32 (d * q is exact there); as f16 it is that value
// rounded once, to nearest even.  The k-quants (types 10..14) are rejected.
// Memory-mapped read-only; tensors are converted when they are uploaded (whisper_ctx.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

namespace wdr {

// bytes per 32-element block of a quantized ggml type, 0 for every other type
inline int ggml_block_bytes(int type) {
  switch (type) {
    case 2: return 18;
    case 3: return 20;
    case 6: return 22;
    case 7: return 24;
    case 8: return 34;
    default: return 0;
  }
}
// the host definition of the block decode: n_blocks raw blocks -> 32 * n_blocks f32 values
void ggml_dequant_f32(int type, const char* blocks, int64_t n_blocks, float* out);

struct GgmlTensor {
  int type = 0;                 // 0 f32, 1 f16, 2 / 3 / 6 / 7 / 8 block-quantized
  std::vector<int64_t> ne;      // ne[0] innermost
  const char* data = nullptr;   // inside the mapping
  int64_t n_elem() const {
    int64_t n = 1;
    for (int64_t x : ne) n *= x;
    return n;
  }
  bool quantized() const { return ggml_block_bytes(type) != 0; }
  size_t n_bytes() const {
    const int bs = ggml_block_bytes(type);
    return bs ? (size_t)(n_elem() / 32) * bs : (size_t)n_elem() * (type == 0 ? 4 : 2);
  }
};

class GgmlFile {
 public:
  explicit GgmlFile(const std::string& path);   // throws std::runtime_error("failed to open model: ...")
  ~GgmlFile();
  GgmlFile(const GgmlFile&) = delete;
  GgmlFile& operator=(const GgmlFile&) = delete;

  int32_t hp[11] = {};                  // n_vocab .. n_mels, ftype
  int n_mel = 0, n_fft = 0;
  std::vector<float> filters;           // [n_mel][n_fft]
  std::vector<std::string> vocab;       // the file's token texts (ids 0..n-1)
  std::map<std::string, GgmlTensor> tensors;

  const GgmlTensor& get(const std::string& name) const;   // throws if absent
  // tensor `name` as f32 / f16 values (row-major, element count checked against n)
  std::vector<float> as_f32(const std::string& name, int64_t n) const;
  std::vector<uint16_t> as_f16(const std::string& name, int64_t n) const;

 private:
  void* map_ = nullptr;
  size_t size_ = 0;
};

}  // namespace wdr
