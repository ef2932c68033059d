// Front-end, normalisation, decoding-rule and alignment kernels (HBM / latency bound).
//
//  k_mel_frames      a4  log-mel: reflect/zero padding, periodic Hann(400), 201-bin DFT
//                        (f32, LDS twiddle table), mel dot in double, log10, global max.
//  k_im2col_mel      a4/a5 clamp (max-8) + (x+4)/4 normalisation fused into the conv1
//                        im2col of one 3000-frame window (f16, ggml im2col precision).
//  k_im2col_conv2    a5  stride-2 im2col of the conv1 output.
//  k_energy          a3  whisper.cpp get_signal_energy, bit-exact (same f32 add order).
//  k_layernorm       a6/a9 ggml_norm (double sums) * gamma + beta -> f16 matmul input.
//  k_embed           a9  token + positional embedding.
//  k_logits_process  a10 whisper.cpp whisper_process_logits + greedy pick + timestamp
//                        probabilities + no-speech probability, one workgroup per row.
//  k_dtw_norm / k_dtw_medmean / k_dtw_dp   a12 DTW preprocessing and the DP
//                        (anti-diagonal wavefront, 2-bit trace in LDS, backtrace).
//  k_synth_fill      synthetic seeded weights (oracle/weights.py hash, bit-identical).
#include "../common.h"
#include "kernels.h"
#include "../prof.h"

namespace wdr {

// ---------------------------------------------------------------- synthetic weights
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  uint64_t z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// dst [rows][dst_cols]; element (r, c < src_cols) is element r*src_cols + c of the named tensor,
// padding columns are zero.  mode 0 = hash, mode 1 = constant cval.
__global__ void k_synth_fill(void* dst, long long rows, int src_cols, int dst_cols, uint64_t seed, float scale,
                             int is_f16, float cval, int mode) {
  const long long n = rows * dst_cols;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const long long r = i / dst_cols;
    const int c = (int)(i - r * dst_cols);
    float w = 0.f;
    if (c < src_cols) {
      if (mode == 0) {
        const uint64_t h = splitmix64(seed + (uint64_t)(r * src_cols + c));
        const float v = (float)(uint32_t)(h >> 40) * 1.1920928955078125e-07f - 1.0f;
        w = v * scale;
      } else {
        w = cval;
      }
    }
    if (is_f16) ((f16*)dst)[i] = (f16)w;
    else ((float*)dst)[i] = w;
  }
}

void launch_synth_fill(void* dst, long long rows, int src_cols, int dst_cols, uint64_t seed, float scale, bool f16out,
                       int mode, float cval, hipStream_t s) {
  const long long n = rows * dst_cols;
  long long blocks = (n + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  if (blocks < 1) blocks = 1;
  WDR_KLAUNCH(k_synth_fill, dim3((unsigned)blocks), dim3(256), 0, s, dst, rows, src_cols, dst_cols, seed, scale,
                     f16out ? 1 : 0, cval, mode);
  WDR_HIP(hipGetLastError());
}

// ---------------------------------------------------------------- log-mel
__device__ __forceinline__ int f2ord(float f) {
  int i = __float_as_int(f);
  return i >= 0 ? i : i ^ 0x7FFFFFFF;
}
__device__ __forceinline__ float ord2f(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7FFFFFFF); }

// frames per workgroup: 2 -- a 5-s segment (~500 frames) is 250 workgroups, the chip's width (8
// per workgroup left ~190 of 256 CUs idle: 151 us per call, profiles/r05/prof_graph); each
// thread's arithmetic is unchanged
constexpr int MEL_FB = 2;

__global__ __launch_bounds__(256) void k_mel_frames(MelArgs a) {
  __shared__ float xs[MEL_FB][400];
  __shared__ float cs[400], sn[400];
  __shared__ float pw[MEL_FB][201];
  __shared__ int bmax;
  const int tid = threadIdx.x;
  const int f0 = blockIdx.x * MEL_FB;
  if (tid == 0) bmax = f2ord(-INFINITY);
  for (int i = tid; i < 400; i += 256) {
    cs[i] = a.cos_tab[i];
    sn[i] = a.sin_tab[i];
  }
  const int n = a.n;
  const int n_eff = n + 200;
  for (int i = tid; i < MEL_FB * 400; i += 256) {
    const int fl = i / 400, j = i % 400;
    const int f = f0 + fl;
    float v = 0.f;
    if (f < a.n_frames) {
      const int p = f * 160 + j;             // index into the padded signal
      if (p < n_eff) {
        if (p >= 200) v = a.x[p - 200];
        else {
          const int src = 200 - p;           // reverse_copy(samples + 1, samples + 201)
          v = src < n ? a.x[src] : 0.f;
        }
      }
      v *= a.hann[j];
    }
    xs[fl][j] = v;
  }
  __syncthreads();
  for (int i = tid; i < MEL_FB * 201; i += 256) {
    const int fl = i / 201, k = i % 201;
    float re = 0.f, im = 0.f;
    int idx = 0;
    for (int j = 0; j < 400; ++j) {
      const float xv = xs[fl][j];
      re = fmaf(xv, cs[idx], re);
      im = fmaf(xv, sn[idx], im);
      idx += k;
      if (idx >= 400) idx -= 400;
    }
    pw[fl][k] = re * re + im * im;
  }
  __syncthreads();
  int lmax = f2ord(-INFINITY);
  for (int i = tid; i < MEL_FB * a.n_mels; i += 256) {
    const int fl = i / a.n_mels, mm = i % a.n_mels;
    const int f = f0 + fl;
    if (f >= a.n_frames) continue;
    const float* flt = a.filters + mm * 201;
    double sum = 0.0;
    for (int k = 0; k < 201; ++k) sum += (double)(pw[fl][k] * flt[k]);
    const double lv = log10(sum > 1e-10 ? sum : 1e-10);
    const float out = (float)lv;
    a.mel[(long long)f * a.n_mels + mm] = out;
    lmax = max(lmax, f2ord(out));
  }
  atomicMax(&bmax, lmax);
  __syncthreads();
  if (tid == 0) atomicMax(a.gmax, bmax);
}

void launch_mel(const MelArgs& a, hipStream_t s) {
  if (a.n_frames > 0) {
    WDR_KLAUNCH(k_mel_frames, dim3(cdiv(a.n_frames, MEL_FB)), dim3(256), 0, s, a);
    WDR_HIP(hipGetLastError());
  }
}

// whisper.cpp's clamp (max - 8) and (x + 4) / 4, in double as there
__device__ __forceinline__ double mel_norm(float raw, float gmax) {
  const double mmax = (double)gmax - 8.0;
  double v = raw;
  float f = raw;
  if (v < mmax) f = (float)mmax;
  return ((double)f + 4.0) / 4.0;
}

// The conv1 operand is mel_norm rounded ONCE, double -> f16 (what k_im2col_mel has always stored:
// the compiler folded an intermediate f32 into the f16 conversion; now it is written that way).
// whisper.cpp keeps the log-mel as f32 and ggml's im2col rounds that to f16 -- two roundings, one
// f16 ulp away on the few elements (3 .. 15 of a window measured) whose f32 value lands on an f16
// tie.  The f32 readback of the window therefore rounds the double TO ODD: f32 carries 13 more
// bits than f16, so rounding that f32 to f16 (numpy's astype, the host im2col of
// encode_from_mel_window) gives exactly the f16 the double rounds to, and the debug single-window
// path feeds conv1 the same bits as every production encode (tests/test_gpu_encoder_kernels.py
// test_im2col_mel, test_encode_batch).  It is within one f32 ulp of the nearest f32.
__device__ __forceinline__ float f32_round_to_odd(double d) {
  float r = (float)d;
  if ((double)r == d) return r;
  unsigned b = __float_as_uint(r);
  if (fabs((double)r) > fabs(d)) b -= 1;   // towards zero (normal range: the window's values are O(1))
  return __uint_as_float(b | 1u);
}

__global__ void k_im2col_mel(Im2colMelArgs a) {
  const long long total = 3000ll * a.kp;
  const float gmax = ord2f(*a.gmax);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int t = (int)(i / a.kp), col = (int)(i % a.kp);
    f16 v = (f16)0.f;
    if (col < a.n_mels * 3) {
      const int ci = col / 3, k = col % 3;
      const int u = t + k - 1;
      if (u >= 0 && u < 3000) {
        const int f = a.seek + u;
        const float raw = f < a.n_fft_frames ? a.mel[(long long)f * a.n_mels + ci] : -10.f;
        v = (f16)mel_norm(raw, gmax);   // one rounding, double -> f16 (see f32_round_to_odd)
      }
    }
    a.out[i] = v;
  }
}

void launch_im2col_mel(const Im2colMelArgs& a, hipStream_t s) {
  WDR_KLAUNCH(k_im2col_mel, dim3(2048), dim3(256), 0, s, a);
  WDR_HIP(hipGetLastError());
}

// conv2's im2col of nb windows in one launch: output row (b, t) = [ci][k] = x_b[2t + k - 1][ci]
// (0 outside the window).  A thread moves 4 channels: three 8-byte loads (rows 2t-1, 2t, 2t+1)
// and the 12 f16 of its columns as three 8-byte stores, rows contiguous, 32-bit index math (the
// element-wise form -- two 64-bit divisions per f16, one launch per window -- moved ~0.65 TB/s).
__global__ __launch_bounds__(256) void k_im2col_conv2(const f16* x, int d, int nb, f16* out) {
  const int q = d >> 2;                       // channel quads per row
  const int total = nb * 1500 * q;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int row = i / q, c4 = i - row * q;
    const int b = row / 1500, t = row - b * 1500;
    const f16* xb = x + (size_t)b * 3000 * d + 4 * c4;
    f16 v[3][4];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int u = 2 * t + k - 1;
      if (u >= 0 && u < 3000) {
        const uint2 w = *reinterpret_cast<const uint2*>(xb + (size_t)u * d);
        __builtin_memcpy(v[k], &w, 8);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[k][j] = (f16)0.f;
      }
    }
    f16 o[12];   // column (4 c4 + j) * 3 + k
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < 3; ++k) o[j * 3 + k] = v[k][j];
    uint2* dst = reinterpret_cast<uint2*>(out + (size_t)row * 3 * d + 12 * c4);
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      uint2 u;
      __builtin_memcpy(&u, o + 4 * w, 8);
      dst[w] = u;
    }
  }
}

void launch_im2col_conv2(const f16* x, int d, int nb, f16* out, hipStream_t s) {
  WDR_CHECK(d % 4 == 0 && nb >= 1 && (long long)nb * 1500 * (d / 4) < (1ll << 31), "im2col conv2: d % 4, nb");
  const int total = nb * 1500 * (d / 4);
  const int grid = std::min((total + 255) / 256, 8192);
  WDR_KLAUNCH(k_im2col_conv2, dim3(grid), dim3(256), 0, s, x, d, nb, out);
  WDR_HIP(hipGetLastError());
}

// read back the normalised window as f32 [n_mels][3000] (debug / tests), rounded to odd so that its
// f16 rounding is the conv1 operand k_im2col_mel stores (f32_round_to_odd)
__global__ void k_mel_window(const float* mel, int n_mels, int n_fft_frames, const int* gmax_ord, int seek, float* out) {
  const float gmax = ord2f(*gmax_ord);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_mels * 3000; i += gridDim.x * blockDim.x) {
    const int ci = i / 3000, u = i % 3000;
    const int f = seek + u;
    const float raw = f < n_fft_frames ? mel[(long long)f * n_mels + ci] : -10.f;
    out[i] = f32_round_to_odd(mel_norm(raw, gmax));
  }
}

void launch_mel_window(const float* mel, int n_mels, int n_fft_frames, const int* gmax, int seek, float* out,
                       hipStream_t s) {
  WDR_KLAUNCH(k_mel_window, dim3(512), dim3(256), 0, s, mel, n_mels, n_fft_frames, gmax, seek, out);
  WDR_HIP(hipGetLastError());
}

__global__ void k_set_int(int* p, int v) { *p = v; }
void launch_gmax_init(int* gmax, hipStream_t s) {
  // the zero-padded tail always exists (n_len > n_fft_frames), so the max starts at -10
  union { float f; int i; } u;
  u.f = -10.f;
  WDR_KLAUNCH(k_set_int, dim3(1), dim3(1), 0, s, gmax, u.i);
  WDR_HIP(hipGetLastError());
}

// ---------------------------------------------------------------- signal energy
__global__ void k_energy(const float* x, int n, float* e) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float sum = 0.f;
  for (int j = -32; j <= 32; ++j) {
    const int p = i + j;
    if (p >= 0 && p < n) sum += fabsf(x[p]);
  }
  e[i] = sum / 65;
}

void launch_energy(const float* x, int n, float* e, hipStream_t s) {
  if (n <= 0) return;
  WDR_KLAUNCH(k_energy, dim3(cdiv(n, 256)), dim3(256), 0, s, x, n, e);
  WDR_HIP(hipGetLastError());
}

__global__ void k_i16_to_f32(const int16_t* in, int n, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (float)in[i] / 32768.0f;
}
void launch_i16_to_f32(const int16_t* in, int n, float* out, hipStream_t s) {
  if (n <= 0) return;
  WDR_KLAUNCH(k_i16_to_f32, dim3(cdiv(n, 256)), dim3(256), 0, s, in, n, out);
  WDR_HIP(hipGetLastError());
}

// ---------------------------------------------------------------- LayerNorm / embedding / KV
__global__ __launch_bounds__(256) void k_layernorm(const float* x, int ldx, const float* g, const float* b, f16* y,
                                                   int ldy, int rows, int d, const int* row_map) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xr = x + (long long)(row_map ? row_map[row] : row) * ldx;
  // d <= 1280: each lane keeps its <= 20 values in registers (fully unrolled: compile-time
  // indices keep them out of scratch); gamma / beta are read only in the output loop, so the
  // kernel stays under 64 VGPRs and fits beside an encoder GEMM tile on a CU
  float v[5][4];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int c = lane * 4 + j * 256;
    const bool ok = c < d;
    const int cc = ok ? c : 0;
    const float4 q = *(const float4*)(xr + cc);
    v[j][0] = ok ? q.x : 0.f; v[j][1] = ok ? q.y : 0.f; v[j][2] = ok ? q.z : 0.f; v[j][3] = ok ? q.w : 0.f;
    s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
  }
  s = wave_sum(s);
  const float mean = s / d;
  float s2 = 0.f;
#pragma unroll
  for (int j = 0; j < 5; ++j)
    if (lane * 4 + j * 256 < d)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float t = v[j][e] - mean;
        s2 += t * t;
      }
  s2 = wave_sum(s2);
  const float scale = 1.0f / sqrtf(s2 / d + 1e-5f);
  f16* yr = y + (long long)row * ldy;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int c = lane * 4 + j * 256;
    if (c >= d) continue;
    const float4 g4 = *(const float4*)(g + c);
    const float4 b4 = *(const float4*)(b + c);
    const float gg[4] = {g4.x, g4.y, g4.z, g4.w}, bb[4] = {b4.x, b4.y, b4.z, b4.w};
    f16x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (f16)((v[j][e] - mean) * scale * gg[e] + bb[e]);
    *(f16x4*)(yr + c) = o;
  }
}

void launch_layernorm(const float* x, int ldx, const float* g, const float* b, f16* y, int ldy, int rows, int d,
                      hipStream_t s) {
  WDR_CHECK(d % 4 == 0 && d <= 1280 && ldx % 4 == 0 && ldy % 4 == 0, "layernorm: unsupported width");
  WDR_KLAUNCH(k_layernorm, dim3(cdiv(rows, 4)), dim3(256), 0, s, x, ldx, g, b, y, ldy, rows, d, nullptr);
  WDR_HIP(hipGetLastError());
}

// the rows row_map[0 .. rows) of x (the logit rows of a rows_forward batch), compacted into y
void launch_layernorm_rows(const float* x, int ldx, const float* g, const float* b, f16* y, int ldy, int rows, int d,
                           const int* row_map, hipStream_t s) {
  WDR_CHECK(d % 4 == 0 && d <= 1280 && ldx % 4 == 0 && ldy % 4 == 0, "layernorm: unsupported width");
  WDR_KLAUNCH(k_layernorm, dim3(cdiv(rows, 4)), dim3(256), 0, s, x, ldx, g, b, y, ldy, rows, d, row_map);
  WDR_HIP(hipGetLastError());
}

__global__ void k_embed(const f16* E, const float* P, const int* tok, const int* pos, int d, float* x) {
  const int r = blockIdx.x;
  const int t = tok[r], p = pos[r];
  for (int c = threadIdx.x; c < d; c += blockDim.x)
    x[(long long)r * d + c] = (float)E[(long long)t * d + c] + P[(long long)p * d + c];
}

void launch_embed(const f16* E, const float* P, const int* tok, const int* pos, int R, int d, float* x, hipStream_t s) {
  WDR_KLAUNCH(k_embed, dim3(R), dim3(256), 0, s, E, P, tok, pos, d, x);
  WDR_HIP(hipGetLastError());
}

// ---------------------------------------------------------------- logits rules
template <typename T>
__device__ __forceinline__ T block_reduce(T v, T* sh, int op) {   // op 0 = max, 1 = sum ; blockDim 1024
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) {
    const T u = __shfl_xor(v, o, 64);
    v = op == 0 ? (v > u ? v : u) : v + u;
  }
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  if (w == 0) {
    v = lane < 16 ? sh[lane] : (op == 0 ? (T)-INFINITY : (T)0);
    for (int o = 32; o > 0; o >>= 1) {
      const T u = __shfl_xor(v, o, 64);
      v = op == 0 ? (v > u ? v : u) : v + u;
    }
    if (lane == 0) sh[0] = v;
  }
  __syncthreads();
  const T r = sh[0];
  __syncthreads();
  return r;
}

// argmax with whisper.cpp's tie rule: the first index holding the maximum (strict <).
__device__ __forceinline__ void amax_merge(float& v, int& i, float v2, int i2) {
  if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}
__device__ void block_argmax(float& v, int& idx, float* shv, int* shi) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(v, o, 64);
    const int i2 = __shfl_xor(idx, o, 64);
    amax_merge(v, idx, v2, i2);
  }
  __syncthreads();
  if (lane == 0) { shv[w] = v; shi[w] = idx; }
  __syncthreads();
  if (w == 0) {
    v = lane < 16 ? shv[lane] : -INFINITY;
    idx = lane < 16 ? shi[lane] : 0x7fffffff;
    for (int o = 32; o > 0; o >>= 1) {
      const float v2 = __shfl_xor(v, o, 64);
      const int i2 = __shfl_xor(idx, o, 64);
      amax_merge(v, idx, v2, i2);
    }
    if (lane == 0) { shv[0] = v; shi[0] = idx; }
  }
  __syncthreads();
  v = shv[0];
  idx = shi[0];
  __syncthreads();
}

__device__ __forceinline__ float rule_mask(float x, int i, const LogitsCtl& c, const VocabIds& v) {
  const bool initial = c.n_tokens == 0;
  if (c.temperature > 0.f) x = x / c.temperature;
  bool masked = false;
  if (v.suppress_blank && initial && (i == v.eot || i == v.space)) masked = true;
  if (i == v.not_ || i == v.sot || i == v.nosp || i == v.solm || i == v.translate || i == v.transcribe || i == v.prev)
    masked = true;
  if (i >= v.lang0 && i < v.lang0 + v.n_lang) masked = true;
  if (c.last_ts) {
    if (c.pen_ts) {
      if (i >= v.beg) masked = true;
    } else if (i < v.eot) {
      masked = true;
    }
  }
  if (initial && v.max_initial_tid >= 0 && i > v.beg + v.max_initial_tid) masked = true;
  if (c.has_ts && i >= v.beg && i < v.beg + c.seek_delta / 2) masked = true;
  // synthetic workload pin (applied after whisper.cpp's own rules)
  if (c.force_kind == 1) return i == c.force_tok ? (masked ? 0.f : x) : -INFINITY;
  if (c.force_kind == 2 && (i == v.eot || i >= v.beg)) masked = true;
  return masked ? -INFINITY : x;
}

// online (max, sum-of-exp) pair
struct MS {
  float m, s;
};
__device__ __forceinline__ MS ms_add(MS a, float x) {
  if (x == -INFINITY) return a;
  if (x > a.m) return MS{x, a.s * __expf(a.m - x) + 1.f};
  return MS{a.m, a.s + __expf(x - a.m)};
}
__device__ __forceinline__ MS ms_merge(MS a, MS b) {
  if (b.m == -INFINITY) return a;
  if (a.m == -INFINITY) return b;
  const float M = fmaxf(a.m, b.m);
  return MS{M, a.s * __expf(a.m - M) + b.s * __expf(b.m - M)};
}
__device__ __forceinline__ MS ms_wave(MS v) {
  for (int o = 32; o > 0; o >>= 1) {
    MS u{__shfl_xor(v.m, o, 64), __shfl_xor(v.s, o, 64)};
    v = ms_merge(v, u);
  }
  return v;
}

constexpr int LG_NB = 32;   // vocabulary slices (workgroups) per row

struct LgStats {   // per (row, slice)
  float m0, s0, m1, s1, mts, sts, mtx, pad;
};
struct LgPick {
  float bp; int bi; float tp; int ti; double tsum;
};

// pass 1: raw and filtered (max, sum-exp), timestamp-range (max, sum-exp), best text logit
__global__ __launch_bounds__(256) void k_logits_stats(const float* logits, int ld, const LogitsCtl* ctls, VocabIds v,
                                                      LgStats* st) {
  __shared__ LgStats sh[4];
  const int b = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  const float* L = logits + (long long)r * ld;
  const LogitsCtl c = ctls[r];
  const int V = v.n_vocab, chunk = (V + LG_NB - 1) / LG_NB;
  const int i0 = b * chunk, i1 = min(V, i0 + chunk);
  MS raw{-INFINITY, 0.f}, all{-INFINITY, 0.f}, ts{-INFINITY, 0.f};
  float mtx = -INFINITY;
  for (int i = i0 + tid; i < i1; i += 256) {
    const float l = L[i];
    raw = ms_add(raw, l);
    const float x = rule_mask(l, i, c, v);
    all = ms_add(all, x);
    if (i >= v.beg) ts = ms_add(ts, x);
    else mtx = fmaxf(mtx, x);
  }
  raw = ms_wave(raw);
  all = ms_wave(all);
  ts = ms_wave(ts);
  mtx = wave_max(mtx);
  const int w = tid >> 6;
  if ((tid & 63) == 0) sh[w] = LgStats{raw.m, raw.s, all.m, all.s, ts.m, ts.s, mtx, 0.f};
  __syncthreads();
  if (tid == 0) {
    MS a{sh[0].m0, sh[0].s0}, bb{sh[0].m1, sh[0].s1}, t{sh[0].mts, sh[0].sts};
    float mx = sh[0].mtx;
    for (int k = 1; k < 4; ++k) {
      a = ms_merge(a, MS{sh[k].m0, sh[k].s0});
      bb = ms_merge(bb, MS{sh[k].m1, sh[k].s1});
      t = ms_merge(t, MS{sh[k].mts, sh[k].sts});
      mx = fmaxf(mx, sh[k].mtx);
    }
    st[r * LG_NB + b] = LgStats{a.m, a.s, bb.m, bb.s, t.m, t.s, mx, 0.f};
  }
}

__device__ __forceinline__ void lg_global(const LgStats* st, int r, LgStats& g) {
  MS a{-INFINITY, 0.f}, bb{-INFINITY, 0.f}, t{-INFINITY, 0.f};
  float mx = -INFINITY;
  for (int k = 0; k < LG_NB; ++k) {
    const LgStats& p = st[r * LG_NB + k];
    a = ms_merge(a, MS{p.m0, p.s0});
    bb = ms_merge(bb, MS{p.m1, p.s1});
    t = ms_merge(t, MS{p.mts, p.sts});
    mx = fmaxf(mx, p.mtx);
  }
  g = LgStats{a.m, a.s, bb.m, bb.s, t.m, t.s, mx, 0.f};
}

// pass 2: probabilities exp(x - lse) (text masked when the timestamp mass wins), first-index
// argmax over them, timestamp argmax and timestamp probability sum (double)
__global__ __launch_bounds__(256) void k_logits_pick(const float* logits, int ld, const LogitsCtl* ctls, VocabIds v,
                                                     const LgStats* st, LgPick* pk) {
  __shared__ LgStats g;
  __shared__ float shv[8];
  __shared__ int shi[8];
  __shared__ double shd[4];
  const int b = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  if (tid == 0) lg_global(st, r, g);
  __syncthreads();
  const float* L = logits + (long long)r * ld;
  const LogitsCtl c = ctls[r];
  const float lse = logf(g.s1) + g.m1;
  const float ts_lp = (g.mts == -INFINITY || !(g.sts > 0.f)) ? -INFINITY : logf(g.sts) + (g.mts - lse);
  const bool mask_text = ts_lp > g.mtx - lse;
  const int V = v.n_vocab, chunk = (V + LG_NB - 1) / LG_NB;
  const int i0 = b * chunk, i1 = min(V, i0 + chunk);
  float bp = 0.f, tp = 0.f;
  int bi = 0x7fffffff, ti = 0x7fffffff;
  double tsum = 0.0;
  for (int i = i0 + tid; i < i1; i += 256) {
    float x = rule_mask(L[i], i, c, v);
    if (mask_text && i < v.beg) x = -INFINITY;
    const float p = x == -INFINITY ? 0.f : __expf(x - lse);
    if (p > 0.f) amax_merge(bp, bi, p, i);
    if (i >= v.beg) {
      tsum += (double)p;
      if (p > 0.f) amax_merge(tp, ti, p, i);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(bp, o, 64);
    const int i2 = __shfl_xor(bi, o, 64);
    amax_merge(bp, bi, v2, i2);
    const float t2 = __shfl_xor(tp, o, 64);
    const int j2 = __shfl_xor(ti, o, 64);
    amax_merge(tp, ti, t2, j2);
  }
  tsum = wave_sum_d(tsum);
  const int w = tid >> 6;
  if ((tid & 63) == 0) {
    shv[w] = bp; shi[w] = bi; shv[4 + w] = tp; shi[4 + w] = ti; shd[w] = tsum;
  }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < 4; ++k) {
      amax_merge(shv[0], shi[0], shv[k], shi[k]);
      amax_merge(shv[4], shi[4], shv[4 + k], shi[4 + k]);
    }
    pk[r * LG_NB + b] = LgPick{shv[0], shi[0], shv[4], shi[4], shd[0] + shd[1] + shd[2] + shd[3]};
  }
}

__global__ void k_logits_final(const float* logits, int ld, const LogitsCtl* ctls, VocabIds v, const LgStats* st,
                               const LgPick* pk, TokOut* out) {
  const int r = blockIdx.x;
  if (threadIdx.x != 0) return;
  LgStats g;
  lg_global(st, r, g);
  const float* L = logits + (long long)r * ld;
  const LogitsCtl c = ctls[r];
  float bp = 0.f, tp = 0.f;
  int bi = 0x7fffffff, ti = 0x7fffffff;
  double tsum = 0.0;
  for (int k = 0; k < LG_NB; ++k) {
    const LgPick& p = pk[r * LG_NB + k];
    amax_merge(bp, bi, p.bp, p.bi);
    amax_merge(tp, ti, p.tp, p.ti);
    tsum += p.tsum;
  }
  const float lse = logf(g.s1) + g.m1;
  TokOut o;
  o.nosp_prob = __expf(L[v.nosp] - (logf(g.s0) + g.m0));
  o.ptsum = (float)tsum;
  o.pt = (float)((double)(ti == 0x7fffffff ? 0.f : tp) / (tsum + 1e-10));
  o.tid = ti == 0x7fffffff ? 0 : ti;
  if (bi == 0x7fffffff) {
    o.id = 0; o.p = 0.f; o.plog = 0.f;
  } else {
    o.id = bi; o.p = bp;
    o.plog = rule_mask(L[bi], bi, c, v) - lse;
  }
  if (o.id >= v.beg) { o.tid = o.id; o.pt = o.p; }
  o.pad = 0;
  out[r] = o;
}

// ---- beam search: top-K processed logits per row (whisper_sample_token_topk).  Candidates are
// ordered by the processed logit (= by probability), ties by lower token id; only finite
// entries are candidates (see oracle/whisper_full.py topk).
struct LgTop {
  float x[BEAM_KMAX];
  int i[BEAM_KMAX];
};

__device__ __forceinline__ bool top_better(float x, int i, float y, int j) { return x > y || (x == y && i < j); }

__global__ __launch_bounds__(256) void k_logits_topk(const float* logits, int ld, const LogitsCtl* ctls, VocabIds v,
                                                     const LgStats* st, int K, LgTop* part) {
  __shared__ LgStats g;
  __shared__ float shv[4];
  __shared__ int shi[4];
  const int b = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  if (tid == 0) lg_global(st, r, g);
  __syncthreads();
  const float* L = logits + (long long)r * ld;
  const LogitsCtl c = ctls[r];
  const float lse = logf(g.s1) + g.m1;
  const float ts_lp = (g.mts == -INFINITY || !(g.sts > 0.f)) ? -INFINITY : logf(g.sts) + (g.mts - lse);
  const bool mask_text = ts_lp > g.mtx - lse;
  const int V = v.n_vocab, chunk = (V + LG_NB - 1) / LG_NB;
  const int i0 = b * chunk, i1 = min(V, i0 + chunk);
  // each thread keeps its best K (sorted) over its strided elements
  float bx[BEAM_KMAX];
  int bi[BEAM_KMAX];
  for (int k = 0; k < BEAM_KMAX; ++k) { bx[k] = -INFINITY; bi[k] = 0x7fffffff; }
  for (int i = i0 + tid; i < i1; i += 256) {
    float x = rule_mask(L[i], i, c, v);
    if (mask_text && i < v.beg) x = -INFINITY;
    if (x == -INFINITY || !top_better(x, i, bx[K - 1], bi[K - 1])) continue;
    int p = K - 1;
    while (p > 0 && top_better(x, i, bx[p - 1], bi[p - 1])) { bx[p] = bx[p - 1]; bi[p] = bi[p - 1]; --p; }
    bx[p] = x; bi[p] = i;
  }
  // K rounds of a block-wide argmax over the threads' current heads
  LgTop out;
  int head = 0;
  for (int k = 0; k < K; ++k) {
    float hv = head < K ? bx[head] : -INFINITY;
    int hi = head < K ? bi[head] : 0x7fffffff;
    float wv = hv;
    int wi = hi;
    for (int o = 32; o > 0; o >>= 1) {
      const float v2 = __shfl_xor(wv, o, 64);
      const int i2 = __shfl_xor(wi, o, 64);
      if (top_better(v2, i2, wv, wi)) { wv = v2; wi = i2; }
    }
    if ((tid & 63) == 0) { shv[tid >> 6] = wv; shi[tid >> 6] = wi; }
    __syncthreads();
    float bv = shv[0];
    int bidx = shi[0];
    for (int q = 1; q < 4; ++q)
      if (top_better(shv[q], shi[q], bv, bidx)) { bv = shv[q]; bidx = shi[q]; }
    __syncthreads();
    out.x[k] = bv;
    out.i[k] = bidx;
    if (head < K && hi == bidx && bidx != 0x7fffffff) ++head;   // indices are unique
  }
  if (tid == 0) part[r * LG_NB + b] = out;
}

__global__ void k_logits_topk_final(const LgStats* st, const LgTop* part, int K, BeamCand* out) {
  const int r = blockIdx.x;
  if (threadIdx.x != 0) return;
  LgStats g;
  lg_global(st, r, g);
  const float lse = logf(g.s1) + g.m1;
  int ptr[LG_NB];
  for (int b = 0; b < LG_NB; ++b) ptr[b] = 0;
  for (int k = 0; k < K; ++k) {
    float bv = -INFINITY;
    int bidx = 0x7fffffff, bb = -1;
    for (int b = 0; b < LG_NB; ++b) {
      if (ptr[b] >= K) continue;
      const float x = part[r * LG_NB + b].x[ptr[b]];
      const int i = part[r * LG_NB + b].i[ptr[b]];
      if (x != -INFINITY && top_better(x, i, bv, bidx)) { bv = x; bidx = i; bb = b; }
    }
    BeamCand c;
    if (bb < 0) {
      c.id = -1; c.p = 0.f; c.plog = -INFINITY;
    } else {
      ptr[bb]++;
      c.id = bidx;
      c.plog = bv - lse;
      c.p = __expf(c.plog);
    }
    out[r * K + k] = c;
  }
}

void launch_logits_topk(const float* logits, int ld, const LogitsCtl* ctls, const VocabIds& v, int R, int K,
                        float* work, BeamCand* out, hipStream_t s) {
  WDR_CHECK(K >= 1 && K <= BEAM_KMAX, "beam size out of range");
  const LgStats* st = (const LgStats*)work;   // written by launch_logits_process
  LgTop* part = (LgTop*)(work + (size_t)R * LG_NB * 8 + (size_t)R * LG_NB * 8);
  WDR_KLAUNCH(k_logits_topk, dim3(LG_NB, R), dim3(256), 0, s, logits, ld, ctls, v, st, K, part);
  WDR_KLAUNCH(k_logits_topk_final, dim3(R), dim3(64), 0, s, st, part, K, out);
  WDR_HIP(hipGetLastError());
}

// temperature sampling (t > 0): the full processed distribution of each row, p and log p,
// for the host-side std::discrete_distribution draw (whisper_sample_token, best = false)
__global__ __launch_bounds__(256) void k_logits_probs(const float* logits, int ld, const LogitsCtl* ctls, VocabIds v,
                                                      const LgStats* st, float* probs, float* logprobs) {
  __shared__ LgStats g;
  const int b = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  if (tid == 0) lg_global(st, r, g);
  __syncthreads();
  const float* L = logits + (long long)r * ld;
  const LogitsCtl c = ctls[r];
  const float lse = logf(g.s1) + g.m1;
  const float ts_lp = (g.mts == -INFINITY || !(g.sts > 0.f)) ? -INFINITY : logf(g.sts) + (g.mts - lse);
  const bool mask_text = ts_lp > g.mtx - lse;
  const int V = v.n_vocab, chunk = (V + LG_NB - 1) / LG_NB;
  const int i0 = b * chunk, i1 = min(V, i0 + chunk);
  for (int i = i0 + tid; i < i1; i += 256) {
    float x = rule_mask(L[i], i, c, v);
    if (mask_text && i < v.beg) x = -INFINITY;
    probs[(long long)r * V + i] = x == -INFINITY ? 0.f : __expf(x - lse);
    logprobs[(long long)r * V + i] = x == -INFINITY ? -INFINITY : x - lse;
  }
}

void launch_logits_probs(const float* logits, int ld, const LogitsCtl* ctls, const VocabIds& v, int R, float* work,
                         float* probs, float* logprobs, hipStream_t s) {
  const LgStats* st = (const LgStats*)work;   // written by launch_logits_process
  WDR_KLAUNCH(k_logits_probs, dim3(LG_NB, R), dim3(256), 0, s, logits, ld, ctls, v, st, probs, logprobs);
  WDR_HIP(hipGetLastError());
}

// beam reorder: copy the first n_rows cached K/V rows of sequence src[p] to dst[p], every layer
__global__ void k_kv_copy(f16* kc, f16* vc, long long seq_stride, int nslot, const int* pairs, int n_rows, int d) {
  const int l = blockIdx.y, p = blockIdx.z;
  const int src = pairs[2 * p], dst = pairs[2 * p + 1];
  const long long n = (long long)n_rows * d / 8;
  const long long base = (long long)l * nslot * seq_stride;
  const f16x8* ks = reinterpret_cast<const f16x8*>(kc + base + src * seq_stride);
  const f16x8* vs = reinterpret_cast<const f16x8*>(vc + base + src * seq_stride);
  f16x8* kd = reinterpret_cast<f16x8*>(kc + base + dst * seq_stride);
  f16x8* vd = reinterpret_cast<f16x8*>(vc + base + dst * seq_stride);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    kd[i] = ks[i];
    vd[i] = vs[i];
  }
}

void launch_kv_copy(f16* kc, f16* vc, long long seq_stride, int nslot, int L, const int* pairs_dev, int n_pairs,
                    int n_rows, int d, hipStream_t s) {
  if (n_pairs <= 0 || n_rows <= 0) return;
  WDR_CHECK(d % 8 == 0, "kv copy: d must be a multiple of 8");
  WDR_KLAUNCH(k_kv_copy, dim3(std::max(1, std::min(64, n_rows * d / 8 / 256 + 1)), L, n_pairs), dim3(256), 0, s,
                     kc, vc, seq_stride, nslot, pairs_dev, n_rows, d);
  WDR_HIP(hipGetLastError());
}

void launch_logits_process(const float* logits, int ld, const LogitsCtl* ctls, const VocabIds& v, int R, float* work,
                           TokOut* out, hipStream_t s) {
  LgStats* st = (LgStats*)work;
  LgPick* pk = (LgPick*)(work + (size_t)R * LG_NB * 8);
  WDR_KLAUNCH(k_logits_stats, dim3(LG_NB, R), dim3(256), 0, s, logits, ld, ctls, v, st);
  WDR_KLAUNCH(k_logits_pick, dim3(LG_NB, R), dim3(256), 0, s, logits, ld, ctls, v, st, pk);
  WDR_KLAUNCH(k_logits_final, dim3(R), dim3(64), 0, s, logits, ld, ctls, v, st, pk, out);
  WDR_HIP(hipGetLastError());
}

// ---------------------------------------------------------------- DTW
// ggml_norm over tokens for every (head, column): float mean from a double sum, v = x - mean,
// double sum of v*v, scale = 1/sqrtf(var + 1e-9).
__global__ void k_dtw_norm(const float* cap, int A, int N, int Tk, int M, float* nrm) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A * M) return;
  const int a = i / M, col = i % M;
  const float* src = cap + (long long)a * N * Tk + col;
  double s = 0.0;
  for (int t = 0; t < N; ++t) s += (double)src[(long long)t * Tk];
  const float mean = (float)(s / N);
  double s2 = 0.0;
  for (int t = 0; t < N; ++t) {
    const float v = src[(long long)t * Tk] - mean;
    s2 += (double)(v * v);
  }
  const float var = (float)(s2 / N);
  const float scale = 1.0f / sqrtf(var + 1e-9f);
  float* dst = nrm + (long long)a * N * M + col;
  for (int t = 0; t < N; ++t) dst[(long long)t * M] = (src[(long long)t * Tk] - mean) * scale;
}

__device__ __forceinline__ void cswap(float& a, float& b) {
  const float lo = fminf(a, b), hi = fmaxf(a, b);
  a = lo;
  b = hi;
}

// median-7 along columns (reflect), mean over heads (double sum), negate; rows [sot_len, N-1)
__global__ void k_dtw_medmean(const float* nrm, int A, int N, int M, int sot_len, float* x) {
  const int rows = N - sot_len - 1;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * M) return;
  const int r = i / M, col = i % M;
  const int t = r + sot_len;
  double sum = 0.0;
  for (int a = 0; a < A; ++a) {
    const float* row = nrm + ((long long)a * N + t) * M;
    float w[7];
#pragma unroll
    for (int o = 0; o < 7; ++o) {
      int idx = col + o - 3;
      if (idx < 0) idx = -idx;
      else if (idx >= M) idx = 2 * (M - 1) - idx;
      w[o] = row[idx];
    }
    // sorting network for 7 elements
    cswap(w[0], w[6]); cswap(w[2], w[3]); cswap(w[4], w[5]);
    cswap(w[0], w[2]); cswap(w[1], w[4]); cswap(w[3], w[6]);
    cswap(w[0], w[1]); cswap(w[2], w[5]); cswap(w[3], w[4]);
    cswap(w[1], w[2]); cswap(w[4], w[6]);
    cswap(w[2], w[3]); cswap(w[4], w[5]);
    cswap(w[1], w[2]); cswap(w[3], w[4]); cswap(w[5], w[6]);
    sum += (double)w[3];
  }
  const float mean = (float)sum / (float)A;
  x[(long long)r * M + col] = mean * -1.0f;
}

constexpr int DTW_NMAX = 256, DTW_MMAX = 1504, DTW_WPR = DTW_MMAX / 16;

// x [N][M] -> t_dtw for each change of the token index along the backtraced path.
__global__ __launch_bounds__(256) void k_dtw_dp(const float* x, int N, int M, int seek, int* times, int* n_times) {
  __shared__ uint32_t tr[DTW_NMAX * DTW_WPR];
  __shared__ float dg[3][DTW_NMAX + 1];
  __shared__ short pi[DTW_NMAX + DTW_MMAX + 4], pj[DTW_NMAX + DTW_MMAX + 4];
  const int tid = threadIdx.x;
  const int i = tid + 1;   // row handled by this thread (1..N)
  for (int k = tid; k <= DTW_NMAX; k += 256) {
    dg[0][k] = INFINITY;
    dg[1][k] = INFINITY;
    dg[2][k] = INFINITY;
  }
  __syncthreads();
  if (tid == 0) dg[0][0] = 0.f;   // diagonal s = 0 holds cost[0][0]
  __syncthreads();
  const float* xr = x + (long long)(i - 1) * M;
  // each thread walks its own row left to right one column per step: keep an 8-deep
  // shift register of x so the global loads run 8 steps ahead of their use.
  float w[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) w[q] = (i <= N && q < M) ? xr[q] : 0.f;
  uint32_t acc = 0;
  for (int s = 2; s <= N + M; ++s) {
    const float* d2 = dg[(s - 2) % 3];
    const float* d1 = dg[(s - 1) % 3];
    float* d0 = dg[s % 3];
    const int j = s - i;
    float nv = INFINITY;
    if (i <= N && j >= 1 && j <= M) {
      const float c0 = d2[i - 1], c1 = d1[i - 1], c2 = d1[i];
      float c;
      uint32_t t;
      if (c0 < c1 && c0 < c2) { c = c0; t = 0; }
      else if (c1 < c0 && c1 < c2) { c = c1; t = 1; }
      else { c = c2; t = 2; }
      nv = w[0] + c;
#pragma unroll
      for (int q = 0; q < 7; ++q) w[q] = w[q + 1];
      w[7] = (j - 1 + 8 < M) ? xr[j - 1 + 8] : 0.f;
      acc |= t << (2 * ((j - 1) & 15));
      if (((j - 1) & 15) == 15 || j == M) {
        tr[(i - 1) * DTW_WPR + ((j - 1) >> 4)] = acc;
        acc = 0;
      }
    }
    if (i <= N) d0[i] = nv;
    if (tid == 0) d0[0] = INFINITY;   // cost[0][s] for s > 0
    __syncthreads();
  }
  if (tid == 0) {
    // backtrace from (N, M); trace[0][:] = 2, trace[:][0] = 1
    int ii = N, jj = M, len = 0;
    while (ii > 0 || jj > 0) {
      pi[len] = (short)(ii - 1);
      pj[len] = (short)(jj - 1);
      ++len;
      int t;
      if (ii == 0) t = 2;
      else if (jj == 0) t = 1;
      else t = (tr[(ii - 1) * DTW_WPR + ((jj - 1) >> 4)] >> (2 * ((jj - 1) & 15))) & 3;
      if (t == 0) { --ii; --jj; }
      else if (t == 1) --ii;
      else --jj;
    }
    int last_v = 0, nt = 0;
    for (int k = len - 1; k >= 0; --k) {
      const int v = pi[k];
      if (v != last_v) {
        times[nt++] = 2 * pj[k] + seek;
        last_v = v;
      }
    }
    *n_times = nt;
  }
}

// One wave per window: lane l owns rows l*R + 1 .. l*R + R (R = ceil(N / 64) <= 4) and keeps
// their last two anti-diagonals in registers; row i-1's values for a lane's first row come from
// lane l-1 by a lane shuffle, so a step of the N + M - 1 anti-diagonals needs no barrier (the
// 256-thread form above paid an LDS round trip and a workgroup barrier per step: 134 us per
// window in the 1-h trace).  The cell arithmetic, its tie rules and the 2-bit trace are the same
// (bit-identical times).  The backtrace keeps the current trace word in a register (a path moves
// along a row for most of its steps) and collects the token times as it walks; the lanes write
// them out in forward order.
// lane l <- lane l-1 across the whole wave (DPP wave_shr:1, a VALU modifier: no LDS round trip)
__device__ __forceinline__ float wave_shr1(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}

template <int R>
__global__ __launch_bounds__(64) void k_dtw_dp_wave(const float* x, int N, int M, int seek, int* times, int* n_times) {
  __shared__ uint32_t tr[DTW_NMAX * DTW_WPR];
  __shared__ int em[DTW_NMAX + DTW_MMAX + 4];
  __shared__ int s_ne;
  const int lane = threadIdx.x;
  float D1[R], D2[R], w[R][8];
  uint32_t acc[R];
  const float* xr[R];
  bool live[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = lane * R + r + 1;
    live[r] = i <= N;
    xr[r] = x + (long long)(live[r] ? i - 1 : 0) * M;
    D1[r] = INFINITY;
    D2[r] = INFINITY;
    acc[r] = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) w[r][q] = (live[r] && q < M) ? xr[r][q] : 0.f;
  }
  for (int s = 2; s <= N + M; ++s) {
    // row i-1 of this lane's first row: the previous lane's last row (row 0 = the boundary:
    // cost[0][0] = 0 on diagonal 0, cost[0][j > 0] = inf)
    float up0 = wave_shr1(D1[R - 1]), diag0 = wave_shr1(D2[R - 1]);
    if (lane == 0) {
      up0 = INFINITY;
      diag0 = s == 2 ? 0.f : INFINITY;
    }
    float nv[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = lane * R + r + 1, j = s - i;
      const float c0 = r == 0 ? diag0 : D2[r - 1], c1 = r == 0 ? up0 : D1[r - 1], c2 = D1[r];
      nv[r] = INFINITY;
      if (live[r] && j >= 1 && j <= M) {
        float c;
        uint32_t t;
        if (c0 < c1 && c0 < c2) { c = c0; t = 0; }
        else if (c1 < c0 && c1 < c2) { c = c1; t = 1; }
        else { c = c2; t = 2; }
        nv[r] = w[r][0] + c;
#pragma unroll
        for (int q = 0; q < 7; ++q) w[r][q] = w[r][q + 1];
        w[r][7] = (j - 1 + 8 < M) ? xr[r][j - 1 + 8] : 0.f;
        acc[r] |= t << (2 * ((j - 1) & 15));
        if (((j - 1) & 15) == 15 || j == M) {
          tr[(i - 1) * DTW_WPR + ((j - 1) >> 4)] = acc[r];
          acc[r] = 0;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      D2[r] = D1[r];
      D1[r] = nv[r];
    }
  }
  __syncthreads();
  if (lane == 0) {
    // backtrace from (N, M) (trace[0][:] = 2, trace[:][0] = 1).  Path point k = (ii - 1, jj - 1);
    // walked forward (k descending) a token time is emitted where the row index changes (from
    // 0 before the first point), so point k is emitted iff its row differs from point k+1's.
    int ii = N, jj = M, ne = 0, pv = 0, pj = 0;
    bool have = false;
    int wr = -1, wc = -1;
    uint32_t word = 0;
    while (ii > 0 || jj > 0) {
      const int vi = ii - 1, vj = jj - 1;
      if (have && pv != vi) em[ne++] = 2 * pj + seek;
      pv = vi;
      pj = vj;
      have = true;
      int t;
      if (ii == 0) t = 2;
      else if (jj == 0) t = 1;
      else {
        const int r = ii - 1, c = (jj - 1) >> 4;
        if (r != wr || c != wc) {
          word = tr[r * DTW_WPR + c];
          wr = r;
          wc = c;
        }
        t = (word >> (2 * ((jj - 1) & 15))) & 3;
      }
      if (t == 0) { --ii; --jj; }
      else if (t == 1) --ii;
      else --jj;
    }
    if (have && pv != 0) em[ne++] = 2 * pj + seek;
    s_ne = ne;
    *n_times = ne;
  }
  __syncthreads();
  const int ne = s_ne;
  for (int k = lane; k < ne; k += 64) times[k] = em[ne - 1 - k];
}

static void launch_dtw_dp(const float* x, int rows, int M, int seek, int* times, int* n_times, hipStream_t s) {
  static const bool old = env_on("WDR_DTW_DP_OLD", false);   // A/B
  if (old) {
    WDR_KLAUNCH(k_dtw_dp, dim3(1), dim3(256), 0, s, x, rows, M, seek, times, n_times);
    return;
  }
  // WDR_DTW_WAVE_MAX = the most rows per lane the one-wave form takes (default 1: it serialises
  // a lane's rows, so above 64 rows the 256-thread form is faster; tools/dtw_bench)
  static const int rmax = env_int("WDR_DTW_WAVE_MAX", 1);
  const int R = (rows + 63) / 64;
  if (R > rmax) {
    WDR_KLAUNCH(k_dtw_dp, dim3(1), dim3(256), 0, s, x, rows, M, seek, times, n_times);
    return;
  }
  switch (R) {
    case 1: WDR_KLAUNCH(k_dtw_dp_wave<1>, dim3(1), dim3(64), 0, s, x, rows, M, seek, times, n_times); break;
    case 2: WDR_KLAUNCH(k_dtw_dp_wave<2>, dim3(1), dim3(64), 0, s, x, rows, M, seek, times, n_times); break;
    case 3: WDR_KLAUNCH(k_dtw_dp_wave<3>, dim3(1), dim3(64), 0, s, x, rows, M, seek, times, n_times); break;
    default: WDR_KLAUNCH(k_dtw_dp_wave<4>, dim3(1), dim3(64), 0, s, x, rows, M, seek, times, n_times); break;
  }
}

void launch_dtw(const float* cap, int A, int N_tok, int Tk, int n_audio, int sot_len, int seek, float* nrm, float* x,
                int* times, int* n_times, hipStream_t s) {
  const int M = n_audio;
  const int rows = N_tok - sot_len - 1;
  WDR_CHECK(rows >= 1 && rows <= DTW_NMAX, "DTW: token count out of range");
  WDR_CHECK(M >= 1 && M <= 1500, "DTW: frame count out of range");
  WDR_KLAUNCH(k_dtw_norm, dim3(cdiv(A * M, 256)), dim3(256), 0, s, cap, A, N_tok, Tk, M, nrm);
  WDR_KLAUNCH(k_dtw_medmean, dim3(cdiv(rows * M, 256)), dim3(256), 0, s, nrm, A, N_tok, M, sot_len, x);
  launch_dtw_dp(x, rows, M, seek, times, n_times, s);
  WDR_HIP(hipGetLastError());
}

void launch_dtw_dp_only(const float* x, int rows, int M, int seek, int* times, int* n_times, hipStream_t s) {
  WDR_CHECK(rows >= 1 && rows <= DTW_NMAX && M >= 1 && M <= 1500, "DTW: shape out of range");
  launch_dtw_dp(x, rows, M, seek, times, n_times, s);
  WDR_HIP(hipGetLastError());
}

}  // namespace wdr

namespace wdr {
// A launch that only instantiates its stream's hardware queue (Context: WDR_PRIME_POOLS):
// `iters` dependent FMAs per lane, nothing read, a store that never happens for finite inputs.
__global__ __launch_bounds__(256) void k_busy(int iters, float* sink) {
  float x = (float)threadIdx.x * 1e-3f;
  for (int i = 0; i < iters; ++i) x = fmaf(x, 0.999f, 1e-4f);
  if (x != x && threadIdx.x == 0) sink[blockIdx.x] = x;
}
void launch_busy(int blocks, int iters, float* sink, hipStream_t s) {
  WDR_KLAUNCH(k_busy, dim3(blocks), dim3(256), 0, s, iters, sink);
  WDR_HIP(hipGetLastError());
}
}  // namespace wdr
