/*
 * wdr.h — C ABI of libwdr, the MI355X-native drop-in for the hot path of
 * tmoroney/whisper-diarize-rs (Engine::transcribe_audio and the five seam calls it
 * makes).
 *
 * Everything is extern "C", plain pointers and sizes; no C++ exceptions cross it.
 * Status convention: int return 0 = ok, < 0 = error; the message is kept per thread
 * and returned by wdr_last_error() (the Rust shim maps it to eyre::Report).
 *
 * Option<T> encoding: Option<bool> -> int8_t (-1 None, 0 false, 1 true);
 * Option<i32/usize/f32/f64> -> value + int8_t has_ flag; Option<String> -> nullable
 * NUL-terminated UTF-8.
 *
 * Reference interface each entry point replaces (file:line in the reference crate):
 *   wdr_engine_new / wdr_engine_free     Engine::new                      src/engine.rs:58-63
 *   wdr_transcribe_audio                 Engine::transcribe_audio         src/engine.rs:65-200
 *   wdr_read_wav                         audio::read_wav                  src/audio.rs:4-24
 *   wdr_vad_get_segments                 vad::get_segments                src/vad.rs:6-85
 *   wdr_vad_merge                        (the crate's own merge, src/vad.rs:33-84)
 *   wdr_context_create / _free           transcribe::create_context       src/transcribe.rs:89-166
 *   wdr_run_pipeline                     transcribe::run_transcription_pipeline src/transcribe.rs:323-535
 *   wdr_segment_list_free                (drop of Vec<Segment>)
 * Not in the reference (additive, opt-in; the reference reads 16 kHz mono 16-bit WAV only):
 *   wdr_audio_info                       header of any supported WAV (host only)
 *   wdr_read_audio                       any supported WAV -> 16 kHz mono int16, converted on the GPU
 *   wdr_engine_set_audio_convert         wdr_transcribe_audio reads its file through wdr_read_audio
 *   wdr_read_audio_channels              any supported WAV -> 16 kHz int16 per channel (planar), on the GPU
 *   wdr_engine_set_channel_split         wdr_transcribe_audio transcribes every channel on its own,
 *                                        speaker = channel
 *   wdr_transcribe_batch / wdr_batch_free many files in one call, each equal to its wdr_transcribe_audio
 *   wdr_run_pipeline_groups              several recordings' segments in one pipeline run (segment groups)
 *   wdr_vad_probs_batch                  wdr_vad_probs of several recordings in one pass
 *   wdr_diarize_frame_classes_batch      wdr_diarize_frame_classes of several recordings in shared forwards
 *   wdr_run_pipeline_groups_diarize      segment groups with speakers: an EmbeddingManager per group
 *   wdr_engine_set_batch_diarize         wdr_transcribe_batch takes enable_diarize, each file as its single call
 * The wdr_dbg_* functions are kernel-level test seams (parity tests call them).
 */
#ifndef WDR_H
#define WDR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WDR_ABI_VERSION 6

typedef struct wdr_engine wdr_engine;
typedef struct wdr_context wdr_context;   /* ~ whisper_rs::WhisperContext (+ its state) */

/* EngineConfig, src/engine.rs:9-18 */
typedef struct {
  const char* cache_dir;                  /* PathBuf; default "./cache" */
  int8_t enable_dtw;                      /* Option<bool>, default Some(true) */
  int8_t enable_flash_attn;               /* Option<bool>, default Some(false) */
  int8_t use_gpu;                         /* Option<bool>, default Some(true) */
  int8_t has_gpu_device;
  int32_t gpu_device;                     /* Option<i32> */
  const char* vad_model_path;             /* Option<String> */
  const char* diarize_segment_model_path; /* Option<String> */
  const char* diarize_embedding_model_path; /* Option<String> */
} wdr_engine_config;

/* AdvancedTranscribe, src/types.rs:16-24 */
typedef struct {
  const char* sampling_strategy;          /* "beam_search" | "greedy" | NULL */
  int8_t has_best_of_or_beam_size; int32_t best_of_or_beam_size;
  int8_t has_n_threads; int32_t n_threads;
  int8_t has_temperature; float temperature;
  int8_t has_max_text_ctx; int32_t max_text_ctx;
  const char* init_prompt;
  int8_t has_diarize_threshold; float diarize_threshold;
} wdr_advanced;

/* TranscribeOptions, src/types.rs:28-45 */
typedef struct {
  int8_t has_offset; double offset;       /* default Some(0.0) */
  const char* model;                      /* default "base" */
  const char* lang;                       /* default Some("auto") */
  int8_t whisper_to_english;              /* default Some(false) */
  const char* translate_target;           /* network translation: out of scope (error if set) */
  int8_t enable_vad;                      /* default Some(true) */
  int8_t enable_diarize;                  /* default None */
  int8_t has_max_speakers; uint64_t max_speakers;
  const wdr_advanced* advanced;           /* nullable */
} wdr_transcribe_options;

/* DiarizeOptions, src/types.rs:93-98: built by Engine::transcribe_audio (src/engine.rs:101-111) and
 * passed to run_transcription_pipeline, whose speaker embeddings + assignment it switches on
 * (src/transcribe.rs:339-345).  A NULL model path selects synthetic seeded weights (no model
 * files exist offline); a non-NULL path is loaded or the call fails. */
typedef struct {
  const char* segment_model_path;         /* String (segmentation-3.0.onnx) */
  const char* embedding_model_path;       /* String (wespeaker_en_voxceleb_CAM++.onnx) */
  float threshold;                        /* f32, the Engine's default 0.5 */
  uint64_t max_speakers;                  /* usize, the Engine maps None / Some(0) to usize::MAX */
} wdr_diarize_options;

/* Synthetic-weights / workload knobs (no checkpoints on this machine).
 * Not part of the reference API; NULL everywhere means defaults. */
typedef struct {
  double weight_std;                      /* default 0.02 */
  double emb_std;                         /* default 0.02 */
  float force_len_rate;                   /* >0: pin decode length (tokens per audio second) */
  int8_t disable_fallback;                /* 1: logprob/entropy fallback thresholds off */
} wdr_synthetic;

/* FormattingOverrides, src/formatting.rs:37-51 (every field optional; Option<bool> as -1/0/1) */
typedef struct {
  int8_t has_max_chars_per_line; uint64_t max_chars_per_line;
  int8_t has_max_lines; uint64_t max_lines;
  int8_t has_cps_cap; double cps_cap;
  int8_t has_split_gap_sec; double split_gap_sec;
  int8_t has_comma_min_chars_before_allow; uint64_t comma_min_chars_before_allow;
  int8_t has_min_word_dur; double min_word_dur;
  int8_t has_min_sub_dur; double min_sub_dur;
  int8_t has_max_sub_dur; double max_sub_dur;
  int8_t has_soft_max_words_per_line; uint64_t soft_max_words_per_line;
  int8_t insert_interword_space;
  int8_t use_grapheme_len;
  int8_t enforce_kinsoku;
  int8_t allow_comma_split;
} wdr_formatting_overrides;

/* WordTimestamp, src/types.rs:64-70 */
typedef struct {
  const char* text;
  double start, end;
  int8_t has_probability; float probability;
} wdr_word;

/* Segment, src/types.rs:74-82 */
typedef struct {
  double start, end;
  const char* text;
  const wdr_word* words; size_t n_words;  /* words == NULL <-> None */
  const char* speaker_id;                 /* NULL <-> None */
} wdr_segment;

typedef struct {
  wdr_segment* segments; size_t n_segments;
  const char* detected_lang;              /* Option<String> (run_transcription_pipeline's second result) */
  const int64_t* speech_index;            /* wdr_run_pipeline only: index of the input SpeechSegment each
                                             segment came from (NULL elsewhere); not in the Rust API */
} wdr_segment_list;

/* SpeechSegment, src/types.rs:86-90 (samples borrowed) */
typedef struct {
  double start, end;
  const int16_t* samples; size_t n_samples;
} wdr_speech_segment;

/* Callbacks, src/engine.rs:35-40 + src/types.rs:12-13; all fire on the calling thread */
typedef struct {
  void* user;
  void (*progress)(void* user, int32_t pct, int32_t type /*0 Download,1 Transcribe,2 Translate*/, const char* label);
  void (*new_segment)(void* user, const wdr_segment* seg);   /* borrowed for the callback only */
  int (*is_cancelled)(void* user);
} wdr_callbacks;

/* per-stage wall-clock accounting of the last run (seconds) */
typedef struct {
  double mel, encode, decode, dtw, vad, total;
  int64_t windows, decode_steps, prefills;
  double lang, prompt_gpu, embed;   /* language detect wall, prompt-prefill GPU time, speaker embeddings */
  /* multi-chain decoding (wdr_context_set_chains): chains used, batched steps launched and
   * the rows they carried, segments re-decoded by the prompt fix-up / the sampled-tail
   * replay, wall time of the speculative and the fix-up phases */
  int64_t chains, batch_launches, batch_rows, fixup_segments, replay_segments;
  double spec_s, fixup_s;
  double batch_step_s;   /* wall of the batched steps (submit -> tokens on the host), summed */
  int64_t early_fixup_segments;   /* of fixup_segments: re-decoded by the early fix-up */
  /* ABI 3: what the batched launches carried besides decode rows -- prompt-prefill rows and DTW
   * re-forward rows (and how many of each), launches holding any (eager), and the cross-K/V
   * reads: one-row / beam groups (VALU kernel) and MFMA row tiles, each one slot per layer */
  int64_t batch_prefill_rows, batch_dtw_rows, batch_prefills, batch_dtws, batch_mixed;
  int64_t batch_xattn_groups, batch_xattn_tiles;
  /* ABI 4: the DTW queue (multi-chain runs: every chain's DTW re-forwards batched off the decode
   * chain) -- passes launched, the rows they carried, windows queued */
  int64_t dtwq_passes, dtwq_rows, dtwq_jobs;
  /* ABI 5: language-detection decoder passes (lang "auto": one per encode-ahead batch, its
   * windows as one-row groups; or one SOT prefill per on-demand segment) and their rows.  A
   * multi-chain run keeps the encode-ahead pass for a plan's first batch only (WDR_LANG_PIGGYBACK,
   * default 1): later segments' detection rows ride in the batched steps and are counted there */
  int64_t lang_passes, lang_rows;
} wdr_stage_times;

const char* wdr_last_error(void);
int wdr_abi_version(void);
int wdr_device_count(void);
/* ABI 5: releases every handle the caller has not freed (engines, contexts with their worker
 * threads, VADs, diarizers, speaker managers) and the process-wide stream pools / profiler
 * buffers, while the HIP runtime is still up.  Registered with atexit() when the first handle is
 * created; a host may call it earlier.  Freeing a handle it released is a no-op.  A handle that
 * an entry point is still using on another thread (a call in flight) is not released; every entry
 * point rejects a released handle with an error, and a released handle's address is never
 * reused by a later one. */
void wdr_shutdown(void);

/* ---- Engine (whole-call drop-in) ---- */
int wdr_engine_new(const wdr_engine_config* cfg, wdr_engine** out);
void wdr_engine_free(wdr_engine* e);
/* Synthetic mode (an explicit opt-in): models the Engine cannot find on disk (ggml-<model>.bin in
 * the cache, the VAD / diarization model files) run on synthetic seeded weights.  Without it a
 * missing whisper model fails with "whisper file doesn't exist" as the reference does
 * (src/transcribe.rs:99-101), and a missing VAD / diarization model fails likewise. */
int wdr_engine_set_synthetic(wdr_engine* e, const wdr_synthetic* syn);
/* Audio conversion (an explicit opt-in).  1 = wdr_transcribe_audio reads its file through
 * wdr_read_audio (on the engine's device): PCM 8 / 16 / 24 / 32-bit or IEEE f32, 1..8 channels,
 * 1000..384000 Hz, downmixed and resampled to 16 kHz mono on the GPU.  0 (default) = the
 * reference's read_wav and its errors.  Not in the Rust API. */
int wdr_engine_set_audio_convert(wdr_engine* e, int8_t on);
/* Channel split (an explicit opt-in, for recordings with one party per channel).  1 =
 * wdr_transcribe_audio reads its file through wdr_read_audio_channels and transcribes every
 * channel on its own, speaker = channel.  0 (default) = today's behaviour.  Independent of
 * wdr_engine_set_audio_convert.  Not in the Rust API.
 * Channel c = 0 .. C-1, in order, is treated as a mono file of that channel: segmented by VAD
 * when enable_vad is 1 (else one segment), one pipeline run of its own (prompt chain, RNG reset,
 * overlap clip, language detection), process_segments with its own VAD mask and its language's
 * preset.  Every segment gets speaker_id = the decimal string of c + 1; the lists are merged by a
 * stable sort on start (ties: lower channel first) and are not clipped against each other.
 * detected_lang is that of the lowest channel that has one.  new_segment fires in channel order
 * (not time order) with the channel's speaker_id; progress reports (c * 100 + pct) / C; a
 * cancelled run ends the call as a cancelled single run ends, and no further channel starts.
 * enable_diarize == 1 fails with "channel split labels speakers by channel: enable_diarize must
 * not be set" before the file is read. */
int wdr_engine_set_channel_split(wdr_engine* e, int8_t on);
/* Diarized batches (an explicit opt-in).  0 (default) = wdr_transcribe_batch refuses enable_diarize
 * == 1 with the message given there.  1 = it takes it, and (*out)[i].list equals
 * wdr_transcribe_audio of file i with the same options -- segments, words, times, speaker ids
 * ("1", "2", .. starting afresh in every file) and detected_lang.  The order of work: both
 * diarization model paths are resolved as the single call resolves them (a failure fails the
 * whole call with its message); every file is read (read errors go on the item); the segmentation
 * windows of all readable files run through shared forwards (wdr_diarize_frame_classes_batch) and
 * are stitched per file; one wdr_run_pipeline_groups_diarize run with a group per file;
 * process_segments per file without a VAD mask.  enable_vad is ignored when diarizing, as in the
 * single call; audio convert composes as without diarization.  With channel split on,
 * enable_diarize == 1 fails before any file is read with the single call's "channel split labels
 * speakers by channel: enable_diarize must not be set".  Not in the Rust API. */
int wdr_engine_set_batch_diarize(wdr_engine* e, int8_t on);
int wdr_transcribe_audio(wdr_engine* e, const char* audio_path, const wdr_transcribe_options* opts,
                         const wdr_formatting_overrides* fmt, const wdr_callbacks* cb, wdr_segment_list** out);
/* Batch transcription (additive, not in the Rust API): n_files recordings in one call, so that
 * short files share the decode chains and the VAD scans run side by side.  (*out)[i].list equals
 * what wdr_transcribe_audio(e, audio_paths[i], opts, fmt, ..) returns on the same engine (segments,
 * words, times, speaker ids, detected_lang) in every engine mode (read_wav, audio convert, channel
 * split; with and without enable_vad): every file -- every channel under channel split -- is one
 * segment group of a single wdr_run_pipeline_groups call.
 * A file that cannot be read gets (*out)[i].error = the message the single call gives
 * ("audio file doesn't exist", the header errors, ..) and list == NULL; the other files are
 * unaffected.  Model not found, translate_target, cancellation and GPU errors fail the whole call
 * as they fail wdr_transcribe_audio.  enable_diarize == 1 fails before any file is read: "batch
 * transcription does not diarize: enable_diarize must not be set" (unless the engine opted in:
 * wdr_engine_set_batch_diarize).  n_files == 0 succeeds with
 * *out == NULL.  new_segment fires in (file, channel, segment) order on the calling thread with
 * the file's index; progress reports finished speech segments over all files.
 * Free *out with wdr_batch_free. */
typedef struct {
  wdr_segment_list* list;                 /* exactly one of list / error is non-NULL */
  const char* error;
} wdr_batch_item;
typedef struct {
  void* user;
  void (*progress)(void* user, int32_t pct, int32_t type, const char* label);
  void (*new_segment)(void* user, size_t file_index, const wdr_segment* seg);
  int (*is_cancelled)(void* user);
} wdr_batch_callbacks;
int wdr_transcribe_batch(wdr_engine* e, const char* const* audio_paths, size_t n_files,
                         const wdr_transcribe_options* opts, const wdr_formatting_overrides* fmt,
                         const wdr_batch_callbacks* cb, wdr_batch_item** out /* [n_files] */);
void wdr_batch_free(wdr_batch_item* items, size_t n_files);
/* stage accounting of the engine's context of `model` (NULL = "base"), as wdr_context_stage_times
 * reports a context's; an error before the engine's first call with that model.
 * wdr_transcribe_batch starts the multi-chain figures (chains, batch_*, fixup_*) afresh */
int wdr_engine_stage_times(wdr_engine* e, const char* model, wdr_stage_times* out);

/* ---- seams ---- */
int wdr_read_wav(const char* path, int16_t** samples, size_t* n);
/* host only: info[5] = {fmt (0 u8, 1 i16, 2 i24, 3 i32, 4 f32), channels, rate, bits, block_align} of a
 * RIFF/WAVE file with format tag 1 (PCM), 3 (IEEE float) or 0xFFFE (extensible, either of them);
 * n_frames = whole frames of its data chunk.  A data size of 0xFFFFFFFF, or past the end of the
 * file, means "to the end of the file" (piped writers); so does a size of 0, unless the rest of the
 * file is empty or a run of whole chunks (LIST ...), in which case the data chunk is empty.  Bytes
 * after an unsized data chunk are all taken as samples, trailing chunks included */
int wdr_audio_info(const char* path, int32_t* info, uint64_t* n_frames);
/* any supported WAV -> 16 kHz mono int16 (free with wdr_free): decode, downmix (mean of the
 * channels) and a zero-phase polyphase Kaiser-sinc resampler, all on the GPU in bounded chunks;
 * sample k of the result sits at k / 16000 s of the file.  A file that wdr_read_wav accepts comes
 * back identical to wdr_read_wav's result, without touching the GPU */
int wdr_read_audio(const char* path, int8_t has_gpu_device, int32_t gpu_device, int16_t** samples, size_t* n);
/* any supported WAV -> 16 kHz int16 per channel, planar: (*samples)[c * *n_per_channel + k];
 * free with wdr_free.  Channel c equals wdr_read_audio of the mono file holding channel c.  A
 * 16 kHz mono 16-bit file comes back as it is, without touching the GPU */
int wdr_read_audio_channels(const char* path, int8_t has_gpu_device, int32_t gpu_device,
                            int16_t** samples, size_t* n_per_channel, int32_t* channels);
/* test seam (host only, no GPU): parse a VAD / diarization model file the way the models load
 * it -- kind 0 whisper.cpp Silero ggml, 1 segmentation-3.0 ONNX, 2 CAM++ ONNX -- and return its
 * tensors under the oracle's names: names_out "name:count\n" per tensor (sorted), data_out the
 * values concatenated in that order.  Free both with wdr_free. */
int wdr_dbg_model_file(int32_t kind, const char* path, char** names_out, float** data_out, size_t* n_values);
/* formatting::process_segments (src/formatting.rs:240-313) with PostProcessConfig::for_language(lang)
 * + overrides (nullable), and a VadMaskOracle over vad_mask (2 doubles per interval) when
 * has_mask (src/engine.rs:192-199).  Free the result with wdr_segment_list_free. */
int wdr_process_segments(const wdr_segment* segs, size_t n_segs, const char* lang, const wdr_formatting_overrides* ov,
                         int8_t has_mask, const double* vad_mask, size_t n_mask, wdr_segment_list** out);
void wdr_free(void* p);
int wdr_vad_merge(const double* starts_cs, const double* ends_cs, size_t n_segs, const int16_t* samples,
                  size_t n_samples, double* mask_out /* [2*n_segs] */, size_t* n_mask,
                  double* merged_out /* [2*n_segs] start,end seconds */, int64_t* merged_idx /* [2*n_segs] */,
                  size_t* n_merged);
/* Silero VAD (src/vad.rs:6-85; whisper.cpp WhisperVadContext + segments_from_samples).
 * model_path: whisper.cpp's ggml-silero-v5.1.2.bin (loaded, or the call fails); NULL selects
 * synthetic seeded weights. */
typedef struct wdr_vad wdr_vad;
int wdr_vad_create(const char* model_path, int8_t has_gpu_device, int32_t gpu_device, wdr_vad** out);
void wdr_vad_free(wdr_vad* v);
/* one probability per 512-sample chunk: probs_out[ceil(n/512)]; us_per_step (nullable) = GPU
 * time of the forward per chunk (the LSTM scan dominates) */
int wdr_vad_probs(wdr_vad* v, const int16_t* samples, size_t n, float* probs_out, double* us_per_step);
/* B independent sequences in one pass (one upload, three launches, one sync; the LSTM scans run
 * one workgroup per sequence): probs_out holds ceil(n[b] / 512) values per sequence, back to back,
 * bit-identical to wdr_vad_probs of each.  n[b] == 0 is legal (samples[b] is not read) */
int wdr_vad_probs_batch(wdr_vad* v, const int16_t* const* samples, const size_t* n, int32_t B,
                        float* probs_out, double* us_per_step);
/* GPU time of the last forward per 512-sample chunk (microseconds) */
int wdr_vad_stats(wdr_vad* v, double* us_per_chunk);
/* whisper.cpp whisper_vad_segments_from_probs with the reference's params (min silence 100 ms):
 * cs_out[2*k] = start_cs, [2*k+1] = end_cs; capacity 2*n_probs */
int wdr_vad_segments_from_probs(const float* probs, size_t n_probs, float* cs_out, size_t* n_out);
/* vad::get_segments: raw mask (seconds, 2 per entry) + merged speech segments whose samples
 * point into `samples` (borrowed).  Free both arrays with wdr_free. */
int wdr_vad_get_segments(wdr_vad* v, const int16_t* samples, size_t n, double** mask_out, size_t* n_mask,
                         wdr_speech_segment** segs_out, size_t* n_segs);

/* pyannote diarization (src/engine.rs:89-122, src/transcribe.rs:339-345, 461-497):
 * segmentation-3.0 + get_segments stitching, Kaldi fbank + CMN, CAM++ embedding.
 * Paths: the ONNX files (segmentation-3.0.onnx, wespeaker_en_voxceleb_CAM++.onnx), whose
 * initializers are read by libwdr's own protobuf reader (loaded, or the call fails); NULL selects
 * synthetic seeded weights for that model. */
typedef struct wdr_diarizer wdr_diarizer;
int wdr_diarizer_create(const char* segment_model_path, const char* embedding_model_path, int8_t has_gpu_device,
                        int32_t gpu_device, wdr_diarizer** out);
void wdr_diarizer_free(wdr_diarizer* d);
/* per-frame argmax class of every 10-s window of the zero-padded input (pyannote-rs
 * find_max_index: last max): cls_out[n_windows * 589], n_windows = n / 160000 + 1;
 * logprobs_out (nullable) [n_windows][589][7] */
int wdr_diarize_frame_classes(wdr_diarizer* d, const int16_t* samples, size_t n, int32_t* cls_out, float* logprobs_out);
/* the same for B recordings at once: file b contributes the n[b] / 160000 + 1 windows of its own
 * zero-padded buffer, the windows are stacked in (file, window) order and run through forwards of
 * up to window_cap windows each (0 = the default, 128; larger values mean 128), so a forward may
 * start or end inside a file.  cls_out / logprobs_out (nullable) hold the per-file results back to
 * back, every window bit-identical to wdr_diarize_frame_classes of its file alone.  n[b] == 0 is
 * legal: one all-zero window, samples[b] is not read.  B <= 0, a NULL samples[b] with n[b] > 0 or
 * window_cap < 0 is an error before anything is launched */
int wdr_diarize_frame_classes_batch(wdr_diarizer* d, const int16_t* const* samples, const size_t* n, int32_t B,
                                    int32_t window_cap, int32_t* cls_out, float* logprobs_out);
/* pyannote_rs::get_segments: one allocation holding the segments and copies of their samples
 * (slices of the zero-padded buffer); free with wdr_free(*segs_out) */
int wdr_diarize_get_segments(wdr_diarizer* d, const int16_t* samples, size_t n, wdr_speech_segment** segs_out,
                             size_t* n_segs);
/* the same stitching from frame classes computed elsewhere (e.g. window shards on several GPUs):
 * cls [n / 160000 + 1][589] of the n-sample file; free with wdr_free(*segs_out) */
int wdr_diarize_segments_from_classes(const int32_t* cls, size_t n_windows, const int16_t* samples, size_t n,
                                      wdr_speech_segment** segs_out, size_t* n_segs);
/* EmbeddingExtractor::compute pieces: features after CMN [T][80] (capacity n/160 + 1 rows), and
 * the 512-d embedding; ok = 0 where the reference's ONNX call fails (fewer than 400 samples) */
int wdr_diarize_fbank(wdr_diarizer* d, const int16_t* samples, size_t n, float* feats_out, size_t* n_frames);
int wdr_diarize_embedding(wdr_diarizer* d, const int16_t* samples, size_t n, float* emb_out, int8_t* ok);
/* B utterances in one batched CAM++ forward (what the pipeline's embedding worker runs):
 * emb_out [B][512], ok[b] as wdr_diarize_embedding's; bit-identical per utterance to it */
int wdr_diarize_embedding_batch(wdr_diarizer* d, const int16_t* const* samples, const size_t* n, int32_t B,
                                float* emb_out, int8_t* ok);
/* GPU time of the last segmentation / embedding call (ms) */
int wdr_diarize_stats(wdr_diarizer* d, double* seg_ms, double* emb_ms);
/* EmbeddingManager + the reference's choice of get_best_speaker_match / search_speaker
 * (src/transcribe.rs:478-497); emb NULL -> "?" (embedding error) */
typedef struct wdr_speakers wdr_speakers;
int wdr_speakers_new(int8_t has_max_speakers, uint64_t max_speakers, wdr_speakers** out);
void wdr_speakers_free(wdr_speakers* m);
int wdr_speakers_assign(wdr_speakers* m, const float* emb, int32_t dim, float threshold, char* id_out, size_t cap);

/* model_path: a whisper.cpp ggml file (missing -> "whisper file doesn't exist").  NULL model_path
 * with a non-NULL syn selects synthetic seeded weights of the named configuration; NULL with
 * NULL syn fails like a missing file. */
int wdr_context_create(const char* model_path, const char* model_name, int8_t has_gpu_device, int32_t gpu_device,
                       int8_t use_gpu, int8_t enable_dtw, int8_t enable_flash_attn, int8_t has_num_samples,
                       uint64_t num_samples, const wdr_synthetic* syn, wdr_context** out);
void wdr_context_free(wdr_context* c);
/* parse a whisper.cpp ggml model file without loading it (no GPU): hparams[11] = n_vocab,
 * n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer, n_text_ctx, n_text_state, n_text_head,
 * n_text_layer, n_mels, ftype; wdr_context_create loads such a file when model_path is given */
int wdr_ggml_info(const char* path, int32_t* hparams, int64_t* n_tensors, int64_t* n_vocab_tokens);
/* Tensor types of such a file (no GPU): counts[16], the number of tensors per ggml type id.  The
 * loader reads 0 f32, 1 f16 and the block-quantized 2 q4_0, 3 q4_1, 6 q5_0, 7 q5_1, 8 q8_0 (the
 * files of whisper.cpp's quantize tool; ftype = base + 1000 * qnt_version); other ids fail. */
int wdr_ggml_tensor_types(const char* path, int64_t* counts /* [16] */);
/* one tensor of such a file as f16 bits (no GPU), quantized types through the host definition:
 * float(d) * q (+ float(m)) in f32, rounded once to f16.  Free *out with wdr_free. */
int wdr_ggml_tensor_f16(const char* path, const char* name, uint16_t** out, size_t* n);
/* diarize: NULL = no speakers (the reference's `None`); else speaker embeddings of every speech
 * segment + EmbeddingManager assignment per whisper segment */
int wdr_run_pipeline(wdr_context* c, const wdr_speech_segment* segs, size_t n_segs, const wdr_transcribe_options* opts,
                     const wdr_diarize_options* diarize, const wdr_synthetic* syn, const wdr_callbacks* cb,
                     wdr_segment_list** out);
/* run_pipeline without the cross-segment overlap clip and without speaker assignment, with
 * speech_index set: building block of the multi-GPU one-file path (wdr/distributed.py), which
 * applies both over the merged, ordered blocks of every GPU */
int wdr_run_pipeline_raw(wdr_context* c, const wdr_speech_segment* segs, size_t n_segs,
                         const wdr_transcribe_options* opts, const wdr_synthetic* syn, wdr_segment_list** out);
/* run_pipeline_raw continuing decoder 0's random-number stream (the multi-GPU one-file path,
 * wdr/distributed.py: a GPU's block of the file starts from the RNG state the blocks before it
 * left, as the reference's one state would, src/transcribe.rs:335): rng_in (NULL = the fresh
 * state's) and rng_out (malloc'd; free with wdr_free) are decoder 0's std::mt19937 state as
 * text; sampled_out[n_segs] = 1 where a segment drew random numbers (t > 0 decoders) */
int wdr_run_pipeline_block(wdr_context* c, const wdr_speech_segment* segs, size_t n_segs,
                           const wdr_transcribe_options* opts, const wdr_synthetic* syn, const char* rng_in,
                           int8_t* sampled_out, char** rng_out, wdr_segment_list** out);
/* Segment groups: group g is segs[group_start[g] .. group_start[g + 1]) (the last one ends at
 * n_segs) and comes out, as out[g], exactly as if it had been the whole input of its own
 * wdr_run_pipeline call without diarization -- prompt chain, decoder 0's random numbers, overlap
 * clip, detected language and speech_index all start afresh at a group start -- while the decode
 * chains are shared by all groups.  group_start is non-decreasing with
 * group_start[0] == 0 and every entry <= n_segs (else an error before any GPU work); an empty
 * group yields an empty list.  group_speaker (nullable, entries nullable): a fixed speaker_id for
 * group g's segments.  new_segment fires in (group, segment) order on the calling thread;
 * progress counts finished segments over all of them.  out: n_groups lists, each freed with
 * wdr_segment_list_free.  n_groups == 0 needs n_segs == 0 and does nothing.  Speaker embeddings
 * are per pipeline call, so more than one group with opts->enable_diarize == 1 is refused:
 * "segment groups do not diarize: more than one group with diarization on"
 * (wdr_run_pipeline_groups_diarize is the entry point that takes them). */
int wdr_run_pipeline_groups(wdr_context* c, const wdr_speech_segment* segs, size_t n_segs,
                            const size_t* group_start, size_t n_groups, const char* const* group_speaker,
                            const wdr_transcribe_options* opts, const wdr_synthetic* syn,
                            const wdr_callbacks* cb, wdr_segment_list** out /* [n_groups] */);
/* Segment groups with speakers: as wdr_run_pipeline_groups without group_speaker, and with
 * wdr_run_pipeline's explicit diarize argument -- NULL = no speakers; else group g's speaker ids
 * are exactly those of its own wdr_run_pipeline call with the same wdr_diarize_options: the
 * EmbeddingManager (max_speakers, threshold) starts afresh at a group's first segment, while one
 * embedding worker runs ahead over the segments of all groups (an embedding depends on its
 * segment's samples only, bit for bit) */
int wdr_run_pipeline_groups_diarize(wdr_context* c, const wdr_speech_segment* segs, size_t n_segs,
                                    const size_t* group_start, size_t n_groups, const wdr_transcribe_options* opts,
                                    const wdr_diarize_options* diarize, const wdr_synthetic* syn,
                                    const wdr_callbacks* cb, wdr_segment_list** out /* [n_groups] */);
void wdr_segment_list_free(wdr_segment_list* l);
/* decode chains of run_pipeline (greedy decoding): n States decode n contiguous blocks of the
 * speech segments concurrently, their greedy steps batched into one n-row step, with an exact
 * prompt-chain fix-up (results identical to one chain).  Default WDR_DECODE_CHAINS or 40,
 * capped by the context's KV pool (max chains fixed at creation).  Not in the Rust API. */
int wdr_context_set_chains(wdr_context* c, int32_t n);
/* GPUs the context runs on: gpu_device Some(d) -> 1 (device d); None -> every visible GPU (up to
 * 8; WDR_DEVICES="a,b,.." lists them), each holding the model, the decode chains spread over
 * them (chain k on GPU k % n) with the same exact prompt fix-up; device_ids (nullable) receives
 * the ordinals, at most `cap` */
int wdr_context_devices(const wdr_context* c, int32_t* n, int32_t* device_ids, int32_t cap);
/* fp8 encoder GEMMs (BASELINE configs[4]): the encoder's qkv / o / fc1 / fc2 projections on the
 * block-scaled fp8 MFMA with MX operands -- OCP e4m3 values, one E8M0 scale per 32 k (weights
 * quantised on first use, activations by the LayerNorm / GELU kernels that produce them);
 * attention, residuals, the cross-K/V projection and the decoder stay f16/f32.  Default off
 * (WDR_FP8_ENCODER=1 turns it on at creation).  Not in the Rust API. */
int wdr_context_set_encoder_fp8(wdr_context* c, int8_t on);
/* test seam: early prompt fix-up 0 off, 1 when the predecessor chain already finished, 2 always
 * (chain k waits for chain k-1 to finish, then redoes its first segments from the known prompt),
 * 3 (default) chain k waits only for chain k-1's speculative pass and redoes from the prompt it
 * left; -1 restores the WDR_EARLY_FIXUP environment default.  The fix-up rounds keep every mode
 * exact. */
int wdr_dbg_set_early_fixup(wdr_context* c, int32_t mode);
/* test seam: the diarization contractions on the f32 MFMA kernel (1, default) or the VALU f32
 * kernel (0) for every later launch in the process */
int wdr_dbg_set_gemm32(int32_t mfma);
/* test seam: the encoder GEMM dispatch plan of a projection of M > 64 rows (csrc/gemm_plan.h) --
 * what launch_proj (fp8 = 0) / launch_proj_fp8 (fp8 = 1) launches for the shape.  knobs null: the
 * process's WDR_GEMM* values; else int32[7] {WDR_GEMM1, WDR_GEMM4, WDR_GEMM4_GM, WDR_GEMM5,
 * WDR_GEMM5_WIDE, WDR_GEMM8N, WDR_GEMM_CUS} as the variables would be set.  plan_out[4] = {kernel
 * (0 k_gemm, 1 k_gemm2, 2 k_gemm4, 3 k_gemm5, 4 k_gemm8, 5 k_gemm8n), grid x, grid y, dynamic LDS
 * bytes}.  Host arithmetic only: never touches the GPU. */
int wdr_dbg_gemm_plan(int32_t fp8, int32_t M, int32_t N, int32_t K, int32_t epi, int32_t ldo, int32_t d,
                      int32_t gemm_ref, const int32_t* knobs, int32_t* plan_out /* [4] */);
/* test seams: stream placement (csrc/streams.h).  Host arithmetic only: neither touches the GPU.
 * wdr_dbg_cu_mask: the CU mask of a stream that leaves n_res of ncu CUs free under reservation
 * pattern pat (only_reserved: the complement), n_words = (ncu + 31) / 32 words; an impossible
 * request fails with the message the stream's creation would throw.
 * wdr_dbg_stream_plan: what stream a role (0 context, 1 step batcher, 2 DTW queue, 3 state's own,
 * 4 state's encode-ahead, 5 state's on-demand encodes, 6 state's DTW) gets on a device of ncu CUs.
 * knobs null: the process's environment; else int32[14] {WDR_ENC_POOL, WDR_ENC_MASK,
 * WDR_ENC_MASK_PAT, WDR_ENC_PRIO, WDR_OWN_POOL, WDR_OWN_MASK, WDR_OWN_PRIO, WDR_ODM_POOL,
 * WDR_ODM_MASK, WDR_BATCH_HWQ, WDR_DTWQ_HWQ, then whether WDR_ENC_POOL / WDR_ENC_MASK /
 * WDR_ODM_POOL is set at all}. */
typedef struct wdr_stream_plan {
  int32_t kind;      /* 0 no stream, 1 priority stream, 2 CU-masked, 3 CU-masked over every CU */
  int32_t prio;      /* kind 1: 0 lowest, 1 middle, 2 highest, 3 created without a priority */
  int32_t pool;      /* kind 2: streams in the shared pool, 0 = a stream of its own */
  int32_t n_words;   /* kinds 2, 3: mask words */
  uint32_t mask[16];
  char tag[32];      /* WDR_STREAM_LOG name at creation, "" = not logged there */
} wdr_stream_plan;
int wdr_dbg_cu_mask(int32_t ncu, int32_t n_res, int32_t pat, int32_t only_reserved, uint32_t* words_out,
                    int32_t n_words);
int wdr_dbg_stream_plan(int32_t role, int32_t ncu, const int32_t* knobs /* [14] or null */,
                        wdr_stream_plan* plan_out);
int wdr_context_stage_times(wdr_context* c, wdr_stage_times* out);
int wdr_context_hparams(wdr_context* c, int32_t* out /* [10] */);

/* ---- live kernel timing (HIP events on the launching stream) for bench.py's roofline:
 * class 1 = MFMA GEMM (encoder / prefill / DTW projections), 2 = decoder GEMV, 3 = flash attention,
 * 4 = decoder cross-attention.  Setting a class resets the counters. */
int wdr_prof_set(int32_t cls);
/* several classes at once: bit (1 << cls) per class; read each with wdr_prof_read_class */
int wdr_prof_set_mask(int32_t mask);
int wdr_prof_read_class(int32_t cls, double* total_ms, int64_t* launches, double* algo_bytes, double* algo_flops);
/* the same sampled launches timed by the kernels' own clock (first wave start -> last wave end,
 * wall_clock64; the span rocprofv3's dispatch timestamps measure) instead of HIP events, which
 * under multi-stream concurrency also absorb the launch's wait for the GPU */
int wdr_prof_read_clock(int32_t cls, double* total_ms, int64_t* launches, double* algo_bytes, double* algo_flops);
int wdr_prof_read(double* total_ms, int64_t* launches, double* algo_bytes, double* algo_flops);

/* ---- whisper_full-level test seam: one state.full() call, raw token data ---- */
typedef struct {
  int32_t id, tid;
  float p, plog, pt, ptsum;
  int64_t t0, t1, t_dtw;
} wdr_token;
typedef struct {
  int64_t t0, t1;
  const char* text;
  const wdr_token* tokens; size_t n_tokens;
} wdr_result_seg;
int wdr_state_full(wdr_context* c, const float* samples, size_t n, const wdr_transcribe_options* opts,
                   const wdr_synthetic* syn, const char* initial_prompt, wdr_result_seg** segs, size_t* n_segs,
                   int32_t* lang_id);
void wdr_result_free(wdr_result_seg* segs, size_t n);

/* ---- kernel-level test seams (host buffers in / out) ---- */
/* the normalised log-mel window at frame `seek`, f32: the double normalisation rounded to odd (within
 * one f32 ulp of the nearest f32), so that rounding it to f16 gives exactly the conv1 operand every
 * production encode stores (one double -> f16 rounding; wdr_dbg_im2col_mel) */
int wdr_dbg_log_mel(wdr_context* c, const float* x, size_t n, int32_t seek, float* window_out /* [n_mels][3000] */);
int wdr_dbg_energy(const float* x, size_t n, float* out);
/* the load-time dequantization kernel: n_blocks raw blocks of ggml type 2 / 3 / 6 / 7 / 8 ->
 * out_f16[32 * n_blocks] (f16 bits), bit-identical to wdr_ggml_tensor_f16's host definition; ms
 * (nullable): mean GPU time of 10 further back-to-back launches on the same buffers */
int wdr_dbg_dequant(int32_t type, const uint8_t* blocks, size_t n_blocks, uint16_t* out_f16, double* ms);
/* the audio conversion of n_frames raw interleaved frames held in memory (fmt / channels / rate as
 * wdr_audio_info reports them) -> 16 kHz mono int16 (free with wdr_free).  host = 1: the host
 * definition (no GPU); host = 0: the kernel path on the current device, bit-identical to it for
 * every chunk_frames (0 = default); ms (nullable, host = 0): mean GPU time of 10 further
 * back-to-back runs of the kernels on resident buffers */
int wdr_dbg_audio_convert(const uint8_t* raw, uint64_t n_frames, int32_t fmt, int32_t channels, int32_t rate,
                          uint64_t chunk_frames, int32_t host, int16_t** out, size_t* n_out, double* ms);
/* test seam, as wdr_dbg_audio_convert, of the channel-keeping conversion: planar
 * (*out)[c * *n_per_channel + k].  host = 1 the definition (channel c = the mono definition on
 * sample c of every frame), 0 the kernels (bit-identical for every chunk_frames); ms as there */
int wdr_dbg_audio_split(const uint8_t* raw, uint64_t n_frames, int32_t fmt, int32_t channels, int32_t rate,
                        uint64_t chunk_frames, int32_t host, int16_t** out, size_t* n_per_channel, double* ms);
/* host only: the resampler's coefficient table of a source rate: L = 16000 / g, M = rate / g
 * (g = gcd), T taps per output and tab[L][T] (free with wdr_free); rate 16000: T = 0 */
int wdr_dbg_resample_table(int32_t rate, int32_t* L, int32_t* M, int32_t* T, float** tab);
/* one v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3) on raw per-lane operands: a / b [64 lanes][32 B],
 * scale registers sa / sb [64] (op_sel 0), out [64 lanes][4] accumulators */
int wdr_dbg_mfma_scale(const uint8_t* a, const uint8_t* b, const int32_t* sa, const int32_t* sb, float* out);
int wdr_dbg_encode(wdr_context* c, const float* mel_window /* [n_mels][3000] */, float* enc_out /* [1500][d] */);
/* cross K/V of the last wdr_dbg_encode window: [1500][n_text_layer][2 (K, V)][d] (f16 -> f32) */
int wdr_dbg_cross_kv(wdr_context* c, float* out);
int wdr_dbg_decode(wdr_context* c, const int32_t* tokens, size_t n, float* logits_out /* [n_vocab] */);
/* prefill tokens[0..n-2], then one decode step of tokens[n-1] (its logits); the decoder-rows
 * contract makes them bit-identical to the n-token prefill's for n <= 8 (larger prefills run
 * their cross-attention on the MFMA tile kernel) */
int wdr_dbg_step(wdr_context* c, const int32_t* tokens, size_t n, float* logits_out /* [n_vocab] */);
/* whisper.cpp's logit rules + greedy pick (k_logits_process) on given logits
 * [R][n_vocab] (R <= 8); per row ctl[7] = {n_tokens, last_ts, pen_ts, has_ts, seek_delta, force_kind
 * (0 none, 1 only force_tok, 2 text only), force_tok} and a temperature; max_initial_ts /
 * suppress_blank as whisper_full_params.  Out: ids [R][2] = {id, tid}, f [R][5] = {p, log p, pt,
 * ptsum, no-speech probability} */
int wdr_dbg_logits(wdr_context* c, const float* logits, int32_t R, const int32_t* ctl, const float* temperature,
                   float max_initial_ts, int32_t suppress_blank, int32_t* ids_out, float* f_out);
/* multi-chain batched step (StepBatcher) with `rows` rows on the last encoded window, `iters`
 * times after prefilling tokens[0..n-2]: host milliseconds per step (probe seam) */
int wdr_dbg_batch_step(wdr_context* c, const int32_t* tokens, size_t n, int32_t rows, int32_t iters,
                       double* ms_per_step);
int wdr_dbg_capture(wdr_context* c, const int32_t* tokens, size_t n, float* cap_out /* [n_aheads][n][1500] */);
int wdr_dbg_dtw(const float* cap, int32_t n_heads, int32_t n_tok, int32_t n_audio, int32_t sot_len, int32_t seek,
                float* x_out /* [n_tok-sot_len-1][n_audio] */, int32_t* times_out, int32_t* n_times);
int wdr_dbg_discrete(const float* w, size_t n, uint32_t seed, int32_t n_draws, int32_t* out);
int wdr_dbg_dtw_dp(const float* x, int32_t rows, int32_t cols, int32_t seek, int32_t* times_out, int32_t* n_times);
/* fp8 (MX e4m3) encoder projection (BASELINE configs[4]): a [M][K] and w [N][K] quantised on the
 * GPU to e4m3 with one E8M0 scale per 32 k, the block-scaled fp8 MFMA GEMM, epilogue as
 * wdr_dbg_proj (7 = GELU written back as e4m3 + scales, returned dequantised); M > 64, N % 256,
 * K % 128.  The quantised bytes and the scale bytes ([rows][K/32], E8M0) are returned (nullable) */
int wdr_dbg_proj_fp8(const uint16_t* a_f16, const uint16_t* w_f16, const float* bias, int32_t M, int32_t N, int32_t K,
                     int32_t epi, float* out, uint8_t* a8_out, uint8_t* a_scale_out, uint8_t* w8_out,
                     uint8_t* w_scale_out);
int wdr_dbg_proj(const uint16_t* a_f16, const uint16_t* w_f16, const float* bias, int32_t M, int32_t N, int32_t K,
                 int32_t epi, float* out /* [M][N] f32 (f16 epilogues are widened) */);
/* epi | WDR_DBG_PROJ_ROWS: the decoder-rows kernel (any M, per-row arithmetic independent of M);
 * projections of <= 64 rows run on it anyway (0x100, the removed decode-step GEMV schedule of
 * ABI <= 4, and 0x400, a split-K residual form tried in round 4, are rejected) */
#define WDR_DBG_PROJ_ROWS 0x200
/* epi | WDR_DBG_PROJ_GEMM1: M > 64 on the register-staged reference tile (k_gemm) whatever the
 * dispatch rule picks -- the tiled GEMM family is bit-identical to it */
#define WDR_DBG_PROJ_GEMM1 0x800
/* epi | WDR_DBG_PROJ_PACKED: the weight packed on the GPU into the row kernel's fragment order
 * (wdr_dbg_pack_rows) and the row kernel run on that layout, any M -- bit for bit the row-major
 * result (the decoder's weights are stored this way when a model is loaded) */
#define WDR_DBG_PROJ_PACKED 0x1000
/* w [N][K] (f16 bits, K % 32 == 0) in fragment order: out [16 ceil(N / 16)][K]; element (n, k) at
 * 512 ((n / 16) (K / 32) + k / 32) + 8 (16 ((k / 8) & 3) + (n & 15)) + (k & 7), pad rows zero */
int wdr_dbg_pack_rows(const uint16_t* w_f16, int32_t N, int32_t K, uint16_t* out);
/* A decoder-rows projection of LayerNorm(x) (x [M][K] f32, gamma / beta [K], K % 128 == 0, K <= 1280): fused = 1
 * normalises inside the row kernel's prologue (every workgroup its own row tiles), 0 = a separate
 * LayerNorm launch into f16 rows first; the two must agree bit for bit at every M (rows_forward
 * fuses up to 64 rows).  epi as wdr_dbg_proj (0 / 1 / 3; out [M][N] f32).  fused | 2: the weight in
 * fragment order (as WDR_DBG_PROJ_PACKED); fused | 4: the rows gathered through the kernel's row map,
 * output row m from x row M - 1 - m */
int wdr_dbg_proj_ln(const float* x, const float* gamma, const float* beta, const uint16_t* w_f16, const float* bias,
                    int32_t M, int32_t N, int32_t K, int32_t epi, int32_t fused, float* out);
int wdr_dbg_attn(const uint16_t* q, const uint16_t* k, const uint16_t* v, int32_t Tq, int32_t Tk, int32_t n_head,
                 int32_t causal, float* out /* [Tq][n_head*64] */);
// decode-step cross-attention over 1500 keys (beam groups / per-row slots; see engine.cpp)
/* decode cross-attention probe: R rows (<= 1024) over S slots [S][1500][2 * 64 H] (K then V per key);
 * grp[r] = size of the group row r leads (0 for followers): groups above 8 rows run the decoder-
 * rows MFMA tile kernel (every row as rows_forward computes it), else the VALU split kernel */
int wdr_dbg_xattn(const uint16_t* q, const uint16_t* kv, const int32_t* row_slot, const int32_t* grp, int32_t R,
                  int32_t S, int32_t H, int32_t iters, float* out);

/* ---- decode-step seams.  Every one checks its arguments on the host and returns an error for an
 * out-of-range value instead of launching: row_seq in [0, n_seq), row_pos in [0, min(T, 448)) (the
 * self-attention kernel holds at most 448 scores), d = 64 H, K in [1, 8], R in [1, 8] logit rows ---- */
/* decode-step self-attention (k_dec_self_attn, one launch, scale 1/8): row r of q [R][64 H] (f16 bits)
 * attends over keys 0 .. row_pos[r] of sequence row_seq[r] of the caches kc / vc [n_seq][T][64 H]
 * (f16 bits); out [R][64 H] (f16 -> f32) */
int wdr_dbg_self_attn(const uint16_t* q, const uint16_t* kc, const uint16_t* vc, int32_t n_seq, int32_t T,
                      const int32_t* row_seq, const int32_t* row_pos, int32_t R, int32_t H, float* out);
/* the decoder's fused Q/K/V projection (row kernel, cache-scatter epilogue): a [M][K], w [3 d][K] (f16
 * bits), bias [3 d] (nullable); row r's Q -> q_out [M][d] (f16 -> f32), its K / V -> row (row_seq[r],
 * row_pos[r]) of kc_io / vc_io [n_seq][T][d] (f16 bits; uploaded, updated, copied back).  K % 32 == 0;
 * the rows must name distinct cache rows */
int wdr_dbg_proj_qkv(const uint16_t* a_f16, const uint16_t* w_f16, const float* bias, int32_t M, int32_t d, int32_t K,
                     const int32_t* row_seq, const int32_t* row_pos, int32_t n_seq, int32_t T, uint16_t* kc_io,
                     uint16_t* vc_io, float* q_out);
/* the same with the weight in fragment order (as WDR_DBG_PROJ_PACKED) */
int wdr_dbg_proj_qkv_packed(const uint16_t* a_f16, const uint16_t* w_f16, const float* bias, int32_t M, int32_t d,
                            int32_t K, const int32_t* row_seq, const int32_t* row_pos, int32_t n_seq, int32_t T,
                            uint16_t* kc_io, uint16_t* vc_io, float* q_out);
/* wdr_dbg_logits' inputs, then the beam-search top-K of the same rows (k_logits_topk +
 * k_logits_topk_final): ids [R][K], f [R][K][2] = {p, log p}, best first, ties by lower id; a row
 * with fewer than K finite candidates ends with {id -1, p 0, log p -inf} */
int wdr_dbg_logits_topk(wdr_context* c, const float* logits, int32_t R, const int32_t* ctl, const float* temperature,
                        float max_initial_ts, int32_t suppress_blank, int32_t K, int32_t* ids_out, float* f_out);
/* wdr_dbg_logits' inputs, then the sampling distribution of the same rows (k_logits_probs):
 * probs / logprobs [R][n_vocab], 0 / -inf on masked tokens */
int wdr_dbg_logits_probs(wdr_context* c, const float* logits, int32_t R, const int32_t* ctl, const float* temperature,
                         float max_initial_ts, int32_t suppress_blank, float* probs_out, float* logprobs_out);
/* the first n_rows self-attention cache rows of decoder sequence seq (0 .. 7, chain 0) in every text
 * layer, k / v [n_text_layer][n_rows][d] f16 bits: write != 0 stores them, 0 reads them back */
int wdr_dbg_kv_rows(wdr_context* c, int32_t seq, int32_t n_rows, int32_t write, uint16_t* k, uint16_t* v);
/* the beam reorder (two k_kv_copy phases through scratch sequences): sequence dst[i] takes the first
 * n_rows cached rows that sequence src[i] held before the call, i < n <= 8; a destination named twice
 * is an error */
int wdr_dbg_kv_reorder(wdr_context* c, const int32_t* src, const int32_t* dst, int32_t n, int32_t n_rows);

/* ---- encoder seams.  Every one checks its arguments on the host and returns an error instead of
 * launching on a bad shape ---- */
/* the bit patterns an encoder seam's device output holds before the launch (NaNs no finite result
 * rounds to): an element the kernel never wrote comes back as one of them */
#define WDR_DBG_SENTINEL_F16 0x7e57
#define WDR_DBG_SENTINEL_F32 0x7fc07e57u
/* conv1's operand as every production encode builds it: the log-mel of x[0 .. n) (as wdr_dbg_log_mel),
 * then k_im2col_mel at frame `seek` exactly as an on-demand window encode launches it.  out_f16
 * [3000][kp] raw f16 bits, row t column 3 ci + k = the normalised log-mel of channel ci at window
 * frame t + k - 1 (0 outside 0 .. 2999), columns [3 n_mels, kp) +0.  kp_out = kp (the model's
 * 3 n_mels rounded up to 32); out_f16 null: only kp_out is set */
int wdr_dbg_im2col_mel(wdr_context* c, const float* x, size_t n, int32_t seek, uint16_t* out_f16, int32_t* kp_out);
/* the encoder-only epilogues of the tiled GEMMs (M > 64, N % 128, K % 32; a [M][K], w [N][K] f16 bits,
 * bias [N] nullable) launched as the encoder launches them; gemm_ref != 0: on the reference tile
 * k_gemm (as WDR_DBG_PROJ_GEMM1), bit-identical to what the dispatch rule picks.
 * epi 4: out f32 [M][N] = gelu(a w^T + bias) + pos[row % pos_rows] (pos [pos_rows][N]; slot_elems unused).
 * epi 6: out f16 bits [M / 1500][slot_elems], the raw cross-K/V slot image of every 1500-row window:
 * column c of row 1500 w + t at slot w, element (c / 64) * 96000 + 64 t + c % 64; needs M % 1500 == 0
 * and slot_elems >= 1500 N (a multiple of 4); pos / pos_rows unused.
 * The device buffer holds the sentinel before the launch and comes back whole */
int wdr_dbg_proj_enc(const uint16_t* a_f16, const uint16_t* w_f16, const float* bias, const float* pos,
                     int32_t pos_rows, int32_t M, int32_t N, int32_t K, int32_t epi, int32_t gemm_ref,
                     int64_t slot_elems, void* out);
/* the encoder's self-attention over nb stacked windows in one launch, with the encoder's own launch
 * arguments: qkv [nb][T][3 * 64 H] f16 bits (Q, K, V of a row side by side, as the qkv projection
 * writes them), non-causal, scale 1/8; out [nb][T][64 H] (f16 -> f32).  nb <= 16, T <= 4096 */
int wdr_dbg_attn_batch(const uint16_t* qkv_f16, int32_t nb, int32_t T, int32_t H, float* out);
/* k_layernorm alone (eps 1e-5, biased variance): x [rows][ldx] f32, g / b [d]; out [rows][d] (f16 ->
 * f32), row r from x row r (row_map null: launch_layernorm) or x row row_map[r] (in [0, rows):
 * launch_layernorm_rows).  d % 4 == 0, d <= 1280, ldx % 4 == 0, ldx >= d */
int wdr_dbg_layernorm(const float* x, int32_t ldx, const float* g, const float* b, int32_t rows, int32_t d,
                      const int32_t* row_map, float* out);
/* one encode-ahead batch without a plan: clip k (int16 PCM, n[k] >= 1 samples) goes through the
 * front half of the encode-ahead loop on ring slot k (samples, log-mel, conv1 operand rows k of the
 * batch buffers, window 0), then the batched encoder runs once over the nb stacked windows (nb = 1
 * .. 4, the encode-ahead batch) into ring slots 0 .. nb - 1 -- no graph, language detection or
 * events.  enc_out [nb][1500][d] (f16 -> f32), xkv_out [nb][1500][n_text_layer][2][d] as
 * wdr_dbg_cross_kv.  The state must be idle (no pipeline running on the context) */
int wdr_dbg_encode_batch(wdr_context* c, const int16_t* const* pcm, const int32_t* n, int32_t nb, float* enc_out,
                         float* xkv_out);

#ifdef __cplusplus
}
#endif
#endif /* WDR_H */
