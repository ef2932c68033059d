#!/usr/bin/env python3
"""xRT benchmark of the MI355X hot path (BASELINE.json metric: audio-sec / wall-sec).

Workload (config.workload): the metric's "large-v3 + DTW + diarize" per GPU — BASELINE.json
configs[3]'s diarized large-v3 pipeline on a 1-h shard per rank, with configs[2]'s greedy
decode (the largest single-GPU configuration) — Whisper large-v3 (synthetic seeded weights,
f16 operands / f32 accumulation), DTW word alignment on, lang "auto", 1 h of synthetic 16 kHz
speech-like audio per rank (3 speakers).  `--seg vad` runs configs[2] exactly (Silero VAD
instead of pyannote).  Synthetic workload pin: the segmentation kernels run
and are timed over the whole shard, the segments handed downstream are the generator's
ground-truth talk spurts, and the decode length is pinned to round(3.3 tok/s x window_s) + 3
tokens per window.  Weak scaling: every rank transcribes its own 1-h shard (seed = rank).

One step = segmentation of the rank's whole shard (pyannote segmentation-3.0, or Silero VAD)
+ run_transcription_pipeline over its speech segments (mel, encoder, cross-K/V, language
detection, prompt prefill, greedy decode, heuristic timestamps, DTW re-forward + alignment,
CAM++ speaker embeddings + speaker assignment, reference glue).  Inputs (PCM) are
host-resident as in the reference API; the PCIe share is negligible (115 MB/h) and included.

N > 1 (wdr/distributed.py): ONE file of N x --seconds of audio (4 h at N = 4:
configs[3]) is transcribed across the N GPUs, one process each over RCCL: pyannote windows
sharded (PCM scattered, frame classes gathered to rank 0), speech segments in N contiguous
blocks (PCM scattered), each rank decodes its block speculatively with its decode chains, the
parallel prompt fix-up rounds (prompts all-gathered) make the text equal to one GPU's, raw
results + speaker embeddings are gathered and merged in file order on rank 0 (overlap clip,
speakers).  Weak scaling: every GPU holds ~--seconds of the file.

Run:  python bench.py [--gpus N --steps K --warmup W]   (N>1 via torch.distributed.run)
A plain run sets up, warms up, times the K steps and prints the line (the live kernel clock
samples inside the timed steps).  --full adds the legs with runs of their own: the beam-5
sub-record (`beam5`) and the CPU baseline (`cpu_baseline`); both are null without it.
--dump-outputs DIR writes the last timed step's results as DIR/<name>.npy (dump_outputs).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "whisper-diarize-rs_amd"))

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: 8.0 TB/s spec
# synthetic weights (no checkpoints offline): N(0, 0.02), embeddings N(0, 0.02) -- the workload of
# every round's bench line (674 windows per 1-h shard).  Not the parity fixtures' "alignment-
# conditioned" N(0, 0.05) / N(0, 0.5): with those the forced final timestamp the model picks per
# window is small, the seek advances less and the same hour becomes ~2x the windows and decode
# steps (round 5 A/B: 1367 batched steps vs 458, 399 vs 759 xRT on one box) -- a different
# workload, so the bench keeps its weights and the +-20 ms word parity is pinned on the
# conditioned ones (tests/test_gpu_configs.py), text + speaker parity on both
BENCH_WSTD, BENCH_EMB_STD = 0.02, 0.02
MFMA_F16_PEAK_TFS = 2500.0  # dense f16/bf16 MFMA
MFMA_FP8_PEAK_TFS = 5000.0  # dense block-scaled fp8 MFMA (MI355X_MICROARCH.md, matrix cores)
PROF_EVERY, PROF_STEP_EVERY = 1, 64   # launches clocked in a sampled decode step, 1 in 64 steps sampled (csrc/prof.cpp step_every)
PROF_ENC_EVERY = 32   # csrc/prof.cpp kEncEvery (encode batches run eagerly for sampling)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--seconds", type=float, default=3600.0, help="audio seconds per rank")
    ap.add_argument("--prof", default="gemm,rows,flash,xattn",
                    help="kernel classes timed live with HIP events (comma list of gemm, rows, flash, xattn; "
                         "'none'): the roofline figure is the one with the largest share of kernel time")
    ap.add_argument("--seg", default="diarize", choices=["diarize", "vad"],
                    help="segmentation stage: pyannote diarization (default) or Silero VAD")
    ap.add_argument("--strategy", default="greedy", choices=["greedy", "beam"],
                    help="greedy (configs[2]) or the reference's default beam search, 5 beams")
    ap.add_argument("--fp8", action="store_true", help="fp8 (e4m3) encoder GEMMs (configs[4])")
    ap.add_argument("--multi", default="ranks", choices=["ranks", "inproc"],
                    help="N > 1: one process per GPU over RCCL (wdr/distributed.py, default) or ONE process "
                         "driving N GPUs through libwdr's gpu_device=None context (the C-ABI path a Rust host "
                         "gets, src/engine.rs:14; under torch.distributed.run only rank 0 works)")
    ap.add_argument("--beam-seconds", type=float, default=900.0,
                    help="N=1 greedy runs: also time the reference's default decode (beam search, 5 beams, "
                         "src/transcribe.rs:22-33) over the first this-many seconds of the shard (0: skip)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the legs that take runs of their own: the beam-5 "
                         "sub-record (--beam-seconds) and the CPU baseline (--cpu-audio; --no-cpu-baseline "
                         "drops it).  A plain run only sets up, warms up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step returned to its caller as DIR/<name>.npy (float64): "
                         "segments, words, their texts and speakers, the segmentation stage's speech spans")
    ap.add_argument("--keepalive", type=int, default=0,
                    help="A/B diagnostic: a host thread keeps a low-priority stream busy with 1-workgroup "
                         "spin kernels of this many cycles during the timed steps (0: off)")
    ap.add_argument("--keepalive-mb", type=int, default=0,
                    help="A/B diagnostic: the keep-alive thread copies buffers of this many MB (HBM "
                         "traffic) instead of spinning")
    ap.add_argument("--no-embed", action="store_true",
                    help="A/B: --seg diarize without speaker embeddings / assignment in the pipeline")
    ap.add_argument("--speakers", type=int, default=0,
                    help="voices in the synthetic audio (default: 3 for --seg diarize, 1 for --seg vad)")
    ap.add_argument("--cpu-audio", type=float, default=60.0,
                    help="audio seconds of the workload the CPU baseline is extrapolated over (rank 0, N=1)")
    return ap.parse_args()


def pmc_traffic(cls):
    """HBM bytes per dispatch of the kernel class from the latest committed PMC pass
    (profiles/rNN/pmc.json, tools/gpu_profile.sh: FETCH_SIZE x2 per the gfx950 correction +
    WRITE_SIZE, separate rocprofv3 --pmc runs).  None if no pass has been committed."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "pmc.json")))
    if not files:
        return None, None
    c = json.load(open(files[-1]))["classes"].get(cls, {})
    if "fetch_size_bytes_per_dispatch" not in c:
        return None, None
    return c["fetch_size_bytes_per_dispatch"] + c.get("write_size_bytes_per_dispatch", 0.0), \
        os.path.relpath(files[-1], ROOT)


# BASELINE.md §3 units of work: encoder + cross-K/V per 30-s window (MFMA flops: the GEMMs --
# conv1, conv2, 32 x (qkv, o, fc1, fc2), the cross-K/V projection -- and the self-attention),
# and a decoder pass's bytes: the decoder weights (streamed once per rows launch, shared by its
# rows) and one slot's cross-K/V (read once per cross-attention group or MFMA row tile).
# rows_weight_bytes: the weight bytes a row-kernel launch streams, by k_skinny's template
# arguments <EPI, MT, NT, W, LN, U> (csrc/kernels/gemm.hip): EPI 5 qkv (3d x d), 2 o / xo (d x d)
# or fc2 (d x 4d: the 16-wave form), 0 xq (d x d), 1 fc1 (4d x d), 3 logits (V x d); large-v3
# d = 1280
_D, _V = 1280, 51866


def rows_weight_bytes(targs):
    f = [x.strip() for x in targs.split(",")]
    epi, waves = int(f[0]), int(f[3]) if len(f) > 3 else 4
    if epi == 2:
        return (4 if waves == 16 else 1) * _D * _D * 2
    return {5: 3 * _D * _D * 2, 0: _D * _D * 2, 1: 4 * _D * _D * 2, 3: _V * _D * 2}.get(epi)


WORK = {"large-v3": {"enc_flops": 2.589e12, "enc_gemm_flops": 2.221e12, "enc_attn_flops": 0.369e12,
                     "dec_weight_bytes": 1.601e9, "xkv_row_bytes": 0.246e9,
                     # the 32 layers' projection weights without the logits (14 d^2 x 2 B each); a
                     # DTW pass stops after the last alignment-head layer: 26 of 32
                     "dec_layer_bytes": 14 * _D * _D * 2 * 32, "dtw_layer_frac": 26 / 32,
                     "rows_weight_bytes": rows_weight_bytes},
        "base.en": {"enc_flops": 96.8e9, "enc_gemm_flops": 87.6e9, "enc_attn_flops": 9.2e9,
                    "dec_weight_bytes": 97.1e6, "xkv_row_bytes": 18.4e6, "dec_layer_bytes": 14 * 512 * 512 * 2 * 6,
                    "dtw_layer_frac": 6 / 6}}


def pipeline_roofline(model, times, t_wall):
    """Whole-pipeline roofline of one step (BASELINE.md §3 'roofline.achieved = T_roof / T_wall'
    with the schedule actually used): encoder windows at the dense f16 MFMA peak; every decoder
    pass at the HBM peak -- each rows launch streams the decoder weights once for all its rows
    (decode steps and prompt prefills in the step batcher, csrc/rows.h), each cross-attention
    group / MFMA row tile reads its slot's cross-K/V once; the DTW queue's passes stream the
    layers up to the last alignment-head layer (large-v3: 26 of 32, no logits) and read each
    job's slot over those layers; the language-detection passes (one per encode-ahead batch, its
    windows as one-row groups) stream every layer and read each row's slot.  Passes outside the
    batcher (one chain: each step, prefill and DTW pass its own launch) count one launch and one
    slot each."""
    w = WORK.get(model)
    if w is None:
        return None
    windows = times["windows"]
    bl = times.get("batch_launches", 0)
    if bl:
        launches = bl
        slot_reads = times.get("batch_xattn_groups", 0) + times.get("batch_xattn_tiles", 0)
    else:
        launches = times["decode_steps"] + times["prefills"] + windows
        slot_reads = launches
    dtw_frac = w.get("dtw_layer_frac", 1.0)
    dtw_passes, dtw_jobs = times.get("dtwq_passes", 0), times.get("dtwq_jobs", 0)
    lang_passes, lang_rows = times.get("lang_passes", 0), times.get("lang_rows", 0)
    t_enc = windows * w["enc_flops"] / (MFMA_F16_PEAK_TFS * 1e12)
    bw = HBM_PEAK_GBS * 1e9
    t_dec = (launches * w["dec_weight_bytes"] + slot_reads * w["xkv_row_bytes"]) / bw
    t_dtw = dtw_frac * (dtw_passes * w["dec_layer_bytes"] + dtw_jobs * w["xkv_row_bytes"]) / bw
    t_lang = (lang_passes * w["dec_weight_bytes"] + lang_rows * w["xkv_row_bytes"]) / bw
    t_roof = t_enc + t_dec + t_dtw + t_lang
    return {"t_roof_s": round(t_roof, 4), "t_wall_s": round(t_wall, 4), "frac": round(t_roof / t_wall, 4),
            "terms_s": {"encoder_mfma": round(t_enc, 4), "decoder_rows_hbm": round(t_dec, 4),
                        "dtw_queue_hbm": round(t_dtw, 4), "lang_detect_hbm": round(t_lang, 4)},
            "rows_launches": launches, "slot_reads": slot_reads, "dtw_passes": dtw_passes, "dtw_jobs": dtw_jobs,
            "lang_passes": lang_passes, "lang_rows": lang_rows}


def trace_roofline(model, fp8=False):
    """The class-wide roofline fractions of the committed rocprofv3 trace of this benched
    configuration (profiles/rNN/prof_graph/: classes.json from tools/prof_summary.py --json, the
    traced run's own bench line for its work counts): achieved = the class's algorithmic work
    over the traced runs / its summed kernel time.  Reproducible from profiles/ alone."""
    import glob
    w = WORK.get(model)
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "prof_graph", "classes.json")))
    if not cands or w is None:
        return None
    d = os.path.dirname(cands[-1])
    try:
        cls = json.load(open(cands[-1]))
        line = json.loads(open(os.path.join(d, "bench_trace.json")).read().splitlines()[0])
    except (OSError, ValueError, IndexError):
        return None
    runs = line["warmup"] + line["steps"]          # the trace covers every run of the command
    c = line["counts"]
    out = {"source": os.path.relpath(d, ROOT), "traced_runs": runs}
    pk = MFMA_FP8_PEAK_TFS if fp8 else MFMA_F16_PEAK_TFS
    # the decoder rows class: every row-kernel launch of the trace (batched steps, prompt
    # prefills, DTW passes, language detection) streams its projection's weights once --
    # N*K*2 bytes by the kernel's epilogue / tiling (csrc/kernels/gemm.hip launch_rows_epi)
    rows_bytes = rows_ms = 0.0
    wb = w.get("rows_weight_bytes")
    stats = os.path.join(d, "run_kernel_stats.csv")
    if wb and os.path.exists(stats):
        import csv
        for r in csv.DictReader(open(stats)):
            nm = r.get("Name", r.get("KernelName", ""))
            if "k_skinny<" in nm:
                key = nm[nm.index("k_skinny<") + 9:].split(">")[0].replace(" ", "")
                b = wb(key)
                if b:
                    rows_bytes += float(r.get("Calls", 0)) * b
                    rows_ms += float(r.get("TotalDurationNs", 0)) * 1e-6
    for k, work, unit in (("gemm", runs * c["windows"] * w["enc_gemm_flops"], "TFLOP/s"),
                          ("flash", runs * c["windows"] * w["enc_attn_flops"], "TFLOP/s"),
                          ("rows", rows_bytes, "GB/s"),
                          ("xattn", runs * (c.get("batch_xattn_groups", 0) + c.get("batch_xattn_tiles", 0))
                           * w["xkv_row_bytes"], "GB/s")):
            k_ms = cls["classes"].get(k, {}).get("total_ms")
            if k == "rows":
                k_ms = rows_ms   # the projection launches the bytes count (the live sampler's set)
            if not k_ms or not work:
                continue
            if unit == "TFLOP/s":
                ach = work / (k_ms * 1e-3) / 1e12
                out[k] = {"achieved": round(ach, 2), "peak": pk if k == "gemm" else MFMA_F16_PEAK_TFS, "unit": unit}
            else:
                ach = work / (k_ms * 1e-3) / 1e9
                out[k] = {"achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": unit}
            out[k]["frac"] = round(ach / out[k]["peak"], 4)
            out[k]["share"] = round(cls["classes"][k].get("share", 0.0), 4)
            out[k]["launches"] = cls["classes"][k]["launches"]
            out[k]["avg_us"] = round(cls["classes"][k]["avg_us"], 3)
    return out


def cpu_baseline(model, segs, audio_target):
    """The CPU restatement (oracle/, numpy f32 over f16-rounded weights/activations as ggml) timed
    on this host at 4 threads (whisper.cpp's default min(4, hw), src/types.rs:19) and at the
    process's BLAS thread count, per stage: one 30-s window through the encoder + cross K/V, a
    prompt prefill, decode steps, a DTW re-forward with alignment-head capture, log-mel.  The
    figures are combined over the first segments of the same shard covering >= audio_target
    seconds of speech with the same schedule the GPU runs (windows, pinned decode lengths,
    prompts, language-detection steps): xRT = the shard time they cover (to the last one's end,
    silences included, the GPU figure's basis) / T_cpu.  Extrapolated, labelled so."""
    import numpy as np
    from threadpoolctl import threadpool_info, threadpool_limits
    from oracle.mel import log_mel, pcm_i16_to_f32
    from oracle.model import DecoderState, Whisper
    from oracle.vocab import Vocab
    from oracle.weights import hparams_for, synth_weights
    from oracle.whisper_full import aheads_for_model_name
    hp = hparams_for(model)
    m = Whisper(hp, synth_weights(hp, std=BENCH_WSTD, emb_std=BENCH_EMB_STD))
    v = Vocab(hp.n_vocab)
    # the workload sample: segments in order until audio_target seconds
    sel, audio = [], 0.0
    for sg in segs:
        sel.append(sg)
        audio += sg.samples.size / 16000.0
        if audio >= audio_target:
            break
    n_win = n_steps = n_lang = 0
    prefill_toks = dtw_toks = 0
    prev_len = 0
    for sg in sel:
        n_len = sg.samples.size // 160
        seek = 0
        n_lang += 1                              # lang auto: one [SOT] step per segment
        while seek + 100 < n_len:
            win = min(3000, n_len - seek)
            L = max(3, int(round(3.3 * win / 100.0)) + 3)
            n_win += 1
            n_steps += L
            prefill_toks += (1 + min(224, prev_len) if prev_len else 0) + 3
            dtw_toks += L + 2
            prev_len = L - 3
            seek += 3000
    pcm0 = pcm_i16_to_f32(sel[0].samples)
    # the host cores this process may use: the box's CPU share (OMP_NUM_THREADS, which the GPU box
    # sets to it), else the affinity mask -- not the machine's CPU count (a 256-thread BLAS on a
    # 16-core share ran 2.4x slower than 4 threads, profiles/r04/bench_head.json).  Timed at
    # whisper.cpp's default 4 threads and at the share; the faster one is reported
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    share = os.environ.get("OMP_NUM_THREADS", "")
    threads_max = min(aff, int(share)) if share.isdigit() and int(share) > 0 else aff
    out = {}
    for threads in sorted({min(4, threads_max), threads_max}):
        with threadpool_limits(limits=threads):
            threads_used = max([i.get("num_threads", 1) for i in threadpool_info()] or [1])
            t = time.perf_counter()
            mel = log_mel(pcm0, hp.n_mels)
            t_mel_per_s = (time.perf_counter() - t) / (pcm0.size / 16000.0)
            win = np.zeros((hp.n_mels, 3000), np.float32)
            win[:, :min(3000, mel.shape[1])] = mel[:, :3000]
            t = time.perf_counter()
            cross = m.cross_kv(m.encode(win))
            t_enc = time.perf_counter() - t
            st = DecoderState(m)
            prompt = [v.sot] + [int(x) for x in np.arange(30) * 97 % v.eot]
            t = time.perf_counter()
            st.forward(prompt, cross)
            t_pre_tok = (time.perf_counter() - t) / len(prompt)
            t = time.perf_counter()
            for k in range(8):
                st.forward([int(100 + k)], cross)
            t_step = (time.perf_counter() - t) / 8
            dt_toks = [v.sot, v.not_] + [int(x) for x in np.arange(40) * 31 % v.eot] + [v.eot]
            t = time.perf_counter()
            DecoderState(m).forward(dt_toks, cross, want_logits=None, aheads=aheads_for_model_name(model))
            t_dtw_tok = (time.perf_counter() - t) / len(dt_toks)
        T = (audio * t_mel_per_s + n_win * t_enc + (n_steps + n_lang) * t_step + prefill_toks * t_pre_tok
             + dtw_toks * t_dtw_tok)
        out[threads] = dict(xrt=float(sel[-1].end) / T, blas_threads=threads_used, t_enc_s=round(t_enc, 3),
                            t_step_ms=round(t_step * 1e3, 2),
                            t_prefill_tok_ms=round(t_pre_tok * 1e3, 2), t_dtw_tok_ms=round(t_dtw_tok * 1e3, 2))
    del m
    sample = ("first %d segments (%.1f s of speech over %.1f s of audio: %d windows, %d decode steps, %d prompt + %d DTW tokens) of "
              "rank 0's shard, extrapolated from per-stage timings (1 encoder window, 8 steps, a 31-token "
              "prefill, a 43-token DTW re-forward) of the numpy oracle" % (len(sel), audio, sel[-1].end, n_win, n_steps,
                                                                         prefill_toks, dtw_toks))
    return out, sample, threads_max


def beam5_record(ctx, dia, vad, pcm, segs, opts, dopts, diarize, args):
    """The reference's DEFAULT decode -- beam search, 5 beams, patience -1 (src/transcribe.rs:22-33)
    -- on the first --beam-seconds of the same shard, same context: segmentation of that audio +
    run_transcription_pipeline over its segments, one untimed run (beam graphs) then two timed."""
    import wdr
    n = int(args.beam_seconds * 16000)
    sub = [s for s in segs if s.end * 16000 <= n]
    if not sub:
        return None
    bopts = wdr.TranscribeOptions(model=args.model, lang="auto", enable_vad=not diarize,
                                  enable_diarize=True if diarize else None, advanced=None)

    def run():
        if diarize:
            dia.get_segments(pcm[:n], materialize=False)
        else:
            vad.get_segments(pcm[:n], materialize=False)
        return ctx.run_pipeline(sub, bopts, diarize_options=dopts)
    run()
    steps = 2
    t0 = time.perf_counter()
    for _ in range(steps):
        run()
    dt = time.perf_counter() - t0
    audio = n / 16000.0
    return {"metric": "audio-sec/wall-sec (xRT)", "value": round(audio * steps / dt, 3), "unit": "audio-sec/wall-sec",
            "strategy": "beam search, 5 beams, patience -1 (reference default, src/transcribe.rs:22-33)",
            "audio_s": audio, "segments": len(sub), "steps": steps, "warmup": 1,
            "ms_per_step": round(dt * 1e3 / steps, 1),
            "note": "same context, weights and pins as the main line; the first %.0f s of its shard" % audio}


def dump_outputs(path, segments, spans=None):
    """--dump-outputs: the last timed step's return value as arrays, one DIR/<name>.npy each
    (float64; 1 h of audio is a few hundred KB in all, so everything is written, nothing sampled).
      segments      [n, 3]   start s, end s, number of words of every output Segment
      words         [m, 4]   index of its segment, start s, end s, probability (NaN: none)
      segment_text  [..]     the segments' texts as Unicode code points, one '\\n' after each
      word_text     [..]     the words' texts, the same way
      speakers      [..]     the segments' speaker ids, the same way (empty line: none)
      speech_spans  [k, 2]   start s, end s of the segmentation stage's speech spans
                             (one-process runs: the stage's own result, not the pinned spurts)"""
    import numpy as np

    def codes(strs):
        return np.array([ord(ch) for s in strs for ch in (s or "") + "\n"], np.float64)
    os.makedirs(path, exist_ok=True)
    words = [(i, w.start, w.end, np.nan if w.probability is None else w.probability)
             for i, s in enumerate(segments) for w in (s.words or [])]
    arrs = {"segments": np.array([(s.start, s.end, len(s.words or [])) for s in segments], np.float64).reshape(-1, 3),
            "words": np.array(words, np.float64).reshape(-1, 4),
            "segment_text": codes([s.text for s in segments]),
            "word_text": codes([w.text for s in segments for w in (s.words or [])]),
            "speakers": codes([s.speaker_id for s in segments])}
    if spans is not None:
        arrs["speech_spans"] = np.array([(a, b) for a, b in spans], np.float64).reshape(-1, 2)
    for name, a in arrs.items():
        np.save(os.path.join(path, name + ".npy"), a)


def main_inproc(args):
    """--multi inproc: ONE process, N GPUs, libwdr's own multi-GPU path (gpu_device = None,
    WDR_DEVICES = 0..N-1 unless set; decode chains spread over the GPUs, chain k on GPU k % N,
    the exact prompt fix-up across them: csrc/engine.cpp).  One file of N x --seconds of audio
    (seeds 0..N-1 concatenated: weak scaling, ~--seconds per GPU).  The pyannote windows are split
    in N contiguous shards, one Diarizer per GPU in its own thread, and stitched in file order
    (Diarizer.segments_from_classes); the segments handed downstream are the generator's
    ground-truth spurts (synthetic pin, as the one-GPU line).  Under torch.distributed.run the
    ranks > 0 only join the barriers (gloo: they never touch a GPU)."""
    import threading
    import numpy as np
    import wdr
    from wdr.synth import synth_speech
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    N = max(1, args.gpus)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group(backend="gloo")
        if rank != 0:
            dist.barrier()   # rank 0's run
            dist.destroy_process_group()
            return
    os.environ.setdefault("WDR_DEVICES", ",".join(str(g) for g in range(N)))
    devs = [int(x) for x in os.environ["WDR_DEVICES"].split(",")]
    diarize = args.seg == "diarize"
    syn = wdr.Synthetic(weight_std=BENCH_WSTD, emb_std=BENCH_EMB_STD, force_len_rate=3.3, disable_fallback=True)
    t_load = time.perf_counter()
    ctx = wdr.WhisperContext(args.model, gpu_device=None, enable_dtw=True, synthetic=syn)
    if args.fp8:
        ctx.set_encoder_fp8(True)
    t_load = time.perf_counter() - t_load
    parts = [synth_speech(args.seconds, seed=r, n_speakers=args.speakers or (3 if diarize else 1)) for r in range(N)]
    pcm = np.concatenate([p for p, _ in parts])
    spurts = [(a + r * args.seconds, b + r * args.seconds) for r, (_, sp) in enumerate(parts) for a, b, _ in sp]
    del parts
    segs = [wdr.SpeechSegment(a, b, pcm[int(round(a * 16000)):int(round(b * 16000))]) for a, b in spurts]
    opts = wdr.TranscribeOptions(model=args.model, lang="auto", enable_vad=not diarize,
                                 enable_diarize=True if diarize else None,
                                 advanced=wdr.AdvancedTranscribe(
                                     sampling_strategy="greedy" if args.strategy == "greedy" else None))
    dopts = wdr.DiarizeOptions.from_options(opts) if diarize else None
    dzs = [wdr.Diarizer(gpu_device=g) for g in devs] if diarize else []
    vad = None if diarize else wdr.Vad(gpu_device=devs[0])
    WIN, FR = 160000, 589
    seg_t = [0.0]

    def segment():
        t = time.perf_counter()
        if diarize:
            W = pcm.size // WIN + 1
            cuts = [round(W * i / len(dzs)) for i in range(len(dzs) + 1)]
            out = [None] * len(dzs)

            def run(i):
                a, b = cuts[i], cuts[i + 1]
                out[i] = dzs[i].frame_classes(pcm[a * WIN:min(pcm.size, b * WIN)])[:b - a] if b > a else \
                    np.zeros((0, FR), np.int32)
            th = [threading.Thread(target=run, args=(i,)) for i in range(len(dzs))]
            for x in th:
                x.start()
            for x in th:
                x.join()
            n = len(wdr.Diarizer.segments_from_classes(np.concatenate(out, 0), pcm))
        else:
            n = len(vad.get_segments(pcm, materialize=False)[1])
        seg_t[0] += time.perf_counter() - t
        return n

    def step():
        segment()
        return ctx.run_pipeline(segs, opts, diarize_options=dopts)
    for _ in range(args.warmup):
        step()
    seg_t[0] = 0.0
    t0 = time.perf_counter()
    n_out = 0
    for _ in range(args.steps):
        out, _ = step()
        n_out += len(out)
    dt = time.perf_counter() - t0
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, out)
    times = ctx.stage_times()
    shard_s = pcm.size / 16000.0
    line = {
        "metric": "audio-sec/wall-sec (xRT), large-v3 + DTW + diarize, 1/2/4/8 MI355X",
        "value": round(shard_s * args.steps / dt, 3), "unit": "audio-sec/wall-sec", "n_gpus": N, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(dt * 1e3 / args.steps, 1), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f16 (f32 accumulate)", "data": "synthetic",
        "config": {"strategy": "greedy" if args.strategy == "greedy" else "beam search, 5 beams (reference default)",
                   "workload": "one file of %d x %.0f s synthetic audio (%d segments, 3 speakers), %s + DTW + %s, "
                               "lang auto, ground-truth spurt segments downstream, decode length pinned and the "
                               "temperature fallback off (disable_fallback: synthetic pin)"
                               % (N, args.seconds, len(segs), args.model, "diarize" if diarize else "Silero VAD"),
                   "model": args.model, "global_batch": len(segs), "seq_len": 1500,
                   "parallelism": "ONE process, libwdr gpu_device=None over devices %s (decode chains spread, "
                                  "exact prompt fix-up across GPUs); pyannote windows sharded per GPU" % devs},
        "roofline": None, "cpu_baseline": None,
        "stages_s": {k: round(v, 3) for k, v in times.items() if isinstance(v, float)},
        "counts": {k: v for k, v in times.items() if isinstance(v, int)},
        "segmentation": {"s_per_step": round(seg_t[0] / args.steps, 4)},
        "devices": ctx.devices, "load_s": round(t_load, 2), "segments_out": n_out // max(1, args.steps),
    }
    print(json.dumps(line), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


def main():
    args = parse()
    if args.multi == "inproc":
        return main_inproc(args)
    import numpy as np
    import torch
    import torch.distributed as dist
    import wdr
    from wdr.synth import synth_speech

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        # WDR_BENCH_BACKEND=gloo + WDR_BENCH_SHARE_GPU=1 rehearse N ranks on a 1-GPU box
        backend = os.environ.get("WDR_BENCH_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
        if os.environ.get("WDR_BENCH_SHARE_GPU") == "1":
            local = 0
        if backend == "nccl":
            torch.cuda.set_device(local)
        dist.init_process_group(backend=backend)
    vad_t = [0.0, 0]

    def barrier():
        if world > 1:
            dist.barrier()
        if torch.cuda.is_available():
            torch.cuda.synchronize()

    diarize = args.seg == "diarize"
    syn = wdr.Synthetic(weight_std=BENCH_WSTD, emb_std=BENCH_EMB_STD, force_len_rate=3.3, disable_fallback=True)
    t_load = time.perf_counter()
    ctx = wdr.WhisperContext(args.model, gpu_device=local, enable_dtw=True, synthetic=syn)
    if args.fp8:
        ctx.set_encoder_fp8(True)
    t_load = time.perf_counter() - t_load
    opts = wdr.TranscribeOptions(model=args.model, lang="auto", enable_vad=not diarize,
                                 enable_diarize=True if diarize else None,
                                 advanced=wdr.AdvancedTranscribe(
                                     sampling_strategy="greedy" if args.strategy == "greedy" else None))
    dopts = wdr.DiarizeOptions.from_options(opts) if diarize and not args.no_embed else None   # src/engine.rs:101-111
    vad = None if diarize else wdr.Vad(gpu_device=local)
    dia = wdr.Diarizer(gpu_device=local) if diarize else None
    lib = wdr._lib.load()
    CLS = {"gemm": 1, "rows": 2, "flash": 3, "xattn": 4}
    prof = [c for c in args.prof.split(",") if c in CLS]
    prof_mask = sum(1 << CLS[c] for c in prof)

    if world > 1:
        # ONE file of world x seconds: rank r synthesises hour r (seed r) in parallel, rank 0
        # assembles the file (not timed); the timed step transcribes it across all ranks
        from wdr import distributed as D
        pcm_r, spurts_r = synth_speech(args.seconds, seed=rank, n_speakers=args.speakers or (3 if diarize else 1))
        parts = [None] * world if rank == 0 else None
        dist.gather_object((pcm_r, [(a + rank * args.seconds, b + rank * args.seconds) for a, b, _ in spurts_r]),
                           parts, dst=0)
        del pcm_r
        pcm, spurts = None, []
        if rank == 0:
            pcm = np.concatenate([p[0] for p in parts])
            spurts = [sp for p in parts for sp in p[1]]
        del parts
        meta = [len(spurts), 0 if pcm is None else pcm.size, sum(b - a for a, b in spurts)]
        obj = [meta]
        dist.broadcast_object_list(obj, src=0)
        segs_n, n_total, speech_total = obj[0]
        shard_s = n_total / 16000.0 / world      # audio per GPU (the weak-scaling unit)
        audio_s = speech_total / world

        def pinned(*_):   # synthetic pin: the generator's talk spurts downstream
            return [wdr.SpeechSegment(a, b, pcm[int(round(a * 16000)):int(round(b * 16000))]) for a, b in spurts]

        def step():
            t = time.perf_counter()
            res = D.transcribe_file(pcm, opts, ctx=ctx, segmentation="diarize" if diarize else "vad",
                                    diarizer=dia, vad=vad, speech_segments_fn=pinned)
            vad_t[0] += time.perf_counter() - t
            vad_t[1] = segs_n
            return res if res is not None else ([], None)
        segs = spans = None
    else:
        pcm, spurts = synth_speech(args.seconds, seed=rank, n_speakers=args.speakers or (3 if diarize else 1))
        segs = [wdr.SpeechSegment(a, b, pcm[int(round(a * 16000)):int(round(b * 16000))]) for a, b, _ in spurts]
        audio_s = float(sum(s.samples.size for s in segs)) / 16000.0   # speech seconds handed to the pipeline
        shard_s = pcm.size / 16000.0                                  # wall-clock audio covered (xRT basis)
        segs_n = len(segs)
        spans = []   # the segmentation stage's (start, end) pairs of the latest step

        def step():
            # the segmentation stage over the whole shard runs and is timed; in synthetic mode the
            # segment list handed downstream is the generator's ground-truth spurt table
            # (BASELINE.md §2 pin)
            t = time.perf_counter()
            if diarize:   # libwdr makes every segment's samples; the Python copy of them is skipped
                spans[:] = dia.get_segments(pcm, materialize=False)
            else:
                spans[:] = vad.get_segments(pcm, materialize=False)[1]
            vad_t[0] += time.perf_counter() - t
            vad_t[1] = len(spans)
            return ctx.run_pipeline(segs, opts, diarize_options=dopts)

    if args.keepalive > 0 or args.keepalive_mb > 0:
        # diagnostic only (profiles/r06/ab_lines_hwq.txt): does activity on a low-priority queue,
        # like the speaker-embedding worker's, change the batched steps' speed?
        import threading
        ka_stop = threading.Event()

        def keepalive():
            st = torch.cuda.Stream(device=local, priority=0)
            with torch.cuda.stream(st):
                if args.keepalive_mb > 0:
                    a = torch.empty(args.keepalive_mb << 18, dtype=torch.float32, device=local)
                    b = torch.empty_like(a)
                while not ka_stop.is_set():
                    if args.keepalive_mb > 0:
                        b.copy_(a)
                        st.synchronize()
                        time.sleep(2e-4)
                    else:
                        torch.cuda._sleep(args.keepalive)
                    st.synchronize()
        ka = threading.Thread(target=keepalive, daemon=True)
        ka.start()
    vad_t = [0.0, 0]
    for _ in range(args.warmup):
        step()
    vad_t = [0.0, 0]
    barrier()
    lib.wdr_prof_set_mask(prof_mask)
    def cg_throttle():
        try:
            kv = dict(ln.split() for ln in open("/sys/fs/cgroup/cpu.stat"))
            return int(kv.get("nr_throttled", 0)), int(kv.get("throttled_usec", 0))
        except (OSError, ValueError):
            return 0, 0
    def thread_cpu():
        # per thread-name CPU ticks of this process (/proc/self/task/*/stat utime + stime)
        out = {}
        for tid in os.listdir("/proc/self/task"):
            try:
                st = open("/proc/self/task/%s/stat" % tid).read()
            except OSError:
                continue
            name = st[st.index("(") + 1:st.rindex(")")]
            f = st[st.rindex(")") + 2:].split()
            out[tid] = (name, int(f[11]) + int(f[12]))
        return out
    tc0 = thread_cpu() if os.environ.get("WDR_BENCH_THREADS") else None
    thr_log = []
    if os.environ.get("WDR_BENCH_THROTTLE_LOG"):
        # diagnostic: when in the timed steps the cgroup's throttled-period count moves (10-ms poll)
        import threading
        thr_stop = threading.Event()

        def thr_poll():
            last = cg_throttle()[0]
            while not thr_stop.is_set():
                n_ = cg_throttle()[0]
                if n_ != last:
                    thr_log.append((round(time.perf_counter() - t0, 3), n_ - last))
                    last = n_
                time.sleep(0.01)
        thr_th = threading.Thread(target=thr_poll, daemon=True)
    th0 = cg_throttle()
    c0 = os.times()
    t0 = time.perf_counter()
    if os.environ.get("WDR_BENCH_THROTTLE_LOG"):
        thr_th.start()
    n_out = 0
    for _ in range(args.steps):
        out, _ = step()
        n_out += len(out)
    barrier()
    dt = time.perf_counter() - t0
    c1 = os.times()
    host_cpu_s = (c1.user - c0.user) + (c1.system - c0.system)   # every thread of this process
    th1 = cg_throttle()
    if os.environ.get("WDR_BENCH_THROTTLE_LOG"):
        thr_stop.set()
        thr_th.join()
    thread_cpu_s = None
    if tc0 is not None:
        tc1, hz = thread_cpu(), os.sysconf("SC_CLK_TCK")
        agg = {}
        for tid, (name, t1) in tc1.items():
            d = t1 - tc0.get(tid, (name, 0))[1]
            a_ = agg.setdefault(name, [0.0, 0])
            a_[0] += d / hz
            a_[1] += 1
        thread_cpu_s = {k: [round(v[0], 2), v[1]] for k, v in sorted(agg.items(), key=lambda kv: -kv[1][0])[:12]}
    if args.keepalive > 0 or args.keepalive_mb > 0:
        ka_stop.set()
        ka.join()
    import ctypes as C
    live, live_ev = {}, {}
    for c in prof:
        ms, nl, by, fl = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        if lib.wdr_prof_read_clock(CLS[c], C.byref(ms), C.byref(nl), C.byref(by), C.byref(fl)) == 0 and nl.value:
            live[c] = (ms.value, nl.value, by.value, fl.value)
        if lib.wdr_prof_read_class(CLS[c], C.byref(ms), C.byref(nl), C.byref(by), C.byref(fl)) == 0 and nl.value:
            live_ev[c] = (ms.value, nl.value)
    lib.wdr_prof_set_mask(0)
    times = ctx.stage_times()
    t = torch.tensor([dt], dtype=torch.float64)
    if world > 1:
        if dist.get_backend() == "nccl":
            t = t.cuda()
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt_max = float(t.item())
    value = world * shard_s * args.steps / dt_max

    # per class: algorithmic flops (MFMA classes) or bytes (HBM classes) per launch / the average
    # duration of its sampled launches, timed by the kernels' own clock (first wave start -> last
    # wave end: rocprofv3's dispatch span; csrc/common.h ProfClock), each sample weighted by
    # 1 / its sampling probability (every class is sampled 1 in 64, csrc/prof.cpp), so
    # `launches_est` estimates the class's launch count; the same launches' HIP start/stop
    # events are reported beside it (under the pipeline's multi-stream concurrency they also
    # absorb the launch's wait for the GPU).
    classes = {}
    for c, (ms, nl, by, fl) in live.items():
        if ms <= 0:
            continue
        if c in ("gemm", "flash"):
            ach = fl / (ms * 1e-3) / 1e12
            # --fp8: the encoder GEMMs run the block-scaled fp8 MFMA, dense peak 5 PF/s
            pk = MFMA_FP8_PEAK_TFS if (args.fp8 and c == "gemm") else MFMA_F16_PEAK_TFS
            r = {"kernel": c, "bound": "mfma", "achieved": round(ach, 2), "peak": pk,
                 "unit": "TFLOP/s", "frac": round(ach / pk, 4), "flops_per_launch": fl / nl}
        else:
            ach = by / (ms * 1e-3) / 1e9
            r = {"kernel": c, "bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS,
                 "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4), "bytes_per_launch": by / nl}
        r.update({"traffic": None, "launches_est": nl, "avg_launch_us": round(ms * 1e3 / nl, 3),
                  "kernel_ms_est": round(ms, 3), "timing": "kernel clock (wall_clock64, first wave -> last wave)"})
        if c in live_ev:
            r["hip_event_avg_launch_us"] = round(live_ev[c][0] * 1e3 / live_ev[c][1], 3)
        tr, src = pmc_traffic(c)
        if tr is not None:
            r["traffic"] = round(tr)
            r["traffic_source"] = src
        # csrc/prof.h: decode-only steps and full encode batches replay hipGraphs; 1 in 64 such
        # steps (1 in 32 such batches) runs eagerly with every (1 in 2) of its launches clocked;
        # always-eager launches (mixed / prefill / DTW batches, partial encode batches) are
        # clocked 1 in 64 -- every launch with probability 1 / 64
        r["sampling"] = ("1 in %d launches (graph-replayed work: decode steps 1 in %d eager, 1 in %d of "
                         "those; encode batches 1 in %d eager, 1 in %d of those)") % (
            PROF_EVERY * PROF_STEP_EVERY, PROF_STEP_EVERY, PROF_EVERY, PROF_ENC_EVERY,
            PROF_EVERY * PROF_STEP_EVERY // PROF_ENC_EVERY)
        classes[c] = r
    # `roofline` = the class with the largest share of kernel time in the committed rocprofv3
    # trace of this benched configuration (profiles/rNN/prof_graph/classes.json; r03: encoder
    # GEMMs 30.7 %, decoder rows 27.3 %, cross-attention 11.2 %, encoder flash 8.7 %), the
    # encoder GEMM class without one.
    trace = trace_roofline(args.model, args.fp8)
    shares = {k: v.get("share", 0.0) for k, v in (trace or {}).items() if isinstance(v, dict) and k in classes}
    pick = max(shares, key=shares.get) if shares else "gemm"
    roof = classes.get(pick) or (max(classes.values(), key=lambda r: r["kernel_ms_est"]) if classes else None)
    if roof is not None:
        roof = dict(roof, dominant_by="rocprofv3 kernel-time share of the benched configuration (%s)"
                    % ((trace or {}).get("source", "no committed trace")))
        if trace and roof["kernel"] in trace:
            # the same class over the whole committed traced run (class-wide work / summed kernel
            # time), reported beside this run's own figures and never in their place:
            # the trace is an earlier command's, taken with host launches serialised
            # (WDR_LAUNCH_LOCK, DESIGN.md "Faults"), so its kernels ran almost one at a time while
            # this run overlaps the encoder with the decode chain
            roof["trace_achieved"] = trace[roof["kernel"]]["achieved"]
            roof["trace_frac"] = trace[roof["kernel"]]["frac"]
            roof["trace_avg_launch_us"] = trace[roof["kernel"]].get("avg_us")
            roof["trace_source"] = "%s (committed rocprofv3 trace, launch-locked)" % trace.get("source")

    pipe = pipeline_roofline(args.model, times, dt / args.steps)

    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, out, spans)

    # the legs with runs of their own (--full)
    beam = None
    if args.full and rank == 0 and world == 1 and args.strategy == "greedy" and args.beam_seconds > 0:
        beam = beam5_record(ctx, dia, vad, pcm, segs, opts, dopts, diarize, args)

    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        ctx.close()
        res, sample, tmax = cpu_baseline(args.model, segs, args.cpu_audio)
        # the faster of the thread counts tried (oversubscribed BLAS pools on a many-core host can
        # be slower than 4 threads); `cores` = the threads that figure used
        best = max(res, key=lambda k: res[k]["xrt"])
        cpu = {"value": round(res[best]["xrt"], 5), "unit": "audio-sec/wall-sec", "cores": res[best]["blas_threads"],
               "kind": "port", "cores_available": tmax,
               "sample": sample, "extrapolated": True, "host_cpus": os.cpu_count(),
               "by_threads": {str(k): {kk: (round(vv, 5) if kk == "xrt" else vv) for kk, vv in r.items()}
                              for k, r in res.items()}}

    if rank == 0:
        line = {
            "metric": "audio-sec/wall-sec (xRT), large-v3 + DTW + diarize, 1/2/4/8 MI355X",
            "value": round(value, 3), "unit": "audio-sec/wall-sec", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(dt_max * 1e3 / args.steps, 1), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": ("fp8 e4m3 encoder GEMMs, f16 elsewhere (f32 accumulate)" if args.fp8 else "f16 (f32 accumulate)"), "data": "synthetic",
            "config": {"strategy": "greedy" if args.strategy == "greedy" else "beam search, 5 beams (reference default)",
                       "encoder_gemms": "fp8 e4m3 (configs[4])" if args.fp8 else "f16",
                       "workload": ("configs[3] per-GPU shard with configs[2]'s greedy decode: %s + DTW + diarize "
                                    "(pyannote segmentation-3.0 run + timed, CAM++ embeddings + speaker assignment), "
                                    "%.0f s synthetic audio per rank (%d segments, %.0f s speech, 3 speakers), lang auto, "
                                    "ground-truth spurt segments downstream, decode length pinned to round(3.3 tok/s x "
                                    "window) + 3 and the temperature fallback off (disable_fallback: synthetic pin)"
                                    if diarize else
                                    "configs[2]: %s + DTW, Silero VAD run + timed, %.0f s synthetic audio per rank "
                                    "(%d segments, %.0f s speech), lang auto, ground-truth spurt segments "
                                    "downstream, decode length pinned to round(3.3 tok/s x window) + 3 and the "
                                    "temperature fallback off (disable_fallback: synthetic pin)") % (args.model, shard_s, segs_n // world, audio_s),
                       "model": args.model, "global_batch": segs_n if world > 1 else segs_n * world, "seq_len": 1500,
                       "parallelism": ("one file of %d x %.0f s over %d GPUs: pyannote windows + speech-segment blocks "
                                       "sharded, parallel prompt fix-up rounds, results gathered (wdr/distributed.py)"
                                       % (world, shard_s, world)) if world > 1 else "1 GPU"},
            "roofline": roof, "roofline_classes": classes, "roofline_trace": trace, "pipeline_roofline": pipe,
            "beam5": beam, "cpu_baseline": cpu,
            "stages_s": {k: round(v, 3) for k, v in times.items() if isinstance(v, float)},
            "counts": {k: v for k, v in times.items() if isinstance(v, int)},
            "segmentation": ({"stage": "pyannote", "s_per_step": round(vad_t[0] / args.steps, 4), "segments": vad_t[1],
                              "windows": n_total // 160000 + 1 if world > 1 else pcm.size // 160000 + 1, "gpu_ms": round(dia.stats()[0], 2)} if diarize else
                             {"stage": "silero", "s_per_step": round(vad_t[0] / args.steps, 4), "segments": vad_t[1],
                              "chunks": ((n_total if world > 1 else pcm.size) + 511) // 512,
                              "us_per_chunk": round(vad.last_us_per_step, 3)}),
            "load_s": round(t_load, 2), "segments_out": n_out // max(1, args.steps),
            # host CPU time of the timed steps (all threads of the process, user + system): the
            # box grants one GPU's process 16 CPUs (cgroup cpu.max)
            "host_cpu": {"cpu_s": round(host_cpu_s, 3), "wall_s": round(dt, 3),
                         "cpus_busy": round(host_cpu_s / max(dt, 1e-9), 2),
                         "cg_throttled": th1[0] - th0[0], "cg_throttled_s": round((th1[1] - th0[1]) * 1e-6, 3),
                         "by_thread_name": thread_cpu_s, "throttle_at_s": thr_log or None,
                         "segmentation_s": round(vad_t[0], 3)},
        }
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()
    # every libwdr handle (context threads, streams, device memory) released while the HIP
    # runtime is up -- not left to interpreter teardown (wdr_shutdown, include/wdr.h)
    lib.wdr_shutdown()


if __name__ == "__main__":
    main()
