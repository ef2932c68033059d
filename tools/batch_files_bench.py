"""Many short recordings: a loop of Engine.transcribe_audio calls against one
Engine.transcribe_batch, and 64 sequential Vad.probs calls against one Vad.probs_batch.

32 synthetic 60-s files (wdr.synth, a different seed each), large-v3 on synthetic weights with DTW,
Silero VAD on, greedy, lang auto.  Every timed section follows one untimed pass of the same work
(context creation, stream pools, graph capture and first-touch allocations are not what is
compared).  The batch's lists are checked against the loop's before anything is printed.

  python tools/batch_files_bench.py               # all four walls, one JSON line
  python tools/batch_files_bench.py --loop-only   # the two loops only: runs on a commit without
                                                  # the batch entry points (the parent, for the A/B)
  python tools/batch_files_bench.py --diarize     # the diarized line: enable_diarize instead of VAD
                                                  # (Engine.set_batch_diarize), and 32 Diarizer.frame_classes
                                                  # calls against one frame_classes_batch (GPU time from
                                                  # wdr_diarize_stats); with --loop-only on the parent too
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "whisper-diarize-rs_amd"))
import wdr  # noqa: E402
from oracle.pipeline import write_wav  # noqa: E402
from wdr.synth import synth_speech  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--vad-sequences", type=int, default=64)
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--diarize", action="store_true")
    a = ap.parse_args()

    pcms = [synth_speech(a.seconds, seed=100 + k, n_speakers=2)[0] for k in range(a.files)]
    res = {"files": a.files, "seconds": a.seconds, "model": a.model, "audio_s": a.files * a.seconds}
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for k, pcm in enumerate(pcms):
            paths.append(os.path.join(d, "f%02d.wav" % k))
            write_wav(paths[-1], pcm)
        syn = wdr.Synthetic(weight_std=0.02, emb_std=0.02, force_len_rate=3.3, disable_fallback=True)
        eng = wdr.Engine(wdr.EngineConfig(cache_dir=d, enable_dtw=True, gpu_device=0), synthetic=syn)
        opts = wdr.TranscribeOptions(model=a.model, lang="auto", enable_vad=True,
                                     enable_diarize=True if a.diarize else None,
                                     advanced=wdr.AdvancedTranscribe(sampling_strategy="greedy"))
        if a.diarize:
            res["diarize"] = True
            if not a.loop_only:
                eng.set_batch_diarize(True)
        for p in paths[:4]:                      # warm-up: context, VAD, streams
            eng.transcribe_audio(p, opts)
        t = time.perf_counter()
        loop = [eng.transcribe_audio(p, opts) for p in paths]
        res["loop_wall_s"] = round(time.perf_counter() - t, 4)
        res["loop_xrt"] = round(res["audio_s"] / res["loop_wall_s"], 1)
        res["segments"] = sum(len(x) for x in loop)
        if a.diarize:
            res["speakers"] = sum(len({s.speaker_id for s in x}) for x in loop)
            res["loop_stage_s"] = {k: round(v, 3) for k, v in eng.stage_times(a.model).items()
                                   if k in ("embed", "decode", "encode", "dtw")}     # the last file's call
        if not a.loop_only:
            eng.transcribe_batch(paths, opts)    # warm-up: the chains' states, the batch's VAD buffers
            t = time.perf_counter()
            got = eng.transcribe_batch(paths, opts)
            res["batch_wall_s"] = round(time.perf_counter() - t, 4)
            res["batch_xrt"] = round(res["audio_s"] / res["batch_wall_s"], 1)
            st = eng.stage_times(a.model)
            res["batch_chains"] = st["chains"]
            if a.diarize:
                res["batch_stage_s"] = {k: round(st[k], 3) for k in ("embed", "decode", "encode", "dtw")}
            assert [g.error for g in got] == [None] * len(paths)
            assert [g.segments for g in got] == loop, "batch and loop disagree"
        eng.close()

    if a.diarize:
        dz = wdr.Diarizer(gpu_device=0)
        one = [dz.frame_classes(x, logprobs=True) for x in pcms]     # warm-up (and the reference)
        gpu_ms = 0.0
        t = time.perf_counter()
        for x in pcms:
            dz.frame_classes(x)
            gpu_ms += dz.stats()[0]
        res["seg_loop_wall_s"] = round(time.perf_counter() - t, 4)
        res["seg_loop_gpu_ms"] = round(gpu_ms, 2)
        res["seg_windows"] = sum(c.shape[0] for c, _ in one)
        if not a.loop_only:
            many = dz.frame_classes_batch(pcms, logprobs=True)
            t = time.perf_counter()
            dz.frame_classes_batch(pcms)
            res["seg_batch_wall_s"] = round(time.perf_counter() - t, 4)
            res["seg_batch_gpu_ms"] = round(dz.stats()[0], 2)
            assert all(np.array_equal(c, d) and np.array_equal(p.view(np.uint32), q.view(np.uint32))
                       for (c, p), (d, q) in zip(one, many)), "batched and per-file segmentation disagree"
        print(json.dumps(res))
        return

    vad = wdr.Vad(gpu_device=0)
    seqs = [pcms[k % len(pcms)] for k in range(a.vad_sequences)]
    one = [vad.probs(x) for x in seqs]           # warm-up (and the reference)
    t = time.perf_counter()
    for x in seqs:
        vad.probs(x)
    res["vad_loop_wall_s"] = round(time.perf_counter() - t, 4)
    if not a.loop_only:
        vad.probs_batch(seqs)
        t = time.perf_counter()
        many = vad.probs_batch(seqs)
        res["vad_batch_wall_s"] = round(time.perf_counter() - t, 4)
        res["vad_batch_us_per_chunk"] = round(vad.last_us_per_step, 4)
        assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(one, many))
    vad.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
