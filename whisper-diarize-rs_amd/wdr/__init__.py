"""Python mirror of the whisper-diarize-rs public API over libwdr's C ABI.

Same names, argument meaning and error behaviour as the reference crate
(src/lib.rs:12-17 re-exports; src/types.rs; src/engine.rs), so a caller of
`Engine::transcribe_audio` finds the same surface.  Every call goes through
libwdr.so (HIP, gfx950); there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import enum
from typing import Callable, List, Optional

import numpy as np

from . import _lib as L

__all__ = ["Engine", "EngineConfig", "TranscribeOptions", "AdvancedTranscribe", "DiarizeOptions", "Segment",
           "WordTimestamp",
           "ProgressType", "Callbacks", "Synthetic", "WhisperContext", "SpeechSegment", "read_wav", "vad_merge",
           "WdrError", "BatchResult", "BatchCallbacks"]

WdrError = L.WdrError


class ProgressType(enum.IntEnum):          # src/types.rs:5-9
    Download = 0
    Transcribe = 1
    Translate = 2


@dataclasses.dataclass
class AdvancedTranscribe:                  # src/types.rs:16-24
    sampling_strategy: Optional[str] = None
    best_of_or_beam_size: Optional[int] = None
    n_threads: Optional[int] = None
    temperature: Optional[float] = None
    max_text_ctx: Optional[int] = None
    init_prompt: Optional[str] = None
    diarize_threshold: Optional[float] = None


@dataclasses.dataclass
class TranscribeOptions:                   # src/types.rs:28-61 (defaults)
    offset: Optional[float] = 0.0
    model: str = "base"
    lang: Optional[str] = "auto"
    whisper_to_english: Optional[bool] = False
    translate_target: Optional[str] = None
    enable_vad: Optional[bool] = True
    enable_diarize: Optional[bool] = None
    max_speakers: Optional[int] = None
    advanced: Optional[AdvancedTranscribe] = None


@dataclasses.dataclass
class WordTimestamp:                       # src/types.rs:64-70
    text: str
    start: float
    end: float
    probability: Optional[float] = None


@dataclasses.dataclass
class Segment:                             # src/types.rs:74-82
    start: float
    end: float
    text: str
    words: Optional[List[WordTimestamp]] = None
    speaker_id: Optional[str] = None


@dataclasses.dataclass
class SpeechSegment:                       # src/types.rs:86-90
    start: float
    end: float
    samples: np.ndarray


@dataclasses.dataclass
class EngineConfig:                        # src/engine.rs:9-33 (defaults)
    cache_dir: str = "./cache"
    enable_dtw: Optional[bool] = True
    enable_flash_attn: Optional[bool] = False
    use_gpu: Optional[bool] = True
    gpu_device: Optional[int] = None
    vad_model_path: Optional[str] = None
    diarize_segment_model_path: Optional[str] = None
    diarize_embedding_model_path: Optional[str] = None


@dataclasses.dataclass
class Callbacks:                           # src/engine.rs:35-40
    progress: Optional[Callable[[int, ProgressType, str], None]] = None
    new_segment_callback: Optional[Callable[[Segment], None]] = None
    is_cancelled: Optional[Callable[[], bool]] = None


@dataclasses.dataclass
class BatchCallbacks:
    """Callbacks of Engine.transcribe_batch: new_segment_callback also gets the file's index."""
    progress: Optional[Callable[[int, ProgressType, str], None]] = None
    new_segment_callback: Optional[Callable[[int, Segment], None]] = None
    is_cancelled: Optional[Callable[[], bool]] = None


@dataclasses.dataclass
class BatchResult:
    """One file of Engine.transcribe_batch: its segments and detected language, or the error the
    single call would have raised for it (then segments is None)."""
    segments: Optional[List[Segment]] = None
    detected_lang: Optional[str] = None
    error: Optional[str] = None


@dataclasses.dataclass
class DiarizeOptions:                      # src/types.rs:93-98
    """Passed to run_transcription_pipeline to switch speakers on (src/transcribe.rs:339-345).
    A None model path selects synthetic seeded weights (no model files offline)."""
    segment_model_path: Optional[str] = None
    embedding_model_path: Optional[str] = None
    threshold: float = 0.5
    max_speakers: int = 2 ** 64 - 1      # usize::MAX, the Engine's mapping of None / Some(0)

    @staticmethod
    def from_options(o: "TranscribeOptions", segment_model_path=None, embedding_model_path=None):
        """The DiarizeOptions Engine::transcribe_audio builds (src/engine.rs:101-111)."""
        thr = o.advanced.diarize_threshold if (o.advanced and o.advanced.diarize_threshold is not None) else 0.5
        mx = o.max_speakers if o.max_speakers else 2 ** 64 - 1
        return DiarizeOptions(segment_model_path, embedding_model_path, thr, mx)


def _dopts(d: Optional[DiarizeOptions], keep):
    if d is None:
        return None
    return keep(L.DiarizeOptions(keep(_s(d.segment_model_path)), keep(_s(d.embedding_model_path)), d.threshold,
                                 d.max_speakers))


@dataclasses.dataclass
class Synthetic:
    """Synthetic-weight / workload-pin knobs (no checkpoints here)."""
    weight_std: float = 0.02
    emb_std: float = 0.02
    force_len_rate: float = 0.0
    disable_fallback: bool = False


def _ob(v):
    return -1 if v is None else (1 if v else 0)


def _s(v):
    return None if v is None else v.encode()


class _Keep:
    """Keeps ctypes buffers alive for the duration of a call."""

    def __init__(self):
        self.objs = []

    def __call__(self, o):
        self.objs.append(o)
        return o


def _opts(o: Optional[TranscribeOptions], keep: _Keep):
    if o is None:
        return None
    t = L.TranscribeOptions()
    t.has_offset = 0 if o.offset is None else 1
    t.offset = o.offset or 0.0
    t.model = keep(_s(o.model))
    t.lang = keep(_s(o.lang))
    t.whisper_to_english = _ob(o.whisper_to_english)
    t.translate_target = keep(_s(o.translate_target))
    t.enable_vad = _ob(o.enable_vad)
    t.enable_diarize = _ob(o.enable_diarize)
    t.has_max_speakers = 0 if o.max_speakers is None else 1
    t.max_speakers = o.max_speakers or 0
    if o.advanced is not None:
        a = o.advanced
        A = L.Advanced()
        A.sampling_strategy = keep(_s(a.sampling_strategy))
        for f in ("best_of_or_beam_size", "n_threads", "temperature", "max_text_ctx", "diarize_threshold"):
            v = getattr(a, f)
            setattr(A, "has_" + f, 0 if v is None else 1)
            setattr(A, f, v or 0)
        A.init_prompt = keep(_s(a.init_prompt))
        keep(A)
        t.advanced = C.pointer(A)
    return keep(t)


def _syn(s: Optional[Synthetic]):
    if s is None:
        return None
    return L.Synthetic(s.weight_std, s.emb_std, s.force_len_rate, 1 if s.disable_fallback else 0)


@dataclasses.dataclass
class FormattingOverrides:                 # src/formatting.rs:37-51
    max_chars_per_line: Optional[int] = None
    max_lines: Optional[int] = None
    cps_cap: Optional[float] = None
    split_gap_sec: Optional[float] = None
    comma_min_chars_before_allow: Optional[int] = None
    min_word_dur: Optional[float] = None
    min_sub_dur: Optional[float] = None
    max_sub_dur: Optional[float] = None
    soft_max_words_per_line: Optional[int] = None
    insert_interword_space: Optional[bool] = None
    use_grapheme_len: Optional[bool] = None
    enforce_kinsoku: Optional[bool] = None
    allow_comma_split: Optional[bool] = None


def _fmt(ov: Optional[FormattingOverrides]):
    if ov is None:
        return None
    f = L.FormattingOverrides()
    for name in ("max_chars_per_line", "max_lines", "cps_cap", "split_gap_sec", "comma_min_chars_before_allow",
                 "min_word_dur", "min_sub_dur", "max_sub_dur", "soft_max_words_per_line"):
        v = getattr(ov, name)
        setattr(f, "has_" + name, 0 if v is None else 1)
        setattr(f, name, v or 0)
    for name in ("insert_interword_space", "use_grapheme_len", "enforce_kinsoku", "allow_comma_split"):
        setattr(f, name, _ob(getattr(ov, name)))
    return f


def _raw_segments(segs: List[Segment], keep: "_Keep"):
    arr = (L.Segment * max(1, len(segs)))()
    for i, sg in enumerate(segs):
        arr[i].start, arr[i].end = sg.start, sg.end
        arr[i].text = keep(sg.text.encode())
        if sg.words is not None:
            w = (L.Word * max(1, len(sg.words)))()
            for k, x in enumerate(sg.words):
                w[k].text = keep(x.text.encode())
                w[k].start, w[k].end = x.start, x.end
                w[k].has_probability = 0 if x.probability is None else 1
                w[k].probability = x.probability or 0.0
            keep(w)
            arr[i].words = C.cast(w, C.POINTER(L.Word))
            arr[i].n_words = len(sg.words)
        arr[i].speaker_id = keep(None if sg.speaker_id is None else sg.speaker_id.encode())
    keep(arr)
    return arr


def process_segments(segments: List[Segment], lang: str = "auto", overrides: Optional[FormattingOverrides] = None,
                     vad_mask=None) -> List[Segment]:
    """formatting::process_segments with PostProcessConfig::for_language(lang) + overrides and
    an optional VAD mask oracle (src/engine.rs:192-199)."""
    lib = L.load()
    keep = _Keep()
    arr = _raw_segments(segments, keep)
    ov = _fmt(overrides)
    m = np.ascontiguousarray(np.asarray(vad_mask if vad_mask is not None else [], np.float64).reshape(-1))
    out = C.POINTER(L.SegmentList)()
    L.check(lib.wdr_process_segments(arr, len(segments), lang.encode(), C.byref(ov) if ov is not None else None,
                                     0 if vad_mask is None else 1, m.ctypes.data_as(C.POINTER(C.c_double)),
                                     m.size // 2, C.byref(out)))
    return _segments(out)[0]


def _segments(lst_ptr, with_index: bool = False, free: bool = True) -> tuple:
    lst = lst_ptr.contents
    index = [int(lst.speech_index[i]) for i in range(lst.n_segments)] if lst.speech_index else None
    out = []
    for i in range(lst.n_segments):
        s = lst.segments[i]
        words = None
        if s.words:
            words = [WordTimestamp(s.words[k].text.decode("utf-8", "replace"), s.words[k].start, s.words[k].end,
                                   s.words[k].probability if s.words[k].has_probability else None)
                     for k in range(s.n_words)]
        out.append(Segment(s.start, s.end, s.text.decode("utf-8", "replace"), words,
                           s.speaker_id.decode() if s.speaker_id else None))
    lang = lst.detected_lang.decode() if lst.detected_lang else None
    if free:
        L.load().wdr_segment_list_free(lst_ptr)
    return (out, lang, index) if with_index else (out, lang)


def _callbacks(cb: Optional[Callbacks], keep: _Keep):
    if cb is None:
        return None
    c = L.Callbacks()
    if cb.progress:
        c.progress = keep(L.PROGRESS_FN(lambda u, p, t, lbl: cb.progress(int(p), ProgressType(t), lbl.decode())))
    if cb.new_segment_callback:
        def seg_cb(u, sp):
            s = sp.contents
            words = None
            if s.words:
                words = [WordTimestamp(s.words[k].text.decode(), s.words[k].start, s.words[k].end,
                                       s.words[k].probability if s.words[k].has_probability else None)
                         for k in range(s.n_words)]
            cb.new_segment_callback(Segment(s.start, s.end, s.text.decode(), words,
                                            s.speaker_id.decode() if s.speaker_id else None))
        c.new_segment = keep(L.SEGMENT_FN(seg_cb))
    if cb.is_cancelled:
        c.is_cancelled = keep(L.CANCEL_FN(lambda u: 1 if cb.is_cancelled() else 0))
    return keep(c)


def read_wav(path: str) -> np.ndarray:
    """audio::read_wav (src/audio.rs:4-24)."""
    lib = L.load()
    p = C.POINTER(C.c_int16)()
    n = C.c_size_t()
    L.check(lib.wdr_read_wav(path.encode(), C.byref(p), C.byref(n)))
    out = np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, np.int16)
    lib.wdr_free(p)
    return out


AUDIO_FORMATS = {"u8": 0, "i16": 1, "i24": 2, "i32": 3, "f32": 4}
AUDIO_SAMPLE_BYTES = {0: 1, 1: 2, 2: 3, 3: 4, 4: 4}


def _take_i16(lib, p, n):
    try:
        return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.int16)
    finally:
        lib.wdr_free(C.cast(p, C.c_void_p))


def audio_info(path: str) -> dict:
    """Header of any supported WAV file (wdr_audio_info; host only): PCM 8 / 16 / 24 / 32-bit or
    IEEE f32, 1..8 channels, 1000..384000 Hz, plain or extensible header.  Not in the reference."""
    lib = L.load()
    info = (C.c_int32 * 5)()
    nf = C.c_uint64()
    L.check(lib.wdr_audio_info(path.encode(), info, C.byref(nf)))
    fmt, ch, rate, bits, align = list(info)
    return {"fmt": fmt, "channels": ch, "rate": rate, "bits": bits, "block_align": align, "n_frames": nf.value}


def read_audio(path: str, gpu_device: Optional[int] = None) -> np.ndarray:
    """Any supported WAV -> 16 kHz mono int16, downmixed and resampled on the GPU (wdr_read_audio).
    A file read_wav accepts comes back identical to read_wav's result without touching the GPU.
    Not in the reference, which reads 16 kHz mono 16-bit files only."""
    lib = L.load()
    p = C.POINTER(C.c_int16)()
    n = C.c_size_t()
    L.check(lib.wdr_read_audio(path.encode(), 0 if gpu_device is None else 1, gpu_device or 0, C.byref(p), C.byref(n)))
    return _take_i16(lib, p, n.value)


def dbg_audio_convert(raw, fmt, channels: int, rate: int, chunk_frames: int = 0, host: bool = False,
                      timing: bool = False):
    """The audio conversion of raw interleaved frames (bytes / uint8 array) of format `fmt` ('u8',
    'i16', 'i24', 'i32', 'f32' or 0..4) -> 16 kHz mono int16 (wdr_dbg_audio_convert).  host=True:
    the host definition, no GPU; else the kernels, in chunks of chunk_frames input frames (0 = the
    default); with timing also the mean GPU milliseconds of 10 further runs of the kernels."""
    lib = L.load()
    f = AUDIO_FORMATS.get(fmt, fmt)
    if f not in AUDIO_SAMPLE_BYTES:
        raise ValueError("unknown sample format %r" % (fmt,))
    if not 1 <= channels <= 8:
        raise ValueError("1 to 8 channels")
    buf = np.ascontiguousarray(np.frombuffer(bytes(raw), np.uint8) if not isinstance(raw, np.ndarray)
                               else raw.view(np.uint8).ravel())
    fb = AUDIO_SAMPLE_BYTES[f] * channels
    if buf.size % fb:
        raise ValueError("%d bytes are not whole %d-byte frames" % (buf.size, fb))
    p = C.POINTER(C.c_int16)()
    n = C.c_size_t()
    ms = C.c_double()
    L.check(lib.wdr_dbg_audio_convert(buf.ctypes.data_as(C.POINTER(C.c_uint8)), buf.size // fb, f, channels, rate,
                                      chunk_frames, 1 if host else 0, C.byref(p), C.byref(n),
                                      C.byref(ms) if timing and not host else None))
    out = _take_i16(lib, p, n.value)
    return (out, ms.value) if timing else out


def read_audio_channels(path: str, gpu_device: Optional[int] = None) -> np.ndarray:
    """Any supported WAV -> 16 kHz int16 [channels][n], every channel resampled on its own on the
    GPU (wdr_read_audio_channels): channel c equals read_audio of the mono file holding channel c.
    A 16 kHz mono 16-bit file comes back as read_wav's result without touching the GPU.  Not in the
    reference."""
    lib = L.load()
    p = C.POINTER(C.c_int16)()
    n = C.c_size_t()
    ch = C.c_int32()
    L.check(lib.wdr_read_audio_channels(path.encode(), 0 if gpu_device is None else 1, gpu_device or 0, C.byref(p),
                                        C.byref(n), C.byref(ch)))
    return _take_i16(lib, p, n.value * ch.value).reshape(ch.value, n.value)


def dbg_audio_split(raw, fmt, channels: int, rate: int, chunk_frames: int = 0, host: bool = False,
                    timing: bool = False):
    """dbg_audio_convert's channel-keeping form (wdr_dbg_audio_split): raw interleaved frames ->
    16 kHz int16 [channels][n_out], no downmix.  host=True: the definition (channel c is the mono
    definition on sample c of every frame), no GPU; else the kernels; timing as there."""
    lib = L.load()
    f = AUDIO_FORMATS.get(fmt, fmt)
    if f not in AUDIO_SAMPLE_BYTES:
        raise ValueError("unknown sample format %r" % (fmt,))
    if not 1 <= channels <= 8:
        raise ValueError("1 to 8 channels")
    buf = np.ascontiguousarray(np.frombuffer(bytes(raw), np.uint8) if not isinstance(raw, np.ndarray)
                               else raw.view(np.uint8).ravel())
    fb = AUDIO_SAMPLE_BYTES[f] * channels
    if buf.size % fb:
        raise ValueError("%d bytes are not whole %d-byte frames" % (buf.size, fb))
    p = C.POINTER(C.c_int16)()
    n = C.c_size_t()
    ms = C.c_double()
    L.check(lib.wdr_dbg_audio_split(buf.ctypes.data_as(C.POINTER(C.c_uint8)), buf.size // fb, f, channels, rate,
                                    chunk_frames, 1 if host else 0, C.byref(p), C.byref(n),
                                    C.byref(ms) if timing and not host else None))
    out = _take_i16(lib, p, n.value * channels).reshape(channels, n.value)
    return (out, ms.value) if timing else out


def dbg_resample_table(rate: int):
    """(L, M, T, tab [L][T] float32): the resampler's coefficient table of a source rate
    (wdr_dbg_resample_table; host only)."""
    lib = L.load()
    l, m, t = C.c_int32(), C.c_int32(), C.c_int32()
    p = C.POINTER(C.c_float)()
    L.check(lib.wdr_dbg_resample_table(rate, C.byref(l), C.byref(m), C.byref(t), C.byref(p)))
    try:
        n = l.value * t.value
        tab = np.ctypeslib.as_array(p, shape=(max(1, n),))[:n].copy().reshape(l.value, t.value)
    finally:
        lib.wdr_free(C.cast(p, C.c_void_p))
    return l.value, m.value, t.value, tab


def vad_merge(segs_cs, samples: np.ndarray):
    """The crate's own post-processing of whisper.cpp VAD segments (src/vad.rs:33-84)."""
    lib = L.load()
    st = np.ascontiguousarray([s for s, _ in segs_cs], np.float64)
    en = np.ascontiguousarray([e for _, e in segs_cs], np.float64)
    n = len(st)
    mask = np.zeros(2 * max(n, 1))
    merged = np.zeros(2 * max(n, 1))
    idx = np.zeros(2 * max(n, 1), np.int64)
    nm, nmr = C.c_size_t(), C.c_size_t()
    smp = np.ascontiguousarray(samples, np.int16)
    L.check(lib.wdr_vad_merge(st.ctypes.data_as(C.POINTER(C.c_double)), en.ctypes.data_as(C.POINTER(C.c_double)), n,
                              smp.ctypes.data_as(C.POINTER(C.c_int16)), smp.size,
                              mask.ctypes.data_as(C.POINTER(C.c_double)), C.byref(nm),
                              merged.ctypes.data_as(C.POINTER(C.c_double)), idx.ctypes.data_as(C.POINTER(C.c_int64)),
                              C.byref(nmr)))
    m = [(mask[2 * i], mask[2 * i + 1]) for i in range(nm.value)]
    out = [SpeechSegment(merged[2 * i], merged[2 * i + 1], smp[idx[2 * i]:idx[2 * i + 1]].copy())
           for i in range(nmr.value)]
    return m, out


def vad_segments_from_probs(probs) -> list:
    """whisper.cpp whisper_vad_segments_from_probs with the reference's VAD params
    (src/vad.rs:21-22): [(start_cs, end_cs)] as f32 values."""
    lib = L.load()
    p = np.ascontiguousarray(probs, np.float32)
    out = np.zeros(2 * max(1, p.size), np.float32)
    n = C.c_size_t()
    L.check(lib.wdr_vad_segments_from_probs(p.ctypes.data_as(C.POINTER(C.c_float)), p.size,
                                            out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n)))
    return [(float(out[2 * i]), float(out[2 * i + 1])) for i in range(n.value)]


class Vad:
    """Silero VAD on the GPU (src/vad.rs:6-85).  model_path: whisper.cpp's ggml-silero-v5.1.2.bin;
    None = synthetic seeded weights."""

    def __init__(self, model_path: Optional[str] = None, gpu_device: Optional[int] = None):
        self._lib = L.load()
        h = C.c_void_p()
        L.check(self._lib.wdr_vad_create(_s(model_path), 0 if gpu_device is None else 1, gpu_device or 0, C.byref(h)))
        self.h = h
        self.last_us_per_step = 0.0

    def probs(self, samples: np.ndarray) -> np.ndarray:
        smp = np.ascontiguousarray(samples, np.int16)
        out = np.zeros((smp.size + 511) // 512, np.float32)
        us = C.c_double()
        L.check(self._lib.wdr_vad_probs(self.h, smp.ctypes.data_as(C.POINTER(C.c_int16)), smp.size,
                                        out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(us)))
        self.last_us_per_step = us.value
        return out

    def probs_batch(self, sequences) -> list:
        """probs() of several independent recordings in one pass (wdr_vad_probs_batch: one upload,
        three launches, one sync; the LSTM scans run side by side, one workgroup each).  Returns one
        array per sequence, bit-identical to probs() of it; empty sequences are legal."""
        smp = [np.ascontiguousarray(x, np.int16).reshape(-1) for x in sequences]
        B = len(smp)
        ptrs = (C.POINTER(C.c_int16) * max(B, 1))(*[x.ctypes.data_as(C.POINTER(C.c_int16)) for x in smp])
        ns = (C.c_size_t * max(B, 1))(*[x.size for x in smp])
        cnt = [(x.size + 511) // 512 for x in smp]
        out = np.zeros(max(1, sum(cnt)), np.float32)
        us = C.c_double()
        L.check(self._lib.wdr_vad_probs_batch(self.h, ptrs, ns, B, out.ctypes.data_as(C.POINTER(C.c_float)),
                                              C.byref(us)))
        self.last_us_per_step = us.value
        ends = np.cumsum([0] + cnt)
        return [out[ends[b]:ends[b + 1]].copy() for b in range(B)]

    def get_segments(self, samples: np.ndarray, materialize: bool = True):
        """-> (mask [(start_s, end_s)], [SpeechSegment]) exactly as vad::get_segments.
        materialize=False returns only the segment (start, end) pairs (no sample copies)."""
        smp = np.ascontiguousarray(samples, np.int16)
        mp, nm = C.POINTER(C.c_double)(), C.c_size_t()
        sp, ns = C.POINTER(L.SpeechSegment)(), C.c_size_t()
        L.check(self._lib.wdr_vad_get_segments(self.h, smp.ctypes.data_as(C.POINTER(C.c_int16)), smp.size,
                                               C.byref(mp), C.byref(nm), C.byref(sp), C.byref(ns)))
        us = C.c_double()
        L.check(self._lib.wdr_vad_stats(self.h, C.byref(us)))
        self.last_us_per_step = us.value
        try:
            mask = [(mp[2 * i], mp[2 * i + 1]) for i in range(nm.value)]
            base = smp.ctypes.data
            segs = []
            for i in range(ns.value):
                s = sp[i]
                if not materialize:
                    segs.append((s.start, s.end))
                    continue
                off = (C.cast(s.samples, C.c_void_p).value - base) // 2
                segs.append(SpeechSegment(s.start, s.end, smp[off:off + s.n_samples].copy()))
        finally:
            self._lib.wdr_free(C.cast(mp, C.c_void_p))
            self._lib.wdr_free(C.cast(sp, C.c_void_p))
        return mask, segs

    def close(self):
        if self.h:
            self._lib.wdr_vad_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SpeakerManager:
    """pyannote_rs::EmbeddingManager as the reference drives it (src/transcribe.rs:478-497)."""

    def __init__(self, max_speakers: Optional[int] = None):
        self._lib = L.load()
        h = C.c_void_p()
        L.check(self._lib.wdr_speakers_new(0 if max_speakers is None else 1, max_speakers or 0, C.byref(h)))
        self.h = h

    def assign(self, emb, threshold: float = 0.5) -> str:
        buf = C.create_string_buffer(32)
        if emb is None:
            L.check(self._lib.wdr_speakers_assign(self.h, None, 0, threshold, buf, 32))
        else:
            e = np.ascontiguousarray(emb, np.float32)
            L.check(self._lib.wdr_speakers_assign(self.h, e.ctypes.data_as(C.POINTER(C.c_float)), e.size, threshold,
                                                  buf, 32))
        return buf.value.decode()

    def __del__(self):
        try:
            self._lib.wdr_speakers_free(self.h)
        except Exception:
            pass


class Diarizer:
    """pyannote segmentation-3.0 + CAM++ on the GPU (src/engine.rs:89-122,
    src/transcribe.rs:461-497).  Model paths: the ONNX files; None = synthetic seeded weights."""

    def __init__(self, gpu_device: Optional[int] = None, segment_model_path: Optional[str] = None,
                 embedding_model_path: Optional[str] = None):
        self._lib = L.load()
        h = C.c_void_p()
        L.check(self._lib.wdr_diarizer_create(_s(segment_model_path), _s(embedding_model_path),
                                              0 if gpu_device is None else 1, gpu_device or 0, C.byref(h)))
        self.h = h

    def frame_classes(self, samples: np.ndarray, logprobs: bool = False):
        smp = np.ascontiguousarray(samples, np.int16)
        nw = smp.size // 160000 + 1
        cls = np.zeros(nw * 589, np.int32)
        lp = np.zeros(nw * 589 * 7, np.float32) if logprobs else None
        L.check(self._lib.wdr_diarize_frame_classes(self.h, smp.ctypes.data_as(C.POINTER(C.c_int16)), smp.size,
                                                    cls.ctypes.data_as(C.POINTER(C.c_int32)),
                                                    lp.ctypes.data_as(C.POINTER(C.c_float)) if logprobs else None))
        cls = cls.reshape(nw, 589)
        return (cls, lp.reshape(nw, 589, 7)) if logprobs else cls

    def frame_classes_batch(self, sequences, logprobs: bool = False, window_cap: int = 0):
        """frame_classes() of several recordings in shared forwards (wdr_diarize_frame_classes_batch:
        all files' windows stacked, up to window_cap -- 0 = the default, 128 -- per forward).  Returns
        one result per sequence, bit-identical to frame_classes() of it; empty sequences are legal."""
        smp = [np.ascontiguousarray(x, np.int16).reshape(-1) for x in sequences]
        B = len(smp)
        ptrs = (C.POINTER(C.c_int16) * max(B, 1))(*[x.ctypes.data_as(C.POINTER(C.c_int16)) for x in smp])
        ns = (C.c_size_t * max(B, 1))(*[x.size for x in smp])
        nw = [x.size // 160000 + 1 for x in smp]
        tot = max(1, sum(nw))
        cls = np.zeros(tot * 589, np.int32)
        lp = np.zeros(tot * 589 * 7, np.float32) if logprobs else None
        L.check(self._lib.wdr_diarize_frame_classes_batch(self.h, ptrs, ns, B, window_cap,
                                                          cls.ctypes.data_as(C.POINTER(C.c_int32)),
                                                          lp.ctypes.data_as(C.POINTER(C.c_float)) if logprobs else None))
        ends = np.cumsum([0] + nw)
        out = []
        for b in range(B):
            c = cls[ends[b] * 589:ends[b + 1] * 589].reshape(nw[b], 589).copy()
            out.append((c, lp[ends[b] * 589 * 7:ends[b + 1] * 589 * 7].reshape(nw[b], 589, 7).copy())
                       if logprobs else c)
        return out

    def get_segments(self, samples: np.ndarray, materialize: bool = True):
        """pyannote_rs::get_segments (wdr_diarize_get_segments: the segments and their samples are
        made in libwdr).  materialize=False returns (start, end) pairs without copying every
        segment's samples a second time into Python arrays (as Vad.get_segments)."""
        smp = np.ascontiguousarray(samples, np.int16)
        sp, ns = C.POINTER(L.SpeechSegment)(), C.c_size_t()
        L.check(self._lib.wdr_diarize_get_segments(self.h, smp.ctypes.data_as(C.POINTER(C.c_int16)), smp.size,
                                                   C.byref(sp), C.byref(ns)))
        try:
            if not materialize:
                return [(sp[i].start, sp[i].end) for i in range(ns.value)]
            return [SpeechSegment(sp[i].start, sp[i].end, np.ctypeslib.as_array(sp[i].samples, (sp[i].n_samples,)).copy()
                                  if sp[i].n_samples else np.zeros(0, np.int16)) for i in range(ns.value)]
        finally:
            self._lib.wdr_free(C.cast(sp, C.c_void_p))

    @staticmethod
    def segments_from_classes(cls: np.ndarray, samples: np.ndarray):
        """pyannote_rs::get_segments' stitching of frame classes [n/160000 + 1][589] computed
        elsewhere (window shards of several GPUs)."""
        smp = np.ascontiguousarray(samples, np.int16)
        c = np.ascontiguousarray(cls, np.int32)
        sp, ns = C.POINTER(L.SpeechSegment)(), C.c_size_t()
        lib = L.load()
        L.check(lib.wdr_diarize_segments_from_classes(c.ctypes.data_as(C.POINTER(C.c_int32)), c.shape[0],
                                                      smp.ctypes.data_as(C.POINTER(C.c_int16)), smp.size,
                                                      C.byref(sp), C.byref(ns)))
        try:
            return [SpeechSegment(sp[i].start, sp[i].end, np.ctypeslib.as_array(sp[i].samples, (sp[i].n_samples,)).copy()
                                  if sp[i].n_samples else np.zeros(0, np.int16)) for i in range(ns.value)]
        finally:
            lib.wdr_free(C.cast(sp, C.c_void_p))

    def fbank(self, samples: np.ndarray) -> np.ndarray:
        smp = np.ascontiguousarray(samples, np.int16)
        out = np.zeros((smp.size // 160 + 1, 80), np.float32)
        nf = C.c_size_t()
        L.check(self._lib.wdr_diarize_fbank(self.h, smp.ctypes.data_as(C.POINTER(C.c_int16)), smp.size,
                                            out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(nf)))
        return out[:nf.value]

    def embedding(self, samples: np.ndarray):
        smp = np.ascontiguousarray(samples, np.int16)
        out = np.zeros(512, np.float32)
        ok = C.c_int8()
        L.check(self._lib.wdr_diarize_embedding(self.h, smp.ctypes.data_as(C.POINTER(C.c_int16)), smp.size,
                                                out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(ok)))
        return out if ok.value else None

    def embedding_batch(self, segments):
        """Embeddings of several utterances in one batched forward (wdr_diarize_embedding_batch):
        a list with None where embedding() would return None."""
        smp = [np.ascontiguousarray(x, np.int16) for x in segments]
        B = len(smp)
        ptrs = (C.POINTER(C.c_int16) * max(B, 1))(*[x.ctypes.data_as(C.POINTER(C.c_int16)) for x in smp])
        ns = (C.c_size_t * max(B, 1))(*[x.size for x in smp])
        out = np.zeros((max(B, 1), 512), np.float32)
        ok = (C.c_int8 * max(B, 1))()
        L.check(self._lib.wdr_diarize_embedding_batch(self.h, ptrs, ns, B, out.ctypes.data_as(C.POINTER(C.c_float)), ok))
        return [out[b].copy() if ok[b] else None for b in range(B)]

    def stats(self):
        a, b = C.c_double(), C.c_double()
        L.check(self._lib.wdr_diarize_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def __del__(self):
        try:
            self._lib.wdr_diarizer_free(self.h)
        except Exception:
            pass


def model_file_tensors(kind: str, path: str) -> dict:
    """Tensors of a VAD / diarization model file as libwdr's loader maps them (oracle names):
    kind 'silero' (whisper.cpp ggml), 'segmentation' / 'campplus' (ONNX).  Host only."""
    lib = L.load()
    k = {"silero": 0, "segmentation": 1, "campplus": 2}[kind]
    names, data, n = C.c_void_p(), C.POINTER(C.c_float)(), C.c_size_t()
    L.check(lib.wdr_dbg_model_file(k, path.encode(), C.byref(names), C.byref(data), C.byref(n)))
    try:
        txt = C.cast(names, C.c_char_p).value.decode()
        flat = np.ctypeslib.as_array(data, (max(1, n.value),))[:n.value].copy()
    finally:
        lib.wdr_free(names)
        lib.wdr_free(C.cast(data, C.c_void_p))
    out, o = {}, 0
    for line in txt.splitlines():
        name, cnt = line.rsplit(":", 1)
        out[name] = flat[o:o + int(cnt)]
        o += int(cnt)
    return out


def ggml_info(path: str) -> dict:
    """Header of a whisper.cpp ggml model file (wdr_ggml_info; parses the whole file, no GPU)."""
    lib = L.load()
    hp = (C.c_int32 * 11)()
    nt, nv = C.c_int64(), C.c_int64()
    L.check(lib.wdr_ggml_info(path.encode(), hp, C.byref(nt), C.byref(nv)))
    keys = ["n_vocab", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer", "n_text_ctx",
            "n_text_state", "n_text_head", "n_text_layer", "n_mels", "ftype"]
    counts = (C.c_int64 * 16)()
    L.check(lib.wdr_ggml_tensor_types(path.encode(), counts))
    ftype = hp[10]
    return {**dict(zip(keys, list(hp))), "n_tensors": nt.value, "n_vocab_tokens": nv.value,
            # quantized files (whisper.cpp's quantize tool): ftype = base + 1000 * qnt_version
            "ftype_base": ftype % 1000, "qnt_version": ftype // 1000,
            "tensor_types": {i: int(c) for i, c in enumerate(counts) if c}}


GGML_QUANT_TYPES = {"q4_0": 2, "q4_1": 3, "q5_0": 6, "q5_1": 7, "q8_0": 8}
GGML_BLOCK_BYTES = {2: 18, 3: 20, 6: 22, 7: 24, 8: 34}


def ggml_tensor_f16(path: str, name: str) -> np.ndarray:
    """One tensor of a whisper.cpp ggml model file as f16, flat (wdr_ggml_tensor_f16; no GPU).
    Quantized tensors go through the host definition of the block decode."""
    lib = L.load()
    out, n = C.POINTER(C.c_uint16)(), C.c_size_t()
    L.check(lib.wdr_ggml_tensor_f16(path.encode(), name.encode(), C.byref(out), C.byref(n)))
    try:
        return np.ctypeslib.as_array(out, (max(1, n.value),))[:n.value].copy().view(np.float16)
    finally:
        lib.wdr_free(C.cast(out, C.c_void_p))


def dbg_dequant(fmt, blocks, timing: bool = False):
    """The load-time dequantization kernel (wdr_dbg_dequant): raw blocks (bytes / uint8 array) of
    format `fmt` ('q4_0' .. 'q8_0' or the ggml type id) -> f16 [32 * n_blocks]; with timing also
    the mean GPU milliseconds of 10 further launches."""
    lib = L.load()
    t = GGML_QUANT_TYPES.get(fmt, fmt)
    raw = np.ascontiguousarray(np.frombuffer(bytes(blocks), np.uint8) if not isinstance(blocks, np.ndarray)
                               else blocks.astype(np.uint8, copy=False).ravel())
    bs = GGML_BLOCK_BYTES[t]
    if raw.size % bs:
        raise ValueError("%d bytes are not whole %d-byte blocks" % (raw.size, bs))
    nb = raw.size // bs
    out = np.empty(nb * 32, np.uint16)
    ms = C.c_double()
    L.check(lib.wdr_dbg_dequant(t, raw.ctypes.data_as(C.POINTER(C.c_uint8)), nb,
                                out.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(ms) if timing else None))
    return (out.view(np.float16), ms.value) if timing else out.view(np.float16)


_U16P, _I32P, _F32P = C.POINTER(C.c_uint16), C.POINTER(C.c_int32), C.POINTER(C.c_float)


def _h16(a):
    """A contiguous float16 copy of a, viewed as its bits."""
    return np.ascontiguousarray(np.asarray(a).astype(np.float16)).view(np.uint16)


def dbg_self_attn(q, kc, vc, row_seq, row_pos, n_head: int) -> np.ndarray:
    """Decode-step self-attention (wdr_dbg_self_attn): q [R][64 H], caches kc / vc [n_seq][T][64 H]
    (rounded to f16); row r attends over keys 0 .. row_pos[r] of sequence row_seq[r].  Returns
    [R][64 H] float32.  Out-of-range rows are an error, never a launch."""
    qb, kb, vb = _h16(q), _h16(kc), _h16(vc)
    rs, rp = np.ascontiguousarray(row_seq, np.int32), np.ascontiguousarray(row_pos, np.int32)
    R, d = qb.shape
    n_seq, T, dk = kb.shape
    if d != 64 * n_head or dk != d or vb.shape != kb.shape or rs.shape != (R,) or rp.shape != (R,):
        raise ValueError("dbg_self_attn: q [R][64 H], kc / vc [n_seq][T][64 H], row_seq / row_pos [R]")
    out = np.zeros((R, d), np.float32)
    L.check(L.load().wdr_dbg_self_attn(qb.ctypes.data_as(_U16P), kb.ctypes.data_as(_U16P), vb.ctypes.data_as(_U16P),
                                       n_seq, T, rs.ctypes.data_as(_I32P), rp.ctypes.data_as(_I32P), R, n_head,
                                       out.ctypes.data_as(_F32P)))
    return out


def dbg_proj_qkv(a, w, bias, row_seq, row_pos, kc, vc, packed=False):
    """The decoder's fused Q/K/V projection with the cache-scatter epilogue (wdr_dbg_proj_qkv):
    a [M][K], w [3 d][K] (rounded to f16), bias [3 d] or None, caches kc / vc [n_seq][T][d] float16.
    packed: the weight in the row kernel's fragment order (wdr_dbg_proj_qkv_packed).
    Returns (q [M][d] float32, kc, vc after the launch: float16 copies, the inputs are not touched)."""
    ab, wb = _h16(a), _h16(w)
    M, K = ab.shape
    d = wb.shape[0] // 3
    kb, vb = _h16(kc).copy(), _h16(vc).copy()
    n_seq, T, dk = kb.shape
    rs, rp = np.ascontiguousarray(row_seq, np.int32), np.ascontiguousarray(row_pos, np.int32)
    if wb.shape != (3 * d, K) or dk != d or vb.shape != kb.shape or rs.shape != (M,) or rp.shape != (M,):
        raise ValueError("dbg_proj_qkv: a [M][K], w [3 d][K], kc / vc [n_seq][T][d], row_seq / row_pos [M]")
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    q = np.zeros((M, d), np.float32)
    fn = L.load().wdr_dbg_proj_qkv_packed if packed else L.load().wdr_dbg_proj_qkv
    L.check(fn(ab.ctypes.data_as(_U16P), wb.ctypes.data_as(_U16P), None if b is None else b.ctypes.data_as(_F32P), M, d, K,
               rs.ctypes.data_as(_I32P), rp.ctypes.data_as(_I32P), n_seq, T, kb.ctypes.data_as(_U16P),
               vb.ctypes.data_as(_U16P), q.ctypes.data_as(_F32P)))
    return q, kb.view(np.float16), vb.view(np.float16)


SENTINEL_F16 = 0x7e57        # include/wdr.h WDR_DBG_SENTINEL_F16 / _F32: what an encoder seam's device
SENTINEL_F32 = 0x7fc07e57    # output holds where the kernel wrote nothing


def dbg_proj_enc(a, w, bias, epi: int, pos=None, gemm_ref: bool = False, slot_elems: int = 0) -> np.ndarray:
    """The encoder-only GEMM epilogues (wdr_dbg_proj_enc): a [M][K], w [N][K] (rounded to f16), bias
    [N] or None.  epi 4: pos [pos_rows][N] -> float32 [M][N] = gelu(a w^T + bias) + pos[row % pos_rows].
    epi 6: -> the raw cross-K/V slot images, float16 [M / 1500][slot_elems], SENTINEL_F16 bits where
    nothing was written.  gemm_ref: the reference tile k_gemm instead of the dispatched kernel."""
    ab, wb = _h16(a), _h16(w)
    M, K = ab.shape
    N = wb.shape[0]
    if wb.shape != (N, K):
        raise ValueError("dbg_proj_enc: a [M][K], w [N][K]")
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    p = None if pos is None else np.ascontiguousarray(pos, np.float32)
    if p is not None and (p.ndim != 2 or p.shape[1] != N):
        raise ValueError("dbg_proj_enc: pos [pos_rows][N]")
    if epi == 6:
        out = np.zeros((max(M // 1500, 1), int(slot_elems)), np.uint16)
    else:
        out = np.zeros((M, N), np.float32)
    L.check(L.load().wdr_dbg_proj_enc(ab.ctypes.data_as(_U16P), wb.ctypes.data_as(_U16P),
                                      None if b is None else b.ctypes.data_as(_F32P),
                                      None if p is None else p.ctypes.data_as(_F32P), 0 if p is None else p.shape[0],
                                      M, N, K, int(epi), 1 if gemm_ref else 0, int(slot_elems),
                                      out.ctypes.data_as(C.c_void_p)))
    return out.view(np.float16) if epi == 6 else out


def dbg_attn_batch(qkv, n_head: int) -> np.ndarray:
    """The encoder's batched self-attention launch (wdr_dbg_attn_batch): qkv [nb][T][3 * 64 H]
    (rounded to f16; Q, K, V of a row side by side) -> float32 [nb][T][64 H]."""
    qb = _h16(qkv)
    if qb.ndim != 3 or qb.shape[2] != 3 * 64 * n_head:
        raise ValueError("dbg_attn_batch: qkv [nb][T][3 * 64 H]")
    nb, T, _ = qb.shape
    out = np.zeros((nb, T, 64 * n_head), np.float32)
    L.check(L.load().wdr_dbg_attn_batch(qb.ctypes.data_as(_U16P), nb, T, n_head, out.ctypes.data_as(_F32P)))
    return out


def dbg_layernorm(x, g, b, d: Optional[int] = None, row_map=None) -> np.ndarray:
    """k_layernorm alone (wdr_dbg_layernorm): x [rows][ldx] float32 (its first d columns are the
    row; d defaults to ldx), g / b [d]; row_map [rows] gathers the input rows.  Returns float32
    [rows][d] (the kernel's f16 output widened)."""
    xc = np.ascontiguousarray(x, np.float32)
    rows, ldx = xc.shape
    d = ldx if d is None else int(d)
    gc, bc = np.ascontiguousarray(g, np.float32), np.ascontiguousarray(b, np.float32)
    if gc.shape != (d,) or bc.shape != (d,):
        raise ValueError("dbg_layernorm: g / b [d]")
    rm = None if row_map is None else np.ascontiguousarray(row_map, np.int32)
    if rm is not None and rm.shape != (rows,):
        raise ValueError("dbg_layernorm: row_map [rows]")
    out = np.zeros((rows, d), np.float32)
    L.check(L.load().wdr_dbg_layernorm(xc.ctypes.data_as(_F32P), ldx, gc.ctypes.data_as(_F32P), bc.ctypes.data_as(_F32P),
                                       rows, d, None if rm is None else rm.ctypes.data_as(_I32P),
                                       out.ctypes.data_as(_F32P)))
    return out


class WhisperContext:
    """transcribe::create_context (src/transcribe.rs:89-166) + its whisper_state."""

    def __init__(self, model_name: str, model_path: Optional[str] = None, gpu_device: Optional[int] = None,
                 use_gpu: Optional[bool] = None, enable_dtw: Optional[bool] = True,
                 enable_flash_attn: Optional[bool] = None, num_samples: Optional[int] = None,
                 synthetic: Optional[Synthetic] = None):
        lib = L.load()
        self._lib = lib
        h = C.c_void_p()
        syn = _syn(synthetic)
        L.check(lib.wdr_context_create(_s(model_path), model_name.encode(), 0 if gpu_device is None else 1,
                                       gpu_device or 0, _ob(use_gpu), _ob(enable_dtw), _ob(enable_flash_attn),
                                       0 if num_samples is None else 1, num_samples or 0,
                                       C.byref(syn) if syn else None, C.byref(h)))
        self.h = h
        self.synthetic = synthetic
        hp = (C.c_int32 * 10)()
        L.check(lib.wdr_context_hparams(h, hp))
        keys = ["n_vocab", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer", "n_text_ctx",
                "n_text_state", "n_text_head", "n_text_layer", "n_mels"]
        self.hparams = dict(zip(keys, list(hp)))

    def close(self):
        if self.h:
            self._lib.wdr_context_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- run_transcription_pipeline (src/transcribe.rs:323-535)
    def run_pipeline(self, speech_segments, options: TranscribeOptions, callbacks: Optional[Callbacks] = None,
                     synthetic: Optional[Synthetic] = None, with_index: bool = False,
                     diarize_options: Optional[DiarizeOptions] = None):
        """transcribe::run_transcription_pipeline(ctx, segments, options, diarize_options, ...)
        -> (segments, detected_lang) [+ the input SpeechSegment index of every output segment
        when with_index].  Speakers are assigned iff diarize_options is given (as the
        reference's Option<DiarizeOptions>)."""
        keep = _Keep()
        arr = (L.SpeechSegment * max(1, len(speech_segments)))()
        for i, s in enumerate(speech_segments):
            smp = keep(np.ascontiguousarray(s.samples, np.int16))
            arr[i] = L.SpeechSegment(s.start, s.end, smp.ctypes.data_as(C.POINTER(C.c_int16)), smp.size)
        out = C.POINTER(L.SegmentList)()
        syn = _syn(synthetic or self.synthetic)
        d = _dopts(diarize_options, keep)
        L.check(self._lib.wdr_run_pipeline(self.h, arr, len(speech_segments), _opts(options, keep),
                                           C.byref(d) if d is not None else None,
                                           C.byref(syn) if syn else None, _callbacks(callbacks, keep),
                                           C.byref(out)))
        return _segments(out, with_index)

    def run_pipeline_groups(self, groups, options: TranscribeOptions, speakers=None,
                            callbacks: Optional[Callbacks] = None, synthetic: Optional[Synthetic] = None,
                            with_index: bool = False, group_start=None,
                            diarize: Optional[DiarizeOptions] = None):
        """Several independent recordings' speech segments in one pipeline run
        (wdr_run_pipeline_groups): groups is a list of lists of SpeechSegment; the result is one
        (segments, detected_lang) [+ speech index] per group, each equal to run_pipeline(group, ...)
        without diarization, while the decode chains are shared by all groups.  speakers: an
        optional fixed speaker_id per group (entries may be None).  group_start (test seam): pass
        the raw group_start array with groups as one flat list of segments.  diarize: speakers are
        assigned per group (wdr_run_pipeline_groups_diarize), each group equal to
        run_pipeline(group, ..., diarize_options=diarize); not together with speakers."""
        if diarize is not None and speakers is not None:
            raise ValueError("a group's speakers are fixed or diarized, not both")
        keep = _Keep()
        if group_start is None:
            flat = [s for g in groups for s in g]
            starts = list(np.cumsum([0] + [len(g) for g in groups])[:-1])
        else:
            flat, starts = list(groups), [int(x) for x in group_start]
        G = len(starts)
        arr = (L.SpeechSegment * max(1, len(flat)))()
        for i, s in enumerate(flat):
            smp = keep(np.ascontiguousarray(s.samples, np.int16))
            arr[i] = L.SpeechSegment(s.start, s.end, smp.ctypes.data_as(C.POINTER(C.c_int16)), smp.size)
        gs = (C.c_size_t * max(1, G))(*[int(x) for x in starts])
        spk = None
        if speakers is not None:
            if len(speakers) != G:
                raise ValueError("one speaker entry per group")
            spk = (C.c_char_p * max(1, G))(*[_s(x) for x in speakers])
        out = (C.POINTER(L.SegmentList) * max(1, G))()
        syn = _syn(synthetic or self.synthetic)
        if diarize is not None:
            d = _dopts(diarize, keep)
            L.check(self._lib.wdr_run_pipeline_groups_diarize(self.h, arr, len(flat), gs, G, _opts(options, keep),
                                                              C.byref(d), C.byref(syn) if syn else None,
                                                              _callbacks(callbacks, keep), out))
        else:
            L.check(self._lib.wdr_run_pipeline_groups(self.h, arr, len(flat), gs, G, spk, _opts(options, keep),
                                                      C.byref(syn) if syn else None, _callbacks(callbacks, keep), out))
        return [_segments(out[g], with_index) for g in range(G)]

    def run_pipeline_raw(self, speech_segments, options: TranscribeOptions, synthetic: Optional[Synthetic] = None):
        """run_pipeline without the cross-segment overlap clip and speaker assignment
        (wdr_run_pipeline_raw): (segments, detected_lang, speech index per segment)."""
        keep = _Keep()
        arr = (L.SpeechSegment * max(1, len(speech_segments)))()
        for i, s in enumerate(speech_segments):
            smp = keep(np.ascontiguousarray(s.samples, np.int16))
            arr[i] = L.SpeechSegment(s.start, s.end, smp.ctypes.data_as(C.POINTER(C.c_int16)), smp.size)
        out = C.POINTER(L.SegmentList)()
        syn = _syn(synthetic or self.synthetic)
        L.check(self._lib.wdr_run_pipeline_raw(self.h, arr, len(speech_segments), _opts(options, keep),
                                               C.byref(syn) if syn else None, C.byref(out)))
        segs, lang, index = _segments(out, True)
        return segs, lang, index or []

    def run_pipeline_block(self, speech_segments, options: TranscribeOptions, rng_in: Optional[str] = None,
                           synthetic: Optional[Synthetic] = None):
        """run_pipeline_raw continuing decoder 0's RNG stream (wdr_run_pipeline_block):
        (segments, detected_lang, speech index per segment, sampled flag per speech segment,
        rng state after the block)."""
        keep = _Keep()
        arr = (L.SpeechSegment * max(1, len(speech_segments)))()
        for i, s in enumerate(speech_segments):
            smp = keep(np.ascontiguousarray(s.samples, np.int16))
            arr[i] = L.SpeechSegment(s.start, s.end, smp.ctypes.data_as(C.POINTER(C.c_int16)), smp.size)
        out = C.POINTER(L.SegmentList)()
        syn = _syn(synthetic or self.synthetic)
        sampled = (C.c_int8 * max(1, len(speech_segments)))()
        rng = C.c_void_p()
        L.check(self._lib.wdr_run_pipeline_block(self.h, arr, len(speech_segments), _opts(options, keep),
                                                 C.byref(syn) if syn else None, _s(rng_in), sampled, C.byref(rng),
                                                 C.byref(out)))
        rng_out = C.cast(rng, C.c_char_p).value.decode()
        self._lib.wdr_free(rng)
        segs, lang, index = _segments(out, True)
        return segs, lang, index or [], [bool(sampled[i]) for i in range(len(speech_segments))], rng_out

    @property
    def devices(self) -> List[int]:
        """GPU ordinals this context runs on (wdr_context_devices): gpu_device=None -> every
        visible GPU, the decode chains spread over them."""
        n = C.c_int32()
        ids = (C.c_int32 * 8)()
        L.check(self._lib.wdr_context_devices(self.h, C.byref(n), ids, 8))
        return [ids[i] for i in range(min(n.value, 8))]

    def set_encoder_fp8(self, on: bool):
        """fp8 (e4m3) encoder GEMMs, BASELINE configs[4] (wdr_context_set_encoder_fp8)."""
        L.check(self._lib.wdr_context_set_encoder_fp8(self.h, 1 if on else 0))

    def set_chains(self, n: int):
        """Decode chains per GPU for run_pipeline calls (wdr_context_set_chains): n blocks of the
        speech segments per GPU decoded concurrently with batched steps, exact prompt fix-up."""
        L.check(self._lib.wdr_context_set_chains(self.h, int(n)))

    def set_early_fixup(self, mode: int):
        """Test seam (wdr_dbg_set_early_fixup): 0 off, 1 after the predecessor finished, 2 forced
        (wait for the predecessor to finish), 3 from the predecessor's speculative prompt (the
        default), -1 env default."""
        L.check(self._lib.wdr_dbg_set_early_fixup(self.h, int(mode)))

    def stage_times(self) -> dict:
        t = L.StageTimes()
        L.check(self._lib.wdr_context_stage_times(self.h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in L.StageTimes._fields_}

    # -- test seams
    def state_full(self, samples_f32: np.ndarray, options: TranscribeOptions, initial_prompt: Optional[str] = None,
                   synthetic: Optional[Synthetic] = None):
        keep = _Keep()
        x = np.ascontiguousarray(samples_f32, np.float32)
        segs = C.POINTER(L.ResultSeg)()
        n = C.c_size_t()
        lang = C.c_int32()
        syn = _syn(synthetic or self.synthetic)
        L.check(self._lib.wdr_state_full(self.h, x.ctypes.data_as(C.POINTER(C.c_float)), x.size, _opts(options, keep),
                                         C.byref(syn) if syn else None, _s(initial_prompt), C.byref(segs), C.byref(n),
                                         C.byref(lang)))
        out = []
        for i in range(n.value):
            s = segs[i]
            toks = [dict(id=t.id, tid=t.tid, p=t.p, plog=t.plog, pt=t.pt, ptsum=t.ptsum, t0=t.t0, t1=t.t1,
                         t_dtw=t.t_dtw) for t in (s.tokens[k] for k in range(s.n_tokens))]
            out.append(dict(t0=s.t0, t1=s.t1, text=s.text.decode(), tokens=toks))
        self._lib.wdr_result_free(segs, n.value)
        return out, lang.value

    def log_mel_window(self, x: np.ndarray, seek: int = 0) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros((self.hparams["n_mels"], 3000), np.float32)
        L.check(self._lib.wdr_dbg_log_mel(self.h, x.ctypes.data_as(C.POINTER(C.c_float)), x.size, seek,
                                          out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def encode(self, mel_window: np.ndarray) -> np.ndarray:
        m = np.ascontiguousarray(mel_window, np.float32)
        out = np.zeros((1500, self.hparams["n_audio_state"]), np.float32)
        L.check(self._lib.wdr_dbg_encode(self.h, m.ctypes.data_as(C.POINTER(C.c_float)),
                                         out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def cross_kv(self) -> np.ndarray:
        """Cross K/V of the last encode() window: [1500][n_text_layer][2][d]."""
        h = self.hparams
        out = np.zeros((1500, h["n_text_layer"], 2, h["n_text_state"]), np.float32)
        L.check(self._lib.wdr_dbg_cross_kv(self.h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def im2col_mel(self, x: np.ndarray, seek: int = 0) -> np.ndarray:
        """conv1's operand rows of the window at frame `seek` of x, as every production encode
        builds them (wdr_dbg_im2col_mel): float16 [3000][kp], column 3 ci + k of row t = channel ci
        at window frame t + k - 1."""
        x = np.ascontiguousarray(x, np.float32)
        kp = C.c_int32()
        L.check(self._lib.wdr_dbg_im2col_mel(self.h, None, 0, 0, None, C.byref(kp)))
        out = np.zeros((3000, kp.value), np.uint16)
        L.check(self._lib.wdr_dbg_im2col_mel(self.h, x.ctypes.data_as(_F32P), x.size, int(seek),
                                             out.ctypes.data_as(_U16P), C.byref(kp)))
        return out.view(np.float16)

    def encode_batch(self, clips):
        """One encode-ahead batch of len(clips) (1 .. 4) windows, window 0 of each int16 clip
        (wdr_dbg_encode_batch): (encoder output [nb][1500][d], cross K/V [nb][1500][n_text_layer][2][d])."""
        pcm = [np.ascontiguousarray(c, np.int16) for c in clips]
        nb = len(pcm)
        h = self.hparams
        ptr = (C.POINTER(C.c_int16) * max(1, nb))(*[p.ctypes.data_as(C.POINTER(C.c_int16)) for p in pcm])
        n = (C.c_int32 * max(1, nb))(*[p.size for p in pcm])
        enc = np.zeros((nb, 1500, h["n_audio_state"]), np.float32)
        xkv = np.zeros((nb, 1500, h["n_text_layer"], 2, h["n_text_state"]), np.float32)
        L.check(self._lib.wdr_dbg_encode_batch(self.h, ptr, n, nb, enc.ctypes.data_as(_F32P), xkv.ctypes.data_as(_F32P)))
        return enc, xkv

    def decode(self, tokens) -> np.ndarray:
        t = np.ascontiguousarray(tokens, np.int32)
        out = np.zeros(self.hparams["n_vocab"], np.float32)
        L.check(self._lib.wdr_dbg_decode(self.h, t.ctypes.data_as(C.POINTER(C.c_int32)), t.size,
                                         out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def step(self, tokens) -> np.ndarray:
        """Prefill tokens[:-1], then one decode step of tokens[-1]: the step's logits."""
        t = np.ascontiguousarray(tokens, np.int32)
        out = np.zeros(self.hparams["n_vocab"], np.float32)
        L.check(self._lib.wdr_dbg_step(self.h, t.ctypes.data_as(C.POINTER(C.c_int32)), t.size,
                                       out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def logit_rules(self, logits, ctls, temps=None, max_initial_ts: float = 1.0, suppress_blank: bool = True):
        """whisper.cpp's logit rules + greedy pick on the GPU (wdr_dbg_logits): logits [R][n_vocab],
        ctls = R dicts of n_tokens / last_ts / pen_ts / has_ts / seek_delta / force_kind / force_tok.
        Returns R dicts: id, tid, p, plog, pt, ptsum, nosp."""
        lg = np.ascontiguousarray(logits, np.float32)
        R = lg.shape[0]
        keys = ("n_tokens", "last_ts", "pen_ts", "has_ts", "seek_delta", "force_kind", "force_tok")
        ctl = np.ascontiguousarray([[int(c.get(k, 0)) for k in keys] for c in ctls], np.int32)
        tt = np.ascontiguousarray(temps if temps is not None else [0.0] * R, np.float32)
        ids = np.zeros((R, 2), np.int32)
        f = np.zeros((R, 5), np.float32)
        L.check(self._lib.wdr_dbg_logits(self.h, lg.ctypes.data_as(C.POINTER(C.c_float)), R,
                                         ctl.ctypes.data_as(C.POINTER(C.c_int32)),
                                         tt.ctypes.data_as(C.POINTER(C.c_float)), float(max_initial_ts),
                                         1 if suppress_blank else 0, ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                         f.ctypes.data_as(C.POINTER(C.c_float))))
        return [dict(id=int(ids[r, 0]), tid=int(ids[r, 1]), p=float(f[r, 0]), plog=float(f[r, 1]), pt=float(f[r, 2]),
                     ptsum=float(f[r, 3]), nosp=float(f[r, 4])) for r in range(R)]

    def _rule_args(self, logits, ctls, temps):
        lg = np.ascontiguousarray(logits, np.float32)
        R = lg.shape[0]
        if lg.shape != (R, self.hparams["n_vocab"]) or len(ctls) != R:
            raise ValueError("logits [R][n_vocab] and R rule states")
        keys = ("n_tokens", "last_ts", "pen_ts", "has_ts", "seek_delta", "force_kind", "force_tok")
        ctl = np.ascontiguousarray([[int(c.get(k, 0)) for k in keys] for c in ctls], np.int32)
        tt = np.ascontiguousarray(temps if temps is not None else [0.0] * R, np.float32)
        if tt.shape != (R,):
            raise ValueError("one temperature per row")
        return lg, R, ctl, tt

    def logits_topk(self, logits, ctls, K: int, temps=None, max_initial_ts: float = 1.0, suppress_blank: bool = True):
        """The beam-search top-K of rows under the logit rules (wdr_dbg_logits_topk; arguments as
        logit_rules): (ids [R][K] int32, p [R][K], log p [R][K]); absent candidates id -1, 0, -inf."""
        lg, R, ctl, tt = self._rule_args(logits, ctls, temps)
        K = int(K)
        ids = np.zeros((R, max(K, 1)), np.int32)
        f = np.zeros((R, max(K, 1), 2), np.float32)
        L.check(self._lib.wdr_dbg_logits_topk(self.h, lg.ctypes.data_as(_F32P), R, ctl.ctypes.data_as(_I32P),
                                              tt.ctypes.data_as(_F32P), float(max_initial_ts),
                                              1 if suppress_blank else 0, K, ids.ctypes.data_as(_I32P),
                                              f.ctypes.data_as(_F32P)))
        return ids, f[:, :, 0].copy(), f[:, :, 1].copy()

    def logits_probs(self, logits, ctls, temps=None, max_initial_ts: float = 1.0, suppress_blank: bool = True):
        """The sampling distribution of rows under the logit rules (wdr_dbg_logits_probs; arguments
        as logit_rules): (probs, logprobs), each [R][n_vocab] float32."""
        lg, R, ctl, tt = self._rule_args(logits, ctls, temps)
        probs, logp = np.zeros_like(lg), np.zeros_like(lg)
        L.check(self._lib.wdr_dbg_logits_probs(self.h, lg.ctypes.data_as(_F32P), R, ctl.ctypes.data_as(_I32P),
                                               tt.ctypes.data_as(_F32P), float(max_initial_ts),
                                               1 if suppress_blank else 0, probs.ctypes.data_as(_F32P),
                                               logp.ctypes.data_as(_F32P)))
        return probs, logp

    def kv_rows(self, seq: int, n_rows: int):
        """The first n_rows self-attention cache rows of decoder sequence seq in every layer
        (wdr_dbg_kv_rows): (k, v), each [n_text_layer][n_rows][d] float16."""
        shape = (self.hparams["n_text_layer"], int(n_rows), self.hparams["n_text_state"])
        k, v = np.zeros(shape, np.uint16), np.zeros(shape, np.uint16)
        L.check(self._lib.wdr_dbg_kv_rows(self.h, int(seq), int(n_rows), 0, k.ctypes.data_as(_U16P),
                                          v.ctypes.data_as(_U16P)))
        return k.view(np.float16), v.view(np.float16)

    def set_kv_rows(self, seq: int, k, v):
        """Store k / v [n_text_layer][n_rows][d] float16 as the first n_rows cache rows of sequence seq."""
        k, v = (np.ascontiguousarray(a, np.float16) for a in (k, v))
        if k.shape != v.shape or k.ndim != 3 or k.shape[0] != self.hparams["n_text_layer"] \
                or k.shape[2] != self.hparams["n_text_state"]:
            raise ValueError("k / v [n_text_layer][n_rows][d]")
        L.check(self._lib.wdr_dbg_kv_rows(self.h, int(seq), k.shape[1], 1, k.view(np.uint16).ctypes.data_as(_U16P),
                                          v.view(np.uint16).ctypes.data_as(_U16P)))

    def kv_reorder(self, moves, n_rows: int):
        """The beam reorder (wdr_dbg_kv_reorder): for every (src, dst) in moves sequence dst takes the
        first n_rows cached rows sequence src held before the call."""
        src = np.ascontiguousarray([m[0] for m in moves], np.int32)
        dst = np.ascontiguousarray([m[1] for m in moves], np.int32)
        L.check(self._lib.wdr_dbg_kv_reorder(self.h, src.ctypes.data_as(_I32P), dst.ctypes.data_as(_I32P), len(moves),
                                             int(n_rows)))

    def batch_step_ms(self, tokens, rows: int, iters: int = 50) -> float:
        """Host ms per multi-chain batched step of `rows` rows on the last encoded window
        (wdr_dbg_batch_step probe seam)."""
        t = np.ascontiguousarray(tokens, np.int32)
        ms = C.c_double()
        L.check(self._lib.wdr_dbg_batch_step(self.h, t.ctypes.data_as(C.POINTER(C.c_int32)), t.size, int(rows),
                                             int(iters), C.byref(ms)))
        return ms.value

    def capture(self, tokens, n_aheads: int) -> np.ndarray:
        t = np.ascontiguousarray(tokens, np.int32)
        out = np.zeros((n_aheads, t.size, 1500), np.float32)
        L.check(self._lib.wdr_dbg_capture(self.h, t.ctypes.data_as(C.POINTER(C.c_int32)), t.size,
                                          out.ctypes.data_as(C.POINTER(C.c_float))))
        return out


class Engine:
    """Engine (src/engine.rs:52-217)."""

    def __init__(self, cfg: Optional[EngineConfig] = None, synthetic: Optional[Synthetic] = None,
                 audio_convert: bool = False, channel_split: bool = False, batch_diarize: bool = False):
        cfg = cfg or EngineConfig()
        lib = L.load()
        self._lib = lib
        self._keep = _Keep()
        c = L.EngineConfig(self._keep(_s(cfg.cache_dir)), _ob(cfg.enable_dtw), _ob(cfg.enable_flash_attn),
                           _ob(cfg.use_gpu), 0 if cfg.gpu_device is None else 1, cfg.gpu_device or 0,
                           self._keep(_s(cfg.vad_model_path)), self._keep(_s(cfg.diarize_segment_model_path)),
                           self._keep(_s(cfg.diarize_embedding_model_path)))
        h = C.c_void_p()
        L.check(lib.wdr_engine_new(C.byref(c), C.byref(h)))
        self.h = h
        if synthetic is not None:
            s = _syn(synthetic)
            L.check(lib.wdr_engine_set_synthetic(h, C.byref(s)))
        if audio_convert:
            self.set_audio_convert(True)
        if channel_split:
            self.set_channel_split(True)
        if batch_diarize:
            self.set_batch_diarize(True)

    def set_batch_diarize(self, on: bool):
        """True: transcribe_batch takes enable_diarize, every file equal to its transcribe_audio
        (speaker ids start afresh in every file); False (default): it refuses it.  Not in the
        reference."""
        L.check(self._lib.wdr_engine_set_batch_diarize(self.h, 1 if on else 0))

    def set_audio_convert(self, on: bool):
        """True: transcribe_audio takes any WAV read_audio takes, converted on the engine's GPU;
        False (default): the reference's read_wav and its errors.  Not in the reference."""
        L.check(self._lib.wdr_engine_set_audio_convert(self.h, 1 if on else 0))

    def set_channel_split(self, on: bool):
        """True: transcribe_audio takes any WAV read_audio_channels takes and transcribes every
        channel on its own; segments carry speaker_id "1", "2", ... = channel, merged by start time.
        enable_diarize must not be set.  False (default): as before.  Not in the reference."""
        L.check(self._lib.wdr_engine_set_channel_split(self.h, 1 if on else 0))

    def transcribe_audio(self, audio_path: str, options: TranscribeOptions,
                         formatting_overrides=None, cb: Optional[Callbacks] = None) -> List[Segment]:
        keep = _Keep()
        out = C.POINTER(L.SegmentList)()
        ov = _fmt(formatting_overrides)
        L.check(self._lib.wdr_transcribe_audio(self.h, audio_path.encode(), _opts(options, keep),
                                               C.byref(ov) if ov is not None else None,
                                               _callbacks(cb, keep), C.byref(out)))
        segs, _ = _segments(out)
        return segs

    def transcribe_batch(self, paths, options: TranscribeOptions, overrides=None,
                         callbacks: Optional[BatchCallbacks] = None) -> List[BatchResult]:
        """Many recordings in one call (wdr_transcribe_batch): result i holds what
        transcribe_audio(paths[i], options, overrides) returns on this engine (and the detected
        language), the decode chains and the VAD pass shared by all files.  A file that cannot be
        read gets its error instead; the others are unaffected.  enable_diarize is refused unless
        the engine was made with batch_diarize (set_batch_diarize)."""
        keep = _Keep()
        n = len(paths)
        arr = (C.c_char_p * max(1, n))(*[_s(p) for p in paths])
        ov = _fmt(overrides)
        cbs = None
        if callbacks is not None:
            cbs = L.BatchCallbacks()
            if callbacks.progress:
                cbs.progress = keep(L.PROGRESS_FN(
                    lambda u, p, t, lbl: callbacks.progress(int(p), ProgressType(t), lbl.decode())))
            if callbacks.new_segment_callback:
                def seg_cb(u, idx, sp):
                    s = sp.contents
                    words = None
                    if s.words:
                        words = [WordTimestamp(s.words[k].text.decode(), s.words[k].start, s.words[k].end,
                                               s.words[k].probability if s.words[k].has_probability else None)
                                 for k in range(s.n_words)]
                    callbacks.new_segment_callback(int(idx), Segment(s.start, s.end, s.text.decode(), words,
                                                                     s.speaker_id.decode() if s.speaker_id else None))
                cbs.new_segment = keep(L.BATCH_SEGMENT_FN(seg_cb))
            if callbacks.is_cancelled:
                cbs.is_cancelled = keep(L.CANCEL_FN(lambda u: 1 if callbacks.is_cancelled() else 0))
        items = C.POINTER(L.BatchItem)()
        L.check(self._lib.wdr_transcribe_batch(self.h, arr if paths is not None else None, n, _opts(options, keep),
                                               C.byref(ov) if ov is not None else None,
                                               C.byref(cbs) if cbs is not None else None, C.byref(items)))
        out = []
        try:
            for i in range(n):
                it = items[i]
                if it.error:
                    out.append(BatchResult(None, None, C.cast(it.error, C.c_char_p).value.decode("utf-8", "replace")))
                else:
                    segs, lang = _segments(it.list, free=False)
                    out.append(BatchResult(segs, lang, None))
        finally:
            self._lib.wdr_batch_free(items, n)
        return out

    def stage_times(self, model: str = "base") -> dict:
        """Stage accounting of the engine's context of `model` after its last call
        (wdr_engine_stage_times; WhisperContext.stage_times' fields)."""
        t = L.StageTimes()
        L.check(self._lib.wdr_engine_stage_times(self.h, model.encode(), C.byref(t)))
        return {f: getattr(t, f) for f, _ in L.StageTimes._fields_}

    def close(self):
        if self.h:
            self._lib.wdr_engine_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
