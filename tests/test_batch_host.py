"""The host side of batch transcription (wdr_transcribe_batch / wdr_run_pipeline_groups /
wdr_vad_probs_batch): what is decided before any GPU work -- the new symbols, the refusals, the
empty batch, and per-file read errors -- with the ABI version where it was."""
import ctypes as C

import numpy as np
import pytest

import wdr
from wdr import _lib as L

NEW = ["wdr_transcribe_batch", "wdr_batch_free", "wdr_run_pipeline_groups", "wdr_vad_probs_batch",
       "wdr_engine_stage_times"]


def test_new_symbols_resolve_and_the_abi_stays(lib):
    assert lib.wdr_abi_version() == 6
    syms = L.header_symbols()
    for name in NEW:
        assert name in syms, name
        assert hasattr(lib, name), name
        assert name in L._SIGS, name
    # wdr_stage_times keeps its layout: the mirror's field count and size
    assert len(L.StageTimes._fields_) == 33 and C.sizeof(L.StageTimes) == 33 * 8
    assert C.sizeof(L.BatchItem) == 2 * C.sizeof(C.c_void_p)


def _raw_batch(lib, eng, paths, n, opts):
    keep = wdr._Keep()
    items = C.POINTER(L.BatchItem)()
    rc = lib.wdr_transcribe_batch(eng.h, paths, n, wdr._opts(opts, keep), None, None, C.byref(items))
    return rc, items, lib.wdr_last_error().decode()


def test_empty_batch_and_null_paths(lib):
    e = wdr.Engine(wdr.EngineConfig())
    assert e.transcribe_batch([], wdr.TranscribeOptions()) == []
    rc, items, _ = _raw_batch(lib, e, None, 0, wdr.TranscribeOptions())
    assert rc == 0 and not items
    lib.wdr_batch_free(items, 0)      # NULL: a no-op
    # NULL paths with a count: an error (the model check would come first: synthetic mode)
    s = wdr.Engine(wdr.EngineConfig(), synthetic=wdr.Synthetic())
    rc, items, msg = _raw_batch(lib, s, None, 3, wdr.TranscribeOptions())
    assert rc != 0 and "audio_paths is NULL" in msg and not items


def test_diarize_is_refused_before_any_file_is_opened(tmp_path):
    e = wdr.Engine(wdr.EngineConfig(cache_dir=str(tmp_path)))
    # neither the path (a directory: opening it as a file would fail otherwise) nor the model (none
    # in this cache) is looked at
    with pytest.raises(wdr.WdrError) as ex:
        e.transcribe_batch([str(tmp_path)], wdr.TranscribeOptions(model="no-such-model", enable_diarize=True))
    assert str(ex.value) == "batch transcription does not diarize: enable_diarize must not be set"


def test_whole_call_errors_are_the_single_calls(tmp_path):
    from oracle.pipeline import write_wav
    wav = str(tmp_path / "a.wav")
    write_wav(wav, np.zeros(16000, np.int16))
    e = wdr.Engine(wdr.EngineConfig(cache_dir=str(tmp_path / "empty_cache")))
    with pytest.raises(wdr.WdrError, match="whisper file doesn't exist"):
        e.transcribe_batch([wav], wdr.TranscribeOptions(model="tiny-test", enable_vad=False))
    s = wdr.Engine(wdr.EngineConfig(cache_dir=str(tmp_path / "empty_cache")), synthetic=wdr.Synthetic())
    with pytest.raises(wdr.WdrError, match="translate_target"):
        s.transcribe_batch([wav], wdr.TranscribeOptions(model="tiny-test", translate_target="fr"))


def test_unreadable_files_get_the_single_calls_messages(tmp_path):
    """Only unreadable files: every item carries transcribe_audio's own message, and nothing
    reaches the GPU (no VAD, no context: this test runs without one)."""
    from oracle.pipeline import write_wav
    ok = str(tmp_path / "ok.wav")
    write_wav(ok, np.zeros(1600, np.int16))
    cut = str(tmp_path / "cut.wav")
    with open(ok, "rb") as src, open(cut, "wb") as dst:
        dst.write(src.read(20))
    junk = str(tmp_path / "junk.wav")
    with open(junk, "wb") as dst:
        dst.write(b"not a wave file at all, but long enough to hold a header's worth")
    paths = [str(tmp_path / "missing.wav"), cut, junk]
    opts = wdr.TranscribeOptions(model="tiny-test")
    s = wdr.Engine(wdr.EngineConfig(cache_dir=str(tmp_path)), synthetic=wdr.Synthetic())
    want = []
    for p in paths:
        with pytest.raises(wdr.WdrError) as ex:
            s.transcribe_audio(p, opts)
        want.append(str(ex.value))
    assert want[0] == "audio file doesn't exist" and len(set(want)) >= 2
    got = s.transcribe_batch(paths, opts)
    assert [g.error for g in got] == want
    assert all(g.segments is None and g.detected_lang is None for g in got)


def test_bad_groups_fail_on_the_host(lib):
    """group_start is checked before the context is touched: a NULL context still gets the handle
    error, a bad array the array's."""
    seg = (L.SpeechSegment * 2)()
    out = (C.POINTER(L.SegmentList) * 2)()
    gs = (C.c_size_t * 2)(0, 1)
    assert lib.wdr_run_pipeline_groups(None, seg, 2, gs, 2, None, None, None, None, out) != 0
    assert "null handle" in lib.wdr_last_error().decode()
    assert lib.wdr_vad_probs_batch(None, None, None, 0, None, None) != 0
    assert "null handle" in lib.wdr_last_error().decode()
