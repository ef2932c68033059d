"""The host side of diarized batches (wdr_engine_set_batch_diarize / wdr_run_pipeline_groups_diarize /
wdr_diarize_frame_classes_batch): what is decided before any GPU work -- the new symbols with the
ABI version where it was, the opt-in and the two refusals around it, the empty batch, and the
batched segmentation's argument errors (a diarizer without model files loads nothing, and touches
no device, until its first forward)."""
import ctypes as C

import numpy as np
import pytest

import wdr
from wdr import _lib as L

NEW = ["wdr_engine_set_batch_diarize", "wdr_run_pipeline_groups_diarize", "wdr_diarize_frame_classes_batch"]
OLD_REFUSAL = "batch transcription does not diarize: enable_diarize must not be set"
SPLIT_REFUSAL = "channel split labels speakers by channel: enable_diarize must not be set"


def test_new_symbols_resolve_and_the_abi_stays(lib):
    assert lib.wdr_abi_version() == 6
    syms = L.header_symbols()
    for name in NEW:
        assert name in syms, name
        assert hasattr(lib, name), name
        assert name in L._SIGS, name
    # additive: the structs the new entry points take keep their layout
    assert C.sizeof(L.DiarizeOptions) == 2 * C.sizeof(C.c_void_p) + 16
    assert C.sizeof(L.BatchItem) == 2 * C.sizeof(C.c_void_p)


def _dia(model="no-such-model"):
    return wdr.TranscribeOptions(model=model, enable_diarize=True)


def test_channel_split_with_diarize_fails_before_anything_is_read(tmp_path):
    """Neither the path (a directory: opening it as a file would fail otherwise) nor the model (none
    in this cache) is looked at: the single call's channel-split message comes first."""
    e = wdr.Engine(wdr.EngineConfig(cache_dir=str(tmp_path)), batch_diarize=True, channel_split=True)
    with pytest.raises(wdr.WdrError) as ex:
        e.transcribe_batch([str(tmp_path)], _dia())
    assert str(ex.value) == SPLIT_REFUSAL
    # the opt-in alone gets past both refusals, to the single call's model check
    e.set_channel_split(False)
    with pytest.raises(wdr.WdrError) as ex:
        e.transcribe_batch([str(tmp_path)], _dia())
    assert str(ex.value) == "whisper file doesn't exist"


def test_off_is_the_default_and_keeps_the_old_message(tmp_path):
    e = wdr.Engine(wdr.EngineConfig(cache_dir=str(tmp_path)))
    with pytest.raises(wdr.WdrError) as ex:
        e.transcribe_batch([str(tmp_path)], _dia())
    assert str(ex.value) == OLD_REFUSAL
    # switched on and off again; and off, channel split does not change the message
    e.set_batch_diarize(True)
    e.set_batch_diarize(False)
    e.set_channel_split(True)
    with pytest.raises(wdr.WdrError) as ex:
        e.transcribe_batch([str(tmp_path)], _dia())
    assert str(ex.value) == OLD_REFUSAL


def test_empty_diarized_batch(lib):
    e = wdr.Engine(wdr.EngineConfig(), batch_diarize=True)
    assert e.transcribe_batch([], _dia()) == []
    keep = wdr._Keep()
    items = C.POINTER(L.BatchItem)()
    assert lib.wdr_transcribe_batch(e.h, None, 0, wdr._opts(_dia(), keep), None, None, C.byref(items)) == 0
    assert not items


def test_missing_diarization_models_fail_the_whole_call(tmp_path):
    """Both model paths are resolved before any file is read, with the single call's messages: a
    configured file that is not there, and (without synthetic mode) nothing in the cache."""
    gone = str(tmp_path / "segmentation-3.0.onnx")
    cfg = wdr.EngineConfig(cache_dir=str(tmp_path), diarize_segment_model_path=gone,
                           diarize_embedding_model_path=str(tmp_path / "cam.onnx"))
    s = wdr.Engine(cfg, synthetic=wdr.Synthetic(), batch_diarize=True)
    with pytest.raises(wdr.WdrError) as ex:
        s.transcribe_batch([str(tmp_path)], _dia("tiny-test"))
    assert str(ex.value) == "segmentation model file doesn't exist: " + gone
    with pytest.raises(wdr.WdrError) as single:
        s.transcribe_audio(str(tmp_path / "x.wav"), _dia("tiny-test"))
    assert str(single.value) == "audio file doesn't exist"      # the single call reads first


def test_group_bounds_and_handles_of_the_diarized_groups(lib):
    seg = (L.SpeechSegment * 2)()
    out = (C.POINTER(L.SegmentList) * 2)()
    gs = (C.c_size_t * 2)(0, 1)
    d = L.DiarizeOptions(None, None, 0.5, 2 ** 64 - 1)
    assert lib.wdr_run_pipeline_groups_diarize(None, seg, 2, gs, 2, None, C.byref(d), None, None, out) != 0
    assert "null handle" in lib.wdr_last_error().decode()
    assert lib.wdr_engine_set_batch_diarize(None, 1) != 0
    assert "null handle" in lib.wdr_last_error().decode()
    with pytest.raises(ValueError):
        wdr.WhisperContext.run_pipeline_groups(None, [[]], wdr.TranscribeOptions(), speakers=["a"],
                                               diarize=wdr.DiarizeOptions())


def test_frame_classes_batch_argument_errors(lib):
    """B <= 0, a negative window_cap, NULL arrays, a NULL file with samples: errors on the host, before
    the segmentation model exists (this test runs without a GPU)."""
    dz = wdr.Diarizer()
    x = np.zeros(100, np.int16)
    ptr = x.ctypes.data_as(C.POINTER(C.c_int16))
    ptrs = (C.POINTER(C.c_int16) * 2)(ptr, None)
    ns = (C.c_size_t * 2)(100, 0)
    cls = np.zeros(2 * 589, np.int32)
    out = cls.ctypes.data_as(C.POINTER(C.c_int32))

    def call(p, n, B, cap, o=out):
        rc = lib.wdr_diarize_frame_classes_batch(dz.h, p, n, B, cap, o, None)
        return rc, lib.wdr_last_error().decode()

    for B in (0, -1):
        rc, msg = call(ptrs, ns, B, 0)
        assert rc != 0 and "file count" in msg, (B, msg)
    rc, msg = call(ptrs, ns, 2, -1)
    assert rc != 0 and "window_cap" in msg
    for p, n, o in ((None, ns, out), (ptrs, None, out), (ptrs, ns, None)):
        rc, msg = call(p, n, 2, 0, o)
        assert rc != 0 and "NULL arrays" in msg
    bad = (C.c_size_t * 2)(100, 7)          # the second file claims samples and has none
    rc, msg = call(ptrs, bad, 2, 0)
    assert rc != 0 and "is NULL" in msg
    with pytest.raises(wdr.WdrError, match="file count"):
        dz.frame_classes_batch([])
    assert lib.wdr_diarize_frame_classes_batch(None, ptrs, ns, 2, 0, out, None) != 0
    assert "null handle" in lib.wdr_last_error().decode()
