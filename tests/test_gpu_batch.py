"""Batch transcription (wdr_transcribe_batch): many recordings in one call, one
batched VAD pass, one grouped pipeline run.  Every file's result must EQUAL what transcribe_audio
gives for it on the same engine -- segments, words, times, speakers, detected language -- in every
engine mode, and a file that cannot be read must carry the single call's message without
disturbing its neighbours."""
import ctypes as C

import numpy as np
import pytest

import wdr
from oracle.pipeline import write_wav
from tests import audio_ref as A
from wdr import _lib as L
from wdr.synth import synth_speech

pytestmark = pytest.mark.gpu
SYN = wdr.Synthetic(weight_std=0.02, emb_std=0.5, force_len_rate=3.3, disable_fallback=True)


def _opts(vad, lang="auto"):
    return wdr.TranscribeOptions(model="tiny-test", lang=lang, enable_vad=vad,
                                 advanced=wdr.AdvancedTranscribe(sampling_strategy="greedy"))


def _single(eng, path, opts):
    """transcribe_audio with the detected language (the Python method drops it), or its error."""
    lib = L.load()
    keep = wdr._Keep()
    out = C.POINTER(L.SegmentList)()
    rc = lib.wdr_transcribe_audio(eng.h, path.encode(), wdr._opts(opts, keep), None, None, C.byref(out))
    if rc != 0:
        return wdr.BatchResult(None, None, lib.wdr_last_error().decode())
    segs, lang = wdr._segments(out)
    return wdr.BatchResult(segs, lang, None)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    root = tmp_path_factory.mktemp("batch")
    f = {"root": str(root)}
    for name, seconds, seed in (("a", 16.0, 3), ("b", 6.0, 7), ("d", 20.0, 4)):
        pcm, spurts = synth_speech(seconds, seed=seed)
        assert len(spurts) >= 1
        f[name] = str(root / (name + ".wav"))
        write_wav(f[name], pcm)
    # 8 kHz stereo, a different talker per channel: an error for the reference's reader, a downmix
    # for audio_convert, two speakers for channel_split
    l, _ = synth_speech(12.0, seed=2)
    r, _ = synth_speech(12.0, seed=5)
    st = np.stack([l[::2], r[::2]], axis=1).astype("<i2")
    f["c"] = A.write_wav(root / "c.wav", st.tobytes(), 1, 2, 8000)
    f["missing"] = str(root / "nowhere.wav")
    f["cut"] = str(root / "cut.wav")
    with open(f["a"], "rb") as src, open(f["cut"], "wb") as dst:
        dst.write(src.read(20))          # ends inside the fmt chunk
    f["list"] = [f["a"], f["missing"], f["b"], f["cut"], f["c"], f["d"]]
    return f


@pytest.fixture(scope="module")
def eng(files):
    e = wdr.Engine(wdr.EngineConfig(cache_dir=files["root"]), synthetic=SYN)
    yield e
    e.close()


@pytest.mark.parametrize("vad", [False, True], ids=["whole", "vad"])
@pytest.mark.parametrize("mode", ["read_wav", "convert", "split"])
def test_batch_equals_the_single_calls(eng, files, mode, vad):
    eng.set_audio_convert(mode == "convert")
    eng.set_channel_split(mode == "split")
    try:
        want = [_single(eng, p, _opts(vad)) for p in files["list"]]
        got = eng.transcribe_batch(files["list"], _opts(vad))
    finally:
        eng.set_audio_convert(False)
        eng.set_channel_split(False)
    print(mode, vad, [(len(w.segments) if w.segments is not None else w.error, w.detected_lang) for w in want])
    assert len(got) == len(want) == 6
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g.segments is None) != (g.error is None), k       # exactly one of them
        assert g.error == w.error, k
        assert g.detected_lang == w.detected_lang, k
        assert g.segments == w.segments, k                         # text, times, words, speakers
    # the unreadable ones in the middle carry the single call's messages, the rest came through
    assert got[1].error == "audio file doesn't exist"
    assert got[3].error is not None and got[3].error != got[1].error
    ok = [k for k in (0, 2, 5) if got[k].segments]
    assert ok == [0, 2, 5], [g.error for g in got]
    assert all(got[k].detected_lang for k in ok)
    if mode == "read_wav":
        assert got[4].error is not None     # stereo, 8 kHz: the reference's reader refuses it
    else:
        assert got[4].segments
    if mode == "split":
        assert {s.speaker_id for s in got[4].segments} == {"1", "2"}
        assert {s.speaker_id for s in got[0].segments} == {"1"}
    else:
        assert all(s.speaker_id is None for k in ok for s in got[k].segments)
    # different files, different results: equality above is not a constant's
    assert [s.text for s in got[0].segments] != [s.text for s in got[5].segments]


def test_requested_language_and_overrides(eng, files):
    ov = wdr.FormattingOverrides(max_chars_per_line=20, max_lines=1)
    paths = [files["a"], files["d"]]
    want = [eng.transcribe_audio(p, _opts(True, "de"), ov) for p in paths]
    got = eng.transcribe_batch(paths, _opts(True, "de"), overrides=ov)
    assert all(want) and [g.segments for g in got] == want
    assert [g.detected_lang for g in got] == ["de", "de"]


def test_callbacks_carry_the_file_index(eng, files):
    seen, pcts = [], []
    cb = wdr.BatchCallbacks(progress=lambda pct, typ, label: pcts.append(pct),
                            new_segment_callback=lambda i, s: seen.append((i, s.speaker_id)))
    eng.set_channel_split(True)
    try:
        got = eng.transcribe_batch(files["list"], _opts(False), callbacks=cb)
    finally:
        eng.set_channel_split(False)
    idx = [i for i, _ in seen]
    assert idx == sorted(idx)                                   # file order
    assert set(idx) == {0, 2, 4, 5}                             # the readable ones
    assert [s for i, s in seen if i == 4] == sorted(s for i, s in seen if i == 4)   # channel by channel
    assert {s for i, s in seen if i == 4} == {"1", "2"}
    assert len(pcts) > 0 and pcts == sorted(pcts) and pcts[-1] == 100
    assert all(g.segments for k, g in enumerate(got) if k in (0, 2, 4, 5))


def test_chains_are_shared_across_files(files):
    """Whole files as one segment each: a single call decodes on one chain, the batch on one chain
    per file -- the files share one pipeline run."""
    e = wdr.Engine(wdr.EngineConfig(cache_dir=files["root"]), synthetic=SYN)
    try:
        paths = [files["a"], files["b"], files["d"], files["a"]]
        single = []
        for p in paths:
            e.transcribe_audio(p, _opts(False))
            single.append(e.stage_times("tiny-test")["chains"])
        got = e.transcribe_batch(paths, _opts(False))
        st = e.stage_times("tiny-test")
        print("chains: single", single, "batch", st["chains"])
        assert st["chains"] > max(single), (st["chains"], single)
        assert st["chains"] == 4 and st["batch_launches"] > 0
        assert got[0].segments == got[3].segments and got[0].segments   # the same file twice
    finally:
        e.close()


def test_cancel_and_refusals(eng, files):
    with pytest.raises(wdr.WdrError) as ex:
        eng.transcribe_batch([files["a"]], wdr.TranscribeOptions(model="tiny-test", enable_diarize=True))
    assert str(ex.value) == "batch transcription does not diarize: enable_diarize must not be set"
    with pytest.raises(wdr.WdrError) as ex:
        eng.transcribe_batch([files["a"], files["b"]], _opts(False),
                             callbacks=wdr.BatchCallbacks(is_cancelled=lambda: True))
    assert str(ex.value) == "failed to transcribe"
    assert eng.transcribe_batch([], _opts(False)) == []
    # the engine is fine afterwards
    assert eng.transcribe_batch([files["b"]], _opts(False))[0].segments == eng.transcribe_audio(files["b"], _opts(False))
