"""Diarized batch transcription (wdr_engine_set_batch_diarize): with enable_diarize
every file's result must EQUAL what transcribe_audio gives for it on the same engine -- segments,
words, times, speaker ids, detected language -- the segmentation windows of all files sharing their
forwards, the files sharing the decode chains and the embedding worker.  A file that cannot be read
carries the single call's message without disturbing its neighbours."""
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


def _opts(thr=None, max_speakers=None, vad=True):
    return wdr.TranscribeOptions(model="tiny-test", lang="auto", enable_vad=vad, enable_diarize=True,
                                 max_speakers=max_speakers,
                                 advanced=wdr.AdvancedTranscribe(sampling_strategy="greedy", diarize_threshold=thr))


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
    root = tmp_path_factory.mktemp("batch_diarize")
    f = {"root": str(root)}
    # two voices, a talk spurt (cut to 4 s) every 10 s over faint noise: the synthetic segmentation
    # weights keep a spurt whole where speech is a small part of its window (dense speech comes out
    # in syllable-long segments, too short for the pinned decode length to give any text)
    src, spurts = synth_speech(40.0, seed=6, n_speakers=2)
    two = np.round(np.random.default_rng(6).standard_normal(16000 * 31) * 30.0).astype(np.int16)   # 4 windows
    for k, (a, b, _) in enumerate(spurts[:3]):
        x = src[int(a * 16000):int(b * 16000)][:64000]
        two[16000 * (1 + 10 * k):16000 * (1 + 10 * k) + x.size] = x
    one, _ = synth_speech(9.0, seed=3)                      # 1 window
    hush = np.round(np.random.default_rng(1).standard_normal(16000 * 4) * 30.0).astype(np.int16)   # -60 dBFS noise
    for name, pcm in (("two", two), ("one", one), ("hush", hush)):
        f[name] = str(root / (name + ".wav"))
        write_wav(f[name], pcm)
    f["missing"] = str(root / "nowhere.wav")
    # 44.1 kHz stereo, a different talker per channel: an error for the reference's reader, a
    # downmix of both voices for audio_convert
    l, _ = synth_speech(12.0, seed=2)
    r, _ = synth_speech(12.0, seed=5)
    idx = (np.arange(int(l.size * 44100 / 16000)) * (16000 / 44100)).astype(np.int64)
    st = np.stack([l[idx], r[idx]], axis=1).astype("<i2")
    f["cd"] = A.write_wav(root / "cd.wav", st.tobytes(), 1, 2, 44100)
    f["list"] = [f["two"], f["one"], f["missing"], f["hush"]]
    return f


@pytest.fixture(scope="module")
def eng(files):
    e = wdr.Engine(wdr.EngineConfig(cache_dir=files["root"]), synthetic=SYN, batch_diarize=True)
    yield e
    e.close()


def _check(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g.segments is None) != (g.error is None), k       # exactly one of them
        assert g.error == w.error, k
        assert g.detected_lang == w.detected_lang, k
        assert g.segments == w.segments, k                         # text, times, words, speakers


@pytest.mark.parametrize("thr,max_speakers", [(None, None), (2.0, None), (2.0, 2)],   # 2.0: no cosine reaches it
                         ids=["default", "several", "two"])
def test_batch_equals_the_single_calls(eng, files, thr, max_speakers):
    opts = _opts(thr, max_speakers)
    want = [_single(eng, p, opts) for p in files["list"]]
    got = eng.transcribe_batch(files["list"], opts)
    print([(len(w.segments), w.detected_lang, sorted({s.speaker_id for s in w.segments}))
           if w.segments is not None else w.error for w in want])
    _check(got, want)
    assert got[2].error == "audio file doesn't exist"
    assert got[0].segments is not None and got[1].segments         # the others came through
    assert all(s.speaker_id is not None for k in (0, 1, 3) for s in got[k].segments)
    if thr is not None:
        # speakers are counted per file, from "1": every file with text starts there, and a file
        # with two segments has two speakers (nothing reaches the threshold)
        assert all(got[k].segments[0].speaker_id == "1" for k in (0, 1, 3) if got[k].segments)
        assert {s.speaker_id for s in got[1].segments} >= {"1", "2"}
    # different files, different results: equality above is not a constant's
    assert [s.text for s in got[0].segments] != [s.text for s in got[1].segments]


def test_enable_vad_is_ignored_when_diarizing(eng, files):
    paths = [files["one"], files["two"]]
    assert [g.segments for g in eng.transcribe_batch(paths, _opts(vad=False))] == \
        [g.segments for g in eng.transcribe_batch(paths, _opts(vad=True))]


def test_audio_convert_composes(eng, files):
    opts = _opts(2.0)
    paths = [files["cd"], files["one"], files["missing"]]
    # the reference's reader refuses the stereo file on the item; its neighbours are unaffected
    plain = eng.transcribe_batch(paths, opts)
    assert plain[0].error is not None and plain[0].error == _single(eng, files["cd"], opts).error
    assert plain[1].segments
    eng.set_audio_convert(True)
    try:
        want = [_single(eng, p, opts) for p in paths]
        got = eng.transcribe_batch(paths, opts)
    finally:
        eng.set_audio_convert(False)
    _check(got, want)
    assert got[0].segments is not None and got[0].error is None
    assert got[1].segments == plain[1].segments
    assert got[2].error == "audio file doesn't exist"


def test_callbacks_carry_the_file_index_and_the_speaker(eng, files):
    seen, pcts = [], []
    cb = wdr.BatchCallbacks(progress=lambda pct, typ, label: pcts.append(pct),
                            new_segment_callback=lambda i, s: seen.append((i, s.speaker_id)))
    got = eng.transcribe_batch(files["list"], _opts(2.0), callbacks=cb)
    idx = [i for i, _ in seen]
    assert idx == sorted(idx) and 1 in idx and set(idx) <= {0, 1, 3}   # file order, the readable ones
    assert all(s is not None for _, s in seen)
    assert [s for i, s in seen if i == 1][:2] == ["1", "2"]
    assert got[1].segments
    assert len(pcts) > 0 and pcts == sorted(pcts) and pcts[-1] <= 100   # finished speech segments over all files


def test_cancel_and_the_switch(eng, files):
    with pytest.raises(wdr.WdrError) as ex:
        eng.transcribe_batch([files["two"], files["one"]], _opts(),
                             callbacks=wdr.BatchCallbacks(is_cancelled=lambda: True))
    assert str(ex.value) == "failed to transcribe"
    # switched off, the refusal is back word for word; on again, the engine is fine
    eng.set_batch_diarize(False)
    try:
        with pytest.raises(wdr.WdrError) as ex:
            eng.transcribe_batch([files["one"]], _opts())
        assert str(ex.value) == "batch transcription does not diarize: enable_diarize must not be set"
    finally:
        eng.set_batch_diarize(True)
    assert eng.transcribe_batch([], _opts()) == []
    assert eng.transcribe_batch([files["one"]], _opts())[0].segments == eng.transcribe_audio(files["one"], _opts())
