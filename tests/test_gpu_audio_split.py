"""One speaker per channel on the GPU: the channel-keeping conversion kernel
against its host definition and against the existing mono definition, bit for bit -- every
format, the awkward frame sizes, every workgroup boundary, every chunk size -- the file reader,
and the Engine's opt-in: each channel transcribed as the mono file of it would be, labelled by
its channel and merged by start time."""
import dataclasses

import numpy as np
import pytest

import wdr
from oracle.pipeline import write_wav
from tests import audio_ref as A
from wdr._lib import WdrError
from wdr.synth import synth_speech

pytestmark = pytest.mark.gpu
SYN = wdr.Synthetic(weight_std=0.02, emb_std=0.5, force_len_rate=3.3, disable_fallback=True)

# (rate, fmt, channels)
CASES = ([(48000, f, 2) for f in (0, 1, 2, 3, 4)]
         + [(44100, 2, 3),      # 9-byte frames: the worst alignment
            (48000, 1, 8),
            (8000, 1, 2),
            (16000, 4, 2),      # no filter: decode, pick, quantize
            (47999, 1, 2),      # 16000 phases
            (48000, 1, 1)])


def _frames_for(n_out, rate):
    """The fewest input frames that give at least n_out outputs (an upsampling rate cannot give
    every count: 8 kHz in gives even counts only)."""
    L, M, _, _ = A.dims(rate)
    n = n_out * M // L
    while A.n_out(n, rate) < n_out:
        n += 1
    while n > 0 and A.n_out(n - 1, rate) >= n_out:
        n -= 1
    return n


def _channel_raw(raw, fmt, channels, c):
    """Sample c of every frame as mono raw bytes."""
    b = np.frombuffer(bytes(raw), np.uint8)
    return b.reshape(-1, channels, A.FMT_BYTES[fmt])[:, c].tobytes()


def _both(raw, fmt, channels, rate, chunk_frames=0):
    got = wdr.dbg_audio_split(raw, fmt, channels, rate, chunk_frames=chunk_frames)
    want = wdr.dbg_audio_split(raw, fmt, channels, rate, host=True)
    assert got.dtype == want.dtype == np.int16 and got.shape == want.shape and got.shape[0] == channels
    return got, want


# a workgroup owns 256 outputs of one channel (AC_WG_OUT, csrc/kernels/audio.hip): a partial
# workgroup, both sides of the workgroup boundary, and three workgroups
@pytest.mark.parametrize("n_out", [255, 256, 257, 513])
@pytest.mark.parametrize("rate,fmt,channels", CASES)
def test_kernel_is_the_definition(rate, fmt, channels, n_out):
    n_in = _frames_for(n_out, rate)
    raw = A.noise_raw(fmt, n_in, channels, seed=rate + 11 * fmt + channels + n_out)
    got, want = _both(raw, fmt, channels, rate)
    assert n_out <= got.shape[1] <= n_out + 1
    assert np.array_equal(got, want)
    # and the last channel against the existing mono seam: not new code on both sides
    c = channels - 1
    mono = wdr.dbg_audio_convert(_channel_raw(raw, fmt, channels, c), fmt, 1, rate, host=True)
    assert np.array_equal(got[c], mono)


@pytest.mark.parametrize("rate,chunks", [(48000, [4096, 1000, 97, 7]), (44100, [441, 100])])
def test_chunk_seams_are_invisible(rate, chunks):
    raw = A.noise_raw(1, 5000, 2, seed=rate + 1)
    ref, want = _both(raw, 1, 2, rate)          # the default chunk: one chunk
    assert np.array_equal(ref, want)
    for cf in chunks:
        assert np.array_equal(wdr.dbg_audio_split(raw, 1, 2, rate, chunk_frames=cf), ref), cf


def test_kernel_f32_specials():
    x = np.frombuffer(A.noise_raw(4, 3000, 2, seed=9), np.float32).copy() * np.float32(1.4)   # some past +-1
    x[::97] = np.nan         # odd strides: the specials land on both channels
    x[5::101] = np.inf
    x[7::103] = -np.inf
    x[11::107] = -0.0
    for rate in (16000, 48000):
        got, want = _both(x.tobytes(), 4, 2, rate)
        assert np.array_equal(got, want)


def test_read_audio_channels_on_a_file(tmp_path):
    raw = A.noise_raw(2, 4800, 2, seed=21)
    path = A.write_wav(tmp_path / "a.wav", raw, 2, 2, 48000, extensible=True,
                       before_data=[A.chunk(b"LIST", b"INFOabc")])
    got = wdr.read_audio_channels(path)
    assert got.shape == (2, 1600)
    assert np.array_equal(got, wdr.dbg_audio_split(raw, 2, 2, 48000, host=True))


def test_timing_seam():
    raw = A.noise_raw(2, 3000, 2, seed=12)
    got, ms = wdr.dbg_audio_split(raw, 2, 2, 48000, timing=True)
    assert np.array_equal(got, wdr.dbg_audio_split(raw, 2, 2, 48000, host=True))
    assert 0.0 < ms < 100.0


# ------------------------------------------------------------------ the Engine
def _up3(pcm):
    """48 kHz by linear interpolation (fidelity is not the point)."""
    t = np.arange(3 * pcm.size) / 3.0
    return np.rint(np.interp(t, np.arange(pcm.size), pcm.astype(np.float64))).astype(np.int16)


@pytest.fixture(scope="module")
def talk(tmp_path_factory):
    root = tmp_path_factory.mktemp("audio_split_engine")
    a, _ = synth_speech(6.0, seed=4)
    b, _ = synth_speech(6.0, seed=7)
    assert not np.array_equal(a, b)
    f = {"root": root, "a": str(root / "a.wav"), "b": str(root / "b.wav")}
    write_wav(f["a"], a)
    write_wav(f["b"], b)
    f["ab"] = A.write_wav(root / "ab.wav", np.stack([a, b], axis=1).astype("<i2").tobytes(), 1, 2, 16000)
    ua, ub = _up3(a), _up3(b)
    f["a48"] = A.write_wav(root / "a48.wav", ua.astype("<i2").tobytes(), 1, 1, 48000)
    f["b48"] = A.write_wav(root / "b48.wav", ub.astype("<i2").tobytes(), 1, 1, 48000)
    f["ab48"] = A.write_wav(root / "ab48.wav", np.stack([ua, ub], axis=1).astype("<i2").tobytes(), 1, 2, 48000)
    # one engine, one cached context: the two switches are flipped per call
    f["eng"] = wdr.Engine(wdr.EngineConfig(cache_dir=str(root)), synthetic=SYN, channel_split=True)
    yield f
    f["eng"].close()


def _mono(talk, path, opts):
    """The existing path: any mono file through audio_convert, no channel split."""
    eng = talk["eng"]
    eng.set_channel_split(False)
    eng.set_audio_convert(True)
    try:
        return eng.transcribe_audio(path, opts)
    finally:
        eng.set_audio_convert(False)
        eng.set_channel_split(True)


def _opts(vad):
    return wdr.TranscribeOptions(model="tiny-test", lang="en", enable_vad=vad,
                                 advanced=wdr.AdvancedTranscribe(sampling_strategy="greedy"))


def _merged(ra, rb):
    both = ([dataclasses.replace(s, speaker_id="1") for s in ra]
            + [dataclasses.replace(s, speaker_id="2") for s in rb])
    return sorted(both, key=lambda s: s.start)      # stable: ties keep the lower channel first


@pytest.mark.parametrize("vad,a,b,ab", [(False, "a", "b", "ab"), (True, "a", "b", "ab"), (False, "a48", "b48", "ab48")],
                         ids=["whole", "vad", "48k"])
def test_engine_channel_split_equals_the_mono_runs(talk, vad, a, b, ab):
    ra = _mono(talk, talk[a], _opts(vad))
    rb = _mono(talk, talk[b], _opts(vad))
    print("segments per channel:", len(ra), len(rb))
    assert len(ra) > 0 and len(rb) > 0
    assert all(s.speaker_id is None for s in ra + rb)
    got = talk["eng"].transcribe_audio(talk[ab], _opts(vad))
    assert got == _merged(ra, rb)                   # text, times, words and speakers
    # a mono file in this mode: the default result, speaker "1"
    if not vad and a == "a":
        assert talk["eng"].transcribe_audio(talk[a], _opts(vad)) == _merged(ra, [])


def test_engine_switch_off_keeps_the_reader(talk):
    eng = talk["eng"]
    eng.set_channel_split(False)
    try:
        with pytest.raises(WdrError) as e:
            eng.transcribe_audio(talk["ab"], _opts(False))
        assert str(e.value) == "expected mono audio file and found 2 channels!"
    finally:
        eng.set_channel_split(True)


def test_engine_callbacks(talk):
    pcts, spk = [], []
    cb = wdr.Callbacks(progress=lambda pct, typ, label: pcts.append(pct),
                       new_segment_callback=lambda s: spk.append(s.speaker_id))
    got = talk["eng"].transcribe_audio(talk["ab"], _opts(False), cb=cb)
    assert len(pcts) > 0 and pcts == sorted(pcts) and pcts[-1] == 100
    assert len(spk) > 0 and set(spk) == {"1", "2"}
    assert spk == sorted(spk)                       # channel order: every "1" before every "2"
    assert {s.speaker_id for s in got} == {"1", "2"}
