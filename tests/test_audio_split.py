"""One speaker per channel, host side (no GPU): the host definition of the
channel-keeping conversion against the existing mono definition -- channel c of the split is, by
definition, the mono conversion of sample c of every frame, so every comparison is exact -- the
file reader's no-GPU case, the rejections, and the Engine's diarization conflict."""
import ctypes as C

import numpy as np
import pytest

import wdr
from tests import audio_ref as A
from wdr import _lib as L
from wdr._lib import WdrError

SYN = wdr.Synthetic(weight_std=0.02, emb_std=0.5, force_len_rate=3.3, disable_fallback=True)
RATES = [48000, 44100, 8000, 16000]
# (fmt, channels)
CASES = [(f, 2) for f in (0, 1, 2, 3, 4)] + [(1, c) for c in (1, 3, 8)]


def _channel_raw(raw, fmt, channels, c):
    """Sample c of every frame as mono raw bytes."""
    sb = A.FMT_BYTES[fmt]
    b = np.frombuffer(bytes(raw), np.uint8)
    return b.reshape(-1, channels, sb)[:, c].tobytes()


def _check_against_mono(raw, fmt, channels, rate, n_in):
    got = wdr.dbg_audio_split(raw, fmt, channels, rate, host=True)
    assert got.dtype == np.int16 and got.shape == (channels, A.n_out(n_in, rate))
    for c in range(channels):
        want = wdr.dbg_audio_convert(_channel_raw(raw, fmt, channels, c), fmt, 1, rate, host=True)
        assert np.array_equal(got[c], want), c
    return got


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("fmt,channels", CASES)
def test_host_split_is_the_mono_definition_per_channel(fmt, channels, rate):
    n_in = 600 + channels
    raw = A.noise_raw(fmt, n_in, channels, seed=rate + 13 * fmt + channels)
    got = _check_against_mono(raw, fmt, channels, rate, n_in)
    for c in range(1, channels):        # the seeds make the channels differ: a mixed-up plane shows
        assert not np.array_equal(got[c], got[0])


def test_no_filter_is_the_deinterleave():
    x = np.random.default_rng(3).integers(-32768, 32768, (700, 2)).astype("<i2")
    got = wdr.dbg_audio_split(x.tobytes(), 1, 2, 16000, host=True)
    assert np.array_equal(got, x.T)


@pytest.mark.parametrize("n_in", [0, 1, 95, 97])   # 0, 1, H - 1, H + 1 at 48 kHz (H = 96)
def test_edge_lengths(n_in):
    raw = A.noise_raw(1, n_in, 2, seed=n_in + 5)
    _check_against_mono(raw, 1, 2, 48000, n_in)


def test_read_audio_channels_of_a_read_wav_file_needs_no_gpu(tmp_path):
    pcm = np.random.default_rng(6).integers(-32768, 32768, 12345).astype(np.int16)
    for ext in (False, True):
        p = A.write_wav(tmp_path / "m.wav", pcm.tobytes(), 1, 1, 16000, extensible=ext,
                        before_data=[A.chunk(b"LIST", b"INFOxyz")])
        got = wdr.read_audio_channels(p)
        assert got.dtype == np.int16 and got.shape == (1, pcm.size)
        assert np.array_equal(got, wdr.read_wav(p)[None, :])
    p = A.write_wav(tmp_path / "e.wav", b"", 1, 1, 16000)
    assert wdr.read_audio_channels(p).shape == (1, 0)


def _raw_split(raw, n_frames, fmt, channels, rate, out=True, n=True):
    """wdr_dbg_audio_split (host) called directly: the wrapper's own argument checks stay out."""
    lib = L.load()
    p = C.POINTER(C.c_int16)()
    nn = C.c_size_t()
    buf = (C.c_uint8 * len(raw)).from_buffer_copy(raw) if raw is not None else None
    rc = lib.wdr_dbg_audio_split(buf, n_frames, fmt, channels, rate, 0, 1, C.byref(p) if out else None,
                                 C.byref(nn) if n else None, None)
    if rc == 0:
        lib.wdr_free(C.cast(p, C.c_void_p))
        return None
    return lib.wdr_last_error().decode()


def test_bad_arguments(tmp_path):
    raw = bytes(64)
    assert _raw_split(raw, 4, 1, 2, 48000) is None
    assert _raw_split(raw, 4, 1, 0, 48000) == "unsupported channel count 0 (1 to 8)"
    assert _raw_split(raw, 4, 1, 9, 48000) == "unsupported channel count 9 (1 to 8)"
    assert _raw_split(raw, 4, 1, 2, 999) == "unsupported sample rate 999 Hz (1000 to 384000)"
    assert _raw_split(raw, 4, 1, 2, 384001) == "unsupported sample rate 384001 Hz (1000 to 384000)"
    assert _raw_split(raw, 4, 5, 2, 48000) == "audio: sample format must be 0 (u8), 1 (i16), 2 (i24), 3 (i32) or 4 (f32)"
    assert _raw_split(raw, 4, -1, 2, 48000) == "audio: sample format must be 0 (u8), 1 (i16), 2 (i24), 3 (i32) or 4 (f32)"
    # null pointers: the input (with frames to read), either output
    assert _raw_split(None, 4, 1, 2, 48000) == "null pointer"
    assert _raw_split(raw, 4, 1, 2, 48000, out=False) == "null pointer"
    assert _raw_split(raw, 4, 1, 2, 48000, n=False) == "null pointer"
    assert _raw_split(None, 0, 1, 2, 48000) is None      # nothing to read
    # the wrapper: a buffer that is not whole frames, a bad format, a bad channel count, a bad rate
    with pytest.raises(ValueError):
        wdr.dbg_audio_split(bytes(5), 1, 2, 48000, host=True)      # short of a second 4-byte frame
    with pytest.raises(ValueError):
        wdr.dbg_audio_split(b"", 5, 2, 48000, host=True)
    for ch in (0, 9):
        with pytest.raises(ValueError):
            wdr.dbg_audio_split(b"", 1, ch, 48000, host=True)
    with pytest.raises(WdrError) as e:
        wdr.dbg_audio_split(bytes(8), 1, 2, 999, host=True)
    assert str(e.value) == "unsupported sample rate 999 Hz (1000 to 384000)"
    # files: the parser's messages reach read_audio_channels unchanged
    for ch, rate, msg in ((9, 44100, "unsupported channel count 9 (1 to 8)"),
                          (2, 999, "unsupported sample rate 999 Hz (1000 to 384000)")):
        p = tmp_path / "bad.wav"
        p.write_bytes(A.wav_bytes(bytes(36), 1, ch, rate))
        with pytest.raises(WdrError) as e:
            wdr.read_audio_channels(str(p))
        assert str(e.value) == msg
    with pytest.raises(WdrError) as e:
        wdr.read_audio_channels(str(tmp_path / "missing.wav"))
    assert str(e.value) == "audio file doesn't exist"


def test_channel_split_refuses_diarization(tmp_path):
    """The check precedes the file read and all device work, so it shows without a GPU."""
    x = np.zeros((1600, 2), "<i2")
    path = A.write_wav(tmp_path / "s.wav", x.tobytes(), 1, 2, 16000)
    eng = wdr.Engine(wdr.EngineConfig(cache_dir=str(tmp_path)), synthetic=SYN, channel_split=True)
    opts = wdr.TranscribeOptions(model="tiny-test", lang="en", enable_vad=False, enable_diarize=True,
                                 advanced=wdr.AdvancedTranscribe(sampling_strategy="greedy"))
    with pytest.raises(WdrError) as e:
        eng.transcribe_audio(path, opts)
    assert str(e.value) == "channel split labels speakers by channel: enable_diarize must not be set"
    eng.close()
