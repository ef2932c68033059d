"""Audio ingest on the GPU: the conversion kernel against the host definition
bit for bit -- every format, the awkward frame sizes, every workgroup boundary, every chunk size
-- read_audio on files, and the Engine's opt-in."""
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
         + [(r, 1, 1) for r in (48000, 44100, 8000, 22050, 12345, 47999)]
         + [(44100, 2, 3),      # 9-byte frames: the worst alignment
            (48000, 1, 6),
            (16000, 4, 2)])     # no filter: decode, downmix, quantize


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


def _both(raw, fmt, channels, rate, chunk_frames=0):
    got = wdr.dbg_audio_convert(raw, fmt, channels, rate, chunk_frames=chunk_frames)
    want = wdr.dbg_audio_convert(raw, fmt, channels, rate, host=True)
    assert got.dtype == want.dtype == np.int16 and got.shape == want.shape
    return got, want


# a workgroup owns 256 outputs (AC_WG_OUT, csrc/kernels/audio.hip): a partial workgroup, both
# sides of the workgroup boundary, and 16 workgroups + 3 outputs
@pytest.mark.parametrize("n_out", [255, 256, 257, 4099])
@pytest.mark.parametrize("rate,fmt,channels", CASES)
def test_kernel_is_the_definition(rate, fmt, channels, n_out):
    n_in = _frames_for(n_out, rate)
    raw = A.noise_raw(fmt, n_in, channels, seed=rate + 11 * fmt + channels + n_out)
    got, want = _both(raw, fmt, channels, rate)
    assert n_out <= got.size <= n_out + 1
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n_in", [0, 1, 95, 97])   # 0, 1, H - 1, H + 1 at 48 kHz (H = 96)
def test_kernel_edge_lengths(n_in):
    raw = A.noise_raw(1, n_in, 2, seed=n_in)
    got, want = _both(raw, 1, 2, 48000)
    assert got.size == A.n_out(n_in, 48000)
    assert np.array_equal(got, want)


def test_kernel_f32_specials():
    x = np.frombuffer(A.noise_raw(4, 3000, 2, seed=9), np.float32).copy() * np.float32(1.4)   # some past +-1
    x[::97] = np.nan
    x[5::101] = np.inf
    x[7::103] = -np.inf
    x[11::107] = -0.0
    for rate in (16000, 48000):
        got, want = _both(x.tobytes(), 4, 2, rate)
        assert np.array_equal(got, want)


def test_timing_seam():
    raw = A.noise_raw(2, 3000, 2, seed=12)
    got, ms = wdr.dbg_audio_convert(raw, 2, 2, 48000, timing=True)
    assert np.array_equal(got, wdr.dbg_audio_convert(raw, 2, 2, 48000, host=True))
    assert 0.0 < ms < 100.0


@pytest.mark.parametrize("rate,chunks", [(48000, [4096, 1000, 97, 7]), (44100, [441, 100])])
def test_chunk_seams_are_invisible(rate, chunks):
    """chunk_frames 97 and 7 are smaller than the 192-tap span at 48 kHz: an output's taps then
    cross many chunks (its own chunk's halo holds them all)."""
    raw = A.noise_raw(1, 5000, 2, seed=rate)
    ref, want = _both(raw, 1, 2, rate)          # the default chunk: one chunk
    assert np.array_equal(ref, want)
    for cf in chunks:
        assert np.array_equal(wdr.dbg_audio_convert(raw, 1, 2, rate, chunk_frames=cf), ref), cf


@pytest.mark.parametrize("rate,fmt,channels,ext", [(48000, 2, 2, True), (44100, 1, 1, False)])
def test_read_audio_on_files(tmp_path, rate, fmt, channels, ext):
    raw = A.noise_raw(fmt, 2 * rate, channels, seed=rate + fmt)
    path = A.write_wav(tmp_path / "a.wav", raw, fmt, channels, rate, extensible=ext,
                       before_data=[A.chunk(b"LIST", b"INFOabc")])
    got = wdr.read_audio(path)
    assert got.size == 32000
    assert np.array_equal(got, wdr.dbg_audio_convert(raw, fmt, channels, rate, host=True))
    d = np.abs(got.astype(np.int32) - A.convert64(raw, fmt, channels, rate).astype(np.int32))
    assert d.max() <= 1 and np.mean(d != 0) <= 0.02


def test_read_audio_equals_read_wav(tmp_path):
    pcm, _ = synth_speech(3.0, seed=2)
    path = str(tmp_path / "a.wav")
    write_wav(path, pcm)
    assert np.array_equal(wdr.read_audio(path), wdr.read_wav(path))
    assert np.array_equal(wdr.read_audio(path, gpu_device=0), pcm)


@pytest.fixture(scope="module")
def speech(tmp_path_factory):
    root = tmp_path_factory.mktemp("audio_engine")
    pcm, _ = synth_speech(12.0, seed=4)
    a = str(root / "a.wav")
    write_wav(a, pcm)
    # the same samples as 16 kHz stereo 32-bit, both channels i16 << 16: converts to exactly pcm
    b = A.write_wav(root / "b.wav", A.encode_i16(np.repeat(pcm, 2), 3), 3, 2, 16000)
    # 48 kHz stereo 16-bit by linear interpolation (fidelity is not the point)
    t = np.arange(3 * pcm.size) / 3.0
    up = np.rint(np.interp(t, np.arange(pcm.size), pcm.astype(np.float64))).astype(np.int16)
    c = A.write_wav(root / "c.wav", np.repeat(up, 2).astype("<i2").tobytes(), 1, 2, 48000)
    return {"root": root, "pcm": pcm, "a": a, "b": b, "c": c}


def test_engine_audio_convert(speech):
    opts = wdr.TranscribeOptions(model="tiny-test", lang="en", enable_vad=False,
                                 advanced=wdr.AdvancedTranscribe(sampling_strategy="greedy"))
    cfg = wdr.EngineConfig(cache_dir=str(speech["root"]))
    assert np.array_equal(wdr.read_audio(speech["b"]), speech["pcm"])
    plain = wdr.Engine(cfg, synthetic=SYN)
    want = plain.transcribe_audio(speech["a"], opts)
    assert len(want) > 0
    # the default engine keeps the reference's reader and its errors
    with pytest.raises(WdrError) as e:
        plain.transcribe_audio(speech["b"], opts)
    assert str(e.value) == "expected mono audio file and found 2 channels!"
    conv = wdr.Engine(cfg, synthetic=SYN, audio_convert=True)
    assert conv.transcribe_audio(speech["b"], opts) == want      # text, times and words
    assert conv.transcribe_audio(speech["a"], opts) == want
    got = conv.transcribe_audio(speech["c"], opts)
    assert len(got) > 0 and abs(got[-1].end - want[-1].end) <= 0.1
    conv.set_audio_convert(False)
    with pytest.raises(WdrError) as e:
        conv.transcribe_audio(speech["c"], opts)
    assert str(e.value) == "expected mono audio file and found 2 channels!"
