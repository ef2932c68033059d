"""Audio ingest on the host (no GPU): the general WAV parser, the resampler's coefficient table,
and the host definition of the conversion to 16 kHz mono int16 against the
float64 reference of tests/audio_ref.py."""
import struct

import numpy as np
import pytest

import wdr
from tests import audio_ref as A
from wdr._lib import WdrError

RATES = [48000, 44100, 8000, 22050, 12345]
TABLE_DIMS = {48000: (1, 3, 192), 44100: (160, 441, 178), 8000: (2, 1, 64), 22050: (320, 441, 90),
              12345: (3200, 2469, 64)}


def _write(tmp_path, data, name="a.wav"):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


# ------------------------------------------------------------------ 1. parser
@pytest.mark.parametrize("extensible", [False, True])
@pytest.mark.parametrize("channels", [1, 2, 3, 6, 8])
@pytest.mark.parametrize("fmt", [0, 1, 2, 3, 4])
def test_audio_info_formats(tmp_path, fmt, channels, extensible):
    raw = A.noise_raw(fmt, 11, channels, seed=fmt * 10 + channels)
    path = A.write_wav(tmp_path / "a.wav", raw, fmt, channels, 44100, extensible=extensible)
    assert wdr.audio_info(path) == {"fmt": fmt, "channels": channels, "rate": 44100, "bits": A.FMT_BITS[fmt],
                                    "block_align": channels * A.FMT_BYTES[fmt], "n_frames": 11}


def test_audio_info_chunk_walk(tmp_path):
    raw = A.noise_raw(2, 9, 3, seed=1)   # 81 bytes: the data chunk itself is odd-sized
    want = {"fmt": 2, "channels": 3, "rate": 48000, "bits": 24, "block_align": 9, "n_frames": 9}
    # an odd-sized LIST chunk (and its pad byte) in front of data
    p = A.write_wav(tmp_path / "list.wav", raw, 2, 3, 48000, before_data=[A.chunk(b"LIST", b"INFOabc")])
    assert wdr.audio_info(p) == want
    # piped output: the data size was never filled in
    for size in (0xFFFFFFFF, 0):
        p = A.write_wav(tmp_path / "pipe.wav", raw, 2, 3, 48000, data_size=size)
        assert wdr.audio_info(p) == want
    # a size past the end of the file is clamped; a trailing partial frame is dropped
    p = A.write_wav(tmp_path / "long.wav", raw, 2, 3, 48000, data_size=5000)
    assert wdr.audio_info(p) == want
    p = A.write_wav(tmp_path / "part.wav", raw + b"\x01\x02\x03\x04", 2, 3, 48000)
    assert wdr.audio_info(p) == want
    # a data size of 0 in front of whole chunks is an empty data chunk, not "to the end"
    p = A.write_wav(tmp_path / "empty.wav", b"", 2, 3, 48000, tail=A.chunk(b"LIST", b"INFOabc"))
    assert wdr.audio_info(p) == dict(want, n_frames=0)
    p = A.write_wav(tmp_path / "empty2.wav", b"", 2, 3, 48000)
    assert wdr.audio_info(p) == dict(want, n_frames=0)
    # chunks after data are not samples
    p = A.write_wav(tmp_path / "tail.wav", raw, 2, 3, 48000, tail=A.chunk(b"LIST", b"INFOabcd" * 4))
    assert wdr.audio_info(p) == want


REJECTS = [
    ("alaw", dict(tag=6, bits=8), "A-law audio is not supported (format tag 6)"),
    ("mulaw", dict(tag=7, bits=8), "mu-law audio is not supported (format tag 7)"),
    ("adpcm", dict(tag=2, bits=4, block_align=256), "ADPCM audio is not supported (format tag 2)"),
    ("ima", dict(tag=0x11, bits=4, block_align=256), "ADPCM audio is not supported (format tag 17)"),
    ("mp3", dict(tag=0x55, bits=0, block_align=1), "unsupported WAV format tag 85"),
    ("f64", dict(tag=3, bits=64), "64-bit float samples are not supported"),
    ("f16", dict(tag=3, bits=16), "float samples must be 32-bit, found 16 bits per sample"),
    ("bits12", dict(bits=12), "unsupported bits per sample: 12 (8, 16, 24 or 32)"),
    ("bits64", dict(bits=64), "unsupported bits per sample: 64 (8, 16, 24 or 32)"),
    ("align", dict(block_align=6), "block align 6 does not match 2 channels of 16 bits"),
]


@pytest.mark.parametrize("name,over,msg", REJECTS, ids=[r[0] for r in REJECTS])
def test_audio_info_rejects_format(tmp_path, name, over, msg):
    p = A.write_wav(tmp_path / "a.wav", bytes(64), 1, 2, 44100, **over)
    with pytest.raises(WdrError) as e:
        wdr.audio_info(p)
    assert str(e.value) == msg
    if over.get("tag") in (6, 7):   # the same through an extensible header's SubFormat
        p = A.write_wav(tmp_path / "x.wav", bytes(64), 1, 2, 44100, extensible=True, **over)
        with pytest.raises(WdrError) as e:
            wdr.audio_info(p)
        assert str(e.value) == msg


def test_audio_info_rejects_header(tmp_path):
    def err(data):
        with pytest.raises(WdrError) as e:
            wdr.audio_info(_write(tmp_path, data))
        return str(e.value)

    raw = bytes(32)
    assert err(A.wav_bytes(raw, 1, 0, 44100, block_align=2)) == "unsupported channel count 0 (1 to 8)"
    assert err(A.wav_bytes(raw, 1, 9, 44100)) == "unsupported channel count 9 (1 to 8)"
    assert err(A.wav_bytes(raw, 1, 1, 999)) == "unsupported sample rate 999 Hz (1000 to 384000)"
    assert err(A.wav_bytes(raw, 1, 1, 384001)) == "unsupported sample rate 384001 Hz (1000 to 384000)"
    assert wdr.audio_info(_write(tmp_path, A.wav_bytes(raw, 1, 1, 1000)))["rate"] == 1000
    assert wdr.audio_info(_write(tmp_path, A.wav_bytes(raw, 1, 1, 384000)))["rate"] == 384000
    short = b"WAVE" + A.chunk(b"fmt ", A.fmt_chunk(1, 1, 16000)[:14]) + A.chunk(b"data", raw)
    assert err(b"RIFF" + struct.pack("<I", len(short)) + short) == "fmt chunk too short (14 bytes)"
    ext = b"WAVE" + A.chunk(b"fmt ", A.fmt_chunk(1, 1, 16000, extensible=True)[:24]) + A.chunk(b"data", raw)
    assert err(b"RIFF" + struct.pack("<I", len(ext)) + ext) == "extensible fmt chunk too short (24 bytes)"
    nofmt = b"WAVE" + A.chunk(b"data", raw)
    assert err(b"RIFF" + struct.pack("<I", len(nofmt)) + nofmt) == "no fmt chunk"
    nodata = b"WAVE" + A.chunk(b"fmt ", A.fmt_chunk(1, 1, 16000)) + A.chunk(b"LIST", b"INFO")
    assert err(b"RIFF" + struct.pack("<I", len(nodata)) + nodata) == "no data chunk"
    good = A.wav_bytes(raw, 1, 1, 16000)
    assert err(b"RF64" + good[4:]) == "RF64 files are not supported"
    assert err(b"RIFX" + good[4:]) == "not a RIFF/WAVE file"
    assert err(good[:8] + b"AVI " + good[12:]) == "not a RIFF/WAVE file"
    assert err(b"") == "not a RIFF/WAVE file"
    with pytest.raises(WdrError) as e:
        wdr.audio_info(str(tmp_path / "missing.wav"))
    assert str(e.value) == "audio file doesn't exist"


def test_audio_info_every_prefix(tmp_path):
    """Every proper prefix of a small valid file is an error and nothing else.  The file is 60
    bytes with `data` in front of `fmt `: a cut anywhere loses the format.  (With `data` last, a
    cut inside the samples is by definition a data size past the end of the file, which is
    clamped: those prefixes are checked to parse, with the frames that are whole.)"""
    raw = A.noise_raw(1, 8, 1, seed=3)
    body = b"WAVE" + A.chunk(b"data", raw) + A.chunk(b"fmt ", A.fmt_chunk(1, 1, 16000))
    full = b"RIFF" + struct.pack("<I", len(body)) + body
    assert len(full) == 60
    assert wdr.audio_info(_write(tmp_path, full))["n_frames"] == 8
    for n in range(len(full)):
        with pytest.raises(WdrError) as e:
            wdr.audio_info(_write(tmp_path, full[:n]))
        # no RIFF/WAVE head; no (whole) fmt chunk header in reach; the fmt chunk's body cut
        want = "not a RIFF/WAVE file" if n < 12 else "no fmt chunk" if n < 44 else "fmt chunk truncated"
        assert str(e.value) == want, n
    usual = A.wav_bytes(raw, 1, 1, 16000)
    assert len(usual) == 60
    for n in range(len(usual)):
        p = _write(tmp_path, usual[:n])
        if n < 44:
            with pytest.raises(WdrError) as e:
                wdr.audio_info(p)
            want = ("not a RIFF/WAVE file" if n < 12 else "no fmt chunk" if n < 20 else "fmt chunk truncated" if n < 36
                    else "no data chunk")
            assert str(e.value) == want, n
        else:
            assert wdr.audio_info(p)["n_frames"] == (n - 44) // 2


# ------------------------------------------------------------------ 2. table
@pytest.mark.parametrize("rate", RATES)
def test_resample_table(rate):
    L, M, T, tab = wdr.dbg_resample_table(rate)
    assert (L, M, T) == TABLE_DIMS[rate]
    assert A.dims(rate) == (L, M, T // 2, T)
    want = A.table64(rate).astype(np.float32)
    assert tab.shape == want.shape == (L, T) and tab.dtype == np.float32
    # within 1 f32 ulp of the double value rounded to f32
    assert np.all(np.abs(tab.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))
    assert abs(float(tab.astype(np.float64).sum()) / L - 1.0) < 1e-3   # unity gain at DC


def test_resample_table_16k_and_bad_rates():
    """Bad rates first: the rejection must not depend on what an earlier call left behind."""
    for r in (0, -5, 999, 384001, 0):
        with pytest.raises(WdrError) as e:
            wdr.dbg_resample_table(r)
        assert str(e.value) == "unsupported sample rate %d Hz (1000 to 384000)" % r
        with pytest.raises(WdrError) as e:
            wdr.dbg_audio_convert(bytes(8), 1, 1, r, host=True)
        assert str(e.value) == "unsupported sample rate %d Hz (1000 to 384000)" % r
    assert wdr.dbg_resample_table(16000)[:3] == (1, 1, 0)
    assert wdr.dbg_resample_table(16000)[:3] == (1, 1, 0)
    for r in (0, 999):
        with pytest.raises(WdrError):
            wdr.dbg_resample_table(r)


# ------------------------------------------------------------------ 3. host definition against float64
HOST_CASES = [(r, 1, 1) for r in RATES + [96000, 47999]] + [(48000, f, 2) for f in (0, 2, 3, 4)] + [(44100, 1, 3)]


def _check_against_float64(got, raw, fmt, channels, rate):
    want = A.convert64(raw, fmt, channels, rate)
    assert got.dtype == np.int16 and got.shape == want.shape
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    differ = float(np.mean(d != 0)) if d.size else 0.0
    print("rate %d fmt %d ch %d: max |diff| %d LSB, %.3f %% of %d samples differ"
          % (rate, fmt, channels, d.max() if d.size else 0, 100 * differ, d.size))
    assert d.size == 0 or d.max() <= 1      # f32 sequential fma against float64: 1 LSB
    assert differ <= 0.02                   # and rarely (a cap; the prototype showed <= 0.35 %)


@pytest.mark.parametrize("rate,fmt,channels", HOST_CASES)
def test_host_definition_against_float64(rate, fmt, channels):
    raw = A.noise_raw(fmt, 6000, channels, seed=rate + 7 * fmt + channels)
    got = wdr.dbg_audio_convert(raw, fmt, channels, rate, host=True)
    assert got.size == A.n_out(6000, rate)
    _check_against_float64(got, raw, fmt, channels, rate)


# ------------------------------------------------------------------ 4. properties of the host definition
def test_identity_of_shifted_i16_stereo():
    pcm = np.random.default_rng(5).integers(-32768, 32768, 4000).astype(np.int16)
    raw = A.encode_i16(np.repeat(pcm, 2), 3)   # both channels i16 << 16
    assert np.array_equal(wdr.dbg_audio_convert(raw, 3, 2, 16000, host=True), pcm)
    for fmt in (1, 2, 4):
        assert np.array_equal(wdr.dbg_audio_convert(A.encode_i16(pcm, fmt), fmt, 1, 16000, host=True), pcm)


def test_read_audio_of_a_read_wav_file_needs_no_gpu(tmp_path):
    pcm = np.random.default_rng(6).integers(-32768, 32768, 12345).astype(np.int16)
    for ext in (False, True):
        p = A.write_wav(tmp_path / "m.wav", pcm.tobytes(), 1, 1, 16000, extensible=ext,
                        before_data=[A.chunk(b"LIST", b"INFOxyz")])
        got = wdr.read_audio(p)
        assert np.array_equal(got, wdr.read_wav(p)) and np.array_equal(got, pcm)
    p = A.write_wav(tmp_path / "e.wav", b"", 1, 1, 16000)
    assert wdr.read_audio(p).size == 0


@pytest.mark.parametrize("rate", [48000, 44100])
def test_click_keeps_its_time(rate):
    x = np.zeros(rate, np.int16)
    x[rate // 2] = 30000
    out = wdr.dbg_audio_convert(x.tobytes(), 1, 1, rate, host=True)
    assert out.size == 16000
    assert int(np.argmax(np.abs(out.astype(np.int32)))) == 8000
    assert out[8000] > 0 and not out[:8000 - 40].any() and not out[8000 + 40:].any()


def test_square_wave_saturates():
    n = 4800
    x = np.where((np.arange(n) // 120) % 2 == 0, 32767, -32768).astype(np.int16)   # 200 Hz, full scale
    out = wdr.dbg_audio_convert(x.tobytes(), 1, 1, 48000, host=True)
    assert out.max() == 32767 and out.min() == -32768     # the overshoot is clamped
    want = A.convert64(x.tobytes(), 1, 1, 48000)
    assert np.abs(out.astype(np.int32) - want.astype(np.int32)).max() <= 1   # never wraps


def test_f32_specials_follow_the_decode_rule():
    s = np.array([np.nan, np.inf, -np.inf, 1.5, -1.5, 1.0, -1.0, 0.5, -0.0, 3e-6], np.float32)
    want = np.array([0, 32767, -32768, 32767, -32768, 32767, -32768, 16384, 0, 0], np.int16)
    assert np.array_equal(wdr.dbg_audio_convert(s.tobytes(), 4, 1, 16000, host=True), want)
    # downmix: (nan -> 0, 1) and (+inf -> 1, -inf -> -1)
    st = np.array([np.nan, 1.0, np.inf, -np.inf, 1.5, 0.5], np.float32)
    assert np.array_equal(wdr.dbg_audio_convert(st.tobytes(), 4, 2, 16000, host=True), [16384, 0, 24576])
    # and through the filter the clamp keeps the values finite
    noise = np.frombuffer(A.noise_raw(4, 1000, 1, seed=8), np.float32).copy()
    noise[::97] = np.nan
    noise[5::101] = np.inf
    noise[7::103] = -1.5
    _check_against_float64(wdr.dbg_audio_convert(noise.tobytes(), 4, 1, 48000, host=True), noise.tobytes(), 4, 1, 48000)


@pytest.mark.parametrize("n_in", [0, 1, 95, 97])   # 0, 1, H - 1, H + 1 at 48 kHz (H = 96)
@pytest.mark.parametrize("rate", [48000, 8000])
def test_edge_lengths(rate, n_in):
    raw = A.noise_raw(1, n_in, 2, seed=n_in)
    got = wdr.dbg_audio_convert(raw, 1, 2, rate, host=True)
    assert got.size == A.n_out(n_in, rate)
    _check_against_float64(got, raw, 1, 2, rate)


def test_bad_arguments():
    for fmt, ch in ((5, 1), (-1, 1)):
        with pytest.raises(ValueError):
            wdr.dbg_audio_convert(b"", fmt, ch, 48000, host=True)
    with pytest.raises(ValueError):
        wdr.dbg_audio_convert(bytes(5), 1, 2, 48000, host=True)
    with pytest.raises(WdrError):
        wdr.dbg_audio_convert(bytes(4), 1, 2, 500, host=True)
