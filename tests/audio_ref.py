"""The independent reference of the audio conversion in numpy float64, and a WAV
writer for every sample format, channel count and rate the library reads.

The conversion here follows the same definition as the library's host code but shares nothing
with it: the filter is evaluated in double and never rounded to f32, and the taps are summed in
double.  What it shares with the definition is the input decode, which is exact in both (every
scale is a power of two; the int32 -> f32 conversion of fmt 3 is part of the definition).
"""
import math
import struct

import numpy as np

FMT_BITS = {0: 8, 1: 16, 2: 24, 3: 32, 4: 32}
FMT_BYTES = {f: b // 8 for f, b in FMT_BITS.items()}
OUT_RATE = 16000
BETA = 9.0


def dims(rate):
    """(L, M, H, T) of a source rate."""
    g = math.gcd(OUT_RATE, rate)
    L, M = OUT_RATE // g, rate // g
    H = -(-32 * M // L) if M > L else 32
    return L, M, H, 2 * H


def n_out(n_in, rate):
    L, M, _, _ = dims(rate)
    return -(-n_in * L // M)


def table64(rate, phases=None):
    """Rows `phases` (default all L) of the coefficient table, float64 [len(phases)][T]."""
    L, M, H, T = dims(rate)
    s = min(1.0, L / M)
    W = 32.0 * M / L if M > L else 32.0
    cut = 0.94 * s
    p = np.arange(L) if phases is None else np.asarray(phases)
    t = p[:, None].astype(np.float64) / L - (np.arange(T)[None, :] - H + 1)
    inside = np.abs(t) < W
    r = np.where(inside, t / W, 0.0)
    g = cut * np.sinc(cut * t) * np.i0(BETA * np.sqrt(1.0 - r * r)) / np.i0(BETA)
    return np.where(inside, g, 0.0)


def decode(raw, fmt, channels):
    """raw interleaved bytes -> float64 [n_frames][channels] (the exact decoded values)."""
    b = np.frombuffer(bytes(raw), np.uint8)
    if fmt == 0:
        x = (b.astype(np.float64) - 128.0) / 128.0
    elif fmt == 1:
        x = b.view("<i2").astype(np.float64) / 32768.0
    elif fmt == 2:
        t = b.reshape(-1, 3).astype(np.int32)
        v = t[:, 0] | t[:, 1] << 8 | t[:, 2] << 16
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        x = v.astype(np.float64) / 8388608.0
    elif fmt == 3:
        x = b.view("<i4").astype(np.float32).astype(np.float64) / 2147483648.0
    elif fmt == 4:
        s = b.view("<f4").astype(np.float64)
        x = np.where(np.isnan(s), 0.0, np.clip(s, -1.0, 1.0))
    else:
        raise ValueError(fmt)
    return x.reshape(-1, channels)


def convert64(raw, fmt, channels, rate):
    """The conversion in float64 -> int16 [n_out]."""
    m = decode(raw, fmt, channels).sum(axis=1) / channels
    n_in = m.size
    L, M, H, T = dims(rate)
    no = n_out(n_in, rate)
    if rate == OUT_RATE:
        acc = m
    else:
        k = np.arange(no, dtype=np.int64)
        j0, p = (k * M) // L, (k * M) % L
        up, inv = np.unique(p, return_inverse=True)
        tab = table64(rate, up)
        mp = np.concatenate([np.zeros(H), m, np.zeros(H + 1)])   # frame j at mp[j + H]
        acc = np.empty(no)
        for a in range(0, no, 4096):                            # bounded working set
            sl = slice(a, min(no, a + 4096))
            idx = (j0[sl, None] + 1) + np.arange(T)[None, :]    # j0 - H + 1 + i, shifted by H
            acc[sl] = (mp[idx] * tab[inv[sl]]).sum(axis=1)
    return np.rint(np.clip(acc * 32768.0, -32768.0, 32767.0)).astype(np.int16)


def noise_raw(fmt, n_frames, channels, seed):
    """Seeded full-scale white noise as raw interleaved bytes."""
    rng = np.random.default_rng(seed)
    n = n_frames * channels
    if fmt == 0:
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if fmt == 1:
        return rng.integers(-32768, 32768, n).astype("<i2").tobytes()
    if fmt == 2:
        return rng.integers(0, 256, 3 * n, dtype=np.uint8).tobytes()
    if fmt == 3:
        return rng.integers(-2 ** 31, 2 ** 31, n).astype("<i4").tobytes()
    return rng.uniform(-1.0, 1.0, n).astype("<f4").tobytes()


def encode_i16(x, fmt):
    """int16-valued samples (any shape, interleaved order) -> raw bytes of an integer format whose
    decoded value is exactly x / 32768 (fmt 1, 2, 3) or the f32 x / 32768 (fmt 4)."""
    x = np.asarray(x, np.int64).ravel()
    if fmt == 1:
        return x.astype("<i2").tobytes()
    if fmt == 2:
        v = (x << 8) & 0xFFFFFF
        return np.stack([v & 255, v >> 8 & 255, v >> 16 & 255], axis=1).astype(np.uint8).tobytes()
    if fmt == 3:
        return (x << 16).astype("<i4").tobytes()
    if fmt == 4:
        return (x.astype(np.float32) / np.float32(32768.0)).astype("<f4").tobytes()
    raise ValueError(fmt)


_GUID_TAIL = bytes([0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71])


def fmt_chunk(fmt, channels, rate, extensible=False, tag=None, bits=None, block_align=None):
    """The body of a `fmt ` chunk; tag / bits / block_align override the consistent values."""
    bits = FMT_BITS[fmt] if bits is None else bits
    tag = (3 if fmt == 4 else 1) if tag is None else tag
    align = channels * bits // 8 if block_align is None else block_align
    head = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, (rate * align) & 0xFFFFFFFF,
                       align & 0xFFFF, bits)
    if not extensible:
        return head
    return head + struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", tag) + _GUID_TAIL


def chunk(name, body, size=None):
    """One RIFF chunk (padded to an even size); size overrides the size field."""
    n = len(body) if size is None else size
    return name + struct.pack("<I", n) + bytes(body) + (b"\0" if len(body) & 1 else b"")


def wav_bytes(raw, fmt, channels, rate, extensible=False, before_data=(), data_size=None, tail=b"", **over):
    """A whole WAV file: `fmt `, the chunks of before_data, `data` (+ tail bytes after it)."""
    body = b"WAVE" + chunk(b"fmt ", fmt_chunk(fmt, channels, rate, extensible, **over))
    for c in before_data:
        body += c
    body += chunk(b"data", raw, data_size) + tail
    return b"RIFF" + struct.pack("<I", len(body) & 0xFFFFFFFF) + body


def write_wav(path, raw, fmt, channels, rate, **kw):
    with open(path, "wb") as f:
        f.write(wav_bytes(raw, fmt, channels, rate, **kw))
    return str(path)
