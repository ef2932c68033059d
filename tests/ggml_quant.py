"""Test infrastructure: ggml's block-quantized tensor types (q4_0 / q4_1 / q5_0 / q5_1 / q8_0) in
numpy -- the reference row quantizers of ggml (quantize_row_*_ref), the arithmetic definition of
the block decode, and writers of whisper.cpp-format model files that hold such tensors (the files
whisper.cpp's `quantize` tool produces: every 2-D weight matrix quantized, ftype = 2000 + base).

A block is 32 consecutive elements of a row; d and m are f16, everything little-endian:
  q4_0 18 B  d, qs[16]          j / j+16: ((qs[j] & 15) - 8) d, ((qs[j] >> 4) - 8) d
  q4_1 20 B  d, m, qs[16]       (qs[j] & 15) d + m, (qs[j] >> 4) d + m
  q5_0 22 B  d, qh u32, qs[16]  bit j / j+16 of qh is the fifth bit; (q - 16) d
  q5_1 24 B  d, m, qh, qs[16]   q d + m
  q8_0 34 B  d, int8 qs[32]     qs[i] d
The decode computes float(d) * q (+ float(m)) in f32 and rounds once to f16 (nearest even)."""
import struct

import numpy as np

from oracle.mel import mel_filters
from oracle.vocab import Vocab
from oracle.weights import hparams_for, synth_weights, tensor_list
from tests.ggml_writer import write_ggml

FORMATS = ("q4_0", "q4_1", "q5_0", "q5_1", "q8_0")
TYPE_ID = {"q4_0": 2, "q4_1": 3, "q5_0": 6, "q5_1": 7, "q8_0": 8}      # ggml tensor type
FTYPE_BASE = {"q4_0": 2, "q4_1": 3, "q8_0": 7, "q5_0": 8, "q5_1": 9}   # ggml ftype (MOSTLY_*)
BLOCK_BYTES = {"q4_0": 18, "q4_1": 20, "q5_0": 22, "q5_1": 24, "q8_0": 34}
DTYPE = {
    "q4_0": np.dtype([("d", "<f2"), ("qs", "u1", 16)]),
    "q4_1": np.dtype([("d", "<f2"), ("m", "<f2"), ("qs", "u1", 16)]),
    "q5_0": np.dtype([("d", "<f2"), ("qh", "<u4"), ("qs", "u1", 16)]),
    "q5_1": np.dtype([("d", "<f2"), ("m", "<f2"), ("qh", "<u4"), ("qs", "u1", 16)]),
    "q8_0": np.dtype([("d", "<f2"), ("qs", "i1", 32)]),
}
assert all(DTYPE[f].itemsize == BLOCK_BYTES[f] for f in FORMATS)


def _inv(d):
    with np.errstate(divide="ignore"):
        return np.where(d != 0, np.float32(1.0) / d, np.float32(0.0)).astype(np.float32)


def _pack_nibbles(blk, q, bits5):
    """q [nb][32] ints -> qs (low nibble element j, high nibble element j + 16) and, for the
    5-bit formats, qh (bit e = fifth bit of element e)."""
    q = q.astype(np.uint32)
    blk["qs"] = ((q[:, :16] & 15) | ((q[:, 16:] & 15) << 4)).astype(np.uint8)
    if bits5:
        blk["qh"] = (((q >> 4) & 1) << np.arange(32, dtype=np.uint32)).sum(axis=1, dtype=np.uint64).astype(np.uint32)


def quantize(fmt, x):
    """ggml's reference quantizer of format `fmt` on x (size a multiple of 32, rows of blocks in
    flat order): the raw block bytes."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 32)
    blk = np.zeros(x.shape[0], DTYPE[fmt])
    if fmt in ("q4_0", "q5_0"):     # d = (the value of largest magnitude, signed) / -8 or -16
        half = 8 if fmt == "q4_0" else 16
        mx = x[np.arange(x.shape[0]), np.abs(x).argmax(axis=1)]
        d = (mx / np.float32(-half)).astype(np.float32)
        q = np.minimum(2 * half - 1, (x * _inv(d)[:, None] + np.float32(half + 0.5)).astype(np.int32))
        blk["d"] = d.astype(np.float16)
        _pack_nibbles(blk, q, fmt == "q5_0")
    elif fmt in ("q4_1", "q5_1"):   # d = (max - min) / 15 or 31, m = min
        qmax = 15 if fmt == "q4_1" else 31
        mn, mx = x.min(axis=1), x.max(axis=1)
        d = ((mx - mn) / np.float32(qmax)).astype(np.float32)
        q = np.minimum(qmax, ((x - mn[:, None]) * _inv(d)[:, None] + np.float32(0.5)).astype(np.int32))
        blk["d"] = d.astype(np.float16)
        blk["m"] = mn.astype(np.float16)
        _pack_nibbles(blk, q, fmt == "q5_1")
    elif fmt == "q8_0":             # d = amax / 127, q = round(x / d)
        d = (np.abs(x).max(axis=1) / np.float32(127)).astype(np.float32)
        v = x * _inv(d)[:, None]
        blk["d"] = d.astype(np.float16)
        blk["qs"] = (np.sign(v) * np.floor(np.abs(v) + np.float32(0.5))).astype(np.int8)   # roundf
    else:
        raise KeyError(fmt)
    return blk.tobytes()


def dequantize(fmt, raw):
    """The arithmetic definition of the block decode: raw block bytes -> f16 [32 * n_blocks]."""
    blk = np.frombuffer(bytes(raw), DTYPE[fmt])
    d = blk["d"].astype(np.float32)[:, None]
    if fmt == "q8_0":
        v = d * blk["qs"].astype(np.float32)
    else:
        qs = blk["qs"]
        q = np.concatenate([qs & 15, qs >> 4], axis=1).astype(np.int32)
        if fmt in ("q5_0", "q5_1"):
            q |= (((blk["qh"][:, None] >> np.arange(32, dtype=np.uint32)) & 1) << 4).astype(np.int32)
        if fmt == "q4_0":
            q -= 8
        if fmt == "q5_0":
            q -= 16
        v = d * q.astype(np.float32)             # exact in f32
        if fmt in ("q4_1", "q5_1"):
            v = v + blk["m"].astype(np.float32)[:, None]
    assert v.dtype == np.float32
    with np.errstate(over="ignore"):
        return v.astype(np.float16).reshape(-1)  # one rounding, to nearest even


for _f in FORMATS:   # quantize_q4_0(x) .. dequantize_q8_0(raw)
    globals()["quantize_" + _f] = (lambda f: lambda x: quantize(f, x))(_f)
    globals()["dequantize_" + _f] = (lambda f: lambda raw: dequantize(f, raw))(_f)


def _header(hp, ftype, words):
    out = bytearray()
    out += struct.pack("<I", 0x67676D6C)
    out += struct.pack("<11i", hp.n_vocab, hp.n_audio_ctx, hp.n_audio_state, hp.n_audio_head, hp.n_audio_layer,
                       hp.n_text_ctx, hp.n_text_state, hp.n_text_head, hp.n_text_layer, hp.n_mels, ftype)
    filt = mel_filters(hp.n_mels).astype("<f4")
    out += struct.pack("<ii", filt.shape[0], filt.shape[1]) + filt.tobytes()
    out += struct.pack("<i", len(words))
    for w in words:
        b = w.encode("utf-8")
        out += struct.pack("<i", len(b)) + b
    return out


def tensor_record(name, type_id, ne, data):
    """One tensor of the file: header (n_dims, name length, type, ne innermost first), name, data."""
    nb = name.encode()
    return struct.pack("<iii", len(ne), len(nb), type_id) + struct.pack("<%di" % len(ne), *ne) + nb + bytes(data)


def is_quantized(shape, kind):
    """What whisper.cpp's quantize tool converts: the 2-D weight matrices."""
    return kind == "w16" and len(shape) == 2


def write_ggml_quant(path, fmt, name="tiny-test", std=0.02, emb_std=0.5):
    """A `name` model file as whisper.cpp's quantize tool writes it: every 2-D weight matrix in
    format `fmt`, the conv weights f16, everything else f32, ftype = 2000 + base.  Returns the
    weights the file decodes to (the dequantized matrices; the rest as oracle.weights has it)."""
    hp = hparams_for(name)
    W = synth_weights(hp, std=std, emb_std=emb_std)
    voc = Vocab(hp.n_vocab)
    out = _header(hp, 2000 + FTYPE_BASE[fmt], voc.id_to_token[:voc.eot])
    for tname, shape, kind in tensor_list(hp):
        a = W[tname]
        if tname in ("encoder.conv1.bias", "encoder.conv2.bias"):
            a = a.reshape(-1, 1)
        ne = list(reversed(a.shape))
        if is_quantized(shape, kind):
            raw = quantize(fmt, a)
            W[tname] = dequantize(fmt, raw).astype(np.float32).reshape(shape)
            out += tensor_record(tname, TYPE_ID[fmt], ne, raw)
        elif kind == "w16":
            out += tensor_record(tname, 1, ne, np.ascontiguousarray(a.astype("<f2")).tobytes())
        else:
            out += tensor_record(tname, 0, ne, np.ascontiguousarray(a.astype("<f4")).tobytes())
    with open(path, "wb") as f:
        f.write(bytes(out))
    return W


def write_ggml_f16_from(path, W, name="tiny-test"):
    """The plain f16 file (tests/ggml_writer.py layout) that holds the weights W."""
    write_ggml(path, name=name, mutate=lambda base: base.update(W))


def write_single_tensor(path, type_id, ne, data, tname="t", ftype=1, truncate=None):
    """A tiny-test header, an empty vocabulary and one tensor; truncate < 0 cuts that many bytes
    off the end of the file."""
    out = _header(hparams_for("tiny-test"), ftype, []) + tensor_record(tname, type_id, ne, data)
    if truncate is not None:
        out = out[:truncate]
    with open(path, "wb") as f:
        f.write(bytes(out))


def _blocks(fmt, d_bits, qs, m_bits=None, qh=None):
    """Blocks from raw fields: d_bits / m_bits u16 f16 bit patterns [nb], qs [nb][16 or 32], qh [nb]."""
    blk = np.zeros(len(d_bits), DTYPE[fmt])
    blk["d"] = np.asarray(d_bits, np.uint16).view(np.float16)
    blk["qs"] = qs
    if "m" in blk.dtype.names:
        blk["m"] = np.asarray(m_bits, np.uint16).view(np.float16)
    if "qh" in blk.dtype.names:
        blk["qh"] = qh
    return blk.tobytes()


def corner_blocks(fmt):
    """Hand-built blocks for the corners of the decode, as raw bytes:
    the 5-bit formats: one block per set bit of qh (32 blocks, qs all zero): the j / j+16 mapping;
    every format: all 16 nibble values in both halves (q8_0: -128 .. 127 spread over the block),
    with d = 1, negative, +0, -0, the smallest and largest f16 subnormals (0x0001, 0x03ff, and
    0x8001), and m negative (also with the subnormal d)."""
    one, half, neg = 0x3C00, 0x3800, 0xBE00           # 1.0, 0.5, -1.5
    d_bits = [one, neg, 0x0000, 0x8000, 0x0001, 0x03FF, 0x8001, 0x2E66]   # .. 0.1 (inexact products)
    m_bits = [half, 0xB400, 0xB400, 0x3555, 0xB400, 0x8001, 0x0000, 0xC100]   # 0.5, -0.25, .., 1/3, .., -2.5
    n = len(d_bits)
    if fmt == "q8_0":
        qs = np.zeros((n, 32), np.int8)
        qs[:] = np.array([-128, 127, -127, 126, -1, 0, 1, 2] + list(range(-60, 60, 5)), np.int8)
        return _blocks(fmt, d_bits, qs)
    j = np.arange(16, dtype=np.uint8)
    qs = np.zeros((n, 16), np.uint8)
    qs[:] = j | ((15 - j) << 4)                       # low halves 0..15, high halves 15..0
    qh = np.full(n, 0xA5C3F00F, np.uint32)
    out = _blocks(fmt, d_bits, qs, m_bits, qh)
    if fmt in ("q5_0", "q5_1"):
        out += _blocks(fmt, [one] * 32, np.zeros((32, 16), np.uint8), [0xB400] * 32,
                       np.uint32(1) << np.arange(32, dtype=np.uint32))
        out += _blocks(fmt, [neg] * 2, qs[:2], [half] * 2, np.array([0xFFFFFFFF, 0x0000FFFF], np.uint32))
    return out
