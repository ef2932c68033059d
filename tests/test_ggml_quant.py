"""The ggml file reader on block-quantized whisper.cpp model files (q4_0 / q4_1 / q5_0 / q5_1 /
q8_0, the files of whisper.cpp's quantize tool), host side only: header and tensor-type
parsing, the scalar host dequantization against the arithmetic definition in
tests/ggml_quant.py bit for bit, the corners of the block decode, and the rejections."""
import collections

import numpy as np
import pytest

import wdr
from oracle.weights import hparams_for, tensor_list
from tests import ggml_quant as Q


def _bits(a):
    return np.ascontiguousarray(a, np.float16).view(np.uint16)


@pytest.fixture(scope="module", params=Q.FORMATS)
def qfile(request, tmp_path_factory):
    fmt = request.param
    path = str(tmp_path_factory.mktemp("ggml_quant") / ("ggml-tiny-test-%s.bin" % fmt))
    W = Q.write_ggml_quant(path, fmt)
    return fmt, path, W


def test_info_of_quantized_file(qfile):
    fmt, path, _ = qfile
    hp = hparams_for("tiny-test")
    info = wdr.ggml_info(path)
    tl = tensor_list(hp)
    assert info["n_tensors"] == len(tl)
    assert info["n_vocab"] == hp.n_vocab and info["n_mels"] == hp.n_mels
    assert info["ftype"] == 2000 + Q.FTYPE_BASE[fmt]
    assert info["ftype_base"] == Q.FTYPE_BASE[fmt] and info["qnt_version"] == 2
    want = collections.Counter(Q.TYPE_ID[fmt] if Q.is_quantized(shape, kind) else 1 if kind == "w16" else 0
                               for _, shape, kind in tl)
    assert want[Q.TYPE_ID[fmt]] > 0 and want[1] == 2 and want[0] > 0
    assert info["tensor_types"] == dict(want)


def test_info_of_f16_file_keeps_its_keys(tmp_path):
    from tests.ggml_writer import write_ggml
    path = str(tmp_path / "m.bin")
    hp, n_tensors, n_words, _ = write_ggml(path)
    info = wdr.ggml_info(path)
    assert info["n_tensors"] == n_tensors and info["n_vocab_tokens"] == n_words and info["ftype"] == 1
    assert info["ftype_base"] == 1 and info["qnt_version"] == 0
    assert set(info["tensor_types"]) == {0, 1} and sum(info["tensor_types"].values()) == n_tensors


@pytest.mark.parametrize("tname", ["encoder.blocks.1.attn.key.weight", "decoder.blocks.0.mlp.2.weight",
                                   "decoder.token_embedding.weight"])
def test_host_dequantization_is_the_definition(qfile, tname):
    """A square attention weight, mlp.2.weight (512 columns) and the token embedding."""
    fmt, path, W = qfile
    got = wdr.ggml_tensor_f16(path, tname)
    want = W[tname].astype(np.float16).reshape(-1)   # W holds dequantize_<fmt>'s f16 values
    assert got.size == want.size
    assert np.array_equal(_bits(got), _bits(want))


def test_unquantized_tensors_of_a_quantized_file(qfile):
    fmt, path, W = qfile
    for tname in ("encoder.conv2.weight", "decoder.positional_embedding", "encoder.conv1.bias"):
        got = wdr.ggml_tensor_f16(path, tname)
        assert np.array_equal(_bits(got), _bits(W[tname].astype(np.float16).reshape(-1)))


@pytest.mark.parametrize("fmt", Q.FORMATS)
def test_block_decode_corners(tmp_path, fmt):
    raw = Q.corner_blocks(fmt)
    nb = len(raw) // Q.BLOCK_BYTES[fmt]
    assert nb * Q.BLOCK_BYTES[fmt] == len(raw) and nb >= 8
    path = str(tmp_path / "c.bin")
    Q.write_single_tensor(path, Q.TYPE_ID[fmt], [32, nb], raw, tname="corner", ftype=2000 + Q.FTYPE_BASE[fmt])
    assert wdr.ggml_info(path)["tensor_types"] == {Q.TYPE_ID[fmt]: 1}
    got = wdr.ggml_tensor_f16(path, "corner")
    want = Q.dequantize(fmt, raw)
    assert np.array_equal(_bits(got), _bits(want))
    # the definition itself, spelled out for the first (d = 1) block
    v = want[:32].astype(np.float32)
    if fmt == "q8_0":
        assert v[0] == -128 and v[1] == 127
    elif fmt == "q4_0":
        assert list(v) == [j - 8 for j in range(16)] + [7 - j for j in range(16)]
    elif fmt == "q4_1":
        assert list(v) == [j + 0.5 for j in range(16)] + [15.5 - j for j in range(16)]
    else:
        hi = [(0xA5C3F00F >> e) & 1 for e in range(32)]
        q = [j | hi[j] << 4 for j in range(16)] + [(15 - j) | hi[16 + j] << 4 for j in range(16)]
        assert list(v) == ([x - 16 for x in q] if fmt == "q5_0" else [x + 0.5 for x in q])
        k = 8                                      # the blocks with qh = 1 << e: only element e has the fifth bit
        one_bit = want[32 * k:32 * (k + 32)].astype(np.float32).reshape(32, 32)
        base, top = (-16.0, 0.0) if fmt == "q5_0" else (-0.25, 15.75)
        assert np.array_equal(one_bit, np.where(np.eye(32, dtype=bool), top, base))


def test_rejections(tmp_path):
    p = str(tmp_path / "bad.bin")
    Q.write_single_tensor(p, 12, [256, 2], bytes(1024))                      # a k-quant (q4_K)
    with pytest.raises(wdr.WdrError, match="unsupported tensor type 12"):
        wdr.ggml_info(p)
    Q.write_single_tensor(p, 8, [48, 2], bytes(3 * 34), tname="odd.weight")  # ne[0] not whole blocks
    with pytest.raises(wdr.WdrError, match="odd.weight.*multiple of 32"):
        wdr.ggml_info(p)
    raw = Q.quantize("q5_0", np.linspace(-1, 1, 64 * 4, dtype=np.float32))
    Q.write_single_tensor(p, 6, [64, 4], raw)
    assert wdr.ggml_info(p)["n_tensors"] == 1
    Q.write_single_tensor(p, 6, [64, 4], raw, truncate=-1)                   # cut inside the tensor's data
    with pytest.raises(wdr.WdrError, match="truncated"):
        wdr.ggml_info(p)
    Q.write_single_tensor(p, 6, [64, 4], raw, truncate=-(len(raw) + 3))      # cut inside its header (the name / ne)
    with pytest.raises(wdr.WdrError, match="truncated"):
        wdr.ggml_info(p)
    with pytest.raises(wdr.WdrError, match="truncated"):
        wdr.ggml_tensor_f16(p, "t")
