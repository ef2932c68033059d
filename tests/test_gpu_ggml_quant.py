"""Block-quantized whisper.cpp model files (q4_0 / q4_1 / q5_0 / q5_1 / q8_0) on the GPU: the
load-time dequantization kernel against the arithmetic definition (tests/ggml_quant.py) bit for
bit, and whole models -- a context made from a quantized file must compute exactly what a
context made from the plain f16 file of the dequantized weights computes, through the debug seams
and through the Engine's cache lookup."""
import shutil

import numpy as np
import pytest

import wdr
from oracle.pipeline import write_wav
from oracle.vocab import Vocab
from oracle.weights import hparams_for
from tests import ggml_quant as Q
from tests.ggml_writer import write_ggml
from wdr.synth import synth_speech

pytestmark = pytest.mark.gpu
SYN = wdr.Synthetic(weight_std=0.02, emb_std=0.5, force_len_rate=3.3, disable_fallback=True)


def _bits(a):
    return np.ascontiguousarray(a, np.float16).view(np.uint16)


def _random_blocks(fmt, nb, seed):
    """Random qs / qh bytes; d and m random finite f16 with |value| <= 1, a share of them zero
    (either sign) or subnormal."""
    rng = np.random.default_rng(seed)
    blk = np.frombuffer(rng.integers(0, 256, nb * Q.BLOCK_BYTES[fmt], dtype=np.uint8).tobytes(), Q.DTYPE[fmt]).copy()
    for field in ("d", "m"):
        if field not in blk.dtype.names:
            continue
        bits = rng.uniform(-1, 1, nb).astype(np.float16).view(np.uint16)
        kind = rng.integers(0, 8, nb)
        sign = rng.integers(0, 2, nb).astype(np.uint16) << 15
        bits = np.where(kind == 0, sign, bits)                                              # +-0
        bits = np.where(kind == 1, sign | rng.integers(1, 0x400, nb).astype(np.uint16), bits)   # subnormal
        blk[field] = bits.astype(np.uint16).view(np.float16)
        assert np.isfinite(blk[field]).all() and np.abs(blk[field].astype(np.float32)).max() <= 1
    return blk.tobytes()


# the kernel's workgroup covers 256 blocks (DQ_WG_BLOCKS, csrc/kernels/quant.hip): one block, a
# partial workgroup, both sides of the workgroup boundary, and 16 workgroups + 3 blocks
@pytest.mark.parametrize("nb", [1, 3, 255, 256, 257, 4099])
@pytest.mark.parametrize("fmt", Q.FORMATS)
def test_dequant_kernel_is_the_definition(fmt, nb):
    raw = _random_blocks(fmt, nb, seed=1000 * Q.TYPE_ID[fmt] + nb)
    got = wdr.dbg_dequant(fmt, raw)
    want = Q.dequantize(fmt, raw)
    assert got.shape == want.shape == (32 * nb,)
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("fmt", Q.FORMATS)
def test_dequant_kernel_corners(fmt):
    raw = Q.corner_blocks(fmt)
    assert np.array_equal(_bits(wdr.dbg_dequant(fmt, raw)), _bits(Q.dequantize(fmt, raw)))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """fmt -> (quantized file, f16 file of its dequantized weights), written once per module."""
    root = tmp_path_factory.mktemp("ggml_quant_gpu")
    made = {}

    def get(fmt):
        if fmt not in made:
            qp, hp = str(root / ("ggml-tiny-test-%s.bin" % fmt)), str(root / ("ggml-tiny-test-%s-as-f16.bin" % fmt))
            W = Q.write_ggml_quant(qp, fmt)
            Q.write_ggml_f16_from(hp, W)
            made[fmt] = (qp, hp)
        return made[fmt]
    return get


@pytest.fixture(scope="module")
def probe():
    hp = hparams_for("tiny-test")
    rng = np.random.default_rng(21)
    mel = (rng.standard_normal((hp.n_mels, 3000)) * 0.4).astype(np.float32)
    v = Vocab(hp.n_vocab)
    return mel, [[v.sot], [v.sot, v.beg, 1234, 40000, 77]]


def _outputs(path, probe):
    mel, prompts = probe
    ctx = wdr.WhisperContext("tiny-test", model_path=path, synthetic=SYN)
    return [ctx.encode(mel)] + [ctx.decode(t) for t in prompts]


@pytest.mark.parametrize("fmt", Q.FORMATS)
def test_context_from_quantized_file(files, probe, fmt, tmp_path):
    """Every tensor landed at its place (qkv concatenation, cross-K/V offsets, token embedding):
    encoder output and logits equal those of the f16 file of the dequantized weights exactly."""
    qpath, hpath = files(fmt)
    got, want = _outputs(qpath, probe), _outputs(hpath, probe)
    for g, w in zip(got, want):
        assert np.isfinite(g).all() and np.array_equal(g, w)
    if fmt == "q4_0":   # and the quantized values were really used: not the unquantized weights'
        plain = str(tmp_path / "plain.bin")
        write_ggml(plain)
        other = _outputs(plain, probe)
        assert all(not np.array_equal(g, o) for g, o in zip(got, other))


def test_engine_loads_cached_quantized_file(files, tmp_path):
    """Engine::transcribe_audio finds ggml-<model>.bin in the hf-hub cache layout whatever its
    tensor types.  The name stays tiny-test: a -q5_0 suffix would select the Small alignment-head
    preset (as in the reference), heads a 2-layer model does not have."""
    qpath, hpath = files("q5_0")
    pcm, _ = synth_speech(10.0, seed=4)
    wav = str(tmp_path / "a.wav")
    write_wav(wav, pcm)
    opts = wdr.TranscribeOptions(model="tiny-test", lang="en", enable_vad=True,
                                 advanced=wdr.AdvancedTranscribe(sampling_strategy="greedy"))
    res = []
    for tag, src in (("q", qpath), ("h", hpath)):
        snap = tmp_path / tag / "models--ggerganov--whisper.cpp" / "snapshots" / "rev0"
        snap.mkdir(parents=True)
        shutil.copy(src, snap / "ggml-tiny-test.bin")
        eng = wdr.Engine(wdr.EngineConfig(cache_dir=str(tmp_path / tag)), synthetic=SYN)
        res.append([(s.text, s.start, s.end) for s in eng.transcribe_audio(wav, opts)])
    assert len(res[0]) > 0
    assert res[0] == res[1]
