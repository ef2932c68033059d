"""The encoder references of tests/encoder_cases.py against the oracle (oracle/model.py's conv stem,
encode and cross_kv at tiny-test), the slot layout against the index arithmetic csrc/common.h
documents, and the defects the GPU tests (tests/test_gpu_encoder_kernels.py) must tell from the
truth: each modelled defect moves a reference by far more than the GPU tests' tolerances.  Plus the
argument checks of the encoder seams, which refuse a bad shape before anything is launched.  CPU only."""
import numpy as np
import pytest

import wdr
from oracle.model import Rounding, Whisper, attention, layer_norm
from oracle.weights import hparams_for, synth_weights
from tests import encoder_cases as ec


@pytest.fixture(scope="module")
def tiny():
    hp = hparams_for("tiny-test")
    W = synth_weights(hp, std=0.02, emb_std=0.5)
    rng = np.random.default_rng(3)
    mels = (rng.standard_normal((2, hp.n_mels, 3000)) * 0.4).astype(np.float32)
    m = Whisper(hp, W)
    enc = [m.encode(mel) for mel in mels]
    return hp, W, m, mels, enc


def test_conv_stem_reference_matches_oracle(tiny):
    hp, W, m, mels, _ = tiny
    mel = mels[0]
    c1 = m.conv1d(mel, W["encoder.conv1.weight"], W["encoder.conv1.bias"], 1)
    a1 = ec.im2col_conv1(ec.f16(mel), kp=256)
    assert (a1[:, 3 * hp.n_mels:] == 0).all() and (a1[0, 0:3 * hp.n_mels:3] == 0).all() and (a1[-1, 2:3 * hp.n_mels:3] == 0).all()
    w1 = np.zeros((hp.n_audio_state, 256))
    w1[:, :3 * hp.n_mels] = ec.conv_w(W["encoder.conv1.weight"])
    np.testing.assert_allclose(a1 @ w1.T + W["encoder.conv1.bias"], c1, rtol=0, atol=2e-5)
    g1 = m.conv_act(c1)
    c2 = m.conv1d(g1.T, W["encoder.conv2.weight"], W["encoder.conv2.bias"], 2)
    # two windows stacked: window 1 must read its own rows (the second copy is shifted data)
    g1b = np.roll(g1, 7, axis=0)
    c2b = m.conv1d(g1b.T, W["encoder.conv2.weight"], W["encoder.conv2.bias"], 2)
    a2 = ec.im2col_conv2(ec.f16(np.concatenate([g1, g1b])), nb=2)
    got = a2 @ ec.conv_w(W["encoder.conv2.weight"]).T + W["encoder.conv2.bias"]
    np.testing.assert_allclose(got[:1500], c2, rtol=0, atol=2e-5)
    np.testing.assert_allclose(got[1500:], c2b, rtol=0, atol=2e-5)
    # window 1's first row has a zero left tap, not window 0's last row
    assert (a2[1500, 0::3] == 0).all() and (a2[1499, 2::3] != 0).any()


def test_layernorm_and_attention_references_match_oracle():
    rng = np.random.default_rng(5)
    x = (100 + rng.standard_normal((9, 260))).astype(np.float32)
    g, b = rng.standard_normal(260).astype(np.float32), rng.standard_normal(260).astype(np.float32)
    np.testing.assert_allclose(ec.layernorm(x, g, b), layer_norm(x, g, b), rtol=0, atol=2e-5)
    rm = np.arange(9)[::-1]
    np.testing.assert_array_equal(ec.layernorm(x, g, b, rm), ec.layernorm(x, g, b)[::-1])
    qkv = rng.standard_normal((2, 70, 3 * 128)).astype(np.float16).astype(np.float32)
    ref = ec.attn_batch(qkv, 2)
    for w in range(2):
        o = attention(qkv[w, :, :128], qkv[w, :, 128:256], qkv[w, :, 256:], 2, Rounding(False))
        np.testing.assert_allclose(ref[w], o, rtol=0, atol=1e-5)
    assert np.abs(ref[0] - ref[1]).max() > 0.1      # the windows differ: a dropped stride would show


def test_slot_layout_follows_common_h(tiny):
    hp, W, m, mels, enc = tiny
    L, H, d = hp.n_text_layer, hp.n_text_head, hp.n_text_state
    cross = m.cross_kv(enc[0])
    kv = np.concatenate([np.concatenate([k, v], axis=1) for k, v in cross], axis=1)     # [1500][L * 2d]
    img = ec.slot_pack(kv, L, H)
    assert img.size == L * 2 * d * 1500
    rng = np.random.default_rng(1)
    for _ in range(200):
        l, h, t, j = rng.integers(L), rng.integers(H), rng.integers(1500), rng.integers(64)
        i = ec.slot_k_index(l, h, t, j, H)
        assert img[i] == cross[l][0][t, 64 * h + j]
        assert img[i + H * ec.SLOT_BLOCK] == cross[l][1][t, 64 * h + j]
        c = l * 2 * d + 64 * h + j                                    # the GEMM column of that K element
        assert i == (c // 64) * ec.SLOT_BLOCK + t * 64 + c % 64       # "its block is c / 64"
    np.testing.assert_array_equal(ec.slot_unpack(np.concatenate([img, np.full(4096, -1.0)]), L, H), kv)


def test_batched_encoder_reference_matches_oracle(tiny):
    """Both windows of a stacked batch equal the oracle's one-window encode within the bounds the
    GPU is held to (tests/test_gpu_whisper.py test_encoder_matches_oracle); the references' only
    differences are fp64 arithmetic and unrounded attention probabilities."""
    hp, W, m, mels, enc = tiny
    got, slots = ec.encode_batch(hp, W, mels)
    for w in range(2):
        err = np.abs(got[w] - enc[w])
        assert err.max() < 5e-3 and err.mean() < 4e-4, (w, err.max(), err.mean())
        cross = m.cross_kv(enc[w])
        kv = ec.slot_unpack(slots[w], hp.n_text_layer, hp.n_text_head).reshape(1500, hp.n_text_layer, 2, -1)
        for l in range(hp.n_text_layer):
            np.testing.assert_allclose(kv[:, l, 0], cross[l][0], rtol=2e-3, atol=2e-3)
            np.testing.assert_allclose(kv[:, l, 1], cross[l][1], rtol=2e-3, atol=2e-3)
    # a defect of the positional wrap (every window-1 row taking rows 1500.. of a longer table is
    # impossible here, so: every row taking row 0) breaks the oracle bound on every window
    bad, _ = ec.encode_batch(hp, W, mels, pos_rows=0)
    for w in range(2):
        err = np.abs(bad[w] - enc[w])
        assert err.max() > 10 * 5e-2 or err.mean() > 10 * 4e-3, (w, err.max(), err.mean())


def test_epilogue_defects_exceed_the_gpu_tolerances():
    """gelu + pos[row % 1500] against pos[0] / pos[row] (no wrap: here clamped), and a slot scatter
    that drops the window stride: each is told from the truth by > 10x the GPU tolerance."""
    rng = np.random.default_rng(2)
    M, N, K = 3000, 128, 64
    a = rng.standard_normal((M, K)).astype(np.float16)
    w = (rng.standard_normal((N, K)) * 0.05).astype(np.float16)
    bias = rng.standard_normal(N) * 0.1
    pos = rng.standard_normal((1500, N))
    ref = ec.proj_gelu_pos(a, w, bias, pos)
    assert np.abs(ec.proj_gelu_pos(a, w, bias, pos[:1]) - ref).max() > 10 * 2e-4
    clamp = ec.gelu(a.astype(np.float64) @ w.astype(np.float64).T + bias) + pos[np.minimum(np.arange(M), 1499)]
    assert np.abs(clamp - ref)[:1500].max() == 0 and np.abs(clamp - ref)[1500:].max() > 10 * 2e-4
    y = (a.astype(np.float64) @ w.astype(np.float64).T).reshape(2, 1500, N)
    i0, i1 = ec.slot_pack(y[0], 1, 1), ec.slot_pack(y[1], 1, 1)
    assert np.abs(i0 - i1).max() > 10 * 2e-3


def test_encoder_seams_refuse_bad_arguments():
    """wdr_dbg_proj_enc / _attn_batch / _layernorm check their arguments on the host and fail with
    their own message before allocating or launching anything."""
    a, w = np.zeros((3000, 64), np.float16), np.zeros((128, 64), np.float16)
    pos = np.zeros((1500, 128), np.float32)
    cases = [
        (lambda: wdr.dbg_proj_enc(a, w, None, 6, slot_elems=128 * 1500 - 4), "slot_elems"),
        (lambda: wdr.dbg_proj_enc(a[:2999], w, None, 6, slot_elems=128 * 1500), "M % 1500"),
        (lambda: wdr.dbg_proj_enc(a, w, None, 6, slot_elems=128 * 1500 + 2), "multiple of 4"),
        (lambda: wdr.dbg_proj_enc(a, w, None, 4), "pos"),
        (lambda: wdr.dbg_proj_enc(a, w, None, 4, pos=np.zeros((3001, 128), np.float32)), "pos_rows"),
        (lambda: wdr.dbg_proj_enc(a, w, None, 3, pos=pos), "epi 4 or 6"),
        (lambda: wdr.dbg_proj_enc(a[:64], w, None, 4, pos=pos[:64]), "M > 64"),
        (lambda: wdr.dbg_proj_enc(a, w[:100], None, 4, pos=pos[:, :100]), "N % 128"),
        (lambda: wdr.dbg_attn_batch(np.zeros((17, 4, 192), np.float16), 1), "bad shape"),
        (lambda: wdr.dbg_attn_batch(np.zeros((1, 4097, 192), np.float16), 1), "bad shape"),
        (lambda: wdr.dbg_layernorm(np.zeros((2, 1284), np.float32), np.zeros(1284), np.zeros(1284)), "d <= 1280"),
        (lambda: wdr.dbg_layernorm(np.zeros((2, 6), np.float32), np.zeros(4), np.zeros(4), d=4), "ldx % 4"),
        (lambda: wdr.dbg_layernorm(np.zeros((2, 8), np.float32), np.zeros(8), np.zeros(8), row_map=[0, 2]), "row_map"),
    ]
    for call, what in cases:
        with pytest.raises(wdr.WdrError, match=what):
            call()
