"""The production encoder path against references: k_im2col_mel (conv1's operand in every production
encode), the encoder-only GEMM epilogues on every tile kernel (conv2's gelu + positional rows, the
cross-K/V slot scatter), the batched self-attention launch, k_layernorm alone, and whole
encode-ahead batches of 1 .. 4 windows -- each against the fp64 references of tests/encoder_cases.py
(checked against the oracle on the CPU by tests/test_encoder_cases.py) and, where the source
promises it, bit for bit against the reference tile / the single-window path.

Tolerances: 2e-4 absolute on f32 outputs (accumulation order; gelu_tanh is within 5e-7 of the tanh
form), rtol = atol = 2e-3 on f16 outputs (f16 rounding, 2^-11 relative), the flash attention's
1e-2 / mean 1.5e-3 (P enters P.V as f16), LayerNorm one f16 ulp (2^-10) + 1e-4, the encoder against
the oracle max 5e-2 / mean 4e-3 as tests/test_gpu_whisper.py holds it."""
import ctypes as C

import numpy as np
import pytest

import wdr
from oracle.mel import log_mel, pcm_i16_to_f32
from oracle.model import Whisper
from oracle.weights import hparams_for, synth_weights
from tests import encoder_cases as ec
from wdr import _lib
from wdr.synth import synth_speech

pytestmark = pytest.mark.gpu

U16 = C.POINTER(C.c_uint16)
F32 = C.POINTER(C.c_float)
I32 = C.POINTER(C.c_int32)
EMB_STD = 0.5
SYN = wdr.Synthetic(weight_std=0.02, emb_std=EMB_STD, force_len_rate=3.3, disable_fallback=True)
KERNELS = {"k_gemm": 0, "k_gemm2": 1, "k_gemm4": 2, "k_gemm5": 3}


@pytest.fixture(scope="module")
def pcm():
    return synth_speech(40.0, seed=0)[0]


def _context(name):
    hp = hparams_for(name)
    return wdr.WhisperContext(name, synthetic=SYN), hp, synth_weights(hp, std=0.02, emb_std=EMB_STD)


@pytest.fixture(scope="module", params=["tiny-test", "tiny-test-ml"])
def model(request):
    ctx, hp, W = _context(request.param)
    yield request.param, ctx, hp, W
    ctx.close()


# ------------------------------------------------------------------ 1. k_im2col_mel
_ORACLE_MEL = {}


def _oracle_mel(pcm, a, b, n_mels):
    """The oracle's log-mel of pcm[a:b], computed once per clip and filter bank."""
    key = (a, b, n_mels)
    if key not in _ORACLE_MEL:
        _ORACLE_MEL[key] = log_mel(pcm_i16_to_f32(pcm[a:b]), n_mels)
    return _ORACLE_MEL[key]


# (first sample, last sample, seek): 7 s at seek 0 (n_fft_frames = 702: most frames take the -10
# fill), 35 s at seek 3000 (the second window: 502 computed frames), 35 s at seek 2000 (computed
# frames end at window frame 1502)
IM2COL_CASES = {"7s_seek0": (2 * 16000, 9 * 16000, 0), "35s_seek3000": (0, 35 * 16000, 3000),
                "35s_seek2000": (0, 35 * 16000, 2000)}


@pytest.mark.parametrize("case", sorted(IM2COL_CASES))
def test_im2col_mel(model, pcm, case):
    """Every element of conv1's operand is float16(log_mel_window)[ci, t + k - 1] bit for bit, the
    taps at window frames -1 and 3000 and the pad columns [3 n_mels, kp) are +0, and the whole
    operand is within 2e-3 plus f16 rounding of the oracle's log-mel.

    The bit-for-bit part pins the operand's rounding too: k_im2col_mel rounds the double
    normalisation once to f16, and log_mel_window reads the window back as f32 rounded to odd so that
    float16() of it is that same f16 (csrc/kernels/elem.hip f32_round_to_odd).  With the window read
    back as the nearest f32 instead, 3 .. 15 elements of these windows were one f16 ulp apart."""
    name, ctx, hp, W = model
    a, b, seek = IM2COL_CASES[case]
    x = pcm_i16_to_f32(pcm[a:b])
    n_fft_frames = min((x.size + 200) // 160 + 1, (x.size + 480000) // 160)
    assert seek < n_fft_frames < seek + 3000                      # the fill starts inside the window
    got = ctx.im2col_mel(x, seek)
    kp = got.shape[1]
    C3 = 3 * hp.n_mels
    assert got.shape == (3000, kp) and kp == (C3 + 31) // 32 * 32
    assert kp - C3 == {"tiny-test": 16, "tiny-test-ml": 0}[name]
    bits = got.view(np.uint16)
    assert (bits[:, C3:] == 0).all()                              # pad columns: +0, not -0 or stale
    assert (bits[0, 0:C3:3] == 0).all() and (bits[2999, 2:C3:3] == 0).all()
    assert len(np.unique(bits[:, :C3])) > 100                     # not a constant image
    ref = ec.im2col_conv1(_oracle_mel(pcm, a, b, hp.n_mels)[:, seek:seek + 3000], kp)
    err = np.abs(got.astype(np.float64) - ref)
    bound = 2e-3 + 2.0 ** -11 * (np.abs(ref) + 2e-3)
    assert (err <= bound).all(), float((err / bound).max())
    win = ctx.log_mel_window(x, seek)
    want = ec.im2col_conv1(win.astype(np.float16), kp).astype(np.float16)
    off = bits != want.view(np.uint16)
    print("im2col_mel %s %s: max err %.3g of the oracle, %d of %d elements off float16(log_mel_window), %d ulp"
          % (name, case, err.max(), off.sum(), off.size,
             np.abs(bits.astype(np.int64) - want.view(np.uint16).astype(np.int64)).max()))
    np.testing.assert_array_equal(bits, want.view(np.uint16))


# ------------------------------------------------------------------ 2. the encoder-only epilogues
def _plan(lib, M, N, K, epi, gemm_ref=0):
    out = (C.c_int32 * 4)()
    _lib.check(lib.wdr_dbg_gemm_plan(0, M, N, K, epi, N, 0, gemm_ref, None, out))
    return out[0]


PROJ_CASES = [(4, 4500, 256, 384, "k_gemm4"), (4, 3000, 256, 384, "k_gemm2"), (4, 4500, 128, 384, "k_gemm2"),
              (6, 4500, 512, 128, "k_gemm4"), (6, 4500, 4096, 64, "k_gemm5"), (6, 3000, 384, 128, "k_gemm2"),
              (6, 1500, 16384, 64, "k_gemm4")]


@pytest.mark.parametrize("epi,M,N,K,kernel", PROJ_CASES)
def test_proj_enc(lib, epi, M, N, K, kernel):
    """EPI_F32_GELU_POS (pos_rows 1500: windows 1 and above wrap) and EPI_XKV (window w -> slot w) on
    the kernel the dispatch rule names: bit-identical to the reference tile k_gemm, within the f32 /
    f16 bound of the fp64 result, and the slot images' sentinel intact outside the N * 1500 written
    elements of every slot."""
    assert _plan(lib, M, N, K, epi) == KERNELS[kernel]
    assert _plan(lib, M, N, K, epi, 1) == KERNELS["k_gemm"]
    rng = np.random.default_rng(epi * 100000 + M + N + K)
    a = rng.standard_normal((M, K)).astype(np.float16)
    w = (rng.standard_normal((N, K)) * 0.05).astype(np.float16)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    y = a.astype(np.float64) @ w.astype(np.float64).T + bias
    if epi == 4:
        pos = rng.standard_normal((1500, N)).astype(np.float32)
        got = wdr.dbg_proj_enc(a, w, bias, 4, pos=pos)
        ref_tile = wdr.dbg_proj_enc(a, w, bias, 4, pos=pos, gemm_ref=True)
        np.testing.assert_array_equal(got.view(np.uint32), ref_tile.view(np.uint32))
        assert np.isfinite(got).all()                             # no element left at the sentinel
        want = ec.gelu(y) + pos.astype(np.float64)[np.arange(M) % 1500]
        print("proj_enc epi 4 %dx%dx%d: max err %.3g" % (M, N, K, np.abs(got - want).max()))
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-4)
        return
    slot = N * 1500 + 4096
    img = wdr.dbg_proj_enc(a, w, bias, 6, slot_elems=slot)
    ref_tile = wdr.dbg_proj_enc(a, w, bias, 6, slot_elems=slot, gemm_ref=True)
    assert img.shape == (M // 1500, slot)
    bits = img.view(np.uint16)
    np.testing.assert_array_equal(bits, ref_tile.view(np.uint16))
    assert (bits[:, N * 1500:] == wdr.SENTINEL_F16).all()         # nothing strays past the slot's image
    assert not np.isnan(img[:, :N * 1500]).any()                  # and every element of it is written
    for wdw in range(M // 1500):
        got = ec.slot_unpack(img[wdw], 1, N // 128).astype(np.float64)
        np.testing.assert_allclose(got, y[wdw * 1500:(wdw + 1) * 1500], rtol=2e-3, atol=2e-3)


# ------------------------------------------------------------------ 3. the batched attention launch
@pytest.mark.parametrize("nb,T,H", [(3, 1500, 2), (2, 100, 1)])
def test_attn_batch(lib, nb, T, H):
    """launch_flash_attn with the encoder's arguments (interleaved ld = 3d rows, per-window strides,
    n_batch = nb): every window within the flash bound of the fp64 attention of ITS rows, and bit for
    bit the one-window launch on that window's de-interleaved Q / K / V."""
    rng = np.random.default_rng(nb * 10000 + T + H)
    d = 64 * H
    qkv = rng.standard_normal((nb, T, 3 * d)).astype(np.float16)
    got = wdr.dbg_attn_batch(qkv, H)
    ref = ec.attn_batch(qkv, H)
    for w in range(nb):
        err = np.abs(got[w] - ref[w])
        print("attn_batch nb %d T %d window %d: max %.3g mean %.3g" % (nb, T, w, err.max(), err.mean()))
        assert err.max() <= 1e-2 and err.mean() < 1.5e-3, (w, err.max(), err.mean())
        q, k, v = (np.ascontiguousarray(qkv[w, :, i * d:(i + 1) * d]).view(np.uint16) for i in range(3))
        one = np.zeros((T, d), np.float32)
        _lib.check(lib.wdr_dbg_attn(q.ctypes.data_as(U16), k.ctypes.data_as(U16), v.ctypes.data_as(U16), T, T, H, 0,
                                    one.ctypes.data_as(F32)))
        np.testing.assert_array_equal(got[w], one, err_msg="window %d" % w)
    # the windows hold different data: another window's result is far outside the bound
    assert min(np.abs(ref[w] - ref[(w + 1) % nb]).max() for w in range(nb)) > 10 * 1e-2


# ------------------------------------------------------------------ 4. k_layernorm alone
def _ln_case(rng, rows, d, mean=0.3, std=2.0):
    x = np.full((rows, d + 8), 1e6, np.float32)                   # ldx = d + 8; the pad must not be read
    x[:, :d] = mean + std * rng.standard_normal((rows, d))
    g = (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32)
    b = (0.1 * rng.standard_normal(d)).astype(np.float32)
    return x, g, b


def _ln_check(got, want):
    print("layernorm %s: max err %.3g" % (got.shape, np.abs(got - want).max()))
    np.testing.assert_allclose(got, want, rtol=2.0 ** -10, atol=1e-4)


@pytest.mark.parametrize("d", [4, 252, 260, 1280])
@pytest.mark.parametrize("rows", [1, 5, 1501])
def test_layernorm(lib, rows, d):
    """One wave per row, four rows per workgroup: a single float4 (d = 4), a ragged first pass (252),
    one lane into the second pass (260), the widest row (1280); 1, 5 and 1501 rows (a last workgroup
    of one row) -- against the fp64 LayerNorm within one f16 ulp."""
    x, g, b = _ln_case(np.random.default_rng(rows * 10000 + d), rows, d)
    _ln_check(wdr.dbg_layernorm(x, g, b, d=d), ec.layernorm(x[:, :d], g, b))


def test_layernorm_large_mean(lib):
    """x = 100 + N(0, 1): the variance must come from (x - mean)^2, not E[x^2] - mean^2."""
    x, g, b = _ln_case(np.random.default_rng(77), 5, 1280, mean=100.0, std=1.0)
    _ln_check(wdr.dbg_layernorm(x, g, b, d=1280), ec.layernorm(x[:, :1280], g, b))


def test_layernorm_row_map(lib):
    """launch_layernorm_rows: output row r from input row row_map[r] (here reversed)."""
    x, g, b = _ln_case(np.random.default_rng(78), 1501, 260)
    rm = np.arange(1501)[::-1]
    got = wdr.dbg_layernorm(x, g, b, d=260, row_map=rm)
    _ln_check(got, ec.layernorm(x[:, :260], g, b, rm))
    np.testing.assert_array_equal(got, wdr.dbg_layernorm(x, g, b, d=260)[::-1])


# ------------------------------------------------------------------ 5 / 6. whole encode-ahead batches
# four clips of different fill: 3 s, 12 s, 29.9 s and 30 s (first sample, samples)
CLIPS = [(0, 3 * 16000), (5 * 16000, 12 * 16000), (8 * 16000, 478400), (10 * 16000, 480000)]


def _singles(ctx, pcm):
    """Every clip through the single-window path log_mel_window -> encode -> cross_kv, once."""
    out = []
    for a, n in CLIPS:
        win = ctx.log_mel_window(pcm_i16_to_f32(pcm[a:a + n]), 0)
        enc = ctx.encode(win)
        out.append((win, enc, ctx.cross_kv()))
    return out


def _encode_batch(ctx, pcm, nb):
    """Window w of an nb-window batch holds clip (w + nb) % 4, so every batch size starts on another
    clip: (the clip index per window, encoder output, cross K/V)."""
    order = [(w + nb) % 4 for w in range(nb)]
    enc, xkv = ctx.encode_batch([pcm[CLIPS[i][0]:CLIPS[i][0] + CLIPS[i][1]] for i in order])
    return order, enc, xkv


def _assert_equals_singles(what, order, enc, xkv, singles):
    for w, i in enumerate(order):
        _, enc1, xkv1 = singles[i]
        print("%s nb %d window %d (clip %d) against its single-window encode: max |d| %.3g encoder, %.3g cross K/V"
              % (what, len(order), w, i, np.abs(enc[w] - enc1).max(), np.abs(xkv[w] - xkv1).max()))
    for w, i in enumerate(order):
        _, enc1, xkv1 = singles[i]
        np.testing.assert_array_equal(enc[w], enc1, err_msg="encoder output, window %d (clip %d)" % (w, i))
        np.testing.assert_array_equal(xkv[w], xkv1, err_msg="cross K/V, window %d (clip %d)" % (w, i))


@pytest.fixture(scope="module")
def tiny_singles(model, pcm):
    name, ctx, hp, W = model
    singles = _singles(ctx, pcm)
    m = Whisper(hp, W)
    return singles, [m.encode(win) for win, _, _ in singles]


@pytest.mark.parametrize("nb", [1, 2, 3, 4])
def test_encode_batch(model, pcm, tiny_singles, nb):
    """A batch of nb windows (clips of different length, so of different fill) through the production
    front end and the batched encoder: every window bit-identical to the single-window path of its
    clip -- "encoder results do not depend on the batch" -- and within the encoder's oracle bounds.

    The single-window reference builds conv1's operand on the host from log_mel_window, the batch
    with k_im2col_mel: the identity also rests on the two giving the same bits (test_im2col_mel)."""
    name, ctx, hp, W = model
    singles, oracle = tiny_singles
    order, enc, xkv = _encode_batch(ctx, pcm, nb)
    for w, i in enumerate(order):
        err = np.abs(enc[w] - oracle[i])
        print("encode_batch %s nb %d window %d (clip %d): max %.3g mean %.3g" % (name, nb, w, i, err.max(), err.mean()))
        assert err.max() < 5e-2 and err.mean() < 4e-3, (w, i, err.max(), err.mean())
    assert np.abs(oracle[0] - oracle[3]).mean() > 10 * 4e-3       # the clips' outputs differ
    _assert_equals_singles("encode_batch " + name, order, enc, xkv, singles)


@pytest.fixture(scope="module")
def base_en(pcm):
    ctx, hp, W = _context("base.en")
    yield ctx, _singles(ctx, pcm)
    ctx.close()


@pytest.mark.parametrize("nb", [3, 4])
def test_encode_batch_base_en(base_en, pcm, nb):
    """base.en's production shapes (d = 512, M = 4500 / 6000: the ping-pong tile kernels on every
    projection, N = 6144 cross-K/V into the slots): bit-identical to the single-window path."""
    ctx, singles = base_en
    order, enc, xkv = _encode_batch(ctx, pcm, nb)
    _assert_equals_singles("encode_batch base.en", order, enc, xkv, singles)
