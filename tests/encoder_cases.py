"""Plain numpy fp64 references of the encoder's front-end and batched kernels (the GPU side:
tests/test_gpu_encoder_kernels.py; their own checks against the oracle: tests/test_encoder_cases.py).

Every function restates its operation from the definition, for nb windows stacked along the rows
the way the encode-ahead batch stacks them (row b * T + t), and shares no code with the library or
with oracle/model.py:

  * conv1 / conv2 as im2col + product (column 3 ci + k, tap u = stride t + k - 1, zero padding);
  * conv2's epilogue: gelu + the positional row of the window-local index (row % 1500);
  * batched non-causal attention on interleaved Q / K / V rows;
  * LayerNorm (eps 1e-5, biased variance), optionally gathering rows;
  * the cross-K/V slot layout of csrc/common.h: head-major [L][2][H][1500][64] per window.
"""
import numpy as np

T_AUDIO = 1500          # encoder positions per 30-s window
T_MEL = 3000            # log-mel frames per window
SLOT_BLOCK = T_AUDIO * 64


def f16(x):
    return np.asarray(x).astype(np.float16).astype(np.float64)


def gelu(x):
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + np.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


# ------------------------------------------------------------------ im2col (k = 3, pad 1)
def im2col_conv1(win, kp=None):
    """win [n_mels][3000] -> [3000][kp]: column 3 ci + k of row t = win[ci][t + k - 1], 0 where the
    tap leaves the window; columns [3 n_mels, kp) zero (kp defaults to 3 n_mels)."""
    win = np.asarray(win, np.float64)
    C, T = win.shape
    kp = 3 * C if kp is None else kp
    out = np.zeros((T, kp))
    for k in range(3):
        u = np.arange(T) + k - 1
        ok = (u >= 0) & (u < T)
        out[ok, k:3 * C:3] = win[:, u[ok]].T
    return out


def im2col_conv2(x, nb=1):
    """x [nb * 3000][d] (nb windows stacked) -> [nb * 1500][3 d]: row b * 1500 + t, column 3 ci + k
    = x[b * 3000 + 2 t + k - 1][ci], 0 where 2 t + k - 1 leaves window b."""
    x = np.asarray(x, np.float64)
    d = x.shape[1]
    assert x.shape[0] == nb * T_MEL
    out = np.zeros((nb * T_AUDIO, 3 * d))
    for b in range(nb):
        xb = x[b * T_MEL:(b + 1) * T_MEL]
        for k in range(3):
            u = 2 * np.arange(T_AUDIO) + k - 1
            ok = (u >= 0) & (u < T_MEL)
            out[b * T_AUDIO + np.nonzero(ok)[0], k::3] = xb[u[ok]]
    return out


def conv_w(w):
    """conv weight [out][in][3] -> the GEMM's [out][3 in] (column 3 ci + k)."""
    return np.asarray(w, np.float64).reshape(w.shape[0], -1)


# ------------------------------------------------------------------ GEMM epilogues
def proj_gelu_pos(a, w, bias, pos):
    """EPI_F32_GELU_POS: gelu(a w^T + bias) + pos[row % pos_rows] (a [M][K], w [N][K], pos [pos_rows][N])."""
    a, w, pos = (np.asarray(v, np.float64) for v in (a, w, pos))
    y = a @ w.T
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    return gelu(y) + pos[np.arange(a.shape[0]) % pos.shape[0]]


def slot_pack(kv, n_layer, n_head):
    """One window's cross K/V, kv [1500][n_layer * 2 * 64 n_head] (column = (layer, K|V, head, dim)
    in that order) -> its slot image: head-major [n_layer][2][n_head][1500][64], flattened."""
    kv = np.asarray(kv)
    assert kv.shape == (T_AUDIO, n_layer * 2 * n_head * 64)
    return kv.reshape(T_AUDIO, n_layer, 2, n_head, 64).transpose(1, 2, 3, 0, 4).reshape(-1)


def slot_unpack(img, n_layer, n_head):
    """The inverse of slot_pack on the first n_layer * 2 * n_head * 1500 * 64 elements of a slot image."""
    n = n_layer * 2 * n_head * SLOT_BLOCK
    img = np.asarray(img).reshape(-1)[:n]
    return img.reshape(n_layer, 2, n_head, T_AUDIO, 64).transpose(3, 0, 1, 2, 4).reshape(T_AUDIO, -1)


def slot_k_index(l, h, t, j, n_head):
    """common.h: layer l, head h: K at (2 l) n_head HS + h HS, V one n_head HS further; key stride 64."""
    return (2 * l * n_head + h) * SLOT_BLOCK + t * 64 + j


# ------------------------------------------------------------------ attention / LayerNorm
def attn_batch(qkv, n_head):
    """qkv [nb][T][3 * 64 H] (Q | K | V per row) -> [nb][T][64 H]: softmax(Q K^T / 8) V per window and
    head, non-causal."""
    qkv = np.asarray(qkv, np.float64)
    nb, T, w = qkv.shape
    d = 64 * n_head
    assert w == 3 * d
    out = np.zeros((nb, T, d))
    for b in range(nb):
        q, k, v = qkv[b, :, :d], qkv[b, :, d:2 * d], qkv[b, :, 2 * d:]
        for h in range(n_head):
            c = slice(64 * h, 64 * (h + 1))
            s = q[:, c] @ k[:, c].T / 8.0
            p = np.exp(s - s.max(1, keepdims=True))
            out[b, :, c] = (p / p.sum(1, keepdims=True)) @ v[:, c]
    return out


def layernorm(x, g, b, row_map=None, eps=1e-5):
    """x [rows][d] -> (x - mean) / sqrt(var + eps) * g + b per row (biased variance); row_map:
    output row r from x row row_map[r]."""
    x = np.asarray(x, np.float64)
    if row_map is not None:
        x = x[np.asarray(row_map)]
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


# ------------------------------------------------------------------ the batched encoder from the parts
def encode_batch(hp, W, mels, pos_rows=T_AUDIO):
    """nb log-mel windows [nb][n_mels][3000] through the encoder as the batch runs it -- every stage
    over the stacked rows, with the rounding points of the ggml graph (f16 matmul operands, f16 Q /
    K / V, probabilities and cross K/V; f32-like residual stream kept in fp64) -- from the references
    above.  Returns (encoder output [nb][1500][d], slot images [nb][L * 2 * d * 1500]).
    pos_rows: the wrap of the positional rows (1500; anything else models a defect)."""
    nb = len(mels)
    d, H = hp.n_audio_state, hp.n_audio_head
    lin = lambda x, w, b: f16(x) @ np.asarray(w, np.float64).T + (0.0 if b is None else np.asarray(b, np.float64))
    a1 = np.concatenate([im2col_conv1(f16(m)) for m in mels])
    c1 = gelu(a1 @ conv_w(W["encoder.conv1.weight"]).T + W["encoder.conv1.bias"])
    a2 = im2col_conv2(f16(c1), nb)
    pos = np.asarray(W["encoder.positional_embedding"], np.float64)
    rows = np.arange(nb * T_AUDIO)
    x = gelu(a2 @ conv_w(W["encoder.conv2.weight"]).T + W["encoder.conv2.bias"]) + pos[rows % pos_rows if pos_rows else 0 * rows]
    for i in range(hp.n_audio_layer):
        p = "encoder.blocks.%d." % i
        h = layernorm(x, W[p + "attn_ln.weight"], W[p + "attn_ln.bias"])
        qkv = np.concatenate([lin(h, W[p + "attn.query.weight"], W[p + "attn.query.bias"]),
                              lin(h, W[p + "attn.key.weight"], None),
                              lin(h, W[p + "attn.value.weight"], W[p + "attn.value.bias"])], axis=1)
        a = attn_batch(f16(qkv).reshape(nb, T_AUDIO, 3 * d), H).reshape(nb * T_AUDIO, d)
        x = x + lin(a, W[p + "attn.out.weight"], W[p + "attn.out.bias"])
        h = layernorm(x, W[p + "mlp_ln.weight"], W[p + "mlp_ln.bias"])
        h = gelu(lin(h, W[p + "mlp.0.weight"], W[p + "mlp.0.bias"]))
        x = x + lin(h, W[p + "mlp.2.weight"], W[p + "mlp.2.bias"])
    enc = layernorm(x, W["encoder.ln_post.weight"], W["encoder.ln_post.bias"])
    cols = []
    for l in range(hp.n_text_layer):
        p = "decoder.blocks.%d.cross_attn." % l
        cols += [lin(enc, W[p + "key.weight"], None), lin(enc, W[p + "value.weight"], W[p + "value.bias"])]
    kv = f16(np.concatenate(cols, axis=1)).reshape(nb, T_AUDIO, -1)
    slots = np.stack([slot_pack(kv[b], hp.n_text_layer, hp.n_text_head) for b in range(nb)])
    return enc.reshape(nb, T_AUDIO, d), slots
