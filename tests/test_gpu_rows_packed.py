"""The decoder row projections on weights stored in MFMA fragment order (ProjArgs::b_packed,
csrc/kernels/gemm.hip k_skinny PK / k_pack_rows): the packed kernel loads the same values into the
same registers in the same k order as the row-major one, so every result must be equal BIT FOR BIT
(np.array_equal on the raw outputs, no tolerance) -- every tiling the dispatch picks, every
epilogue, the fused LayerNorm prologue and the row map; the packer against the layout formula; and
a whole tiny-model decode with WDR_ROWS_PACKED=0 (all weights row-major) against the default."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import wdr
from wdr import _lib

pytestmark = pytest.mark.gpu

U16 = C.POINTER(C.c_uint16)
F32 = C.POINTER(C.c_float)

ROWS = 0x200      # include/wdr.h WDR_DBG_PROJ_ROWS
PACKED = 0x1000   # include/wdr.h WDR_DBG_PROJ_PACKED
EPI_F16, EPI_F16_GELU, EPI_F32_RESID, EPI_F32 = 0, 1, 2, 3

# rows: MT = 1; two row tiles; the paired tiles above 32 rows; mt = 4 (the K > 2048 pairing); mt = 5
MS = (1, 17, 33, 49, 65)
# N x K: three strips, two k-steps | N % 16 != 0, the pad strip | K > 2048: 16 waves, ragged last
# k batch | wide N, 32 columns per workgroup, an odd strip count | the real d
SHAPES = [(48, 64), (40, 64), (32, 2080), (4112, 64), (1280, 1280)]


def _bits(a):
    return np.ascontiguousarray(a.astype(np.float16)).view(np.uint16)


def _proj(lib, a, w, bias, epi, out0=None):
    M, K = a.shape
    N = w.shape[0]
    out = np.zeros((M, N), np.float32) if out0 is None else out0.copy()
    ab, wb = _bits(a), _bits(w)
    _lib.check(lib.wdr_dbg_proj(ab.ctypes.data_as(U16), wb.ctypes.data_as(U16), bias.ctypes.data_as(F32), M, N, K, epi,
                                out.ctypes.data_as(F32)))
    return out


def _inputs(N, K, seed, mx=max(MS)):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((mx, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    base = rng.standard_normal((mx, N)).astype(np.float32)
    return a, w, bias, base


@pytest.mark.parametrize("N,K", SHAPES)
def test_packed_equals_row_major(lib, N, K):
    """wdr_dbg_proj on the row kernel: f16, f16 + GELU, f32 residual and f32 epilogues."""
    a, w, bias, base = _inputs(N, K, N * 7 + K)
    for M in MS:
        for epi in (EPI_F16, EPI_F16_GELU, EPI_F32_RESID, EPI_F32):
            o0 = base[:M] if epi == EPI_F32_RESID else None
            row = _proj(lib, a[:M], w, bias, epi | ROWS, o0)
            pk = _proj(lib, a[:M], w, bias, epi | ROWS | PACKED, o0)
            assert np.isfinite(row).all() and np.abs(row).max() > 0
            assert np.array_equal(row.view(np.uint32), pk.view(np.uint32)), (N, K, M, epi)


@pytest.mark.parametrize("d,K", [(64, 64), (1280, 1280)])
def test_packed_qkv_cache_epilogue(d, K):
    """EPI_QKV_CACHE: Q rows and the K / V rows scattered into the caches."""
    a, w, bias, _ = _inputs(3 * d, K, d + 1)
    rng = np.random.default_rng(d)
    n_seq, T = 2, 64
    kc = rng.standard_normal((n_seq, T, d)).astype(np.float16)
    vc = rng.standard_normal((n_seq, T, d)).astype(np.float16)
    for M in MS:
        seq, pos = np.arange(M) % n_seq, np.arange(M) // n_seq
        q0, k0, v0 = wdr.dbg_proj_qkv(a[:M], w, bias, seq, pos, kc, vc)
        q1, k1, v1 = wdr.dbg_proj_qkv(a[:M], w, bias, seq, pos, kc, vc, packed=True)
        assert not np.array_equal(k0.view(np.uint16), kc.view(np.uint16))
        assert np.array_equal(q0.view(np.uint32), q1.view(np.uint32)), M
        assert np.array_equal(k0.view(np.uint16), k1.view(np.uint16)), M
        assert np.array_equal(v0.view(np.uint16), v1.view(np.uint16)), M


def _proj_ln(lib, x, g, b, w, bias, epi, flags):
    M, K = x.shape
    N = w.shape[0]
    out = np.zeros((M, N), np.float32)
    wb = _bits(w)
    _lib.check(lib.wdr_dbg_proj_ln(x.ctypes.data_as(F32), g.ctypes.data_as(F32), b.ctypes.data_as(F32),
                                   wb.ctypes.data_as(U16), bias.ctypes.data_as(F32), M, N, K, epi, flags,
                                   out.ctypes.data_as(F32)))
    return out


FUSED, LN_PACKED, ROW_MAP = 1, 2, 4   # include/wdr.h wdr_dbg_proj_ln `fused` bits


@pytest.mark.parametrize("N,K", [(48, 128), (40, 128), (4112, 128), (1280, 1280)])
def test_packed_ln_prologue_and_row_map(lib, N, K):
    """The fused LayerNorm prologue (narrow 16-row and wide 32-row tiles) and EPI_F32 with the row
    map, on the fused rows and on separately normalised rows."""
    rng = np.random.default_rng(N + K)
    x = np.ascontiguousarray((rng.standard_normal((max(MS), K)) * 2.0 + 0.3).astype(np.float32))
    g = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    b = (0.1 * rng.standard_normal(K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) * 0.03).astype(np.float32)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    for M in MS:
        xm = np.ascontiguousarray(x[:M])
        for epi, flags in ((EPI_F16, FUSED), (EPI_F16_GELU, FUSED), (EPI_F32, FUSED | ROW_MAP), (EPI_F32, ROW_MAP)):
            row = _proj_ln(lib, xm, g, b, w, bias, epi, flags)
            pk = _proj_ln(lib, xm, g, b, w, bias, epi, flags | LN_PACKED)
            assert np.isfinite(row).all() and np.abs(row).max() > 0
            assert np.array_equal(row.view(np.uint32), pk.view(np.uint32)), (N, K, M, epi, flags)
        if M > 1:   # the map is live: row m comes from x row M - 1 - m
            plain = _proj_ln(lib, xm, g, b, w, bias, EPI_F32, FUSED)
            mapped = _proj_ln(lib, xm, g, b, w, bias, EPI_F32, FUSED | ROW_MAP)
            assert np.array_equal(mapped, plain[::-1])


def _packed_index(N, K):
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    tile = (n >> 4) * (K // 32) + (k >> 5)
    return tile * 512 + (((k >> 3) & 3) * 16 + (n & 15)) * 8 + (k & 7)


@pytest.mark.parametrize("N,K", [(48, 64), (40, 64), (1280, 1280)])
def test_packer_round_trip(lib, N, K):
    """k_pack_rows against the layout formula: element (n, k) carries the bit pattern n K + k (every
    element distinct at 48 x 64 and 40 x 64; modulo a prime at 1280 x 1280), the pad rows are zero."""
    w = ((np.arange(N * K, dtype=np.int64) % 65521) + 1).astype(np.uint16).reshape(N, K)
    NP = (N + 15) // 16 * 16
    out = np.full(NP * K, 0xFFFF, np.uint16)
    _lib.check(lib.wdr_dbg_pack_rows(w.ctypes.data_as(U16), N, K, out.ctypes.data_as(U16)))
    want = np.zeros(NP * K, np.uint16)
    want[_packed_index(N, K).ravel()] = w.ravel()
    assert np.array_equal(out, want)
    if NP > N:
        pad = _packed_index(NP, K)[N:].ravel()
        assert pad.size == (NP - N) * K and not out[pad].any()


_CHILD = r"""
import hashlib, json, sys
import numpy as np
sys.path[:0] = [%(root)r, %(pkg)r]
import wdr
g = np.load(%(npz)r)
ctx = wdr.WhisperContext("tiny-test", synthetic=wdr.Synthetic(weight_std=0.02, emb_std=0.5))
ctx.encode(np.ascontiguousarray(g["mel"], np.float32))
toks = [int(t) for t in g["tokens"]]
h = hashlib.sha256()
pre = ctx.decode(toks)
h.update(np.ascontiguousarray(pre).tobytes())
for _ in range(6):
    lg = ctx.step(toks)
    h.update(np.ascontiguousarray(lg).tobytes())
    toks.append(int(np.argmax(lg)))
ctx.close()
print("RESULT " + json.dumps({"tokens": toks, "sha": h.hexdigest(), "finite": bool(np.isfinite(pre).all())}))
"""


def test_row_major_switch_same_decode(tmp_path):
    """WDR_ROWS_PACKED=0 keeps every decoder weight row-major (the former behaviour): a tiny-model
    prefill and six greedy steps on the golden mel / prompt give the same tokens and the same logits
    bytes as the default packed load.  A fresh child process per setting (the switch is read at load)."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    script = tmp_path / "decode_child.py"
    script.write_text(_CHILD % {"root": root, "pkg": os.path.join(root, "whisper-diarize-rs_amd"),
                                "npz": os.path.join(here, "golden", "whisper_tiny.npz")})
    res = []
    for setting in (None, "0"):
        env = dict(os.environ)
        env.pop("WDR_ROWS_PACKED", None)
        if setting is not None:
            env["WDR_ROWS_PACKED"] = setting
        p = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        res.append(json.loads(line[len("RESULT "):]))
    assert res[0]["finite"] and len(res[0]["tokens"]) == 11
    assert res[0]["tokens"] == res[1]["tokens"]
    assert res[0]["sha"] == res[1]["sha"]
