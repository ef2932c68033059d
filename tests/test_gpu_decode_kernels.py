"""The decode-step kernels against plain fp64 references (tests/decode_cases.py, checked on the CPU
by tests/test_decode_cases.py): KV-cache self-attention (k_dec_self_attn), the QKV projection's
cache-scatter epilogue, the beam top-K (k_logits_topk / k_logits_topk_final), the sampling
distribution (k_logits_probs), the beam reorder of the KV cache (State::kv_reorder / k_kv_copy)
and LayerNorm at every model width.  Every seam checks its arguments on the host; no case here is
out of range.  Each test prints the largest error it measured before it asserts."""
import ctypes as C

import numpy as np
import pytest

import wdr
from oracle.vocab import Vocab
from tests import decode_cases as dc
from wdr import _lib

pytestmark = pytest.mark.gpu

U16 = C.POINTER(C.c_uint16)
F32 = C.POINTER(C.c_float)
ROWS = 0x200   # include/wdr.h WDR_DBG_PROJ_ROWS


def _attn(case, rows=None):
    sel = slice(None) if rows is None else rows
    return wdr.dbg_self_attn(case["q"][sel], case["kc"], case["vc"], case["row_seq"][sel], case["row_pos"][sel],
                             case["H"])


def _ref(case):
    return dc.self_attn_ref(case["q"], case["kc"], case["vc"], case["row_seq"], case["row_pos"], case["H"])


def _check_attn(name, got, ref):
    assert np.isfinite(got).all(), name
    err = np.abs(got - ref)
    print("%s: max |err| %.3e, mean %.3e (atol %.3e)" % (name, err.max(), err.mean(), dc.ATTN_ATOL))
    np.testing.assert_allclose(got, ref, rtol=0, atol=dc.ATTN_ATOL, err_msg=name)


# ------------------------------------------------------------------ self-attention
@pytest.mark.parametrize("nk", dc.ONEHOT_NK)
def test_self_attn_key_sweep(lib, nk):
    """One-hot probe, nk rows at pos nk - 1, row j on key j: every P.V loop boundary (16 keys in
    flight, 8, singles), the 64-key score passes and their clamped tail, the full 448-score array.
    A missing, doubled or shifted key is an O(1) error here (test_onehot_probe_is_onehot)."""
    case = dc.onehot_probe(nk)
    _check_attn("one-hot nk=%d" % nk, _attn(case), _ref(case))


@pytest.mark.parametrize("H", [2, 6, 20])
def test_self_attn_random_rows(lib, H):
    """40 rows over 5 sequences, random (seq, pos) with repeats, pos 0 and 447."""
    case = dc.random_rows_case(H)
    got = _attn(case)
    _check_attn("random rows H=%d" % H, got, _ref(case))
    seq, pos = case["row_seq"], case["row_pos"]
    twins = [(a, b) for a in range(len(seq)) for b in range(a) if seq[a] == seq[b] and pos[a] == pos[b]]
    assert twins
    # batch independence: a row alone, a row among a few others, bit for bit
    for r in (0, 1, 7, 20, 39):
        np.testing.assert_array_equal(_attn(case, slice(r, r + 1)), got[r:r + 1], err_msg="row %d alone" % r)
    np.testing.assert_array_equal(_attn(case, slice(5, 22)), got[5:22])
    back = np.arange(len(seq))[::-1].copy()
    np.testing.assert_array_equal(_attn(case, back), got[back])


def test_self_attn_reads_no_row_beyond(lib):
    """One row per sequence; every cache row from nk on is NaN in K and V: a read past the row's
    keys (an unclamped score pass, a P.V loop one group too far) shows as a NaN."""
    case = dc.read_beyond_case()
    _check_attn("read-beyond", _attn(case), _ref(case))


@pytest.mark.parametrize("n", [8, 37])
def test_self_attn_prefill_shape(lib, n):
    """Rows 0 .. n - 1 of one sequence at pos = row, as a prompt prefill launches them: causal by
    position, random and one-hot (row i on its own, last key)."""
    case = dc.prefill_case(n)
    _check_attn("prefill n=%d" % n, _attn(case), _ref(case))
    hot = dc.onehot_probe(n, prefill=True)
    _check_attn("prefill one-hot n=%d" % n, _attn(hot), _ref(hot))


# ------------------------------------------------------------------ QKV projection, cache epilogue
def _proj(lib, a, w, bias, epi):
    M, K = a.shape
    N = w.shape[0]
    out = np.zeros((M, N), np.float32)
    ab, wb = (np.ascontiguousarray(x.astype(np.float16)).view(np.uint16) for x in (a, w))
    _lib.check(lib.wdr_dbg_proj(ab.ctypes.data_as(U16), wb.ctypes.data_as(U16), bias.ctypes.data_as(F32), M, N, K, epi,
                                out.ctypes.data_as(F32)))
    return out


@pytest.mark.parametrize("M,d,K", [(1, 128, 128), (5, 128, 128), (17, 384, 384), (64, 128, 128), (65, 128, 128),
                                   (33, 1280, 1280)])
def test_qkv_cache_epilogue(lib, M, d, K):
    """The fused Q/K/V row projection scatters K / V into cache rows (row_seq, row_pos): distinct
    shuffled rows of 3 sequences x 32 positions over a sentinel pattern.  Q and the written rows
    equal the plain f16 row projection's columns bit for bit; nothing else in the caches changes."""
    rng = np.random.default_rng([M, d, K])
    n_seq, T = 3, 32
    a = rng.standard_normal((M, K)).astype(np.float16)
    w = (rng.standard_normal((3 * d, K)) * 0.05).astype(np.float16)
    bias = (rng.standard_normal(3 * d) * 0.1).astype(np.float32)
    cell = rng.permutation(n_seq * T)[:M]
    seq, pos = (cell // T).astype(np.int32), (cell % T).astype(np.int32)
    kc0 = rng.integers(0, 0x7C00, (n_seq, T, d), dtype=np.uint16)
    vc0 = rng.integers(0, 0x7C00, (n_seq, T, d), dtype=np.uint16)
    q, kc, vc = wdr.dbg_proj_qkv(a, w, bias, seq, pos, kc0.view(np.float16), vc0.view(np.float16))
    plain = _proj(lib, a, w, bias, 0 | ROWS).astype(np.float16)
    np.testing.assert_array_equal(q.astype(np.float16).view(np.uint16), plain[:, :d].view(np.uint16))
    np.testing.assert_array_equal(q, plain[:, :d].astype(np.float32))
    want_k, want_v = kc0.copy(), vc0.copy()
    want_k[seq, pos] = plain[:, d:2 * d].view(np.uint16)
    want_v[seq, pos] = plain[:, 2 * d:].view(np.uint16)
    np.testing.assert_array_equal(kc.view(np.uint16), want_k)
    np.testing.assert_array_equal(vc.view(np.uint16), want_v)
    # the plain projection itself against the fp64 product (f16 output rounding)
    ref = a.astype(np.float64) @ w.T.astype(np.float64) + bias
    np.testing.assert_allclose(plain.astype(np.float64), ref, rtol=2e-3, atol=2e-3)


# ------------------------------------------------------------------ beam top-K, sampling distribution
@pytest.fixture(scope="module", params=sorted(dc.MODELS))
def rule_ctx(request):
    v = Vocab(dc.MODELS[request.param])
    ctx = wdr.WhisperContext(request.param, synthetic=wdr.Synthetic())
    yield v, dc.topk_cases(v), ctx
    ctx.close()


def _chunks(cases):
    for i in range(0, len(cases), 8):   # up to 8 rows per call, each row its own rule state
        yield cases[i:i + 8]


def _rules(ctx, fn, v, cs, temps, *a):
    return fn(np.stack([c["x"] for c in cs]), [dc.rule_state(v, c) for c in cs], *a, temps=temps,
              max_initial_ts=dc.MAX_INITIAL_TS, suppress_blank=dc.SUPPRESS_BLANK)


@pytest.mark.parametrize("K", dc.TOPK_KS)
def test_beam_topk(rule_ctx, K):
    """ids and order identical to the oracle's top-K (ties by lower id across threads, waves and
    slices; absent candidates -1 / 0 / -inf), log p within 2e-3 of the fp64 log-softmax, p = exp."""
    v, cases, ctx = rule_ctx
    worst_lp = worst_p = 0.0
    for cs in _chunks(cases):
        temps = [c["temp"] for c in cs]
        ids, p, lp = _rules(ctx, ctx.logits_topk, v, cs, temps, K)
        greedy = _rules(ctx, ctx.logit_rules, v, cs, temps) if K == 1 else None
        for r, c in enumerate(cs):
            st, _, lps, _ = dc.oracle_logits(v, c, c["temp"])
            want = st.topk(lps, K)
            want += [-1] * (K - len(want))
            assert ids[r].tolist() == want, (c["name"], K, ids[r].tolist(), want)
            _, ref = dc.topk_ref(v, c, K)
            for k, i in enumerate(want):
                if i < 0:
                    assert p[r, k] == 0.0 and lp[r, k] == -np.inf, (c["name"], k)
                    continue
                worst_lp = max(worst_lp, abs(lp[r, k] - ref[k]))
                worst_p = max(worst_p, abs(p[r, k] / np.exp(ref[k]) - 1.0))
                assert abs(lp[r, k] - ref[k]) <= dc.LOGP_ATOL, (c["name"], k, lp[r, k], ref[k])
                assert abs(p[r, k] - np.exp(ref[k])) <= dc.LOGP_ATOL * np.exp(ref[k]), (c["name"], k)
            if K == 1:
                assert greedy[r]["id"] == ids[r, 0], (c["name"], greedy[r]["id"], ids[r, 0])
    print("top-%d: max |log p err| %.3e, max rel p err %.3e (bound %.1e)" % (K, worst_lp, worst_p, dc.LOGP_ATOL))


@pytest.mark.parametrize("temp", dc.SAMPLE_TEMPS)
def test_sampling_distribution(rule_ctx, temp):
    """k_logits_probs: 0 / -inf exactly on the oracle's masked set, elsewhere finite and within
    2e-3 of the fp64 log-softmax; rows sum to 1; the argmax is the greedy id."""
    v, cases, ctx = rule_ctx
    worst_lp = worst_p = worst_sum = 0.0
    for cs in _chunks(cases):
        temps = [temp] * len(cs)
        probs, logp = _rules(ctx, ctx.logits_probs, v, cs, temps)
        greedy = _rules(ctx, ctx.logit_rules, v, cs, temps)
        for r, c in enumerate(cs):
            _, lg, _, _ = dc.oracle_logits(v, c, temp)
            masked = lg == -np.inf
            ref = dc.logits_ref(v, c, temp)["logp"]
            assert np.all(probs[r][masked] == 0.0) and np.all(logp[r][masked] == -np.inf), c["name"]
            fin = ~masked
            assert np.isfinite(logp[r][fin]).all() and np.isfinite(probs[r][fin]).all(), c["name"]
            e_lp = np.abs(logp[r][fin] - ref[fin]).max()
            e_p = np.abs(probs[r][fin] / np.exp(ref[fin]) - 1.0).max()
            e_sum = abs(float(probs[r].astype(np.float64).sum()) - 1.0)
            worst_lp, worst_p, worst_sum = max(worst_lp, e_lp), max(worst_p, e_p), max(worst_sum, e_sum)
            assert e_lp <= dc.LOGP_ATOL, (c["name"], e_lp)
            assert e_p <= dc.LOGP_ATOL, (c["name"], e_p)
            assert e_sum <= 2e-3, (c["name"], e_sum)
            assert int(np.argmax(probs[r])) == greedy[r]["id"], c["name"]
    print("sampling t=%.1f: max |log p err| %.3e, max rel p err %.3e, max |sum - 1| %.3e"
          % (temp, worst_lp, worst_p, worst_sum))


# ------------------------------------------------------------------ KV reorder
@pytest.fixture(scope="module", params=["tiny-test", "base.en"])
def kv_ctx(request):
    ctx = wdr.WhisperContext(request.param, synthetic=wdr.Synthetic())
    h = ctx.hparams
    assert h["n_text_ctx"] == dc.T_CTX
    k, v = dc.kv_pattern(h["n_text_layer"], h["n_text_state"])
    yield ctx, k, v
    ctx.close()


def _read_all(ctx):
    rows = [ctx.kv_rows(s, dc.T_CTX) for s in range(dc.NSEQ)]
    return (np.stack([r[i].view(np.uint16) for r in rows]) for i in (0, 1))


@pytest.mark.parametrize("moves", sorted(dc.MOVE_SETS))
def test_kv_reorder(kv_ctx, moves):
    """State::kv_reorder (two k_kv_copy phases through scratch sequences; the grid-stride copy
    capped at 64 blocks): a swap, a 3-cycle, a fan-out and a full 8-permutation at 1 .. 448 rows.
    Every layer, bit for bit: moved rows, the destination's rows past n_rows and every sequence
    that is no destination."""
    ctx, k0, v0 = kv_ctx
    for n_rows in dc.REORDER_ROWS:
        for s in range(dc.NSEQ):
            ctx.set_kv_rows(s, k0[s].view(np.float16), v0[s].view(np.float16))
        ctx.kv_reorder(dc.MOVE_SETS[moves], n_rows)
        k, v = _read_all(ctx)
        np.testing.assert_array_equal(k, dc.reorder_ref(k0, dc.MOVE_SETS[moves], n_rows), err_msg="K n_rows=%d" % n_rows)
        np.testing.assert_array_equal(v, dc.reorder_ref(v0, dc.MOVE_SETS[moves], n_rows), err_msg="V n_rows=%d" % n_rows)


def test_kv_rows_roundtrip(kv_ctx):
    ctx, k0, v0 = kv_ctx
    for s in range(dc.NSEQ):
        ctx.set_kv_rows(s, k0[s].view(np.float16), v0[s].view(np.float16))
    k, v = _read_all(ctx)
    np.testing.assert_array_equal(k, k0)
    np.testing.assert_array_equal(v, v0)
    part = ctx.kv_rows(3, 37)[1].view(np.uint16)
    np.testing.assert_array_equal(part, v0[3][:, :37])


# ------------------------------------------------------------------ LayerNorm widths
@pytest.mark.parametrize("K", dc.LN_WIDTHS)
def test_layernorm_widths(lib, K):
    """k_layernorm and the row kernel's fused LayerNorm prologue at every model width (tiny 384,
    base 512, small 768, medium 1024, large 1280, the test models' 128): an identity projection
    (f32 out) returns the f16 LayerNorm row exactly.  Against the fp64 LayerNorm within the f16
    rounding of the result; fused and split bit-equal."""
    x, g, b = dc.layernorm_case(K)
    eye = np.ascontiguousarray(np.eye(K, dtype=np.float16)).view(np.uint16)
    zero = np.zeros(K, np.float32)
    worst = 0.0
    for M in dc.LN_ROWS:
        ref = dc.layernorm_ref(x[:M], g, b)
        outs = []
        for fused in (1, 0):
            out = np.zeros((M, K), np.float32)
            xc = np.ascontiguousarray(x[:M])
            _lib.check(lib.wdr_dbg_proj_ln(xc.ctypes.data_as(F32), g.ctypes.data_as(F32), b.ctypes.data_as(F32),
                                           eye.ctypes.data_as(U16), zero.ctypes.data_as(F32), M, K, K, 3, fused,
                                           out.ctypes.data_as(F32)))
            outs.append(out)
        worst = max(worst, float((np.abs(outs[0] - ref) / (dc.LN_ATOL + dc.LN_RTOL * np.abs(ref))).max()))
        np.testing.assert_array_equal(outs[0], outs[1], err_msg="M=%d fused != split" % M)
        np.testing.assert_array_equal(outs[0], outs[0].astype(np.float16).astype(np.float32))   # f16 rows
        np.testing.assert_allclose(outs[0], ref, rtol=dc.LN_RTOL, atol=dc.LN_ATOL, err_msg="M=%d" % M)
    print("layernorm d=%d: worst error / bound %.3f (rtol 2^-10, atol 1e-5)" % (K, worst))


# ------------------------------------------------------------------ argument validation (host only)
def test_context_seams_reject_out_of_range_arguments(kv_ctx):
    """Every refusal happens on the host, before any launch (the context-free seams' refusals are
    checked without a GPU in tests/test_decode_cases.py)."""
    ctx, k0, v0 = kv_ctx
    V = ctx.hparams["n_vocab"]
    for K in (0, 9):
        with pytest.raises(wdr.WdrError, match="K out of range"):
            ctx.logits_topk(np.zeros((1, V), np.float32), [{}], K)
    with pytest.raises(wdr.WdrError, match="1..8 rows"):
        ctx.logits_topk(np.zeros((9, V), np.float32), [{}] * 9, 2)
    with pytest.raises(wdr.WdrError, match="1..8 rows"):
        ctx.logits_probs(np.zeros((9, V), np.float32), [{}] * 9)
    for moves, n_rows, msg in (([(0, 1), (2, 1)], 4, "named twice"), ([(0, 8)], 4, "sequence out of range"),
                               ([(-1, 0)], 4, "sequence out of range"), ([(0, 1)], 0, "row count out of range"),
                               ([(0, 1)], dc.T_CTX + 1, "row count out of range"),
                               ([(i, i) for i in range(8)] + [(0, 1)], 4, "1..8 moves")):
        with pytest.raises(wdr.WdrError, match=msg):
            ctx.kv_reorder(moves, n_rows)
    for seq, n, msg in ((8, 4, "sequence out of range"), (-1, 4, "sequence out of range"),
                        (0, 0, "row count out of range"), (0, dc.T_CTX + 1, "row count out of range")):
        with pytest.raises(wdr.WdrError, match=msg):
            ctx.kv_rows(seq, n)
