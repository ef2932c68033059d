"""The decode-step kernel cases (tests/decode_cases.py) are strong enough: the references agree
with the oracle, the conditions the GPU comparisons rely on hold (separated or bit-equal top-K
candidates, a clear text-versus-timestamp decision, one-hot probes that are one-hot), and every
modelled kernel defect ("mutant" reference) is told from the true reference by more than ten times
the tolerance the GPU tests (tests/test_gpu_decode_kernels.py) use, or by its ids.  CPU only."""
import numpy as np
import pytest

import wdr
from oracle.vocab import Vocab
from tests import decode_cases as dc


@pytest.fixture(scope="module", params=sorted(dc.MODELS))
def vocab_cases(request):
    v = Vocab(dc.MODELS[request.param])
    return v, dc.topk_cases(v)


# ------------------------------------------------------------------ logit rules / top-K / sampling
def test_logits_reference_agrees_with_oracle(vocab_cases):
    v, cases = vocab_cases
    for c in cases:
        for temp in dc.TOPK_TEMPS:
            st, lg, lps, probs = dc.oracle_logits(v, c, temp)
            ref = dc.logits_ref(v, c, temp)
            np.testing.assert_array_equal(ref["x"] == -np.inf, lg == -np.inf, err_msg=c["name"])
            fin = lg > -np.inf
            np.testing.assert_array_equal(ref["x"][fin], lg[fin], err_msg=c["name"])
            # the oracle's f32 log-softmax against the fp64 one
            np.testing.assert_allclose(lps[fin], ref["logp"][fin], rtol=0, atol=1e-4, err_msg=c["name"])
            np.testing.assert_array_equal(lps[~fin], -np.inf)
            for K in dc.TOPK_KS:
                ids, _ = dc.topk_ref(v, c, K, temp)
                want = st.topk(lps, K)
                assert ids == want + [-1] * (K - len(want)), (c["name"], temp, K)


def test_topk_cases_cover_what_they_claim(vocab_cases):
    v, cases = vocab_cases
    V, W = v.n_vocab, dc.slice_width(v.n_vocab)
    assert W == 1621 and V - W * (dc.LG_NB - 1) < W          # 32 slices, a short last one
    by = {c["name"]: c for c in cases}
    top = {n: dc.topk_ref(v, c, 8)[0] for n, c in by.items()}
    assert len({i // W for i in top["one_per_slice"]}) == 8 and W * 31 + 2 in top["one_per_slice"]
    assert {i // W for i in top["one_slice"]} == {7}
    assert [i // W for i in top["thread_stride"][:7]] == [11] * 7
    assert len({(i % W) % dc.LG_THREADS for i in top["thread_stride"][:7]}) == 1
    assert top["ties_slice"][:5] == [1620, 1621, 1622, 3241, 3242]
    assert top["ties_wave"][:4] == [W * 5 + 63, W * 5 + 64, W * 5 + 255, W * 5 + 256]
    assert top["last_slice_ts"][0] == V - 1 and min(top["last_slice_ts"]) >= v.beg
    assert top["flat_ts"][1] == V - 1 and min(top["flat_ts"]) >= v.beg
    assert top["force_only"] == [dc.A] + [-1] * 7 and top["force_only_masked"] == [v.sot] + [-1] * 7
    assert dc.logits_ref(v, by["force_only_masked"], 0.0)["logp"][v.sot] == 0.0
    masked = {n: dc.logits_ref(v, c, c["temp"])["mask_text"] for n, c in by.items()}
    assert masked["last_slice_ts"] and masked["flat_ts"] and masked["text_ts"]
    assert not masked["ts_text_mix"] and not masked["initial"] and not masked["flat_text"]
    assert v.eot in top["ts_text_mix"] and any(i >= v.beg for i in top["ts_text_mix"])
    # flat rows: every slice holding text carries about 1 / 31 of the mass
    p = np.exp(dc.logits_ref(v, by["flat_text"], 1.0)["logp"])
    per = np.add.reduceat(p, np.arange(0, V, W))
    assert per[:31].min() > 0.9 / 31 and per[:31].max() < 1.1 / 31


def test_topk_candidates_separated_and_decision_clear(vocab_cases):
    """Any two of the first K + 1 candidates are bit-equal (a deliberate tie) or >= 1e-2 apart,
    and the text mask is decided by >= 0.5 nat: f32 rounding on the GPU cannot reorder them."""
    v, cases = vocab_cases
    for c in cases:
        for temp in dc.TOPK_TEMPS:
            ref = dc.logits_ref(v, c, temp)
            assert ref["margin"] >= 0.5, (c["name"], temp, ref["margin"])
            ids, _ = dc.topk_ref(v, c, max(dc.TOPK_KS), temp, extra=1)
            x = np.array([ref["x"][i] for i in ids if i >= 0], np.float64)
            gap = np.abs(x[:, None] - x[None, :])
            assert np.all((gap == 0) | (gap >= 1e-2)), (c["name"], temp)
            if temp in dc.SAMPLE_TEMPS:
                # the sampling test's row sums: the mass the text mask removes is negligible
                fin = ref["logp"] > -np.inf
                assert abs(np.exp(ref["logp"][fin]).sum() - 1.0) < 5e-4, (c["name"], temp)


def _topk_differs(v, cases, mutant):
    for c in cases:
        for K in dc.TOPK_KS:
            ids, lp = dc.topk_ref(v, c, K)
            mi, mlp = dc.topk_ref(v, c, K, mutant=mutant)
            if ids != mi:
                return True
            d = [abs(a - b) for a, b in zip(lp, mlp) if np.isfinite(a)]
            if d and max(d) > 10 * dc.LOGP_ATOL:
                return True
    return False


@pytest.mark.parametrize("mutant", dc.LOGIT_MUTANTS)
def test_logit_mutants_are_distinguished(vocab_cases, mutant):
    v, cases = vocab_cases
    assert _topk_differs(v, cases, mutant)
    if mutant == "lse_skip_slice":
        # told by the values alone, on the flat row
        c = next(c for c in cases if c["name"] == "flat_text")
        ids, lp = dc.topk_ref(v, c, 8)
        mi, mlp = dc.topk_ref(v, c, 8, mutant=mutant)
        assert ids == mi and min(abs(a - b) for a, b in zip(lp, mlp)) > 10 * dc.LOGP_ATOL


# ------------------------------------------------------------------ self-attention
@pytest.mark.parametrize("nk", dc.ONEHOT_NK)
def test_onehot_probe_is_onehot(nk):
    case = dc.onehot_probe(nk)
    assert dc.off_target_mass(case) < 1e-5
    # a one-hot row returns its target's V
    ref = dc.self_attn_ref(case["q"], case["kc"], case["vc"], case["row_seq"], case["row_pos"], case["H"])
    np.testing.assert_allclose(ref, case["vc"][0, :nk].astype(np.float64), rtol=0, atol=1e-4)
    # dropping a row's target key moves its output by more than 1.9
    worst = np.inf
    for r in range(0, nk, max(1, nk // 16)):
        keep = np.delete(np.arange(nk), r)
        kc, vc = case["kc"][:, keep], case["vc"][:, keep]
        if nk == 1:
            got = np.zeros_like(ref[:1])
        else:
            got = dc.self_attn_ref(case["q"][r:r + 1], kc, vc, [0], [nk - 2], case["H"])
        worst = min(worst, np.abs(got - ref[r]).max())
    assert worst > 1.9, worst


def test_onehot_probe_prefill_form():
    for n in (8, 37):
        assert dc.off_target_mass(dc.onehot_probe(n, prefill=True)) < 1e-5


def _attn_cases():
    yield from (dc.onehot_probe(nk) for nk in dc.ONEHOT_EDGE)
    yield dc.onehot_probe(37, prefill=True)
    yield dc.random_rows_case(2)
    yield dc.prefill_case(37)


@pytest.mark.parametrize("mutant", dc.ATTN_MUTANTS)
def test_attention_mutants_are_distinguished(mutant):
    worst = 0.0
    for case in map(dc.finite_cache, _attn_cases()):
        a = (case["q"], case["kc"], case["vc"], case["row_seq"], case["row_pos"], case["H"])
        worst = max(worst, np.abs(dc.self_attn_ref(*a) - dc.self_attn_ref(*a, mutant=mutant)).max())
    assert worst > 10 * dc.ATTN_ATOL, worst
    assert worst > 1.9          # the one-hot probes turn the defect into an O(1) error


def test_attention_tolerance_value():
    assert dc.ATTN_ATOL == pytest.approx(4.0e-3, abs=1e-5)
    for H in (2, 6, 20):
        c = dc.random_rows_case(H)
        assert np.abs(c["vc"].astype(np.float64)).max() <= dc.V_CLIP
        assert {0, dc.T_CTX - 1} <= set(c["row_pos"].tolist())
        pairs = list(zip(c["row_seq"].tolist(), c["row_pos"].tolist()))
        assert len(set(pairs)) < len(pairs)                   # repeats


# ------------------------------------------------------------------ KV reorder
@pytest.mark.parametrize("mutant", dc.REORDER_MUTANTS)
def test_reorder_mutants_are_distinguished(mutant):
    k, _ = dc.kv_pattern(1, 16)
    moves = dc.MOVE_SETS["swap"]
    assert all(np.any(dc.reorder_ref(k, moves, n) != dc.reorder_ref(k, moves, n, mutant)) for n in dc.REORDER_ROWS)


def test_reorder_reference():
    k, v = dc.kv_pattern(2, 16)
    assert np.any(k != v)
    for name, moves in dc.MOVE_SETS.items():
        assert len({d for _, d in moves}) == len(moves), name      # a destination at most once
        new = dc.reorder_ref(k, moves, 37)
        for s, d in moves:
            np.testing.assert_array_equal(new[d, :, :37], k[s, :, :37])
            np.testing.assert_array_equal(new[d, :, 37:], k[d, :, 37:])
        for s in set(range(dc.NSEQ)) - {d for _, d in moves}:
            np.testing.assert_array_equal(new[s], k[s])
    assert sorted(d for _, d in dc.MOVE_SETS["perm8"]) == list(range(8))


# ------------------------------------------------------------------ seam argument checks
def test_context_free_seams_validate_on_the_host(lib):
    """wdr_dbg_self_attn / wdr_dbg_proj_qkv refuse out-of-range rows and shapes by their own
    message, before they allocate or launch anything (so this runs without a GPU)."""
    case = dc.prefill_case(8)
    for seq, pos, msg in (([0] * 7 + [1], None, "row_seq out of range"), ([-1] + [0] * 7, None, "row_seq out of range"),
                          (None, [0] * 7 + [dc.T_CTX], "row_pos out of range"), (None, [-1] + [0] * 7, "row_pos out of range")):
        with pytest.raises(wdr.WdrError, match=msg):
            wdr.dbg_self_attn(case["q"], case["kc"], case["vc"], case["row_seq"] if seq is None else seq,
                              case["row_pos"] if pos is None else pos, case["H"])
    with pytest.raises(wdr.WdrError, match="row_pos out of range"):       # pos 4 .. 7 past a 4-row cache
        wdr.dbg_self_attn(case["q"], case["kc"][:, :4], case["vc"][:, :4], case["row_seq"], case["row_pos"], case["H"])
    big = np.zeros((1, 500, 128), np.float16)
    with pytest.raises(wdr.WdrError, match="row_pos out of range"):       # 448 scores at most, whatever T
        wdr.dbg_self_attn(case["q"][:1], big, big, [0], [448], case["H"])
    with pytest.raises(wdr.WdrError, match="bad shape"):
        wdr.dbg_self_attn(np.zeros((1, 64 * 33), np.float16), np.zeros((1, 4, 64 * 33), np.float16),
                          np.zeros((1, 4, 64 * 33), np.float16), [0], [0], 33)
    a = np.zeros((2, 128), np.float16)
    w = np.zeros((384, 128), np.float16)
    kc = np.zeros((3, 32, 128), np.float16)
    for seq, pos, msg in (([0, 3], [0, 1], "row_seq out of range"), ([0, 0], [0, 32], "row_pos out of range"),
                          ([1, 1], [5, 5], "named twice")):
        with pytest.raises(wdr.WdrError, match=msg):
            wdr.dbg_proj_qkv(a, w, None, seq, pos, kc, kc)
    with pytest.raises(wdr.WdrError, match="bad shape"):       # d = 96 is no multiple of 64
        wdr.dbg_proj_qkv(np.zeros((2, 96), np.float16), np.zeros((288, 96), np.float16), None, [0, 1], [0, 0],
                         np.zeros((3, 32, 96), np.float16), np.zeros((3, 32, 96), np.float16))
    with pytest.raises(wdr.WdrError, match="bad shape"):       # K % 32
        wdr.dbg_proj_qkv(np.zeros((2, 48), np.float16), np.zeros((384, 48), np.float16), None, [0, 1], [0, 0], kc, kc)
