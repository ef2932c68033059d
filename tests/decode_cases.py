"""Cases and plain fp64 references for the decode-step kernels (tests/test_decode_cases.py checks
them on the CPU, tests/test_gpu_decode_kernels.py runs the kernels against them): KV-cache
self-attention, the beam top-K and the sampling distribution under the logit rules, the beam
reorder of the KV cache, LayerNorm.  Only numpy and the oracle package.

Every reference takes a `mutant` name: the same arithmetic with one deliberate defect of the kind
a kernel could have (a dropped key, a reversed tie rule, a vocabulary slice missing from the
log-sum-exp ...).  The CPU tests require each mutant to be told from the true reference by the
margin the GPU tests use, so a kernel with that defect would fail them; nothing mutated ever runs
on a GPU.
"""
import types

import numpy as np

from oracle.vocab import LANGS
from oracle.whisper_full import FullParams, Token, WhisperState

# ------------------------------------------------------------------ self-attention
T_CTX = 448                # cache rows per sequence (n_text_ctx; the kernel's score array)
V_CLIP = 4.0
# P enters P.V rounded to f16 (2^-11 relative per term, worst case all of one sign: 2^-11 max|V|),
# the output is rounded to f16 (2^-11 |o| <= 2^-11 max|V|), 1e-4 for the f32 summation order and
# __expf
ATTN_ATOL = 2.0 ** -10 * V_CLIP + 1e-4
ONEHOT_NK = (1, 2, 3, 4, 5, 28, 29, 32, 33, 60, 61, 64, 65, 68, 69, 127, 128, 129, 192, 193, 447, 448)
ONEHOT_EDGE = (1, 2, 5, 64, 65, 448)
ATTN_MUTANTS = ("drop_last_key", "key_shift", "own_key_excluded")


def self_attn_ref(q, kc, vc, row_seq, row_pos, H, mutant=None, probs=False):
    """fp64 softmax(q.k / 8).V per head; row r over keys 0 .. row_pos[r] of sequence row_seq[r].
    q [R][64 H], kc / vc [n_seq][T][64 H].  Rows past a row's keys are never read (they may hold
    NaN).  probs: also the list of per-row probabilities [H][nk]."""
    q = np.asarray(q, np.float64)
    T = kc.shape[1]
    out = np.zeros((q.shape[0], H * 64))
    plist = []
    for r in range(q.shape[0]):
        nk = int(row_pos[r]) + 1
        if mutant == "own_key_excluded":
            nk -= 1
        if nk == 0:
            plist.append(np.zeros((H, 0)))
            continue
        idx = np.arange(nk)
        if mutant == "key_shift":
            idx = np.minimum(idx + 1, T - 1)
        k = np.asarray(kc[row_seq[r]][idx], np.float64).reshape(nk, H, 64)
        v = np.asarray(vc[row_seq[r]][idx], np.float64).reshape(nk, H, 64)
        s = np.einsum("hd,khd->hk", q[r].reshape(H, 64), k) / 8.0
        p = np.exp(s - s.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        if mutant == "drop_last_key":      # scored and normalised, lost in P.V
            p = p.copy()
            p[:, -1] = 0.0
        out[r] = np.einsum("hk,khd->hd", p, v).reshape(-1)
        plist.append(p)
    return (out, plist) if probs else out


def _clip_v(rng, shape):
    return np.clip(rng.standard_normal(shape), -V_CLIP, V_CLIP).astype(np.float16)


def _nan_cache(n_seq, d):
    return np.full((n_seq, T_CTX, d), np.nan, np.float16)


def onehot_probe(nk, H=2, prefill=False, seed=0):
    """One-hot key probe: K[j] random +-1 over the 64 dims of every head, q_j = 4 K[j], so row j's
    score is 32 on key j and 0.5 * (a sum of 64 random signs) elsewhere: its output is V[j] unless
    a key is missing, doubled or shifted -- an O(1) error instead of ~1 / nk.  nk rows on sequence 0,
    all at pos nk - 1 (prefill: row i at pos i, targeting its own, last key).  Cache rows from nk
    on hold NaN in K and V.  Returns dict(q, kc, vc, row_seq, row_pos, H, target)."""
    rng = np.random.default_rng([seed, nk, H, int(prefill)])
    d = H * 64
    k = rng.choice(np.array([-1.0, 1.0]), size=(nk, d)).astype(np.float16)
    kc, vc = _nan_cache(1, d), _nan_cache(1, d)
    kc[0, :nk] = k
    vc[0, :nk] = _clip_v(rng, (nk, d))
    pos = np.arange(nk) if prefill else np.full(nk, nk - 1)
    return dict(q=(4 * k).astype(np.float16), kc=kc, vc=vc, row_seq=np.zeros(nk, np.int32),
                row_pos=pos.astype(np.int32), H=H, target=np.arange(nk))


def off_target_mass(case):
    """Largest probability mass a row of a one-hot probe puts off its target key (any head)."""
    _, pl = self_attn_ref(case["q"], case["kc"], case["vc"], case["row_seq"], case["row_pos"], case["H"], probs=True)
    worst = 0.0
    for r, p in enumerate(pl):
        off = np.delete(p, case["target"][r], axis=1)
        worst = max(worst, float(off.sum(1).max()) if off.size else 0.0)
    return worst


def random_rows_case(H, seed=1):
    """40 rows over 5 sequences of 448 cached rows: random (seq, pos) with repeats, pos 0 and 447
    among them; q, k ~ N(0, 1), v clipped to +-4."""
    rng = np.random.default_rng([seed, H])
    n_seq, R, d = 5, 40, H * 64
    kc = rng.standard_normal((n_seq, T_CTX, d)).astype(np.float16)
    vc = _clip_v(rng, (n_seq, T_CTX, d))
    seq = rng.integers(0, n_seq, R)
    pos = rng.integers(0, T_CTX, R)
    seq[:4], pos[:4] = (0, 4, 4, 2), (0, T_CTX - 1, T_CTX - 1, 0)
    seq[20], pos[20] = seq[7], pos[7]          # a repeat away from its twin
    return dict(q=rng.standard_normal((R, d)).astype(np.float16), kc=kc, vc=vc, row_seq=seq.astype(np.int32),
                row_pos=pos.astype(np.int32), H=H)


def read_beyond_case(H=2, seed=2):
    """One row per sequence, nk = 1, 29, 64, 129, 447 keys; every cache row from nk on is NaN."""
    rng = np.random.default_rng([seed, H])
    nks = (1, 29, 64, 129, 447)
    d = H * 64
    kc, vc = _nan_cache(len(nks), d), _nan_cache(len(nks), d)
    for s, nk in enumerate(nks):
        kc[s, :nk] = rng.standard_normal((nk, d)).astype(np.float16)
        vc[s, :nk] = _clip_v(rng, (nk, d))
    return dict(q=rng.standard_normal((len(nks), d)).astype(np.float16), kc=kc, vc=vc,
                row_seq=np.arange(len(nks), dtype=np.int32), row_pos=np.array(nks, np.int32) - 1, H=H)


def prefill_case(n, H=2, seed=3):
    """Rows 0 .. n - 1 of one sequence at pos = row (a prompt prefill: causal by position)."""
    rng = np.random.default_rng([seed, n, H])
    d = H * 64
    kc, vc = _nan_cache(1, d), _nan_cache(1, d)
    kc[0, :n] = rng.standard_normal((n, d)).astype(np.float16)
    vc[0, :n] = _clip_v(rng, (n, d))
    return dict(q=rng.standard_normal((n, d)).astype(np.float16), kc=kc, vc=vc, row_seq=np.zeros(n, np.int32),
                row_pos=np.arange(n, dtype=np.int32), H=H)


def finite_cache(case):
    """The case with its NaN cache rows zeroed (for the mutants that read one row further)."""
    c = dict(case)
    c["kc"], c["vc"] = np.nan_to_num(case["kc"], nan=0.0), np.nan_to_num(case["vc"], nan=0.0)
    return c


# ------------------------------------------------------------------ logit rules, top-K, sampling
MODELS = {"tiny-test": 51864, "tiny-test-ml": 51866}
LG_NB = 32                 # vocabulary slices per row (k_logits_stats / k_logits_topk)
LG_THREADS = 256           # a thread sees elements i0 + t + 256 j of its slice
TOPK_KS = (1, 2, 5, 8)
TOPK_TEMPS = (0.0, 0.5, 1.0)
SAMPLE_TEMPS = (0.5, 1.0)
LOGP_ATOL = 2e-3           # the bound of tests/test_logit_rules.py on these probabilities
LOGIT_MUTANTS = ("tie_high", "lse_skip_slice", "last_slice_ignored", "thread_list_short")
LSE_SKIPPED_SLICE = 13
A, B = 100, 200            # two ordinary text tokens
MAX_INITIAL_TS, SUPPRESS_BLANK = 1.0, True


def slice_width(V):
    return (V + LG_NB - 1) // LG_NB


def topk_cases(v):
    """Rows for the top-K / sampling kernels: dicts of name, x [V] f32 logits, hist (token ids so
    far), has_ts, seek_delta, force (None or (kind, token)) and the row's top-K temperature."""
    V, W = v.n_vocab, slice_width(v.n_vocab)
    rng = np.random.default_rng(V)
    text_only = [A, v.beg + 10, v.beg + 12]      # two timestamps last: every timestamp masked
    out = []

    def add(name, x, hist, has_ts=False, seek_delta=0, force=None):
        out.append(dict(name=name, x=x.astype(np.float32), hist=list(hist), has_ts=has_ts, seek_delta=seek_delta,
                        force=force, temp=TOPK_TEMPS[len(out) % 3]))

    def base(val=-20.0):
        return np.full(V, val, np.float32)

    def ladder(x, idx, top=6.0, step=0.5):
        for r, i in enumerate(idx):
            x[i] = top - step * r
        return x

    # winners one per slice, ranks scrambled against the slice order (the merge has to sort);
    # first / last element of a slice, the five text tokens of the short last slice
    sl = (17, 3, 30, 0, 31, 9, 24, 12, 5)
    off = (0, W - 1, 255, 256, 2, 63, 64, 700, 1000)
    add("one_per_slice", ladder(base(), [W * s + o for s, o in zip(sl, off)]), text_only, True, 24)
    # all winners in one slice: four waves, two on one thread (5 and 261)
    add("one_slice", ladder(base(), [W * 7 + o for o in (5, 64, 130, 200, 261, 700, 1300, W - 1, 63)]), text_only,
        True, 24)
    # the top 7 on one thread's stride (every element thread 37 of slice 11 sees), ranks scrambled
    idx = [W * 11 + 37 + 256 * j for j in (3, 0, 6, 2, 5, 1, 4)] + [W * 20 + 9, W * 2 + 1000]
    add("thread_stride", ladder(base(), idx), text_only, True, 24)
    # exact ties across slice boundaries: 1620 | 1621, 1622 and 3241 | 3242
    x = base()
    x[[W - 1, W, W + 1]] = 5.0
    x[[2 * W - 1, 2 * W]] = 4.0
    add("ties_slice", ladder(x, [8000, 20000, 30000, 40000], 3.0), text_only, True, 24)
    # exact ties across wave boundaries (lanes 63 | 64), a thread's two strides (255 | 256) and two
    # far slices
    i0 = W * 5
    x = base()
    x[[i0 + 63, i0 + 64]] = 5.0
    x[[i0 + 255, i0 + 256]] = 4.0
    x[i0 + 1000] = 3.5
    x[[i0 + 300, W * 20 + 7]] = 3.0
    add("ties_wave", ladder(x, [44000, 12], 2.5), text_only, True, 24)
    # timestamps (all in the short last slice) carry the mass: text masked; V - 1 wins, a tie
    x = base()
    x[A], x[W * 31 + 2] = -5.0, -6.0
    x[[v.beg + 3, V - 2]] = 5.0
    ladder(x, [V - 1, v.beg + 700], 6.0)
    ladder(x, [v.beg, v.beg + 1, v.beg + 255, v.beg + 256, v.beg + 1000, v.beg + 1200], 4.5)
    add("last_slice_ts", x, [B])
    # text keeps the upper hand over the timestamp mass: text, EOT and timestamps interleaved
    x = base()
    for i, val in ((A, 6.0), (W * 9 + 4, 5.0), (v.eot, 4.0), (v.beg + 100, 3.0), (v.beg + 900, 2.5), (W * 31 + 2, 2.25),
                   (30000, 2.0), (V - 1, 1.5), (5, 1.0), (45000, 0.5)):
        x[i] = val
    add("ts_text_mix", x, [B])
    # flat text: every slice carries ~1 / 31 of the mass (a slice missing from the log-sum-exp
    # moves it by ~0.03); planted winners 0.25 apart above the flat part
    x = rng.uniform(-1.0, 1.0, V).astype(np.float32)
    add("flat_text", ladder(x, [W * s + 123 for s in (29, 1, 16, 8, 22, 4, 30, 11, 19)], 3.0, 0.25), text_only, True, 24)
    # flat timestamps over a low text floor: text masked, the short last slice alone
    x = rng.uniform(-1.0, 1.0, V).astype(np.float32)
    x[:v.beg] -= 12.0
    x[[v.beg + 256, v.beg + 257]] = 2.25
    x[[v.beg + 63, v.beg + 64]] = 1.75
    ladder(x, [v.beg + 5, V - 1, V - 2], 3.0, 0.25)
    ladder(x, [v.beg + 800], 2.0)
    ladder(x, [v.beg + 1100, v.beg + 1300], 1.5, 0.25)
    add("flat_ts", x, [B])
    # the synthetic pin: one finite candidate (its own logit; 0 when the rules mask it)
    x = base(-3.0)
    x[A] = 9.0
    add("force_only", x, [B], force=(1, A))
    add("force_only_masked", x.copy(), [B], force=(1, v.sot))
    # the initial step: EOT, " " and timestamps above beg + 50 masked
    x = base()
    x[v.eot], x[v.token_to_id[" "]], x[v.beg + 51], x[v.beg + 50] = 9.0, 8.0, 9.0, -2.0
    add("initial", ladder(x, [A, B, W * 3 + 1, W * 30 + 77, 7, W * 14, W * 15 - 1, 26000, W * 27 + 255]), [])
    # after text + timestamp: text masked by rule, EOT by the timestamp mass, timestamps monotone
    x = base()
    x[A], x[v.eot], x[v.beg + 11] = 9.0, -4.0, 9.0
    add("text_ts", ladder(x, [v.beg + 12, v.beg + 30, V - 1, v.beg + 13, v.beg + 600, v.beg + 268, v.beg + 269,
                              v.beg + 1400, V - 2]), [B, v.beg + 12], True, 24)
    return out


def rule_state(v, case):
    """The row's rule state as wdr_dbg_logits takes it."""
    hist = case["hist"]
    c = dict(n_tokens=len(hist), last_ts=int(len(hist) > 0 and hist[-1] >= v.beg),
             pen_ts=int(len(hist) < 2 or hist[-2] >= v.beg), has_ts=int(case["has_ts"]), seek_delta=case["seek_delta"])
    if case["force"] is not None:
        c["force_kind"], c["force_tok"] = case["force"]
    return c


def oracle_logits(v, case, temp):
    """(logits, logprobs, probs) of oracle.whisper_full.WhisperState.process_logits and the state."""
    st = WhisperState.__new__(WhisperState)
    st.v = v
    st.m = types.SimpleNamespace(hp=types.SimpleNamespace(n_audio_ctx=1500))
    p = FullParams(strategy="greedy", max_initial_ts=MAX_INITIAL_TS, suppress_blank=SUPPRESS_BLANK)
    f = None
    if case["force"] is not None:
        f = ("only", case["force"][1]) if case["force"][0] == 1 else ("text", None)
    lg, lps, probs = st.process_logits(case["x"], [Token(id=t) for t in case["hist"]], case["has_ts"],
                                       case["seek_delta"], p, temp, f)
    return st, lg, lps, probs


def _processed(v, case, temp):
    """The rules on the row before the text-versus-timestamp decision: f32 logits, -inf = masked."""
    x = case["x"].astype(np.float32).copy()
    hist = case["hist"]
    if temp > 0:
        x /= np.float32(temp)
    m = np.zeros(v.n_vocab, bool)
    if SUPPRESS_BLANK and not hist:
        m[[v.eot, v.token_to_id[" "]]] = True
    m[[v.not_, v.sot, v.nosp, v.solm, v.translate, v.transcribe, v.prev]] = True
    m[v.sot + 1:v.sot + 1 + len(LANGS)] = True
    if hist and hist[-1] >= v.beg:
        if len(hist) < 2 or hist[-2] >= v.beg:
            m[v.beg:] = True
        else:
            m[:v.eot] = True
    if not hist and MAX_INITIAL_TS > 0:
        m[v.beg + int(round(MAX_INITIAL_TS / 0.02)) + 1:] = True
    if case["has_ts"]:
        m[v.beg:v.beg + case["seek_delta"] // 2] = True
    if case["force"] is not None:
        kind, tok = case["force"]
        if kind == 1:
            keep = np.float32(0.0) if m[tok] else x[tok]
            m[:] = True
            m[tok] = False
            x[tok] = keep
        else:
            m[v.eot] = True
            m[v.beg:] = True
    x[m] = -np.inf
    return x


def _lse(x):
    fin = x[x > -np.inf].astype(np.float64)
    if fin.size == 0:
        return -np.inf
    return float(np.log(np.exp(fin - fin.max()).sum()) + fin.max())


def logits_ref(v, case, temp, mutant=None):
    """fp64 reference of the processed distribution: dict(x: processed f32 logits with masked text
    at -inf, logp: fp64 log-softmax taken before the text mask (whisper.cpp does not renormalise),
    mask_text, margin: |timestamp log-mass - best text log-prob| in nats)."""
    V, W = v.n_vocab, slice_width(v.n_vocab)
    x = _processed(v, case, temp)
    seen = x.copy()
    if mutant == "lse_skip_slice":
        seen[W * LSE_SKIPPED_SLICE:W * (LSE_SKIPPED_SLICE + 1)] = -np.inf
    if mutant == "last_slice_ignored":
        seen[W * (LG_NB - 1):] = -np.inf
    lse = _lse(seen)
    ts_lp = _lse(seen[v.beg:]) - lse
    text = seen[:v.beg]
    max_text = float(text.max()) - lse if text.size else -np.inf
    mask_text = ts_lp > max_text
    margin = abs(ts_lp - max_text) if np.isfinite(ts_lp) and np.isfinite(max_text) else np.inf
    if mask_text:
        x[:v.beg] = -np.inf
    if mutant == "last_slice_ignored":
        x[W * (LG_NB - 1):] = -np.inf
    logp = np.where(x > -np.inf, x.astype(np.float64) - lse, -np.inf)
    return dict(x=x, logp=logp, mask_text=bool(mask_text), margin=float(margin), V=V)


def topk_ref(v, case, K, temp=None, mutant=None, extra=0):
    """(ids, logp) of the K (+ extra) best candidates: by processed logit, ties by lower id, only
    finite entries; padded with (-1, -inf)."""
    ref = logits_ref(v, case, case["temp"] if temp is None else temp, mutant)
    x = ref["x"]
    fin = np.nonzero(x > -np.inf)[0]
    tie = -fin if mutant == "tie_high" else fin
    if mutant == "thread_list_short":
        # the per-thread sorted list one short: a thread hands at most K - 1 of its elements on
        W = slice_width(v.n_vocab)
        grp = (fin // W) * LG_THREADS + (fin % W) % LG_THREADS
        o = np.lexsort((tie, -x[fin].astype(np.float64), grp))
        g = grp[o]
        first = np.r_[0, np.nonzero(np.diff(g))[0] + 1]
        rank = np.arange(g.size) - np.repeat(first, np.diff(np.r_[first, g.size]))
        keep = o[rank < K - 1]
        fin, tie = fin[keep], tie[keep]
    order = fin[np.lexsort((tie, -x[fin].astype(np.float64)))][:K + extra]
    ids = [int(i) for i in order] + [-1] * (K + extra - order.size)
    return ids, [float(ref["logp"][i]) if i >= 0 else -np.inf for i in ids]


# ------------------------------------------------------------------ KV reorder
NSEQ = 8
MOVE_SETS = {
    "swap": [(0, 1), (1, 0)],
    "cycle3": [(0, 1), (1, 2), (2, 0)],
    "fanout": [(0, 1), (0, 2), (0, 3), (0, 4)],
    "perm8": list(zip(range(8), (3, 0, 7, 1, 6, 2, 5, 4))),
}
REORDER_ROWS = (1, 3, 37, 224, 448)
REORDER_MUTANTS = ("short_by_one_row", "one_phase")


def kv_pattern(L, d, seed=5):
    """Distinct cache contents of sequences 0 .. 7: (k, v) [8][L][448][d] f16 bit patterns
    (finite, so they compare as numbers too)."""
    rng = np.random.default_rng([seed, L, d])
    return tuple(rng.integers(0, 0x7C00, (NSEQ, L, T_CTX, d), dtype=np.uint16) for _ in range(2))


def reorder_ref(cache, moves, n_rows, mutant=None):
    """cache [8][L][448][d] after the beam reorder: sequence dst holds the first n_rows rows that
    sequence src held before it, for every (src, dst)."""
    n = n_rows - 1 if mutant == "short_by_one_row" else n_rows
    new = cache.copy()
    for src, dst in moves:
        # one phase, no scratch: a later move reads what an earlier one wrote
        new[dst, :, :n] = (new if mutant == "one_phase" else cache)[src, :, :n]
    return new


# ------------------------------------------------------------------ LayerNorm
LN_WIDTHS = (128, 384, 512, 768, 1024, 1280)
LN_ROWS = (1, 3, 4, 5, 64, 65)
LN_RTOL, LN_ATOL = 2.0 ** -10, 1e-5   # f16 rounding of the result (2^-11) + f32 statistics


def layernorm_case(K, seed=6):
    rng = np.random.default_rng([seed, K])
    M = max(LN_ROWS)
    x = (rng.standard_normal((M, K)) * 2.0 + 0.3).astype(np.float32)
    g = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    b = (0.1 * rng.standard_normal(K)).astype(np.float32)
    return x, g, b


def layernorm_ref(x, g, b):
    x = x.astype(np.float64)
    return (x - x.mean(1, keepdims=True)) / np.sqrt(x.var(1, keepdims=True) + 1e-5) * g + b
