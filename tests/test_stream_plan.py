"""Stream placement (csrc/streams.cpp) through wdr_dbg_cu_mask / wdr_dbg_stream_plan: host
arithmetic, no GPU.  Which stream a piece of the pipeline runs on -- priority, CU mask, dedicated
hardware queue, shared pool -- moved the benchmark more than any kernel did for several rounds,
and a slipped rule would show only there.  These tests pin it.

tests/golden/stream_plan_table.csv was produced once by the placement code of the commit before
it became a function: dedicated_stream, masked_pool_stream, the three *_masked_stream wrappers
and the `if` ladders of Context / State / StepBatcher / DtwQueue, copied verbatim into a
throwaway program whose HIP calls were stubs that recorded their arguments, one process per row
(the old code read its knobs into statics).  It was never produced from cu_mask / stream_plan.
Columns: `call` is the HIP creation call (prio_* = hipStreamCreateWithPriority, no_prio =
hipStreamCreateWithFlags, cumask = hipExtStreamCreateWithCUMask, none = no stream), `created` how
many streams the first request of a process created (a pool is created whole), `shared` whether
the stream came from a pool, `notes` the WDR_STREAM_LOG tags in order, `mask` the CU mask words
(word 0 first) or error:<message>."""
import csv
import ctypes as C
import os

import pytest

from wdr import _lib

TABLE = os.path.join(os.path.dirname(__file__), "golden", "stream_plan_table.csv")
ROWS = list(csv.DictReader(open(TABLE)))
MASK_ROWS = [r for r in ROWS if r["kind"] == "mask"]
PLAN_ROWS = [r for r in ROWS if r["kind"] == "plan"]
KNOBS = ["WDR_ENC_POOL", "WDR_ENC_MASK", "WDR_ENC_MASK_PAT", "WDR_ENC_PRIO", "WDR_OWN_POOL", "WDR_OWN_MASK",
         "WDR_OWN_PRIO", "WDR_ODM_POOL", "WDR_ODM_MASK", "WDR_BATCH_HWQ", "WDR_DTWQ_HWQ"]
DEFAULTS = [2, 32, 1, 0, -1, 0, 0, 4, 32, 0, 0]
CALLS = {(0, None): "none", (1, 0): "prio_lowest", (1, 1): "prio_middle", (1, 2): "prio_highest", (1, 3): "no_prio"}
# State::State logs these itself, after whatever the plan's stream logged at its creation
ROLE_NOTE = {3: "state-own", 4: "state-es"}


def _hex(words):
    return ":".join("%08x" % w for w in words)


def _mask(lib, ncu, n_res, pat, only):
    n = (ncu + 31) // 32
    out = (C.c_uint32 * n)()
    if lib.wdr_dbg_cu_mask(ncu, n_res, pat, only, out, n) != 0:
        return "error:" + lib.wdr_last_error().decode()
    return _hex(out)


def _plan(lib, role, ncu, knobs=None):
    out = _lib.StreamPlan()
    kn = None if knobs is None else (C.c_int32 * 14)(*knobs)
    if lib.wdr_dbg_stream_plan(role, ncu, kn, out) != 0:
        return dict(call="error", created="", shared="", notes="", mask="error:" + lib.wdr_last_error().decode())
    masked = out.kind in (2, 3)
    tag = out.tag.decode()
    created = 0 if out.kind == 0 else max(1, out.pool)
    notes = [tag] * created if tag else []
    if role in ROLE_NOTE:
        notes.append(ROLE_NOTE[role])
    return dict(call="cumask" if masked else CALLS[(out.kind, out.prio if out.kind == 1 else None)], created=str(created),
                shared=str(int(out.pool > 0)), notes="|".join(notes), mask=_hex(out.mask[:out.n_words]) if masked else "")


def _clear_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def test_table_covers_the_grid():
    masks = {(int(r["ncu"]), int(r["pat"]), int(r["n_res"]), int(r["only_reserved"])) for r in MASK_ROWS}
    for ncu in (256, 304, 64, 40):
        assert {(ncu, 1, n, 0) for n in (0, 8, 16, 24, 32)} <= masks
        assert {(ncu, 0, n, 0) for n in (-1, 0, 1, 8, 32, ncu - 1)} <= masks
        assert (ncu, 0, ncu, 0) in masks and (ncu, 1, ncu, 0) in masks          # n_res >= ncu
    assert {(256, 1, 8, 1), (256, 1, 32, 1), (304, 1, 32, 1), (256, 1, 0, 1), (256, 1, 12, 1), (256, 1, 12, 0)} <= masks
    plans = {(int(r["ncu"]), int(r["role"]), r["env"]) for r in PLAN_ROWS}
    want = ["", "WDR_ENC_POOL=-1 WDR_ENC_MASK=-1", "WDR_ENC_POOL=0", "WDR_ENC_POOL=3", "WDR_ENC_PRIO=1", "WDR_ENC_PRIO=2",
            "WDR_OWN_POOL=2 WDR_OWN_MASK=8", "WDR_OWN_PRIO=1", "WDR_OWN_PRIO=2", "WDR_ODM_POOL=-1", "WDR_ODM_POOL=0",
            "WDR_BATCH_HWQ=1", "WDR_BATCH_HWQ=2", "WDR_DTWQ_HWQ=1", "WDR_DTWQ_HWQ=2"]
    assert {(ncu, role, s) for ncu in (256, 304) for role in range(7) for s in want} <= plans


def test_cu_mask_matches_the_parent(lib):
    bad = []
    for r in MASK_ROWS:
        got = _mask(lib, int(r["ncu"]), int(r["n_res"]), int(r["pat"]), int(r["only_reserved"]))
        if got != r["mask"]:
            bad.append((r["ncu"], r["n_res"], r["pat"], r["only_reserved"], got, r["mask"]))
    assert not bad, bad[:5]
    errs = {r["mask"] for r in MASK_ROWS if r["mask"].startswith("error:")}
    assert errs == {"error:masked stream: must leave at least one CU", "error:WDR_ENC_MASK_PAT=1: 0, 8, 16, 24 or 32 CUs"}


@pytest.mark.parametrize("setting", sorted({r["env"] for r in PLAN_ROWS}))
def test_stream_plan_matches_the_parent(lib, monkeypatch, setting):
    """Knobs through the process environment, as the library reads them."""
    _clear_env(monkeypatch)
    env = dict(kv.split("=") for kv in setting.split())
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    # the same setting as explicit knobs (values, then which of the gate knobs are set at all)
    knobs = [int(env.get(k, d)) for k, d in zip(KNOBS, DEFAULTS)]
    knobs += [int(k in env) for k in ("WDR_ENC_POOL", "WDR_ENC_MASK", "WDR_ODM_POOL")]
    rows = [r for r in PLAN_ROWS if r["env"] == setting]
    assert len(rows) == 14
    for r in rows:
        want = {k: r[k] for k in ("call", "created", "shared", "notes", "mask")}
        role, ncu = int(r["role"]), int(r["ncu"])
        assert _plan(lib, role, ncu) == want, (setting, role, ncu)
        assert _plan(lib, role, ncu, knobs) == want, (setting, role, ncu, "explicit knobs")


def test_gate_opens_on_a_set_knob_not_its_value(lib):
    """WDR_ENC_POOL=2 is the default value, but set it opens the masked pool on a 304-CU device,
    and there the reservation is the top bits."""
    knobs = DEFAULTS + [0, 0, 0]
    assert _plan(lib, 4, 304, knobs)["call"] == "prio_lowest"
    assert _plan(lib, 5, 304, knobs)["call"] == "none"
    p = _plan(lib, 4, 304, DEFAULTS + [1, 0, 0])
    assert (p["call"], p["created"], p["shared"]) == ("cumask", "2", "1")
    assert p["mask"] == _mask(lib, 304, 32, 1, 0) == _hex([0xFFFFFFFF] * 8 + [0xFFFF, 0])
    assert _plan(lib, 5, 304, DEFAULTS + [0, 0, 1])["call"] == "cumask"


def _bits(hexmask):
    v = 0
    for i, w in enumerate(hexmask.split(":")):
        v |= int(w, 16) << (32 * i)
    return v


def test_mask_popcount(lib):
    n = 0
    for ncu in (256, 304, 64, 40):
        for pat in (0, 1):
            for n_res in (-1, 0, 1, 8, 16, 24, 32, ncu - 1):
                m = _mask(lib, ncu, n_res, pat, 0)
                if m.startswith("error:"):
                    assert pat == 1 and ncu == 256 and (n_res % 8 != 0 or n_res > 32), (ncu, pat, n_res, m)
                    continue
                assert bin(_bits(m)).count("1") == ncu - max(0, n_res), (ncu, pat, n_res)
                assert _bits(m) >> ncu == 0
                n += 1
    assert n >= 48


@pytest.mark.parametrize("n_res", [0, 8, 16, 24, 32])
def test_pattern_1_leaves_every_xcd_the_same_share(lib, n_res):
    """Under both numberings the reservation was designed for: mask bit c is CU c % 32 of XCD
    c // 32, or CU c // 8 of XCD c % 8."""
    free = ~_bits(_mask(lib, 256, n_res, 1, 0)) & ((1 << 256) - 1)
    for xcd_of in (lambda c: c // 32, lambda c: c % 8):
        per = [0] * 8
        for c in range(256):
            if free >> c & 1:
                per[xcd_of(c)] += 1
        assert per == [n_res // 8] * 8, (n_res, per)


@pytest.mark.parametrize("n_res", [8, 16, 24, 32])
def test_only_reserved_is_the_complement(lib, n_res):
    pool, rest = _bits(_mask(lib, 256, n_res, 1, 0)), _bits(_mask(lib, 256, n_res, 1, 1))
    assert pool ^ rest == (1 << 256) - 1 and pool & rest == 0
    # the complement follows pattern 1 whatever pattern is asked for
    assert _mask(lib, 256, n_res, 0, 1) == _mask(lib, 256, n_res, 1, 1)


@pytest.mark.parametrize("ncu,n_res", [(304, 32), (256, 0), (256, 12), (64, 8)])
def test_only_reserved_falls_through_to_every_cu(lib, ncu, n_res):
    assert _bits(_mask(lib, ncu, n_res, 1, 1)) == (1 << ncu) - 1
