"""The encoder GEMM dispatch rule (csrc/gemm_plan.cpp) through wdr_dbg_gemm_plan: host arithmetic,
no GPU.  Every GEMM kernel is bit-identical to k_gemm by design, so the bit-identity tests pass
whichever kernel ran; a slipped threshold would show only as a slower bench.  These tests pin it.

tests/golden/gemm_plan_table.csv was produced once by the dispatch rule of the commit before the
rule became a function (its `if` chains in launch_epi / launch_epi8, copied verbatim into a
throwaway program): column `kernel` with WDR_GEMM3=0, i.e. with k_gemm3 retired, `parent_kernel`
with that commit's own defaults.  Grid: d in {384, 512, 768, 1024, 1280} (knob variants: 384,
768, 1280); qkv (N = 3d, K = d), o (d, d), fc1 (4d, d), fc2 (d, 4d), cross-K/V (2 d n_text_layer,
d) with oracle.weights.hparams_for's layer counts (4 / 6 / 32; Whisper small / medium: 12 / 24),
and qkv with the EPI_QKV_CACHE epilogue and its d argument (3d, d; f16 only);
M in {65, 300, 1500, 3000, 4200, 6000, 12000}; f16 and, for the shapes launch_proj_fp8 accepts,
fp8; plus the shapes of the GPU bit-identity tests, and a variant "unaligned" (default knobs, ldo
or EPI_QKV_CACHE's d raised by 2)."""
import csv
import ctypes as C
import os

import pytest

from wdr import _lib

TABLE = os.path.join(os.path.dirname(__file__), "golden", "gemm_plan_table.csv")
KERNELS = ["k_gemm", "k_gemm2", "k_gemm4", "k_gemm5", "k_gemm8", "k_gemm8n"]   # GemmKernel, csrc/gemm_plan.h
# {WDR_GEMM1, WDR_GEMM4, WDR_GEMM4_GM, WDR_GEMM5, WDR_GEMM5_WIDE, WDR_GEMM8N, WDR_GEMM_CUS}: the defaults
KNOB_NAMES = ["WDR_GEMM1", "WDR_GEMM4", "WDR_GEMM4_GM", "WDR_GEMM5", "WDR_GEMM5_WIDE", "WDR_GEMM8N", "WDR_GEMM_CUS"]
DEFAULTS = [0, -1, 4, 0, 1, 1, 0]


def _rows():
    with open(TABLE, newline="") as f:
        return list(csv.DictReader(f))


ROWS = _rows()
VARIANTS = sorted({r["variant"] for r in ROWS})


def _knobs(variant):
    k = list(DEFAULTS)
    for part in variant.split("+"):
        if "=" in part:
            name, v = part.split("=")
            k[KNOB_NAMES.index(name)] = int(v)
    return k


def _plan(lib, fp8, M, N, K, epi, ldo, d=0, gemm_ref=0, knobs=None):
    out = (C.c_int32 * 4)()
    kn = None if knobs is None else (C.c_int32 * 7)(*knobs)
    _lib.check(lib.wdr_dbg_gemm_plan(fp8, M, N, K, epi, ldo, d, gemm_ref, kn, out))
    return KERNELS[out[0]], out[1], out[2], out[3]


def _row_plan(lib, r, knobs):
    return _plan(lib, int(r["fp8"]), int(r["M"]), int(r["N"]), int(r["K"]), int(r["epi"]), int(r["ldo"]), int(r["qkv_d"]),
                 int(r["gemm_ref"]), knobs)


def _want(r):
    return r["kernel"], int(r["grid_x"]), int(r["grid_y"]), int(r["lds"])


def test_table_covers_the_grid():
    d = [r for r in ROWS if r["variant"] == "default"]
    f16 = [r for r in d if r["fp8"] == "0" and not r["proj"].startswith("test_")]
    assert len(f16) == 5 * 6 * 7
    assert {r["proj"] for r in f16} == {"qkv", "o", "fc1", "fc2", "xkv", "qkv_cache"}
    assert {int(r["M"]) for r in f16} == {65, 300, 1500, 3000, 4200, 6000, 12000}
    # fp8: every projection but cross-K/V (launch_proj_fp8 has no EPI_XKV), every model size
    assert len([r for r in d if r["fp8"] == "1"]) == 5 * 4 * 7
    assert set(VARIANTS) >= {"default", "WDR_GEMM1=1", "WDR_GEMM4=0", "WDR_GEMM4=1", "WDR_GEMM5=1", "WDR_GEMM5_WIDE=0",
                             "WDR_GEMM8N=0", "WDR_GEMM_CUS=8", "WDR_GEMM_CUS=100", "gemm_ref"}


def test_default_dispatch_equals_the_parent_table(lib):
    """Default knobs, explicit and as the process reads them (the suite sets no WDR_GEMM*): kernel,
    grid and dynamic LDS of every shape; and the parent never chose k_gemm3 for any of them --
    the kernel this table's commit removed was dead under the shipped dispatch."""
    assert not any(k in os.environ for k in KNOB_NAMES)
    rows = [r for r in ROWS if r["variant"] == "default"]
    for r in rows:
        assert r["parent_kernel"] == r["kernel"] != "k_gemm3", r
        assert _row_plan(lib, r, DEFAULTS) == _want(r), r
        assert _row_plan(lib, r, None) == _want(r), r


@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "default"])
def test_knob_dispatch_equals_the_parent_table(lib, variant):
    rows = [r for r in ROWS if r["variant"] == variant]
    assert rows
    for r in rows:
        assert _row_plan(lib, r, _knobs(variant)) == _want(r), r
        # the parent differed only where it fell to k_gemm3 (WDR_GEMM4=0, or an output the
        # four-column epilogue cannot store): k_gemm2 / k_gemm now
        assert r["parent_kernel"] in (r["kernel"], "k_gemm3"), r
        if r["parent_kernel"] == "k_gemm3":
            assert variant in ("WDR_GEMM4=0", "unaligned") and r["kernel"] in ("k_gemm", "k_gemm2"), r
    if variant == "unaligned":   # ldo + 2, or EPI_QKV_CACHE's d + 2: nothing but k_gemm can store it
        assert {r["kernel"] for r in rows} == {"k_gemm"}


def test_knob_semantics(lib):
    f16 = [r for r in ROWS if r["fp8"] == "0"]
    # WDR_GEMM1=1 and gemm_ref put everything on k_gemm, whatever else is set
    for v in ("WDR_GEMM1=1", "gemm_ref", "gemm_ref+WDR_GEMM4=1"):
        assert {r["kernel"] for r in f16 if r["variant"] == v} == {"k_gemm"}
    # WDR_GEMM4=0: no ping-pong f16 kernel at all
    assert {r["kernel"] for r in f16 if r["variant"] == "WDR_GEMM4=0"} <= {"k_gemm", "k_gemm2"}
    # WDR_GEMM5=1: the narrow shapes (N < 2048, fewer than 192 256 x 256 tiles) at M >= 4096 on k_gemm5
    narrow = [r for r in f16 if r["variant"] == "WDR_GEMM5=1" and int(r["N"]) < 2048 and int(r["M"]) >= 4096 and
              int(r["N"]) % 128 == 0 and int(r["K"]) % 64 == 0 and (int(r["N"]) // 256) * -(-int(r["M"]) // 256) < 192]
    assert narrow and {r["kernel"] for r in narrow} == {"k_gemm5"}
    # WDR_GEMM5_WIDE=0: fc1 leaves k_gemm5; nothing runs on it under the other defaults
    assert "k_gemm5" in {r["kernel"] for r in f16 if r["variant"] == "default"}
    assert "k_gemm5" not in {r["kernel"] for r in f16 if r["variant"] == "WDR_GEMM5_WIDE=0"}
    # WDR_GEMM8N=0: k_gemm8n only where N has no 256-column tiling
    for r in ROWS:
        if r["variant"] == "WDR_GEMM8N=0" and r["fp8"] == "1":
            assert (r["kernel"] == "k_gemm8n") == (int(r["N"]) % 256 != 0), r
    # WDR_GEMM_CUS: the persistent grid is the knob rounded down to a multiple of 8, never more than the
    # tile count; the other kernels (fp8 included) ignore it
    for cus in (8, 100):
        for r in ROWS:
            if r["variant"] != "WDR_GEMM_CUS=%d" % cus:
                continue
            base = [b for b in ROWS if b["variant"] == "default" and all(b[c] == r[c] for c in
                                                                           ("fp8", "proj", "M", "N", "K", "epi"))][0]
            assert r["kernel"] == base["kernel"]
            tiles = int(base["grid_x"])
            if r["kernel"] in ("k_gemm4", "k_gemm5"):
                assert int(r["grid_x"]) == min(cus // 8 * 8, tiles), r
            else:
                assert (r["grid_x"], r["grid_y"]) == (base["grid_x"], base["grid_y"]), r


def test_shapes_the_gpu_tests_rely_on(lib):
    """tests/test_gpu_kernels.py: test_encoder_gemm_tiles (M = 4200, K = 256) reaches k_gemm4 at
    N = 1280 and 2560 and k_gemm5 at N = 5120; test_gemm2_tiles_bit_identical (M = 300 / 1500,
    K = 512, N = 1280) reaches k_gemm2 -- for every epilogue those tests run, and their
    WDR_DBG_PROJ_GEMM1 reference runs on k_gemm."""
    for epi in (0, 1, 2, 3):
        for N, want in ((1280, "k_gemm4"), (2560, "k_gemm4"), (5120, "k_gemm5")):
            assert _plan(lib, 0, 4200, N, 256, epi, N)[0] == want
            assert _plan(lib, 0, 4200, N, 256, epi, N, gemm_ref=1)[0] == "k_gemm"
        for M in (300, 1500):
            assert _plan(lib, 0, M, 1280, 512, epi, 1280)[0] == "k_gemm2"
            assert _plan(lib, 0, M, 1280, 512, epi, 1280, gemm_ref=1)[0] == "k_gemm"
    # the table (the parent's rule) says the same
    t = {(r["proj"], r["N"], r["M"]): r["kernel"] for r in ROWS if r["variant"] == "default" and r["proj"].startswith("test_")}
    assert t[("test_encoder_gemm_tiles", "1280", "4200")] == t[("test_encoder_gemm_tiles", "2560", "4200")] == "k_gemm4"
    assert t[("test_encoder_gemm_tiles", "5120", "4200")] == "k_gemm5"
    assert t[("test_gemm2_tiles_bit_identical", "1280", "300")] == t[("test_gemm2_tiles_bit_identical", "1280", "1500")] == "k_gemm2"


def test_unaligned_output_goes_to_k_gemm(lib):
    """An ldo (or EPI_QKV_CACHE d) that is no multiple of 4 rules out the four-column epilogue of
    every tiled kernel: k_gemm.  (No caller passes one; before k_gemm3 was retired some such
    shapes reached it.)"""
    assert _plan(lib, 0, 6000, 5120, 1280, 3, 5122)[0] == "k_gemm"
    assert _plan(lib, 0, 6000, 3840, 1280, 5, 3840, d=1282)[0] == "k_gemm"
    assert _plan(lib, 0, 6000, 3840, 1280, 5, 3840, d=1280)[0] == "k_gemm4"
