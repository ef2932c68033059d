"""Segment groups that diarize (wdr_run_pipeline_groups_diarize): every group must
come out EXACTLY as one run_pipeline(group, .., diarize_options) call of its own gives it -- text,
times, words, speech index, detected language and speaker_id.  The speaker manager starts afresh
at a group's first segment, while one embedding worker runs ahead over all groups' segments.

SEVERAL: a threshold no cosine reaches, so every speech segment opens a new speaker and the ids
count the segments of a group ("1", "2", ..): a manager carried across a group boundary would go on
counting.  NEAR: 0.9999, which the synthetic embeddings of some utterances reach and others do not.
ONE: max_speakers = 1.  TWO: two speakers opened, then the reference's best match.  DEFAULT: the
Engine's threshold 0.5 without a speaker limit."""
import dataclasses

import pytest

import wdr
from wdr.synth import synth_speech

pytestmark = pytest.mark.gpu

GREEDY = wdr.TranscribeOptions(lang="auto", advanced=wdr.AdvancedTranscribe(sampling_strategy="greedy"))
BEAM = wdr.TranscribeOptions(lang="auto")   # the reference's default: beam search, 5 beams
SYN = wdr.Synthetic(weight_std=0.02, emb_std=0.5, force_len_rate=3.3, disable_fallback=True)
SEVERAL = wdr.DiarizeOptions(threshold=2.0)
NEAR = wdr.DiarizeOptions(threshold=0.9999)
ONE = wdr.DiarizeOptions(max_speakers=1)
TWO = wdr.DiarizeOptions(threshold=2.0, max_speakers=2)
DEFAULT = wdr.DiarizeOptions()


def _plain(res):
    segs, lang, index = res
    return [dataclasses.asdict(s) for s in segs], lang, index


def _ids(res):
    return [s["speaker_id"] for s in res[0]]


@pytest.fixture(scope="module")
def env16():
    mp = pytest.MonkeyPatch()
    mp.setenv("WDR_DECODE_CHAINS", "16")   # KV pool sized for 16 chains at creation
    yield
    mp.undo()


@pytest.fixture(scope="module")
def ctx(env16):
    c = wdr.WhisperContext("tiny-test", synthetic=SYN)
    yield c
    c.close()


@pytest.fixture(scope="module")
def speech():
    pcm, spurts = synth_speech(80.0, seed=11, n_speakers=2)
    segs = [wdr.SpeechSegment(a, b, pcm[int(round(a * 16000)):int(round(b * 16000))]) for a, b, _ in spurts]
    assert len(segs) >= 11
    return segs


@pytest.fixture(scope="module")
def groups(speech):
    return [speech[:2], [], speech[2:5], speech[5:]]


class Refs:
    """One run_pipeline call per group at one chain, computed once per (options, diarize)."""

    def __init__(self, ctx):
        self.ctx, self.memo = ctx, {}

    def __call__(self, key, groups, opts, dia):
        if key not in self.memo:
            self.ctx.set_chains(1)
            # an empty group is an empty list without a language (lang "auto" has nothing to detect on)
            self.memo[key] = [_plain(self.ctx.run_pipeline(g, opts, with_index=True, diarize_options=dia))
                              if g else ([], None, None) for g in groups]
        return self.memo[key]


@pytest.fixture(scope="module")
def refs(ctx):
    return Refs(ctx)


def _run(ctx, groups, opts, dia, chains, callbacks=None):
    ctx.set_chains(chains)
    return [_plain(r) for r in ctx.run_pipeline_groups(groups, opts, diarize=dia, with_index=True, callbacks=callbacks)]


@pytest.mark.parametrize("chains", [1, 4, 16])
def test_groups_equal_one_call_per_group_greedy(ctx, groups, refs, chains):
    want = refs("greedy-several", groups, GREEDY, SEVERAL)
    got = _run(ctx, groups, GREEDY, SEVERAL, chains)
    print(chains, [_ids(g) for g in got])
    assert got == want
    assert got[1] == ([], None, None)
    # every group counts its own speakers from "1": one per speech segment that gave a result
    for g in got:
        index = g[2] or []
        assert _ids(g) == [str(1 + sorted(set(index)).index(i)) for i in index]
    assert len(set(_ids(got[3]))) >= 3
    if chains > 1:
        assert ctx.stage_times()["chains"] == min(chains, sum(len(g) for g in groups))


def test_groups_equal_one_call_per_group_beam(ctx, groups, refs):
    want = refs("beam-several", groups, BEAM, SEVERAL)
    assert _run(ctx, groups, BEAM, SEVERAL, 4) == want
    assert any(s["speaker_id"] not in (None, "1") for g in want for s in g[0])


@pytest.mark.parametrize("name,dia", [("one", ONE), ("two", TWO), ("near", NEAR), ("default", DEFAULT)])
def test_speaker_limits_and_the_default_threshold(ctx, groups, refs, name, dia):
    want = refs("greedy-" + name, groups, GREEDY, dia)
    got = _run(ctx, groups, GREEDY, dia, 4)
    print(name, [_ids(g) for g in got])
    assert got == want
    assert all(s["speaker_id"] is not None for g in got for s in g[0])
    if name == "one":
        assert {i for g in got for i in _ids(g)} == {"1"}
    if name == "two":
        assert {i for g in got for i in _ids(g)} == {"1", "2"}
    if name == "near":
        assert len({i for i in _ids(got[3])}) >= 2


def test_one_segment_groups(ctx, speech, refs):
    """Every block of every chain starts on a group boundary, and every group has one speaker."""
    singles = [[s] for s in speech]
    want = refs("greedy-singles", singles, GREEDY, SEVERAL)
    for chains in (4, 16):
        got = _run(ctx, singles, GREEDY, SEVERAL, chains)
        assert got == want
        assert {i for g in got for i in _ids(g)} == {"1"}


def test_the_manager_restart_matters(ctx, speech, groups, refs):
    """The control: the same segments as ONE group label the later groups differently (the manager
    goes on counting where the groups' own calls start at "1"), while the text is the grouped run's
    wherever the prompt chain agrees -- so the equality above is not something any run would give."""
    want = refs("greedy-several", groups, GREEDY, SEVERAL)
    ctx.set_chains(1)
    whole, _, index = _plain(ctx.run_pipeline(speech, GREEDY, with_index=True, diarize_options=SEVERAL))
    lo, differ = 0, 0
    for g, ref in zip(groups, want):
        part = [s["speaker_id"] for s, i in zip(whole, index) if lo <= i < lo + len(g)]
        if lo == 0:
            assert part == _ids(ref)              # the first group starts the manager either way
        elif g and part != _ids(ref):
            differ += 1
        lo += len(g)
    assert differ == 2, (differ, [s["speaker_id"] for s in whole])
    # one group through the new entry point is run_pipeline
    got = _run(ctx, [speech], GREEDY, SEVERAL, 4)
    assert len(got) == 1 and got[0][0] == whole and got[0][2] == index


def test_no_diarize_options_means_no_speakers(ctx, groups):
    ctx.set_chains(4)
    plain = [_plain(r) for r in ctx.run_pipeline_groups(groups, GREEDY, with_index=True)]
    assert all(s["speaker_id"] is None for g in plain for s in g[0])
    # the explicit argument switches speakers on, whatever opts.enable_diarize says; nothing else moves
    got = _run(ctx, groups, GREEDY, SEVERAL, 4)
    strip = [([dict(s, speaker_id=None) for s in g[0]], g[1], g[2]) for g in got]
    assert strip == plain


def test_callbacks_fire_in_group_segment_order(ctx, groups, refs):
    want = refs("greedy-several", groups, GREEDY, SEVERAL)
    order, pcts = [], []
    cb = wdr.Callbacks(progress=lambda pct, typ, label: pcts.append(pct),
                       new_segment_callback=lambda s: order.append((s.speaker_id, s.text)))
    got = _run(ctx, groups, GREEDY, SEVERAL, 4, callbacks=cb)
    assert got == want
    assert order == [(s["speaker_id"], s["text"]) for g in want for s in g[0]]
    assert len(pcts) > 0 and pcts == sorted(pcts) and pcts[-1] == 100
