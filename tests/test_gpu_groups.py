"""Segment groups (wdr_run_pipeline_groups): several recordings' speech segments in
one pipeline run, sharing the decode chains.  Every group must come out EXACTLY as one
run_pipeline call of its own gives it -- prompt chain, decoder 0's random numbers, overlap clip,
detected language and speech index restart at a group's first segment -- wherever the chains'
blocks are cut: on a group boundary, in the middle of a group, across three groups."""
import dataclasses

import numpy as np
import pytest

import wdr
from wdr._lib import WdrError
from wdr.synth import synth_speech

pytestmark = pytest.mark.gpu

GREEDY = wdr.TranscribeOptions(lang="auto", advanced=wdr.AdvancedTranscribe(sampling_strategy="greedy"))
BEAM = wdr.TranscribeOptions(lang="auto")   # the reference's default: beam search, 5 beams
SAMPLED = wdr.TranscribeOptions(lang="auto", advanced=wdr.AdvancedTranscribe(sampling_strategy="greedy",
                                                                             temperature=0.4))


def _segs(pcm, spurts):
    return [wdr.SpeechSegment(a, b, pcm[int(round(a * 16000)):int(round(b * 16000))]) for a, b, _ in spurts]


def _split(segs, sizes):
    """sizes, then the rest as the last group."""
    out, i = [], 0
    for n in sizes:
        out.append(segs[i:i + n])
        i += n
    assert i < len(segs)
    return out + [segs[i:]]


def _plain(res):
    segs, lang, index = res
    return [dataclasses.asdict(s) for s in segs], lang, index


class Case:
    """A context, grouped segments, and the per-group reference: one run_pipeline call per group
    at one chain, computed once."""

    def __init__(self, syn, groups, opts):
        self.ctx = wdr.WhisperContext("tiny-test", synthetic=syn)
        self.groups, self.opts = groups, opts
        self.ctx.set_chains(1)
        # an empty group is an empty list without a language (lang "auto" has nothing to detect on)
        self.ref = [_plain(self.ctx.run_pipeline(g, opts, with_index=True)) if g else ([], None, None)
                    for g in groups]

    def run(self, chains, speakers=None):
        self.ctx.set_chains(chains)
        got = self.ctx.run_pipeline_groups(self.groups, self.opts, speakers=speakers, with_index=True)
        return [_plain(r) for r in got]


@pytest.fixture(scope="module")
def env16():
    mp = pytest.MonkeyPatch()
    mp.setenv("WDR_DECODE_CHAINS", "16")   # KV pool sized for 16 chains at creation
    yield
    mp.undo()


@pytest.fixture(scope="module")
def speech():
    pcm, spurts = synth_speech(80.0, seed=11, n_speakers=2)
    segs = _segs(pcm, spurts)
    assert len(segs) >= 11
    return segs


SYN = wdr.Synthetic(weight_std=0.02, emb_std=0.5, force_len_rate=3.3, disable_fallback=True)


@pytest.fixture(scope="module")
def greedy(env16, speech):
    c = Case(SYN, _split(speech, [1, 3, 0, 5]), GREEDY)
    yield c
    c.ctx.close()


@pytest.fixture(scope="module")
def beam(env16, speech):
    c = Case(SYN, _split(speech, [1, 3, 0, 5]), BEAM)
    yield c
    c.ctx.close()


@pytest.fixture(scope="module")
def singles(env16, speech):
    c = Case(SYN, [[s] for s in speech], GREEDY)
    yield c
    c.ctx.close()


@pytest.mark.parametrize("chains", [1, 2, 4, 16])
def test_groups_equal_one_call_per_group_greedy(greedy, chains):
    got = greedy.run(chains)
    assert [len(g[0]) for g in got] == [len(r[0]) for r in greedy.ref]
    assert got == greedy.ref
    assert got[2] == ([], None, None)
    if chains > 1:
        assert greedy.ctx.stage_times()["chains"] == min(chains, sum(len(g) for g in greedy.groups))


def test_the_prompt_break_matters(greedy, speech):
    """Sanity for the fixture: in the one ungrouped run, some group's segments come out different
    from the group's own run (their first segment saw the previous group's text as its prompt) --
    so equality above is not something any run would give."""
    greedy.ctx.set_chains(1)
    whole, _, index = _plain(greedy.ctx.run_pipeline(speech, GREEDY, with_index=True))
    differ, lo = 0, 0
    for g, (ref, _, ref_index) in zip(greedy.groups, greedy.ref):
        part = [s for s, i in zip(whole, index) if lo <= i < lo + len(g)]
        if lo > 0 and g and [s["text"] for s in part] != [s["text"] for s in ref]:
            differ += 1
        lo += len(g)
    assert differ >= 1
    # and the first group, which starts the file either way, is the same up to the clip of its
    # last segment against the next group's first
    first = [s for s, i in zip(whole, index) if i < len(greedy.groups[0])]
    assert [s["text"] for s in first] == [s["text"] for s in greedy.ref[0][0]]


@pytest.mark.parametrize("chains", [1, 4, 16])
def test_groups_equal_one_call_per_group_beam(beam, chains):
    assert beam.run(chains) == beam.ref


@pytest.mark.parametrize("chains", [2, 4, 16])
def test_one_segment_groups(singles, chains):
    """Every block of every chain starts on a group boundary: nothing is ever redone."""
    assert singles.run(chains) == singles.ref
    st = singles.ctx.stage_times()
    assert st["fixup_segments"] == 0, st


def test_fallback_replay_is_per_group(env16):
    """whisper.cpp's thresholds on ~12-s segments (as test_forced_early_fixup_is_exact): the
    temperature ladder draws random numbers, so a segment depends on every earlier draw of its
    group -- and on none of another group's.  The sampled-tail replay must run, per group."""
    syn = wdr.Synthetic(weight_std=0.02, emb_std=0.5, force_len_rate=3.3, disable_fallback=False)
    pcm, spurts = synth_speech(90.0, seed=13, n_speakers=2)
    merged, cur = [], []
    for sp in spurts:
        cur.append(sp)
        if cur[-1][1] - cur[0][0] >= (12.0 if len(merged) % 2 == 0 else 0.0):
            merged.append((cur[0][0], cur[-1][1], None))
            cur = []
    segs = _segs(pcm, merged)
    assert len(segs) >= 7
    c = Case(syn, _split(segs, [1, 3, 0]), GREEDY)
    try:
        for chains in (4, 2):
            assert c.run(chains) == c.ref, chains
            st = c.ctx.stage_times()
            assert st["replay_segments"] > 0, st
        assert c.run(1) == c.ref
    finally:
        c.ctx.close()


def test_sampled_from_the_first_window_takes_one_chain(env16, speech):
    """temperature > 0: one chain, the segment loop -- its RNG and prompt reset at a group start."""
    c = Case(SYN, _split(speech[:8], [1, 3, 0]), SAMPLED)
    try:
        assert c.run(4) == c.ref
        st = c.ctx.stage_times()
        assert st["chains"] == 1 and st["batch_launches"] == 0, st   # the loop, not the chains
        assert sum(len(r[0]) for r in c.ref) >= 5
    finally:
        c.ctx.close()


def test_one_group_is_run_pipeline(greedy, speech):
    for chains in (1, 4):
        greedy.ctx.set_chains(chains)
        want = _plain(greedy.ctx.run_pipeline(speech, GREEDY, with_index=True))
        got = greedy.ctx.run_pipeline_groups([speech], GREEDY, with_index=True)
        assert len(got) == 1 and _plain(got[0]) == want


def test_group_speakers_and_callbacks(greedy):
    order, pcts = [], []
    cb = wdr.Callbacks(progress=lambda pct, typ, label: pcts.append(pct),
                       new_segment_callback=lambda s: order.append((s.speaker_id, s.start)))
    labels = ["a", None, "c", "d", "e"]
    greedy.ctx.set_chains(4)
    got = greedy.ctx.run_pipeline_groups(greedy.groups, GREEDY, speakers=labels, callbacks=cb)
    for (segs, lang), (ref, ref_lang, _), lab in zip(got, greedy.ref, labels):
        assert lang == ref_lang
        assert [dataclasses.asdict(s) for s in segs] == [dict(r, speaker_id=lab) for r in ref]
    # (group, segment) order on the calling thread; progress over all segments
    want = [(lab, r["start"]) for (ref, _, _), lab in zip(greedy.ref, labels) for r in ref]
    assert [o[0] for o in order] == [w[0] for w in want]
    assert len(pcts) > 0 and pcts == sorted(pcts) and pcts[-1] == 100


def test_bad_groups_are_refused(greedy, speech):
    ctx = greedy.ctx
    for starts in ([1, 3], [0, 5, 3], [0, len(speech) + 1]):
        with pytest.raises(WdrError) as e:
            ctx.run_pipeline_groups(speech, GREEDY, group_start=starts)
        assert "group_start" in str(e.value), starts
    dia = dataclasses.replace(GREEDY, enable_diarize=True)
    with pytest.raises(WdrError) as e:
        ctx.run_pipeline_groups([speech[:2], speech[2:4]], dia)
    assert "do not diarize" in str(e.value)
