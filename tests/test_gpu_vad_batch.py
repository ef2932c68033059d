"""The batched Silero scan (k_vad_lstm_batch, VadModel::probs_batch): B independent recordings in
one pass, one workgroup per recurrence.  Every sequence's probabilities must be the single-sequence
kernel's bit for bit -- the two kernels share the scan's body -- whatever sits beside it in the
batch: empty sequences (a workgroup that leaves before its first barrier), the chunk edges, both
sides of an xg prefetch round (kPF = 8 steps; the prefetch of the last sequence must stop at the
batch's end), a long scan, and more workgroups than the GPU has CUs."""
import numpy as np
import pytest

import wdr

pytestmark = pytest.mark.gpu

CH = 512
EDGES = [1, 511, 512, 513, 8 * CH, 9 * CH, 17 * CH - 3]


def _seq(n, seed):
    """n samples of speech-band noise bursts: loud and quiet stretches, so probabilities move."""
    r = np.random.default_rng(seed)
    x = r.normal(0.0, 3000.0, n) * (0.15 + 0.85 * (np.sin(np.arange(n) * (2 * np.pi / 4000.0) + seed) > 0))
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def vad():
    v = wdr.Vad()
    yield v
    v.close()


@pytest.fixture(scope="module")
def ref(vad):
    """probs() of a sequence, computed once per (length, seed) and never changed."""
    cache = {}

    def get(n, seed):
        if (n, seed) not in cache:
            p = vad.probs(_seq(n, seed))
            assert p.dtype == np.float32 and p.shape == ((n + CH - 1) // CH,)
            p.setflags(write=False)
            cache[(n, seed)] = p
        return cache[(n, seed)]
    return get


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(vad, ref, lens, seed0=100):
    seqs = [_seq(n, seed0 + k) for k, n in enumerate(lens)]
    got = vad.probs_batch(seqs)
    assert len(got) == len(lens)
    for k, n in enumerate(lens):
        want = ref(n, seed0 + k)
        assert got[k].shape == want.shape, (k, n)
        assert np.array_equal(_bits(got[k]), _bits(want)), (k, n)
    return got


@pytest.mark.parametrize("n", [0] + EDGES)
def test_batch_of_one(vad, ref, n):
    _check(vad, ref, [n])


@pytest.mark.parametrize("lens", [[0, 513], [9 * CH, 0], [8 * CH, 17 * CH - 3], [0, 0]])
def test_batch_of_two(vad, ref, lens):
    _check(vad, ref, lens)


def test_batch_of_seven_with_empty_first_middle_last(vad, ref):
    got = _check(vad, ref, [0, 1, 511, 0, 513, 17 * CH - 3, 0])
    assert [g.size for g in got] == [0, 1, 1, 0, 2, 17, 0]


def test_every_edge_beside_a_long_scan(vad, ref):
    """One ~3000-chunk sequence in the middle of the chunk-edge lengths: the short workgroups end
    long before it, and the last sequence ends the batch a few steps past a prefetch round."""
    lens = EDGES[:4] + [3001 * CH - 77] + EDGES[4:]
    got = _check(vad, ref, lens, seed0=300)
    assert got[4].size == 3001
    # sanity: the model reacts to its input -- different sequences, different probabilities,
    # and the long one is not a constant
    assert not np.array_equal(got[4][:17], got[-1])
    assert np.unique(_bits(got[4])).size > 100


def test_three_hundred_short_sequences(vad, ref):
    """More workgroups than CUs (256): some wait for a free CU, some are empty."""
    r = np.random.default_rng(5)
    lens = [int(x) for x in r.integers(1, 6 * CH, 300)]
    for k in (0, 150, 299):
        lens[k] = 0
    _check(vad, ref, lens, seed0=1000)


def test_order_does_not_matter(vad, ref):
    lens = [513, 0, 9 * CH, 8 * CH, 1, 17 * CH - 3, 511]
    seqs = [_seq(n, 100 + k) for k, n in enumerate(lens)]
    fwd = vad.probs_batch(seqs)
    rev = vad.probs_batch(seqs[::-1])[::-1]
    for a, b in zip(fwd, rev):
        assert np.array_equal(_bits(a), _bits(b))
    # two different sequences of one length do not share a result
    a, b = vad.probs_batch([_seq(9 * CH, 1), _seq(9 * CH, 2)])
    assert a.shape == b.shape and not np.array_equal(_bits(a), _bits(b))
    assert vad.last_us_per_step > 0.0
