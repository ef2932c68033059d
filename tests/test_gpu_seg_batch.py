"""Segmentation of several recordings in shared forwards (SegModel::frame_classes_batch through
wdr_diarize_frame_classes_batch: k_seg_stage lays the files' windows out, the SincNet im2cols run one
launch over all windows).  The forward is per window, so every file's classes must be EQUAL and its
log-probabilities the same BITS as frame_classes of that file alone -- wherever a forward starts or
ends: between files, inside a file, at a file whose last window is all padding.

Lengths: 0 (one all-zero window, the pointer is not read), 1, a short file, one sample short of a
window, exactly one window (a second, all-zero window follows), one sample past it, and 2.5 windows."""
import numpy as np
import pytest

import wdr
from wdr.synth import synth_speech

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 8000, 159999, 160000, 160001, 400000]


@pytest.fixture(scope="module")
def dz():
    return wdr.Diarizer()


@pytest.fixture(scope="module")
def files():
    """Different audio in every file: slices of one two-voice recording at different offsets."""
    pcm, _ = synth_speech(30.0, seed=5, n_speakers=2)
    out = []
    for k, n in enumerate(LENGTHS):
        a = 0 if n == 400000 else 16000 + 9000 * k
        out.append(pcm[a:a + n].copy())
        assert out[-1].size == n
    return out


@pytest.fixture(scope="module")
def ref(dz, files):
    """frame_classes of every file alone, computed once."""
    return [dz.frame_classes(x, logprobs=True) for x in files]


def _same(got, want):
    assert len(got) == len(want)
    for k, ((c, lp), (rc, rlp)) in enumerate(zip(got, want)):
        assert c.shape == rc.shape and lp.shape == rlp.shape, k
        np.testing.assert_array_equal(c, rc, err_msg="classes of file %d" % k)
        np.testing.assert_array_equal(lp.view(np.uint32), rlp.view(np.uint32), err_msg="log-prob bits of file %d" % k)


def test_the_reference_is_not_trivial(ref):
    assert [r[0].shape[0] for r in ref] == [n // 160000 + 1 for n in LENGTHS]
    assert (ref[-1][0] != 0).any() and (ref[-1][0] == 0).any()          # speech and silence
    assert not np.array_equal(ref[-1][1][0], ref[-1][1][1])             # windows differ
    # the all-padding window after exactly 160000 samples is the empty file's window
    np.testing.assert_array_equal(ref[4][1][1].view(np.uint32), ref[0][1][0].view(np.uint32))
    assert np.isfinite(ref[0][1]).all()


@pytest.mark.parametrize("order", ["forward", "reversed"])
@pytest.mark.parametrize("cap", [0, 1, 3])
def test_batch_equals_each_file_alone(dz, files, ref, cap, order):
    """cap 3 over windows 1 1 1 | 1 2 | 2 1 | 2: a forward boundary between files and inside the
    400000-sample file (reversed: 3 | 2 1 | 1 1 1 | 1 1, inside the 160000-sample one, whose second
    window is all padding)."""
    idx = list(range(len(files)))
    if order == "reversed":
        idx.reverse()
    got = dz.frame_classes_batch([files[i] for i in idx], logprobs=True, window_cap=cap)
    _same(got, [ref[i] for i in idx])
    assert dz.stats()[0] > 0


def test_a_batch_of_one_and_classes_only(dz, files, ref):
    for i in (0, 4, 6):
        _same(dz.frame_classes_batch([files[i]], logprobs=True), [ref[i]])
    got = dz.frame_classes_batch(files)          # logprobs_out NULL
    for c, (rc, _) in zip(got, ref):
        np.testing.assert_array_equal(c, rc)


def test_the_same_file_twice_and_a_cap_above_the_default(dz, files, ref):
    got = dz.frame_classes_batch([files[6], files[6], files[0], files[6]], logprobs=True, window_cap=1000)
    _same(got, [ref[6], ref[6], ref[0], ref[6]])
