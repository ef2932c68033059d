"""wdr.synth: the generator's samples do not depend on how many threads compute its syllables,
and its random draws keep their order (the spurt table of a seed is pinned)."""
import numpy as np

from wdr import synth


def test_synth_speech_is_thread_count_independent(monkeypatch):
    got = {}
    for n in (1, 2, 5):
        monkeypatch.setattr(synth, "_threads", lambda n=n: n)
        got[n] = synth.synth_speech(20.0, seed=3, n_speakers=3)
    pcm, spurts = got[1]
    assert pcm.dtype == np.int16 and pcm.size == 320000
    assert spurts == [(0.9951875, 3.7288125, 0), (4.66775, 9.353625, 1), (10.21, 15.964, 2)]
    for n in (2, 5):
        assert np.array_equal(got[n][0], pcm) and got[n][1] == spurts
    # -12 dBFS RMS inside a spurt, the -60 dBFS noise floor outside
    a, b, _ = spurts[1]
    x = pcm[int(a * 16000):int(b * 16000)].astype(np.float64) / 32767.0
    assert abs(20 * np.log10(np.sqrt(np.mean(x ** 2))) + 12.0) < 0.1
    q = pcm[int(16.5 * 16000):].astype(np.float64) / 32767.0
    assert abs(20 * np.log10(np.sqrt(np.mean(q ** 2))) + 60.0) < 1.0


def test_threads_follow_the_cpu_share(monkeypatch):
    monkeypatch.setenv("OMP_NUM_THREADS", "1")
    assert synth._threads() == 1
    monkeypatch.delenv("OMP_NUM_THREADS")
    assert 1 <= synth._threads() <= 16
