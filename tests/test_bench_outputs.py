"""bench.py's command line and --dump-outputs writer (host only: no GPU, no run of the benchmark)."""
import os
import sys

import numpy as np

import bench
import wdr


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (3, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_arrays(tmp_path):
    segs = [wdr.Segment(0.5, 2.0, " héllo wörld", [wdr.WordTimestamp(" héllo", 0.5, 1.0, 0.25),
                                                   wdr.WordTimestamp(" wörld", 1.0, 2.0, None)], "SPEAKER_01"),
            wdr.Segment(3.0, 4.0, "", None, None),
            wdr.Segment(4.0, 5.5, " x", [wdr.WordTimestamp(" x", 4.0, 5.5, 1.0)], "SPEAKER_00")]
    d = str(tmp_path / "out")
    bench.dump_outputs(d, segs, [(0.25, 2.5), (3.0, 6.0)])
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert sorted(got) == ["segment_text", "segments", "speakers", "speech_spans", "word_text", "words"]
    assert all(a.dtype == np.float64 for a in got.values())
    np.testing.assert_array_equal(got["segments"], [[0.5, 2.0, 2], [3.0, 4.0, 0], [4.0, 5.5, 1]])
    np.testing.assert_array_equal(got["words"], [[0, 0.5, 1.0, 0.25], [0, 1.0, 2.0, np.nan], [2, 4.0, 5.5, 1.0]])
    np.testing.assert_array_equal(got["speech_spans"], [[0.25, 2.5], [3.0, 6.0]])

    def text(a):
        return "".join(chr(int(c)) for c in a).split("\n")[:-1]
    assert text(got["segment_text"]) == [" héllo wörld", "", " x"]
    assert text(got["word_text"]) == [" héllo", " wörld", " x"]
    assert text(got["speakers"]) == ["SPEAKER_01", "", "SPEAKER_00"]
    # no output segments, no spans given: empty arrays of the same shapes, no speech_spans file
    e = str(tmp_path / "empty")
    bench.dump_outputs(e, [])
    assert np.load(os.path.join(e, "segments.npy")).shape == (0, 3)
    assert np.load(os.path.join(e, "words.npy")).shape == (0, 4)
    assert not os.path.exists(os.path.join(e, "speech_spans.npy"))
