"""Which streams a run creates, and in what order (WDR_STREAM_LOG=1: one `[wdr-stream] <tag>
<pointer>` line on stderr per stream created or handed out).  Stream kind, priority and the
order in which hardware queues first carry work set the pace of every batched decode launch
(DESIGN.md §5 "Hardware queues"), and nothing else in the suite would notice a stream that moved.

tests/golden/stream_log.json was recorded on an MI355X from the build of the commit before stream
placement moved into csrc/streams.cpp, before the refactored build ran at all: this module's
child script with that commit's library and Python binding on its path (WDR_AB_LIB alone does
not do here: this commit's binding also binds two entry points that library lacks), twice per
setting, with equal results.  If a sequence differs, a stream moved: fix the code, not the
fixture.

The lines before the marker come from the context's single-threaded construction and are
compared as an exact sequence; the whole run is compared as a multiset of tags, since the
streams made lazily (states, step batcher, DTW queue, capture streams) come from several host
threads."""
import collections
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "stream_log.json")
MARKER = "[wdr-stream-test] constructed"

SETTINGS = {
    "default": {},
    "all_plain": {"WDR_ENC_POOL": "-1", "WDR_ENC_MASK": "-1", "WDR_ODM_POOL": "-1"},
}
# every variable that places a stream or primes a queue: a child starts from none of them
PLACEMENT = ["WDR_ENC_POOL", "WDR_ENC_MASK", "WDR_ENC_MASK_PAT", "WDR_ENC_PRIO", "WDR_OWN_POOL", "WDR_OWN_MASK",
             "WDR_OWN_PRIO", "WDR_ODM_POOL", "WDR_ODM_MASK", "WDR_BATCH_HWQ", "WDR_DTWQ_HWQ", "WDR_PRIME_POOLS",
             "WDR_PRIME_LOWQ", "WDR_DTWQ_EARLY", "WDR_LOWQ_AT_PIPE", "WDR_BATCHERS", "WDR_PREFILL_SPLIT", "WDR_NO_GRAPH",
             "WDR_ENC_GRAPH", "WDR_ENC_THREAD", "WDR_DTW_QUEUE"]

_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(pkg)r]
import wdr
from wdr.synth import synth_speech
diarize = %(diarize)r
syn = wdr.Synthetic(weight_std=0.02, emb_std=0.5, force_len_rate=3.3, disable_fallback=True)
ctx = wdr.WhisperContext("tiny-test", synthetic=syn)
sys.stderr.write(%(marker)r + "\n")
sys.stderr.flush()
pcm, spurts = synth_speech(30.0, seed=0, n_speakers=2)   # 5 segments: both chains decode
segs = [wdr.SpeechSegment(a, b, pcm[int(round(a * 16000)):int(round(b * 16000))]) for a, b, _ in spurts]
opts = wdr.TranscribeOptions(lang="auto", enable_diarize=True if diarize else None,
                             advanced=wdr.AdvancedTranscribe(sampling_strategy="greedy"))
dopts = wdr.DiarizeOptions.from_options(opts) if diarize else None
out, lang = ctx.run_pipeline(segs, opts, diarize_options=dopts)
ctx.close()
print("RESULT %%d segments" %% len(out))
"""


def stream_log(tmp_path, setting, root=ROOT, diarize=False):
    """(tags logged before the marker, tags of the whole run), from a fresh child process."""
    script = os.path.join(str(tmp_path), "stream_log_child.py")
    with open(script, "w") as f:
        f.write(_CHILD % {"root": root, "pkg": os.path.join(root, "whisper-diarize-rs_amd"), "diarize": diarize,
                          "marker": MARKER})
    env = {k: v for k, v in os.environ.items() if k not in PLACEMENT and k != "WDR_AB_LIB"}
    env.update(setting)
    env.update({"WDR_STREAM_LOG": "1", "WDR_DECODE_CHAINS": "2"})
    p = subprocess.run([sys.executable, script], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "RESULT " in p.stdout and MARKER in p.stderr
    head, _, tail = p.stderr.partition(MARKER)
    tags = lambda text: re.findall(r"^\[wdr-stream\] (\S+) ", text, re.M)
    return tags(head), tags(head) + tags(tail)


@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_stream_log_matches_the_parent(tmp_path, name):
    want = json.load(open(GOLDEN))[name]
    before, whole = stream_log(tmp_path, SETTINGS[name])
    assert before == want["construction"]
    assert dict(collections.Counter(whole)) == want["run"]
    assert len(whole) > len(before) > 0
