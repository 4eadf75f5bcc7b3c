"""bench.py on the GPU with the smallest models (whisper-test + llama-tiny): the result line
carries the contract keys, --steps sets the number of timed steps, --dump-outputs writes the last
step's transcript and intent as float32 arrays, and the concurrent-session measurement runs only
with --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--asr", "whisper-test", "--llm", "llama-tiny", "--audio-s", "2", "--concurrent", "2"] + extra
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_result_line_and_dump(tmp_path):
    d = tmp_path / "dump"
    res = _bench(["--dump-outputs", str(d)])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in res, key
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert res["valid_intents"] == "3/3"
    assert "concurrent" not in res  # measured only with --full
    files = sorted(p.name for p in d.iterdir())
    assert files == ["intent_json_utf8.npy", "transcript_utf8.npy"]
    total = 0
    for name in files:
        a = np.load(d / name)
        assert a.dtype == np.float32 and a.ndim == 1
        total += a.nbytes
    assert total <= 64 << 20
    intent = json.loads(bytes(np.load(d / "intent_json_utf8.npy").astype(np.uint8)).decode("utf-8"))
    assert intent["intents"], intent


def test_full_run_measures_the_concurrent_sessions():
    res = _bench(["--full"])
    assert res["steps"] == 3 and res["concurrent"]["sessions_per_rank"] == 2
