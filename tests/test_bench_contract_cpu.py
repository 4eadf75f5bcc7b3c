"""bench.py's launch contract, checked without a GPU: `--gpus N` with fewer visible GPUs fails
loudly (never times fewer GPUs than requested), a torchrun WORLD_SIZE that disagrees with
--gpus is refused, and with no GPU at all the single-GPU run exits with a clear message instead
of timing a CPU fallback."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    env.pop("WORLD_SIZE", None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=300)


def test_bench_refuses_more_gpus_than_visible():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0 and "refusing to time fewer GPUs" in (r.stdout + r.stderr)


def test_bench_refuses_world_size_mismatch():
    r = _run(["--gpus", "2"], {"WORLD_SIZE": "4", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=4" in (r.stdout + r.stderr)


def test_bench_needs_a_gpu():
    r = _run(["--steps", "1", "--warmup", "0"])
    assert r.returncode != 0 and "needs a GPU" in (r.stdout + r.stderr)


def test_bench_full_and_dump_outputs_are_accepted():
    """--full and --dump-outputs parse (the run then stops where every GPU-less run stops)."""
    r = _run(["--steps", "1", "--warmup", "0", "--full", "--dump-outputs", "unused"])
    assert r.returncode != 0 and "needs a GPU" in (r.stdout + r.stderr)


def test_dump_outputs_writes_float32_arrays(tmp_path):
    import json

    import numpy as np

    import bench  # (tests/conftest.py puts the repository root on sys.path)

    out = {"version": "1.0", "intents": [{"type": "search", "args": {"query": "café"}}], "confidence": 0.5}
    d = tmp_path / "dump"
    bench.dump_outputs(str(d), "search café", out)
    assert sorted(p.name for p in d.iterdir()) == ["intent_json_utf8.npy", "transcript_utf8.npy"]
    t, j = np.load(d / "transcript_utf8.npy"), np.load(d / "intent_json_utf8.npy")
    assert t.dtype == np.float32 and j.dtype == np.float32
    assert bytes(t.astype(np.uint8)).decode("utf-8") == "search café"
    assert json.loads(bytes(j.astype(np.uint8)).decode("utf-8")) == out
