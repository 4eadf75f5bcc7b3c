"""What the wire audio ingest costs (ops.ingest, csrc/ingest) on a 30 s window:

    python tools/ingest_timing.py [--iters 200] [--md out.md] [--json out.jsonl]

* the launch's time from HIP events around back-to-back launches, for every encoding x {8000, 44100,
  48000} Hz x {1, 2} channels (the channels' mean; at two channels also one channel selected): once
  on one window that stays in cache ("hot": enqueued from Python, and again as 50 launches captured
  into a graph, which takes the host's enqueue rate out of a launch of a few microseconds), once
  rotating over more windows than the 256 MB last-level cache holds ("cold": every launch reads its
  bytes from HBM; enqueued from Python);
* beside it ``ops.pcm16_to_f32`` -- the two-point interpolation this replaces for such input -- on
  the mono 48 kHz and 16 kHz windows, the same way;
* the host-to-device copy of each window (pageable, as AsrEngine.wire_to_audio issues it: the larger
  window is what a higher rate or a second channel costs before any kernel runs);
* one whisper-tiny final pass (random-init weights, 40 tokens, the window already on the device), and
  every launch as a share of it.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import voice_enabled_browser_automation_amd.ops as ops  # noqa: E402
from voice_enabled_browser_automation_amd.asr.wire import ENCODINGS, AudioFormat  # noqa: E402

SECONDS = 30
COLD_BYTES = 768 << 20


def window(fmt: AudioFormat, seed: int) -> np.ndarray:
    g = np.random.default_rng(seed)
    n = SECONDS * fmt.sample_rate * fmt.channels
    if fmt.encoding == "linear16":
        return g.integers(-20000, 20000, n).astype("<i2").view(np.uint8)
    return g.integers(0, 256, n).astype(np.uint8)


def event_us(fn, bufs, iters: int) -> float:
    """us per call of fn(buf) over ``iters`` back-to-back calls rotating over ``bufs``."""
    for b in bufs[:2]:
        fn(b)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(iters):
        fn(bufs[i % len(bufs)])
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def graph_us(fn, buf, launches: int = 50, replays: int = 8) -> float:
    """us per call with the host out of the way: ``launches`` calls captured into one graph, replayed
    ``replays`` times between two events.  (A launch of a few microseconds is otherwise timed at the
    rate Python can enqueue it.)"""
    fn(buf)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        fn(buf)
        with torch.cuda.graph(g, stream=s):
            for _ in range(launches):
                fn(buf)
        g.replay()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(replays):
            g.replay()
        t1.record()
        torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / (launches * replays)


def copy_us(host: np.ndarray, reps: int = 20) -> float:
    t = torch.from_numpy(host)
    xs = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t.to("cuda", non_blocking=True)
        torch.cuda.synchronize()
        xs.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(xs[2:])


def measure(name: str, host: np.ndarray, make_fn, iters: int) -> dict:
    dev = torch.from_numpy(host).to("cuda")
    n_cold = max(2, COLD_BYTES // host.nbytes + 1)
    cold = [dev.clone() for _ in range(n_cold)]
    fn = make_fn()
    return dict(what=name, window_bytes=int(host.nbytes), hot_us=round(event_us(fn, [dev], iters), 2),
                hot_graph_us=round(graph_us(fn, dev), 2), cold_us=round(event_us(fn, cold, iters), 2),
                cold_windows=n_cold, h2d_copy_us=round(copy_us(host), 1))


def final_pass_ms(reps: int = 7) -> float:
    from voice_enabled_browser_automation_amd.asr.engine import AsrEngine
    from voice_enabled_browser_automation_amd.models.config import get_config
    from voice_enabled_browser_automation_amd.models.whisper import WhisperModel
    from voice_enabled_browser_automation_amd.tokenizer import load_tokenizer

    model = WhisperModel(get_config("whisper-tiny"), device=torch.device("cuda"), seed=0)
    eng = AsrEngine(model, load_tokenizer("whisper"), max_sessions=1)
    audio = torch.from_numpy(np.random.default_rng(0).standard_normal(SECONDS * 16000).astype(np.float32) * 0.1).cuda()
    xs = []
    for _ in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.decode_many([audio], exact_tokens=40)
        torch.cuda.synchronize()
        xs.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(xs[2:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--md", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-pass", action="store_true", help="skip the whisper-tiny final pass")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ingest_timing needs a GPU: nothing is measured without one")
    ops.ext()
    ops.ingest_ext()
    recs = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        recs.append(rec)

    seed = 0
    for enc in ENCODINGS:
        for rate in (8000, 44100, 48000):
            for channels, channel in ((1, None), (2, None), (2, 1)):
                fmt = AudioFormat(enc, rate, channels, channel)
                out = torch.empty(SECONDS * 16000, dtype=torch.float32, device="cuda")
                seed += 1
                mix = "mono" if channels == 1 else ("mean of 2" if channel is None else "channel 1 of 2")
                emit(measure(f"ingest {enc} {rate} {mix}", window(fmt, seed),
                             lambda fmt=fmt, out=out: (lambda raw: ops.ingest(raw, fmt, out=out)), a.iters))
    for rate in (48000, 16000):
        host = window(AudioFormat("linear16", rate, 1), 100 + rate)
        out = torch.empty(SECONDS * 16000, dtype=torch.float32, device="cuda")
        emit(measure(f"pcm16_to_f32 {rate} mono (parent)", host,
                     lambda rate=rate, out=out: (lambda raw: ops.pcm16_to_f32(raw.view(torch.int16), in_rate=rate,
                                                                             out=out)), a.iters))
        fmt = AudioFormat("linear16", rate, 1)
        if rate == 16000:
            emit(measure("ingest linear16 16000 mono (pass-through)", host,
                         lambda fmt=fmt, out=out: (lambda raw: ops.ingest(raw, fmt, out=out)), a.iters))
    if not a.no_pass:
        ms = final_pass_ms()
        emit(dict(what="whisper-tiny final pass (30 s window, 40 tokens)", ms=round(ms, 3)))
        for r in recs:
            if "hot_us" in r:
                r["share_of_pass_hot_pct"] = round(r["hot_graph_us"] / (ms * 1e3) * 100, 3)
                r["share_of_pass_cold_pct"] = round(r["cold_us"] / (ms * 1e3) * 100, 3)
    if a.json:
        with open(a.json, "w") as fh:
            fh.writelines(json.dumps(r) + "\n" for r in recs)
    if a.md:
        with open(a.md, "w") as fh:
            fh.write("| launch (30 s window) | window bytes | hot us | hot us, in a graph | cold us | H2D copy us | "
                     "share of pass, hot | cold |\n|---|---|---|---|---|---|---|---|\n")
            for r in recs:
                if "hot_us" in r:
                    fh.write(f"| {r['what']} | {r['window_bytes']} | {r['hot_us']} | {r['hot_graph_us']} | {r['cold_us']} | {r['h2d_copy_us']} | "
                             f"{r.get('share_of_pass_hot_pct', 'n/a')} % | {r.get('share_of_pass_cold_pct', 'n/a')} % |\n")
                else:
                    fh.write(f"\n{r['what']}: {r['ms']} ms\n")


if __name__ == "__main__":
    main()
