"""What n-best rescoring costs (LLMIntentEngine.rescore, ops.seq_logprob, POST /rescore) -- Llama-3-8B
with random-init weights (the scores are arbitrary then; only the times mean anything):

    python tools/rescore_timing.py [--model llama3-8b] [--dtype bf16] [--n 30] [--md out.md] [--json out.jsonl]

For K = 5 alternatives of about 8 and about 16 scored tokens each (behind the cached prompt head):

* the engine call's wall time, submit -> result on an idle engine, stepped from this thread as the
  scheduler thread steps it, and the GPU time of its scoring iterations (HIP events around the
  step() calls that admit, prefill, run the ragged step with the scored rows, the LM head over them
  and the seq_logprob call; 80 scored rows exceed the 64-row step and take two iterations);
* the ``POST /rescore`` round trip through the brain service on the loopback interface (the scheduler
  thread running);
* the seq_logprob call's own time on as many rows of the model's vocabulary, from HIP events around
  back-to-back calls: on rows that stay hot in cache, and rotating over more rows than the 256 MB
  last-level cache holds.
"""
import argparse
import asyncio
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import voice_enabled_browser_automation_amd.ops as ops  # noqa: E402
from voice_enabled_browser_automation_amd.brain.intent_engine import LLMIntentEngine  # noqa: E402
from voice_enabled_browser_automation_amd.brain.prompt import turn_tail  # noqa: E402
from voice_enabled_browser_automation_amd.models.config import get_config  # noqa: E402
from voice_enabled_browser_automation_amd.models.llama import LlamaModel  # noqa: E402
from voice_enabled_browser_automation_amd.runtime.engine import LLMEngine  # noqa: E402
from voice_enabled_browser_automation_amd.tokenizer import load_tokenizer  # noqa: E402

FIRST = ["search", "open", "scroll", "click", "find"]
WORDS = "for the cheapest wireless earbuds with noise cancelling and a long battery life under fifty dollars today".split()


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))] if xs else float("nan")


def summary(xs):
    return dict(n=len(xs), p50=round(statistics.median(xs), 3), p95=round(pct(xs, 0.95), 3), min=round(min(xs), 3),
                max=round(max(xs), 3)) if xs else dict(n=0)


def alternatives(ie, tokens: int, salt: int):
    """Five alternatives that differ from their first word on, each grown word by word to ``tokens``
    ids after the text's opening quote (``salt`` varies them from call to call)."""
    base = len(ie.tok.encode("".join(turn_tail("", ie.chat_format))))
    out = []
    for k, first in enumerate(FIRST):
        words = [first]
        i = salt + k
        while len(ie.tok.encode("".join(turn_tail(" ".join(words), ie.chat_format)))) - base < tokens:
            words.append(WORDS[i % len(WORDS)])
            i += 1
        out.append(" ".join(words))
    return out


def engine_calls(ie, tokens: int, n: int):
    wall, gpu, rows, its = [], [], [], []
    for i in range(n):
        alts = alternatives(ie, tokens, i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        r = ie.submit_rescore(alts)
        e0.record()
        steps = 0
        while not r.done:
            ie.step()
            steps += 1
        e1.record()
        wall.append((time.perf_counter() - t0) * 1e3)
        if r.error is not None:
            raise r.error
        torch.cuda.synchronize()
        gpu.append(e0.elapsed_time(e1))
        rows.append(sum(r.result["scored_tokens"]))
        its.append(steps)
    return wall, gpu, rows, its


def http_calls(ie, tokens: int, n: int):
    from aiohttp.test_utils import TestClient, TestServer

    from voice_enabled_browser_automation_amd.brain.server import build_app

    bodies = [{"alternatives": alternatives(ie, tokens, i)} for i in range(n)]

    async def go():
        out = []
        async with TestClient(TestServer(build_app(ie))) as c:
            for b in bodies:
                t0 = time.perf_counter()
                resp = await c.post("/rescore", json=b)
                await resp.json()
                assert resp.status == 200
                out.append((time.perf_counter() - t0) * 1e3)
        return out

    return asyncio.run(go())


def kernel_time(ie, rows: int, hot: bool, iters: int = 200):
    """us per seq_logprob call over ``rows`` rows of the model's vocabulary, five sequences (HIP events
    around ``iters`` back-to-back calls)."""
    V = ie.engine.model.cfg.vocab_size
    dev = ie.dev
    n_buf = 1 if hot else max(2, (768 << 20) // (rows * V * 4))
    bufs = [torch.randn(rows, V, device=dev) * 3.0 for _ in range(n_buf)]
    target = torch.randint(0, V, (rows,), dtype=torch.int32, device=dev)
    seq = (torch.arange(rows, device=dev) % 5).to(torch.int32)
    target[-5:] = -1
    acc = [torch.zeros(ops.RESCORE_MAX_SEQ, device=dev) for _ in range(2)]
    lp = torch.empty(rows, device=dev)
    es = ie.end_set()
    for b in bufs[:2]:
        ops.seq_logprob(b, V, target, es, seq, ops.RESCORE_MAX_SEQ, acc_in=acc[0], lp=lp, acc_out=acc[1])
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(iters):
        ops.seq_logprob(bufs[i % n_buf], V, target, es, seq, ops.RESCORE_MAX_SEQ, acc_in=acc[0], lp=lp, acc_out=acc[1])
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp8"))
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--md", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ops.ext()
    ops.rescore_ext()
    m = LlamaModel(get_config(a.model), device=torch.device("cuda"), seed=1, wdtype=a.dtype)
    eng = LLMEngine(m, max_seqs=16, max_model_len=4096)
    eng.capture_all()
    ie = LLMIntentEngine(eng, load_tokenizer("llama3"), budget_chars=512, temperature=0.1)
    recs = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        recs.append(rec)

    # warm: the prefix cache, the step graphs of the buckets, the libraries
    ie.turn("scroll down")
    for tokens in (8, 16):
        for i in range(3):
            r = ie.rescore(alternatives(ie, tokens, 100 + i))
    emit(dict(what="setup", model=a.model, dtype=a.dtype, K=5, common_prefix_tokens=r["common_prefix_tokens"],
              cached_prefix_tokens=r["cached_prefix_tokens"], chained=bool(eng.stats.get("chained_steps", 0))))
    turn = [ie.turn("search for the cheapest wireless earbuds")["ms"] for _ in range(a.n)]
    emit(dict(what="turn_probe_wall_ms", note="the yardstick: one probe, same engine", **summary(turn)))
    for tokens in (8, 16):
        wall, gpu, rows, its = engine_calls(ie, tokens, a.n)
        emit(dict(what="rescore_wall_ms", tokens=tokens, scored_rows=summary(rows), iterations=summary(its),
                  **summary(wall)))
        emit(dict(what="scoring_iterations_gpu_ms", tokens=tokens, **summary(gpu)))
    for tokens in (8, 16):
        emit(dict(what="http_rescore_round_trip_ms", tokens=tokens, **summary(http_calls(ie, tokens, a.n))))
    ie.stop()
    for rows in (40, 80, 256):
        for hot in (True, False):
            emit(dict(what="seq_logprob_call_us", rows=rows, cache="hot" if hot else "rotating over 768 MB",
                      us=round(kernel_time(ie, rows, hot), 2)))
    emit(dict(what="engine", **{k: v for k, v in eng.stats.items() if isinstance(v, (int, float))},
              rescores=ie.batch_stats.get("rescores", 0), rescore_rows=ie.batch_stats.get("rescore_rows", 0)))
    if a.json:
        with open(a.json, "w") as fh:
            fh.writelines(json.dumps(r) + "\n" for r in recs)
    if a.md:
        with open(a.md, "w") as fh:
            fh.write("| measurement | value |\n|---|---|\n")
            for r in recs:
                what = r.pop("what")
                fh.write(f"| {what} | `{json.dumps(r)}` |\n")


if __name__ == "__main__":
    main()
