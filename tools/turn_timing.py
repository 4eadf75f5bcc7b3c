"""What the turn-completion probe costs (LLMIntentEngine.turn, ops.set_logprob) -- Llama-3-8B with
random-init weights (p_end is arbitrary then; only the times mean anything):

    python tools/turn_timing.py [--model llama3-8b] [--dtype bf16] [--n 40] [--md out.md] [--json out.jsonl]

* the probe's wall time alone: submit -> result on an idle engine (prefix cached: admission prefill
  of the ~10-20 suffix rows, one ragged step with a logits row, the set_logprob launch, a stream
  synchronise), stepped from this thread as the scheduler thread steps it;
* the same while 1 and while 8 parse requests decode (finished parses are replaced, so the load is
  steady); the probe's iteration then also decodes a token for each of them;
* a decode iteration's wall time with a probe in it against one without, under the same loads: the
  admission prefill (its own forward) and the rest (the step with the probe's row, the LM head with
  one more row, set_logprob, the synchronise) separately;
* the set_logprob kernel's own time on rows of the model's vocabulary, from HIP events around
  back-to-back launches: on one row that stays hot in cache, and rotating over more rows than the
  256 MB last-level cache holds.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import voice_enabled_browser_automation_amd.ops as ops  # noqa: E402
from voice_enabled_browser_automation_amd.brain.intent_engine import LLMIntentEngine  # noqa: E402
from voice_enabled_browser_automation_amd.brain.prompt import COMMANDS, messages_for  # noqa: E402
from voice_enabled_browser_automation_amd.models.config import get_config  # noqa: E402
from voice_enabled_browser_automation_amd.models.llama import LlamaModel  # noqa: E402
from voice_enabled_browser_automation_amd.runtime.engine import LLMEngine  # noqa: E402
from voice_enabled_browser_automation_amd.tokenizer import load_tokenizer  # noqa: E402

TEXTS = [" ".join(c.split()[:k]) for c in COMMANDS for k in range(1, len(c.split()) + 1)]


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))] if xs else float("nan")


def summary(xs):
    return dict(n=len(xs), p50=round(statistics.median(xs), 3), p95=round(pct(xs, 0.95), 3), min=round(min(xs), 3),
                max=round(max(xs), 3)) if xs else dict(n=0)


def probe_under_load(ie, load: int, n: int):
    """n probes, one at a time, while ``load`` parse requests decode.  Returns the probes' wall ms
    (submit -> done), the wall ms of the iterations with a probe in them split into (admission
    prefill, rest), and the wall ms of the iterations without one (no admission either)."""
    parses, k = [], 0

    def top_up():
        nonlocal k
        parses[:] = [r for r in parses if not r.done]
        while len(parses) < load:
            parses.append(ie.submit(messages_for({"text": COMMANDS[k % len(COMMANDS)], "context": {}})))
            k += 1

    wall, with_probe, plain = [], [], []
    for i in range(n):
        top_up()
        for _ in range(3):  # the load is admitted and decoding; plain iterations are timed here
            fresh = bool(ie.waiting)
            t0 = time.perf_counter()
            ie.step()
            dt = (time.perf_counter() - t0) * 1e3
            if load and not fresh and ie.active:
                plain.append(dt)
            top_up()
        if ie.waiting:  # (a parse finished in the last step: admit its replacement before the probe)
            ie.step()
        a0 = ie.timing["admit_prefill_ms"]
        t0 = time.perf_counter()
        p = ie.submit_turn(TEXTS[i % len(TEXTS)])
        steps = 0
        while not p.done:
            ie.step()
            steps += 1
        dt = (time.perf_counter() - t0) * 1e3
        if p.error is not None:
            raise p.error
        wall.append(dt)
        if steps == 1:
            admit = ie.timing["admit_prefill_ms"] - a0
            with_probe.append((admit, dt - admit))
    while any(not r.done for r in parses):  # drain
        ie.step()
    return wall, with_probe, plain


def kernel_time(ie, rows: int, hot: bool, iters: int = 200):
    """us per set_logprob launch over ``rows`` rows of the model's vocabulary (HIP events around
    ``iters`` back-to-back launches)."""
    V = ie.engine.model.cfg.vocab_size
    dev = ie.dev
    n_buf = 1 if hot else max(2, (768 << 20) // (rows * V * 4))
    bufs = [torch.randn(rows, V, device=dev) * 3.0 for _ in range(n_buf)]
    out = torch.empty(rows, 2, device=dev)
    es = ie.end_set()
    for b in bufs[:2]:
        ops.set_logprob(b, V, es, out=out)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(iters):
        ops.set_logprob(bufs[i % n_buf], V, es, out=out)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp8"))
    ap.add_argument("--n", type=int, default=40)
    ap.add_argument("--md", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ops.ext()
    ops.turn_ext()
    m = LlamaModel(get_config(a.model), device=torch.device("cuda"), seed=1, wdtype=a.dtype)
    eng = LLMEngine(m, max_seqs=16, max_model_len=4096)
    eng.capture_all()
    ie = LLMIntentEngine(eng, load_tokenizer("llama3"), budget_chars=512, temperature=0.1)
    recs = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        recs.append(rec)

    # warm: the prefix cache, the step graphs of the probe's buckets, the libraries
    for t in TEXTS[:6]:
        r = ie.turn(t)
    ie.parse({"text": "scroll down", "context": {}})
    emit(dict(what="setup", model=a.model, dtype=a.dtype, end_set_ids=len(ie.end_set_ids()),
              prompt_tokens=r["prompt_tokens"], cached_prefix_tokens=r["cached_prefix_tokens"],
              chained=bool(eng.stats.get("chained_steps", 0))))
    for load in (0, 1, 8):
        wall, with_probe, plain = probe_under_load(ie, load, a.n)
        emit(dict(what="probe_wall_ms", load=load, **summary(wall)))
        if with_probe:
            emit(dict(what="probe_iteration_ms", load=load, admit_prefill=summary([x for x, _ in with_probe]),
                      step_with_probe_row=summary([y for _, y in with_probe])))
        if plain:
            emit(dict(what="plain_iteration_ms", load=load, **summary(plain)))
    for rows in (1, 8):
        for hot in (True, False):
            emit(dict(what="set_logprob_kernel_us", rows=rows, cache="hot" if hot else "rotating over 768 MB",
                      us=round(kernel_time(ie, rows, hot), 2)))
    emit(dict(what="engine", **{k: v for k, v in eng.stats.items() if isinstance(v, (int, float))},
              probes=ie.batch_stats.get("probes", 0)))
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
