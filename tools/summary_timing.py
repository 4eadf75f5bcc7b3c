"""What a summary costs (LLMIntentEngine.summary, ops.nucleus_step) -- the bench model (Llama-3-8B)
with random-init weights: the text is arbitrary then; only the times mean anything.

    python tools/summary_timing.py [--model llama3-8b] [--dtype bf16] [--n 5] [--md out.md] [--json out.jsonl]

* the nucleus launch at the Llama-3 vocabulary for 1 and 8 rows, top_k 50 and 1024 (and pass-through
  rows, what parse rows riding along cost), next to the existing sampler launch on the same rows:
  HIP events around back-to-back launches, rotating over more logits than stay hot in L2;
* a whole summary of a ~1.5k-token page: wall time, decode steps, the host's iteration time, against
  the same engine's parse of a command (a decode step is the unit a summary is made of).

No time is gated anywhere: this is the record of the kernel's cost relative to the sampler launch and
to a decode step, measured in one run.
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
from voice_enabled_browser_automation_amd.models.config import get_config  # noqa: E402
from voice_enabled_browser_automation_amd.models.llama import LlamaModel  # noqa: E402
from voice_enabled_browser_automation_amd.runtime.engine import LLMEngine  # noqa: E402
from voice_enabled_browser_automation_amd.tokenizer import load_tokenizer  # noqa: E402

V = ops.NUCLEUS_MAX_VOCAB
SENTENCE = ("The store lists wireless earbuds with active noise cancelling, a charging case that holds thirty hours "
            "of battery, and free shipping on orders over thirty-five dollars this week. ")


def stats(xs):
    return dict(n=len(xs), p50=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))


def launch_times(rows: int, top_k: int, top_p: float, iters: int = 100):
    """(us per nucleus launch, us per sampler launch) on the same ``rows`` rows of the Llama-3
    vocabulary: random logits in +-6, a mask with 90 % of the ids allowed, a history of 64 ids."""
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(rows * 10000 + top_k)
    n_buf = 8
    bufs = [(torch.rand(rows, V, generator=g) * 12.0 - 6.0).to(dev) for _ in range(n_buf)]
    words = (V + 31) // 32
    mask = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, words), generator=g, dtype=torch.int64).to(torch.int32)
    mask |= torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, words), generator=g, dtype=torch.int64).to(torch.int32)
    mask = mask.to(dev)
    out, n_kept = torch.zeros(rows, words, dtype=torch.int32, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev)
    f = lambda v: torch.full((rows,), v, dtype=torch.float32, device=dev)  # noqa: E731
    T, p, th = f(0.7), f(top_p), f(1.1)
    k = torch.full((rows,), top_k, dtype=torch.int32, device=dev)
    hist = torch.randint(0, V, (rows, 64), generator=g).to(torch.int32).to(dev)
    seed, step = torch.tensor([7], dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    toks = torch.zeros(rows, dtype=torch.int32, device=dev)
    pv, pi = torch.zeros(rows * 64, device=dev), torch.zeros(rows * 64, dtype=torch.int32, device=dev)

    def nucleus(i):
        ops.nucleus_step(bufs[i % n_buf], mask, out, n_kept, T, p, k, th, hist, vocab=V)

    def sampler(i):
        ops.sample(bufs[i % n_buf], mask=out, temperature=T, seed=seed, step=step, out_tokens=toks, part_val=pv,
                   part_idx=pi)

    res = []
    for fn in (nucleus, sampler):
        for i in range(n_buf):
            fn(i)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(iters):
            fn(i)
        t1.record()
        torch.cuda.synchronize()
        res.append(t0.elapsed_time(t1) * 1e3 / iters)
    return res[0], res[1], float(n_kept.float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp8"))
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--max-chars", type=int, default=300)
    ap.add_argument("--md", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ops.ext()
    ops.nucleus_ext()
    recs = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        recs.append(rec)

    for rows in (1, 8):
        for top_k, top_p, what in ((50, 0.9, "top_k 50, top_p 0.9"), (1024, 0.9, "top_k 1024, top_p 0.9"),
                                   (0, 1.0, "pass-through (top_k 0, top_p 1)")):
            nu, sa, kept = launch_times(rows, top_k, top_p)
            emit(dict(what="launch_us", rows=rows, rows_are=what, nucleus_us=round(nu, 2), sampler_us=round(sa, 2),
                      nucleus_over_sampler=round(nu / sa, 2), mean_n_kept=round(kept, 1)))

    m = LlamaModel(get_config(a.model), device=torch.device("cuda"), seed=1, wdtype=a.dtype)
    eng = LLMEngine(m, max_seqs=4, max_model_len=4096)
    eng.capture_all()
    tok = load_tokenizer("llama3")
    ie = LLMIntentEngine(eng, tok, budget_chars=512, temperature=0.1)
    page = SENTENCE * 44
    # warm: both heads' prefix cache, the summary grammar, the step graphs
    ie.parse({"text": "scroll down", "context": {}})
    ie.summary(page, "Earbuds", "https://shop.example/earbuds", max_chars=a.max_chars)
    walls, steps, per_step, parse_step = [], [], [], []
    for _ in range(a.n):
        it0 = ie.batch_stats["iterations"]
        t0 = time.perf_counter()
        r = ie.summary(page, "Earbuds", "https://shop.example/earbuds", max_chars=a.max_chars)
        dt = (time.perf_counter() - t0) * 1e3
        walls.append(dt)
        steps.append(r["decode_steps"])
        st = ie.last_summary_stats
        per_step.append(st["decode_ms"] / max(1, ie.batch_stats["iterations"] - it0))
        ie.parse({"text": "search wireless earbuds", "context": {}})
        ps = ie.last_stats
        parse_step.append(ps["decode_ms"] / max(1, ps["decode_steps"]))
    emit(dict(what="summary_wall_ms", model=a.model, dtype=a.dtype, page_tokens=r["page_tokens"],
              prompt_tokens=r["prompt_tokens"], cached_prefix_tokens=r["cached_prefix_tokens"], max_chars=a.max_chars,
              truncated=r["truncated"], **stats(walls)))
    emit(dict(what="summary_decode_steps", **stats(steps)))
    emit(dict(what="summary_ms_per_iteration", **stats(per_step)))
    emit(dict(what="parse_ms_per_decode_step", **stats(parse_step)))
    emit(dict(what="engine", chained=bool(eng.stats.get("chained_steps", 0)), **ie.summary_stats))
    if a.json:
        with open(a.json, "w") as fh:
            fh.writelines(json.dumps(r) + "\n" for r in recs)
    if a.md:
        with open(a.md, "w") as fh:
            fh.write("| measurement | value |\n|---|---|\n")
            for r in recs:
                r = dict(r)
                what = r.pop("what")
                fh.write(f"| {what} | `{json.dumps(r)}` |\n")


if __name__ == "__main__":
    main()
