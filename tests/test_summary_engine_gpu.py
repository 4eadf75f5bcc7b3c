"""Summary requests through LLMIntentEngine on the GPU (llama-tiny with random-init weights, strict
native mode, captured step graphs), with the engine's defaults and with the masked LM head, the
zero-copy buffers and the spin wait all off.  Every traced step of a summary is held to the oracle of
tests/nucleus_oracle.py (the kernel's mask equals the oracle's, the sampled token is kept); the
result is {"summary": str} within max_chars; a greedy parse yields the same text alone and with a
summary sharing its iterations; a parse-only run makes no nucleus launch; a turn probe alongside
still matches its oracle; the parse head's cached length survives a summary; nothing leaks."""
import json

import numpy as np
import pytest

import nucleus_oracle as no
import turn_oracle as to
import voice_enabled_browser_automation_amd.ops as ops
from voice_enabled_browser_automation_amd.brain.intent_engine import LLMIntentEngine
from voice_enabled_browser_automation_amd.brain.prompt import messages_for
from voice_enabled_browser_automation_amd.contracts import ParseResponse, safe_parse
from voice_enabled_browser_automation_amd.models.config import LLAMA_PRESETS
from voice_enabled_browser_automation_amd.models.llama import LlamaModel
from voice_enabled_browser_automation_amd.runtime.engine import LLMEngine
from voice_enabled_browser_automation_amd.tokenizer import load_tokenizer

pytestmark = pytest.mark.gpu

OFF = ("VWA_MASKED_HEAD", "VWA_ZERO_COPY", "VWA_SPIN_WAIT")
PAGE = ("Wireless earbuds with active noise cancelling are on sale this week. Battery life is up to thirty hours "
        "with the case. Free shipping on orders over thirty-five dollars. ") * 3
SAMPLING = dict(max_chars=48, temperature=0.8, top_p=0.85, top_k=40, penalty=1.2)
TEXTS = ["search wireless earbuds", "go back"]


@pytest.fixture(scope="module")
def model():
    ops.ext()
    ops.nucleus_ext()  # fail loudly if a library is missing
    return LlamaModel(LLAMA_PRESETS["llama-tiny"], device="cuda", seed=1)


def make(model, temperature=0.0):
    eng = LLMEngine(model, max_seqs=8, max_model_len=2048)
    ie = LLMIntentEngine(eng, load_tokenizer("llama3"), budget_chars=160, temperature=temperature, seed=7)
    ie.keep_summary_trace = True
    return eng, ie


def check_trace(ie, req, V):
    steps = [tr for tr in ie.last_summary_trace if tr["request"] is req]
    assert len(steps) == req.steps == len(req.sampled) >= 1
    H = ie.summary_history
    ambiguous = 0
    for s, tr in enumerate(steps):
        assert tr["step"] == s and tr["token"] == req.sampled[s]
        assert tr["history"].tolist() == (req.sampled[:s][-H:] + [-1] * H)[:H]
        ambiguous += no.check_trace_step(tr, V)
    return len(steps), ambiguous


def run(ie, parses, summaries=0, probe_at=None):
    reqs = [ie.submit(messages_for({"text": t, "context": {}})) for t in parses]
    summ = [ie.submit_summary(PAGE, "Earbuds", "https://shop.example/earbuds", **SAMPLING) for _ in range(summaries)]
    probes, it = [], 0
    while not all(r.done for r in reqs + summ + probes):
        for text in (probe_at or {}).get(it, ()):
            probes.append(ie.submit_turn(text))
        ie.step()
        it += 1
        assert it < 2000
    for r in reqs + summ + probes:
        if r.error is not None:
            raise r.error
    return reqs, summ, probes


@pytest.mark.parametrize("flags", ["defaults", "all_off"])
def test_summaries_alone_and_among_parses_and_probes(model, flags, monkeypatch):
    if flags == "all_off":
        for k in OFF:
            monkeypatch.setenv(k, "0")
    V = model.cfg.vocab_size
    # greedy parses alone: no nucleus launch
    eng0, plain = make(model)
    assert (plain.masked_head, plain.zero_copy, plain.spin_wait) == ((True,) * 3 if flags == "defaults" else (False,) * 3)
    launches0 = ops.nucleus_launches
    alone, _, _ = run(plain, TEXTS)
    assert ops.nucleus_launches == launches0 and plain.summary_stats["nucleus_launches"] == 0

    eng, ie = make(model)
    assert eng.use_graphs
    ie.keep_turn_trace = True
    ie.parse({"text": "go back", "context": {}})
    ie.parse({"text": "scroll down", "context": {}})
    cached_before = ie.last_stats["cached_prefix_tokens"]
    sids0, free0 = sorted(eng.free_sids), eng.blocks.n_free()
    # a summary alone
    _, (first,), _ = run(ie, [], summaries=1)
    n, amb = check_trace(ie, first, V)
    assert ops.nucleus_launches - launches0 == n == ie.summary_stats["nucleus_launches"]
    res = first.result
    assert json.loads(first.text) == {"summary": res["summary"]} and isinstance(res["summary"], str)
    assert res["chars"] == len(res["summary"]) <= 48 and not res["truncated"] and res["cached_prefix_tokens"] == 0
    assert sorted(eng.free_sids) == sids0 and not eng.seqs and eng.blocks.n_free() == free0

    # the same parses with a summary sharing their iterations and a probe on the way
    shared, (second,), (probe,) = run(ie, TEXTS, summaries=1, probe_at={1: ["scroll down"]})
    assert [r.text for r in shared] == [r.text for r in alone], "a summary changed a greedy answer"
    assert all(safe_parse(ParseResponse, json.loads(r.text)).success for r in shared)
    m, a2 = check_trace(ie, second, V)
    assert second.result["cached_prefix_tokens"] > 0, "the summary head is cached, too"
    both = [tr for tr in ie.last_summary_trace if tr["request"] is second and tr["rows"] > 1]
    assert both and all(tr["row"] == tr["rows"] - 1 for tr in both), "summary rows come after the parse rows"
    (tr,) = ie.last_turn_trace
    row = tr["logits"].numpy()
    lp, A = to.reference(row[None], V, tr["set"].numpy())
    out = tr["out"].numpy().astype(np.float64)
    assert abs(out[0] - lp[0]) <= to.lp_bound(V, A[0], lp[0]) and abs(out[1] - A[0]) <= to.lse_bound(V, A[0])
    assert probe.result["p_end"] > 0.0

    # the two heads: the next parse finds the parse head where it was
    ie.parse({"text": "scroll down", "context": {}})
    assert ie.last_stats["cached_prefix_tokens"] == cached_before > 900
    assert eng.stats["graph_replays"] > 0
    assert sorted(eng.free_sids) == sids0 and not eng.seqs and eng.blocks.n_free() == free0
    print(f"MEASURED summary ({flags}) steps {n + m} ambiguous rows {amb + a2} "
          f"mean n_kept {ie.summary_stats['n_kept_sum'] / max(1, ie.summary_stats['summary_tokens']):.3g}")

