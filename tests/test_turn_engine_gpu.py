"""Turn probes through LLMIntentEngine on the GPU (llama-tiny with random-init weights, strict native
mode, captured step graphs): alone and concurrent with three parse requests, with the engine's
defaults and with the masked LM head, the zero-copy buffers and the spin wait all off.  Every probe
is held to the f64 oracle of tests/turn_oracle.py on its traced logits row; the traced row is
bit-equal, on every vocabulary column, to the unmasked LM head of the same step (so no vocab tile
of a probe's row was skipped); every parse is schema-valid; no sequence or KV block leaks."""
import json
import math

import numpy as np
import pytest
import torch

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


@pytest.fixture(scope="module")
def model():
    ops.ext()
    ops.turn_ext()  # fail loudly if a library is missing
    return LlamaModel(LLAMA_PRESETS["llama-tiny"], device="cuda", seed=1)


def drive(ie, eng, reqs, probe_at=None):
    """Step until ``reqs`` and the probes submitted on the way (``probe_at``: iteration -> texts)
    are done.  After every step that retired probes, their traced rows are compared, bit for bit,
    with the unmasked LM head of that step's hidden rows.  Returns (probes, largest error / bound)."""
    probes, it, seen, worst = [r for r in reqs if r.kind == "turn"], 0, len(ie.last_turn_trace), 0.0
    V = eng.model.cfg.vocab_size
    probe_at = probe_at or {}
    while not all(r.done for r in reqs) or not all(p.done for p in probes) or it <= max(probe_at, default=-1):
        for text in probe_at.get(it, ()):
            probes.append(ie.submit_turn(text))
        ie.step()
        it += 1
        assert it < 2000
        new = ie.last_turn_trace[seen:]
        seen += len(new)
        if not new:
            continue
        full = eng.head_logits(col_mask=None).float().cpu()
        for tr in new:
            row = tr["logits"]
            assert row.shape[0] >= V and torch.equal(full[tr["row"], :V].view(torch.int32), row[:V].view(torch.int32)), \
                f"probe {tr['text']!r} (logits row {tr['row']}): its row differs from the unmasked LM head's"
            lp, A = to.reference(row.numpy()[None], V, tr["set"].numpy())
            out = tr["out"].numpy().astype(np.float64)
            e_lp, b_lp = abs(out[0] - lp[0]), to.lp_bound(V, A[0], lp[0])
            e_A, b_A = abs(out[1] - A[0]), to.lse_bound(V, A[0])
            assert e_lp <= b_lp and e_A <= b_A, (tr["text"], out, lp, A)
            worst = max(worst, e_lp / b_lp, e_A / b_A)
    for r in list(reqs) + probes:
        if r.error is not None:
            raise r.error
    return probes, worst


@pytest.mark.parametrize("flags", ["defaults", "all_off"])
def test_probes_alone_and_among_parses(model, flags, monkeypatch):
    if flags == "all_off":
        for k in OFF:
            monkeypatch.setenv(k, "0")
    eng = LLMEngine(model, max_seqs=8, max_model_len=2048)
    ie = LLMIntentEngine(eng, load_tokenizer("llama3"), budget_chars=200, temperature=0.1, seed=7)
    assert (ie.masked_head, ie.zero_copy, ie.spin_wait) == ((True,) * 3 if flags == "defaults" else (False,) * 3)
    assert eng.use_graphs
    ie.keep_turn_trace = True
    sids0, free0 = sorted(eng.free_sids), eng.blocks.n_free()

    # alone: probe-only iterations, no sampler launch
    alone = [ie.submit_turn("search for."), ie.submit_turn("scroll down")]
    _, worst = drive(ie, eng, alone)
    third, w = drive(ie, eng, [ie.submit_turn("scroll down")])
    worst = max(worst, w)
    assert int(ie.d_step.item()) == 0 and ie.batch_stats["sampled"] == 0 and ie.batch_stats["probes"] == 3
    assert third[0].result["cached_prefix_tokens"] > 900
    for p in alone + third:
        assert 0.0 < p.result["p_end"] <= 1.0 and p.result["p_end"] == math.exp(p.result["logprob"])
    assert sorted(eng.free_sids) == sids0 and not eng.seqs and eng.blocks.n_free() == free0

    # among three parses: with them at admission, and while they decode
    parses = [ie.submit(messages_for({"text": t, "context": {}}))
              for t in ("search wireless earbuds", "open the second result", "go back")]
    first = [ie.submit_turn("open the"), ie.submit_turn("go back")]
    probes, w = drive(ie, eng, parses + first, {2: ["search wireless"], 5: ["scroll", "scroll down"], 6: ["go"]})
    worst = max(worst, w)
    assert len(probes) == 6 and ie.batch_stats["probes"] == 9 and len(ie.last_turn_trace) == 9
    assert sorted(tr["row"] for tr in ie.last_turn_trace[3:5]) == [3, 4], "probe rows come after the sampled rows"
    for r in parses:
        assert safe_parse(ParseResponse, json.loads(r.text)).success
    assert eng.stats["graph_replays"] > 0
    assert sorted(eng.free_sids) == sids0 and not eng.seqs and eng.blocks.n_free() == free0
    print(f"MEASURED turn probes ({flags}) err/bound {worst:.6g}")
