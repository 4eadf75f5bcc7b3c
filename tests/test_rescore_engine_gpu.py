"""N-best rescoring through LLMIntentEngine on the GPU (llama-tiny with random-init weights, strict
native mode, captured step graphs): alone, in pieces, and beside three parse requests, with the engine's
defaults and with the masked LM head, the zero-copy buffers and the spin wait all off.  Every traced
ops.seq_logprob call is held to the f64 oracle of tests/rescore_oracle.py and to the definition
(rescore_oracle.check_call); the traced rows are bit-equal, on every vocabulary column, to the unmasked
LM head of the same step (so no vocab tile of a scored row was skipped); every parse is schema-valid;
no sequence, KV block or running-sum slot leaks."""
import json

import pytest
import torch

import rescore_oracle as ro
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
ALTS = ["sort by price", "sore by price.", "sort by", " sort by price ", ""]


@pytest.fixture(scope="module")
def model():
    ops.ext()
    ops.rescore_ext()  # fail loudly if a library is missing
    return LlamaModel(LLAMA_PRESETS["llama-tiny"], device="cuda", seed=1)


def drive(ie, eng, reqs):
    """Step until ``reqs`` are done.  After every step that scored rows, the traced rows are compared,
    bit for bit, with the unmasked LM head of that step's hidden rows."""
    it, seen = 0, len(ie.last_rescore_trace)
    V = eng.model.cfg.vocab_size
    while not all(r.done for r in reqs):
        ie.step()
        it += 1
        assert it < 2000
        new = ie.last_rescore_trace[seen:]
        seen += len(new)
        if not new:
            continue
        full = eng.head_logits(col_mask=None).float().cpu()
        for tr in new:
            assert tr["logits"].shape[1] >= V and torch.equal(full[tr["rows"], :V].view(torch.int32),
                                                              tr["logits"][:, :V].view(torch.int32)), \
                f"{tr['texts']} (logits rows {tr['rows']}): the rows differ from the unmasked LM head's"
    for r in reqs:
        if r.error is not None:
            raise r.error


@pytest.mark.parametrize("flags", ["defaults", "all_off"])
def test_rescore_alone_in_pieces_and_among_parses(model, flags, monkeypatch):
    if flags == "all_off":
        for k in OFF:
            monkeypatch.setenv(k, "0")
    eng = LLMEngine(model, max_seqs=8, max_model_len=2048)
    ie = LLMIntentEngine(eng, load_tokenizer("llama3"), budget_chars=200, temperature=0.1, seed=7)
    assert (ie.masked_head, ie.zero_copy, ie.spin_wait) == ((True,) * 3 if flags == "defaults" else (False,) * 3)
    assert eng.use_graphs
    ie.keep_rescore_trace = True
    sids0, free0 = sorted(eng.free_sids), eng.blocks.n_free()
    launches = ops.seq_logprob_launches

    # alone: no sampler launch, one seq_logprob call per iteration with scored rows
    a = ie.submit_rescore(ALTS)
    drive(ie, eng, [a])
    ro.check_call(ie, ALTS, a.result, ie.last_rescore_trace)
    assert a.result["cached_prefix_tokens"] == 0 and a.result["scores"][0] == a.result["scores"][3]
    assert ops.seq_logprob_launches - launches == len(ie.last_rescore_trace) == 1
    b = ie.submit_rescore(ALTS[:2])
    n0 = len(ie.last_rescore_trace)
    drive(ie, eng, [b])
    ro.check_call(ie, ALTS[:2], b.result, ie.last_rescore_trace[n0:])
    assert b.result["cached_prefix_tokens"] > 900
    n0 = len(ie.last_rescore_trace)
    one = ie.rescore(["scroll down"])
    ro.check_call(ie, ["scroll down"], one, ie.last_rescore_trace[n0:])
    assert one["scored_tokens"] == [1] and ie.last_rescore_trace[-1]["target"].tolist() == [-1]
    assert int(ie.d_step.item()) == 0 and ie.batch_stats["sampled"] == 0 and ie.batch_stats["rescores"] == 3
    assert sorted(eng.free_sids) == sids0 and not eng.seqs and eng.blocks.n_free() == free0

    # in pieces: a row budget below the feeds
    ie.max_rows = 3
    texts = ["open the second result in a new tab", "open the second result in a new tap", "open"]
    n0 = len(ie.last_rescore_trace)
    c = ie.submit_rescore(texts)
    drive(ie, eng, [c])
    ie.max_rows = eng.bufs.max_rows
    assert len(ie.last_rescore_trace) - n0 > 2 and all(len(tr["rows"]) <= 3 for tr in ie.last_rescore_trace[n0:])
    ro.check_call(ie, texts, c.result, ie.last_rescore_trace[n0:])

    # among three parses: with them at admission
    parses = [ie.submit(messages_for({"text": t, "context": {}}))
              for t in ("search wireless earbuds", "open the second result", "go back")]
    n0 = len(ie.last_rescore_trace)
    d = ie.submit_rescore(["go back", "go bag", "go back"])
    drive(ie, eng, parses + [d])
    mine = ie.last_rescore_trace[n0:]
    ro.check_call(ie, ["go back", "go bag", "go back"], d.result, mine)
    assert all(tr["rows"][0] >= 3 for tr in mine), "scored rows come after the sampled rows"
    for r in parses:
        assert safe_parse(ParseResponse, json.loads(r.text)).success
    assert eng.stats["graph_replays"] > 0
    assert sorted(eng.free_sids) == sids0 and not eng.seqs and eng.blocks.n_free() == free0
    assert sorted(ie._score_free) == list(range(ops.RESCORE_MAX_SEQ)) and not ie.active and not ie.waiting
