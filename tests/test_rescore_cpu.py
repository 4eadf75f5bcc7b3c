"""N-best rescoring below the services, on the CPU reference engine (llama-tiny):
LLMIntentEngine.rescore() against the definition -- every traced ops.seq_logprob call against the f64
oracle of tests/rescore_oracle.py, the targets against the alternatives' ids, the running sums as a
chain from zero, scores[i] the last acc_out of its sequence -- and the traps of step(): pieces of a
long feed, chain recovery, rows beside parse requests, iterations without scored rows."""
import json

import numpy as np
import pytest
import torch

import rescore_oracle as ro
from rescore_oracle import KEYS, check_call
from voice_enabled_browser_automation_amd import ops
from voice_enabled_browser_automation_amd.brain import intent_engine as ie_mod
from voice_enabled_browser_automation_amd.brain.intent_engine import (FakeIntentEngine, IntentEngineError,
                                                                      LLMIntentEngine)
from voice_enabled_browser_automation_amd.brain.prompt import messages_for, turn_text
from voice_enabled_browser_automation_amd.brain.tp_engine import TPIntentEngine
from voice_enabled_browser_automation_amd.contracts import ParseResponse, safe_parse
from voice_enabled_browser_automation_amd.models.config import LLAMA_PRESETS
from voice_enabled_browser_automation_amd.models.llama import LlamaModel
from voice_enabled_browser_automation_amd.runtime.engine import LLMEngine
from voice_enabled_browser_automation_amd.tokenizer import load_tokenizer

ALTS = ["sort by price", "sore by price.", "sort by", " sort by price ", "sort by price", ""]


@pytest.fixture(scope="module")
def model():
    return LlamaModel(LLAMA_PRESETS["llama-tiny"], device="cpu", seed=1)


def make(model, **kw):
    eng = LLMEngine(model, max_seqs=8, max_model_len=2048, kv_blocks=1200)
    ie = LLMIntentEngine(eng, load_tokenizer("llama3"), budget_chars=160, temperature=0.0, **kw)
    ie.keep_rescore_trace = True
    return eng, ie


def test_rescore_equals_the_definition_and_leaks_nothing(model):
    eng, ie = make(model)
    sids0, free0 = sorted(eng.free_sids), eng.blocks.n_free()
    calls = []
    real = ops.seq_logprob
    ie_mod.ops.seq_logprob = lambda *a, **k: calls.append(ie.batch_stats["iterations"]) or real(*a, **k)
    try:
        got = ie.rescore(ALTS)
        check_call(ie, ALTS, got, ie.last_rescore_trace)
        assert got["cached_prefix_tokens"] == 0 and got["ms"] > 0
        # duplicates are scored once and share the value: four distinct strings, four sequences
        assert got["scores"][0] == got["scores"][3] == got["scores"][4] and len(set(got["scores"])) == 4
        assert sorted(set(ie.last_rescore_trace[0]["texts"])) == sorted({turn_text(t) for t in ALTS})
        # "" is the common prefix itself: one row, the end-set term; "sort by" is a prefix of "sort by price"
        assert got["scored_tokens"][5] == 1 and got["prompt_tokens"][5] == got["common_prefix_tokens"]
        assert got["scored_tokens"][2] < got["scored_tokens"][0]
        # nothing was sampled, one call per iteration with scored rows
        assert int(ie.d_step) == 0 and ie.batch_stats["sampled"] == 0 and len(calls) == len(set(calls)) == 1
        assert ie.batch_stats["rescores"] == 1 and ie.batch_stats["rescore_rows"] == \
            sum(dict(zip(map(turn_text, ALTS), got["scored_tokens"])).values())
        assert ie.engine_stats()["rescores"] == 1 and ie.engine_stats()["rescore_rows"] == ie.batch_stats["rescore_rows"]
        assert sorted(eng.free_sids) == sids0 and not eng.seqs and eng.blocks.n_free() == free0
        assert sorted(ie._score_free) == list(range(ops.RESCORE_MAX_SEQ)) and not ie.active and not ie.waiting

        # K = 1: the end-set term only, which is what the turn probe answers; the head is cached now
        ie.last_rescore_trace.clear()
        one = ie.rescore(["scroll down."])
        check_call(ie, ["scroll down."], one, ie.last_rescore_trace)
        assert one["scored_tokens"] == [1] and one["cached_prefix_tokens"] > 900
        assert one["common_prefix_tokens"] == one["prompt_tokens"][0]
        n_calls = len(calls)
        turn = ie.turn("scroll down")
        # (the same row of the same forward through two ops: two f32 roundings of one value)
        assert abs(one["scores"][0] - turn["logprob"]) <= 4 * ro.U * abs(turn["logprob"])
        # an iteration without scored rows makes no seq_logprob call: the probe, then a parse
        out = ie.parse({"text": "scroll down", "context": {}})
        assert safe_parse(ParseResponse, out).success and len(calls) == n_calls
        assert sorted(eng.free_sids) == sids0 and eng.blocks.n_free() == free0
    finally:
        ie_mod.ops.seq_logprob = real


def test_a_long_feed_is_scored_in_pieces(model):
    texts = ["open the second result in a new tab", "open the second result in a new tap", "open"]
    _, plain = make(model)
    want = plain.rescore(texts)
    eng, ie = make(model)
    ie.max_rows = 3
    got = ie.rescore(texts)
    assert max(got["scored_tokens"]) > 6 and len(ie.last_rescore_trace) > len(plain.last_rescore_trace) + 2
    assert all(len(tr["rows"]) <= 3 for tr in ie.last_rescore_trace)
    check_call(ie, texts, got, ie.last_rescore_trace)
    for k in ("scored_tokens", "common_prefix_tokens", "prompt_tokens"):
        assert got[k] == want[k]
    # the same rows in other steps: the same sums up to the rows' own bounds
    for a, b, n in zip(got["scores"], want["scores"], got["scored_tokens"]):
        assert abs(a - b) <= 1e-3 * n
    assert not eng.seqs and not ie.active


TEXTS4 = ["search wireless earbuds", "open the second result", "scroll down", "go back"]


def run_beside(ie, rescore_at):
    reqs = [ie.submit(messages_for({"text": t, "context": {}})) for t in TEXTS4]
    jobs, it = [], 0
    while not all(r.done for r in reqs) or not all(j.done for j in jobs):
        if it in rescore_at:
            jobs.append(ie.submit_rescore(rescore_at[it]))
        ie.step()
        it += 1
    for r in reqs + jobs:
        if r.error is not None:
            raise r.error
    return [r.text for r in reqs], jobs


def test_parses_decoded_beside_a_rescore_equal_the_parses_without(model):
    _, plain = make(model)
    want, _ = run_beside(plain, {})
    eng, ie = make(model)
    seen = []
    head_logits = eng.head_logits

    def spy(col_mask=None, mask_rows=1, gather=True):
        seen.append((None if col_mask is None else col_mask[:mask_rows].clone(), mask_rows, eng._head_rows.shape[0]))
        return head_logits(col_mask=col_mask, mask_rows=mask_rows, gather=gather)

    eng.head_logits = spy
    ie.masked_head = True
    alts = {0: ["sort by price", "sore by price"], 3: ["go back", "go bag", "go back"]}
    got, jobs = run_beside(ie, alts)
    assert got == want, "a rescore changed a greedy answer"
    assert int(ie.d_step) == int(plain.d_step) and ie.batch_stats["sampled"] == plain.batch_stats["sampled"]
    assert ie.batch_stats["iterations"] == plain.batch_stats["iterations"]
    # the two calls' pieces, in order
    for job, at in zip(jobs, (0, 3)):
        mine = [tr for tr in ie.last_rescore_trace if set(tr["texts"]) & set(alts[at])]
        check_call(ie, alts[at], job.result, mine)
    # every LM head call covered all its rows with mask rows; the scored rows -- the last ones, after
    # the sampled rows -- were all ones, and they are the rows the trace names
    assert all(m is not None and rows == total == m.shape[0] for m, rows, total in seen)
    with_score = [(m, total) for m, _, total in seen if (m == -1).all(1).any()]
    assert len(with_score) == len(ie.last_rescore_trace)
    for (m, total), tr in zip(with_score, ie.last_rescore_trace):
        k = len(tr["rows"])
        assert (m == -1).all(1).tolist() == [False] * (total - k) + [True] * k
        assert tr["rows"] == list(range(total - k, total)) and total - k == 4
    assert not eng.seqs and len(eng.free_sids) == 8


def test_a_failed_chained_step_is_scored_again_from_the_same_sums(model):
    texts = ["go back", "go bag"]
    eng, ie = make(model)
    want = ie.rescore(texts)  # (and the prefix cache is warm)
    ie.last_rescore_trace.clear()
    bump = torch.zeros(eng.bufs.logits_local.shape[1])
    bump[ie.end_set_ids()] = 3.0
    calls = []
    eng.step_fail_word = lambda: torch.ones(1, dtype=torch.int64) if not calls else None

    def recover():
        calls.append(len(ie.last_rescore_trace))
        return eng.head_logits() + bump  # "the re-run step's logits": not the ones the first launch read

    eng.recover_step = recover
    req = ie.submit(messages_for({"text": "go back", "context": {}}))
    job = ie.submit_rescore(texts)
    first = None
    while not (req.done and job.done):
        ie.step()
        first = first if first is not None else eng.head_logits().clone()
    assert calls == [1] and req.error is None and job.error is None
    # the failed launch's record is gone; the one kept started from zero and read the re-run logits
    assert len(ie.last_rescore_trace) == 1
    check_call(ie, texts, job.result, ie.last_rescore_trace)
    assert float(ie.last_rescore_trace[0]["acc_in"].abs().sum()) == 0.0
    tr = ie.last_rescore_trace[0]
    assert tr["rows"][0] == 1 and torch.equal(tr["logits"], first[tr["rows"]] + bump)
    assert job.result["scores"] != want["scores"]
    assert safe_parse(ParseResponse, json.loads(req.text)).success
    assert not eng.seqs


def test_background_scheduler_serves_rescore_async(model):
    eng, ie = make(model)
    ie.start()
    try:
        fut = ie.rescore_async(["scroll down", "scroll town"])
        parse = ie.submit_async(messages_for({"text": "go back", "context": {}}))
        res = fut.result(timeout=300)
        assert set(res) == KEYS and len(res["scores"]) == 2
        assert safe_parse(ParseResponse, json.loads(parse.result(timeout=300))).success
        assert ie.rescore(["go"])["scored_tokens"] == [1]  # rescore() goes through the running scheduler
    finally:
        ie.stop()
    assert not eng.seqs


def test_bad_arguments_raise(model):
    _, ie = make(model)
    for bad in ([], ["a"] * 9, "scroll down", [1, 2], ["ok", None], None):
        with pytest.raises(IntentEngineError):
            ie.submit_rescore(bad)
    assert not ie.waiting


def test_only_the_llm_engine_has_rescore():
    for cls in (TPIntentEngine, FakeIntentEngine):
        for name in ("rescore", "rescore_async", "submit_rescore"):
            assert not hasattr(cls, name), f"{cls.__name__}.{name}"
    fake = FakeIntentEngine(fn=ie_mod.keyword_intents)  # the keyword engine
    assert not hasattr(fake, "rescore_async")
    for name in ("rescore", "rescore_async", "submit_rescore"):
        assert callable(getattr(LLMIntentEngine, name))
