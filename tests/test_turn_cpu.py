"""The turn-completion probe below the services, on the CPU: the reference op against the f64
oracle, the end set, the probe's prompt, and LLMIntentEngine.turn() on llama-tiny -- the traced
logits row against the oracle, the prefix cache, no leaked sequence or KV block, probe-only
iterations, and the traps of step(): mask rows, sampler rows, chain recovery."""
import json
import math

import numpy as np
import pytest
import torch

import turn_oracle as to
from voice_enabled_browser_automation_amd.brain import intent_engine as ie_mod
from voice_enabled_browser_automation_amd.brain.intent_engine import FakeIntentEngine, LLMIntentEngine
from voice_enabled_browser_automation_amd.brain.prompt import llama3_chat, messages_for, plain_chat, turn_tail, turn_text
from voice_enabled_browser_automation_amd.brain.tp_engine import TPIntentEngine
from voice_enabled_browser_automation_amd.contracts import ParseResponse, safe_parse
from voice_enabled_browser_automation_amd.models.config import LLAMA_PRESETS
from voice_enabled_browser_automation_amd.models.llama import LlamaModel
from voice_enabled_browser_automation_amd.runtime.engine import LLMEngine
from voice_enabled_browser_automation_amd.tokenizer import load_tokenizer


# ----------------------------------------------------------------------------- the op
@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "per_row"])
@pytest.mark.parametrize("vocab,rows", [(1, 1), (31, 3), (33, 8), (257, 8)])
def test_the_reference_op_matches_the_oracle(vocab, rows, per_row):
    for ld in (vocab, vocab + 3):
        for shift in range(len(to.ROLES)):
            case = to.make_case(rows, vocab, ld, per_row, seed=100 * vocab + shift, shift=shift)
            to.check(case, to.launch(case, "cpu"), f"V={vocab} ld={ld} shift={shift}")


# ----------------------------------------------------------------------------- the end set
@pytest.mark.parametrize("kind", ["llama3", "gpt2"])
def test_the_end_set_holds_the_ids_that_close_a_string(kind):
    tok = load_tokenizer(kind)
    ids = ie_mod.end_set_ids(tok)
    tb = tok.token_bytes()
    assert ids and len(set(ids)) == len(ids)
    assert not set(ids) & tok.special_ids
    assert all(tb[i].startswith(b'"') for i in ids)
    assert set(ids) == {i for i, b in enumerate(tb) if b.startswith(b'"')}  # and every such id
    assert tok.encode('"')[0] in ids


# ----------------------------------------------------------------------------- the prompt
TEXTS = ['search for', 'say "hello" to him', 'path C:\\temp\\x', 'café zoë 日本語', 'scroll down.', 'go back?!  ',
         '  open the second result …', 'wait, ', 'a', 'type "quoted\\"']


@pytest.mark.parametrize("fmt", [llama3_chat, plain_chat], ids=["llama3", "plain"])
@pytest.mark.parametrize("text", TEXTS)
def test_turn_tail_is_a_prefix_of_the_parse_tail(text, fmt):
    t = turn_text(text)
    assert t == t.strip() and t and t[-1] not in ".?!,;:…"
    head, tail = turn_tail(text, fmt)
    for context in ({}, {"url": "https://example.com", "last_intents": []}):
        p_head, p_tail = fmt(messages_for({"text": t, "context": context}))
        assert head == p_head, "one cached prefix serves /parse and the probe"
        assert p_tail.startswith(tail) and len(tail) < len(p_tail)
        assert p_tail[len(tail)] == '"', "the cut is right before the quote that closes the text"
    # the cut is inside the string: what it holds after {"text":" decodes to t once it is closed
    inner = tail[tail.rindex('{"text":') + len('{"text":'):]
    assert json.loads(inner + '"') == t


def test_turn_text_strips_only_the_end():
    assert turn_text("  search for.  ") == "search for"
    assert turn_text("scroll down . ?!") == "scroll down"
    assert turn_text("e.g. this, that") == "e.g. this, that"
    assert turn_text("…") == ""


# ----------------------------------------------------------------------------- the engine
@pytest.fixture(scope="module")
def model():
    return LlamaModel(LLAMA_PRESETS["llama-tiny"], device="cpu", seed=1)


def make(model, **kw):
    eng = LLMEngine(model, max_seqs=8, max_model_len=2048, kv_blocks=1200)
    ie = LLMIntentEngine(eng, load_tokenizer("llama3"), budget_chars=160, temperature=0.0, **kw)
    ie.keep_turn_trace = True
    return eng, ie


def assert_trace_matches_oracle(ie, tr, got=None):
    row = tr["logits"].numpy()
    V = row.shape[0]
    lp, A = to.reference(row[None], V, tr["set"].numpy())
    out = tr["out"].numpy().astype(np.float64)
    assert abs(out[0] - lp[0]) <= to.lp_bound(V, A[0], lp[0]) and abs(out[1] - A[0]) <= to.lse_bound(V, A[0])
    if got is not None:
        assert got["logprob"] == float(tr["out"][0]) and got["p_end"] == math.exp(got["logprob"])
        assert 0.0 < got["p_end"] <= 1.0 and got["prompt_tokens"] == len(tr["ids"])
    # the set the kernel read is the end set, packed to the model's vocabulary
    on = np.flatnonzero(to.allowed(tr["set"].numpy()[0], tr["set"].shape[1] * 32))
    assert on.tolist() == ie.end_set_ids() and tr["set"].shape[1] * 32 >= V


def test_turn_equals_the_oracle_is_prefix_cached_and_leaks_nothing(model):
    eng, ie = make(model)
    sids0, free0 = sorted(eng.free_sids), eng.blocks.n_free()
    a = ie.turn("search for.")
    assert set(a) == {"p_end", "logprob", "prompt_tokens", "cached_prefix_tokens", "ms"}
    assert a["cached_prefix_tokens"] == 0 and a["ms"] > 0
    step0, sampled0 = int(ie.d_step), ie.batch_stats["sampled"]
    b = ie.turn("scroll down")
    assert b["cached_prefix_tokens"] > 900 and b["prompt_tokens"] - b["cached_prefix_tokens"] < 40
    assert len(ie.last_turn_trace) == 2
    for got, tr in zip((a, b), ie.last_turn_trace):
        assert_trace_matches_oracle(ie, tr, got)
    assert ie.last_turn_trace[0]["text"] == "search for." and ie.last_turn_trace[0]["ids"] == \
        ie.tok.encode("".join(turn_tail("search for", llama3_chat)))
    # a probe-only iteration launches no sampler
    assert (int(ie.d_step), ie.batch_stats["sampled"]) == (step0, sampled0) == (0, 0)
    assert ie.batch_stats["probes"] == 2 and not ie.active and not ie.waiting
    # every sequence id and KV block is back (the published head's blocks stay evictable: free)
    assert sorted(eng.free_sids) == sids0 and not eng.seqs and eng.blocks.n_free() == free0
    # the probe's prefix serves /parse and the other way round
    out = ie.parse({"text": "scroll down", "context": {}})
    assert safe_parse(ParseResponse, out).success and ie.last_stats["cached_prefix_tokens"] > 900
    assert ie.turn("scroll down")["logprob"] == b["logprob"]
    assert sorted(eng.free_sids) == sids0 and eng.blocks.n_free() == free0


def test_the_trace_is_off_by_default(model):
    eng = LLMEngine(model, max_seqs=2, max_model_len=2048, kv_blocks=400)
    ie = LLMIntentEngine(eng, load_tokenizer("llama3"), budget_chars=160)
    assert ie.keep_turn_trace is False
    ie.turn("go back")
    assert ie.last_turn_trace == []
    assert ie.batch_stats["probes"] == 1


TEXTS4 = ["search wireless earbuds", "open the second result", "scroll down", "go back"]


def run_interleaved(ie, probe_at):
    """Four greedy parses; probes are submitted with them (iteration 0) and at the iterations of
    ``probe_at`` while they decode.  Returns (answers, probe requests, per-iteration records)."""
    reqs = [ie.submit(messages_for({"text": t, "context": {}})) for t in TEXTS4]
    probes, it = [], 0
    while not all(r.done for r in reqs) or not all(p.done for p in probes):
        for text in probe_at.get(it, ()):
            probes.append(ie.submit_turn(text))
        ie.step()
        it += 1
    for r in reqs + probes:
        if r.error is not None:
            raise r.error
    return [r.text for r in reqs], probes


def test_parses_with_probes_interleaved_equal_the_parses_without(model):
    _, plain = make(model)
    want, _ = run_interleaved(plain, {})
    assert plain.batch_stats["iterations"] > 7, "the last probe below would find the parses done"
    eng, ie = make(model)
    seen = []
    head_logits = eng.head_logits

    def spy(col_mask=None, mask_rows=1, gather=True):
        seen.append((None if col_mask is None else col_mask[:mask_rows].clone(), mask_rows, eng._head_rows.shape[0]))
        return head_logits(col_mask=col_mask, mask_rows=mask_rows, gather=gather)

    eng.head_logits = spy
    ie.masked_head = True
    got, probes = run_interleaved(ie, {0: ["search for", "scroll down"], 3: ["open the"], 4: ["go back.", "go"],
                                       7: ["search wireless"]})
    assert got == want, "a probe changed a greedy answer"
    assert all(safe_parse(ParseResponse, json.loads(t)).success for t in got)
    # the sampler ran as often, and drew as many rows, as it would have without the probes
    assert int(ie.d_step) == int(plain.d_step) and ie.batch_stats["sampled"] == plain.batch_stats["sampled"]
    assert ie.batch_stats["iterations"] == plain.batch_stats["iterations"]
    assert len(probes) == 6 == len(ie.last_turn_trace) == ie.batch_stats["probes"]
    for p, tr in zip(probes, ie.last_turn_trace):
        assert_trace_matches_oracle(ie, tr, p.result)
    # every LM head call covered all its rows with mask rows, and the probes' rows -- the last
    # ones, after the sampled rows -- were all ones: no vocab tile of theirs may be skipped
    assert all(m is not None and rows == total == m.shape[0] for m, rows, total in seen)
    with_probes = [(m, total) for m, _, total in seen if (m == -1).all(1).any()]
    assert len(with_probes) == 4
    for (m, total), k in zip(with_probes, (2, 1, 2, 1)):
        ones = (m == -1).all(1)
        assert ones.tolist() == [False] * (total - k) + [True] * k
    assert sorted(r["row"] for r in ie.last_turn_trace[:2]) == [4, 5]
    assert not eng.seqs and len(eng.free_sids) == 8


def test_a_failed_chained_step_recomputes_the_probe_from_the_rerun_logits(model):
    eng, ie = make(model)
    ie.turn("warm the prefix cache")
    ie.last_turn_trace.clear()
    bump = torch.zeros(eng.bufs.logits_local.shape[1])
    bump[ie.end_set_ids()] = 3.0
    calls = []
    eng.step_fail_word = lambda: torch.ones(1, dtype=torch.int64) if not calls else None

    def recover():
        calls.append(1)
        return eng.head_logits() + bump  # "the re-run step's logits": not the ones the first launch read

    eng.recover_step = recover
    req = ie.submit(messages_for({"text": "go back", "context": {}}))
    probe = ie.submit_turn("go back")
    first = None
    while not (req.done and probe.done):
        ie.step()
        first = first if first is not None else eng.head_logits()[1].clone()
    assert calls == [1] and req.error is None and probe.error is None
    tr = ie.last_turn_trace[0]
    assert tr["row"] == 1 and torch.equal(tr["logits"], first + bump)
    assert_trace_matches_oracle(ie, tr, probe.result)
    assert safe_parse(ParseResponse, json.loads(req.text)).success


def test_background_scheduler_serves_turn_async(model):
    eng, ie = make(model)
    ie.start()
    try:
        futs = [ie.turn_async(t) for t in ("search for", "scroll down")]
        parse = ie.submit_async(messages_for({"text": "go back", "context": {}}))
        res = [f.result(timeout=300) for f in futs]
        assert all(0.0 < r["p_end"] <= 1.0 for r in res)
        assert safe_parse(ParseResponse, json.loads(parse.result(timeout=300))).success
        assert ie.turn("go")["prompt_tokens"] > 900  # turn() goes through the running scheduler
    finally:
        ie.stop()
    assert not eng.seqs


def test_only_the_llm_engine_has_turn():
    for cls in (TPIntentEngine, FakeIntentEngine):
        for name in ("turn", "turn_async", "submit_turn"):
            assert not hasattr(cls, name), f"{cls.__name__}.{name}"
    fake = FakeIntentEngine(fn=ie_mod.keyword_intents)  # the keyword engine
    assert not hasattr(fake, "turn_async")
    for name in ("turn", "turn_async", "submit_turn"):
        assert callable(getattr(LLMIntentEngine, name))
