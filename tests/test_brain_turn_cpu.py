"""Brain ``POST /turn``: 200 with the engine's dict, 400 for a bad body, 501 for an engine without
``turn_async``, 500 for an engine error; no serial lock; ``/parse`` and ``/health`` unaffected."""
import asyncio
import math
from concurrent.futures import Future

from aiohttp.test_utils import TestClient, TestServer

from voice_enabled_browser_automation_amd.brain.intent_engine import FakeIntentEngine, keyword_intents
from voice_enabled_browser_automation_amd.brain.server import build_app

ANSWER = {"p_end": 0.75, "logprob": math.log(0.75), "prompt_tokens": 1003, "cached_prefix_tokens": 976, "ms": 1.5}


class TurnEngine(FakeIntentEngine):
    """The keyword engine plus a scripted ``turn_async``."""

    def __init__(self, answer=None, fail=None):
        super().__init__(fn=keyword_intents)
        self.answer, self.turn_fail, self.turn_calls = answer or ANSWER, fail, []

    def turn_async(self, text):
        self.turn_calls.append(text)
        fut: Future = Future()
        if self.turn_fail is not None:
            fut.set_exception(self.turn_fail)
        else:
            fut.set_result(dict(self.answer))
        return fut


def session(engine, fn):
    async def go():
        app = build_app(engine)
        async with TestClient(TestServer(app)) as c:
            return await fn(app, c)

    return asyncio.run(go())


def call(engine, method, path, json=None, data=None):
    async def fn(_app, c):
        r = await c.request(method, path, json=json, data=data)
        return r.status, await r.json()

    return session(engine, fn)


def test_turn_answers_with_the_engines_dict():
    eng = TurnEngine()
    st, j = call(eng, "POST", "/turn", {"text": "search for", "context": {"url": "https://example.com"}})
    assert (st, j) == (200, ANSWER) and eng.turn_calls == ["search for"]
    assert call(eng, "POST", "/turn", {"text": "scroll down"})[0] == 200


def test_turn_rejects_a_bad_body():
    eng = TurnEngine()
    for body in ({}, {"text": ""}, {"text": "   "}, {"text": 5}, {"text": None}, {"text": ["go"]}, [1], "go",
                 {"context": {}}, {"text": "go", "context": "x"}):
        st, j = call(eng, "POST", "/turn", body)
        assert st == 400 and j["error"] == "invalid_request" and j["detail"], body
    st, j = call(eng, "POST", "/turn", data=b"{not json")
    assert st == 400 and j["error"] == "invalid_request"
    assert eng.turn_calls == []


def test_turn_is_unsupported_by_an_engine_without_it():
    for eng in (FakeIntentEngine(fn=keyword_intents), FakeIntentEngine({})):
        assert call(eng, "POST", "/turn", {"text": "go back"}) == (501, {"error": "turn_unsupported"})
    # a bad body is still a bad body
    assert call(FakeIntentEngine({}), "POST", "/turn", {"text": ""})[0] == 400


def test_turn_reports_an_engine_error_as_parse_does():
    st, j = call(TurnEngine(fail=RuntimeError("kv cache exhausted")), "POST", "/turn", {"text": "go back"})
    assert (st, j) == (500, {"error": "llm_error", "detail": "kv cache exhausted"})

    class Raises(TurnEngine):
        def turn_async(self, text):
            raise ValueError("boom")

    assert call(Raises(), "POST", "/turn", {"text": "go back"}) == (500, {"error": "llm_error", "detail": "boom"})


def test_a_log_probability_at_minus_infinity_stays_json():
    st, j = call(TurnEngine(answer=dict(ANSWER, p_end=0.0, logprob=-math.inf)), "POST", "/turn", {"text": "go"})
    assert st == 200 and j["p_end"] == 0.0 and j["logprob"] is None


def test_turn_does_not_wait_for_the_serial_lock_and_counts_in_metrics():
    async def fn(app, c):
        async with app["lock"]:  # a serial engine's /parse in flight
            r = await asyncio.wait_for(c.post("/turn", json={"text": "go back"}), 10)
            assert r.status == 200
        await c.post("/turn", json={"text": ""})
        assert (await c.post("/parse", json={"text": "scroll down"})).status == 200
        return await (await c.get("/metrics")).json()

    snap = session(TurnEngine(), fn)
    flat = str(snap)
    assert "turn_ok" in flat and "turn_ms" in flat
    assert snap["counters"]["turn_ok"] == 1 and snap["counters"]["ok"] == 1


def test_parse_and_health_are_unaffected():
    eng = TurnEngine()
    assert call(eng, "GET", "/health") == (200, {"status": "ok", "service": "brain-ts"})
    plain = FakeIntentEngine(fn=keyword_intents)
    for body in ({"text": "scroll down"}, {"text": "search for shoes", "context": {"url": "https://a.example"}},
                 {"text": ""}, {}):
        assert call(eng, "POST", "/parse", body) == call(plain, "POST", "/parse", body), body
    assert eng.turn_calls == []


def test_turn_through_the_llm_engine_on_cpu():
    from voice_enabled_browser_automation_amd.brain.intent_engine import LLMIntentEngine
    from voice_enabled_browser_automation_amd.models.config import LLAMA_PRESETS
    from voice_enabled_browser_automation_amd.models.llama import LlamaModel
    from voice_enabled_browser_automation_amd.runtime.engine import LLMEngine
    from voice_enabled_browser_automation_amd.tokenizer import load_tokenizer

    eng = LLMEngine(LlamaModel(LLAMA_PRESETS["llama-tiny"], device="cpu", seed=1), max_seqs=4, max_model_len=2048,
                    kv_blocks=800)
    ie = LLMIntentEngine(eng, load_tokenizer("llama3"), budget_chars=160)

    async def fn(_app, c):
        a = await (await c.post("/turn", json={"text": "search for."})).json()
        b = await (await c.post("/turn", json={"text": "search for"})).json()
        p = await c.post("/parse", json={"text": "scroll down"})
        return a, b, p.status

    a, b, parse_status = session(ie, fn)
    assert set(a) == {"p_end", "logprob", "prompt_tokens", "cached_prefix_tokens", "ms"}
    assert 0.0 < a["p_end"] <= 1.0 and a["logprob"] == b["logprob"]  # (the trailing period is stripped)
    assert b["cached_prefix_tokens"] > 900 and parse_status == 200
    assert not eng.seqs
