"""Brain ``POST /summarize``: 200 with the engine's dict, 400 for a bad body, 501 for an engine without
``summary_async`` (the keyword engine), 500 for an engine error; ``/metrics`` counts summaries, their
tokens and the mean n_kept; ``/parse`` and ``/health`` unaffected."""
import asyncio
from concurrent.futures import Future

from aiohttp.test_utils import TestClient, TestServer

from voice_enabled_browser_automation_amd.brain import server as brain_server
from voice_enabled_browser_automation_amd.brain.intent_engine import FakeIntentEngine, keyword_intents
from voice_enabled_browser_automation_amd.brain.server import build_app

KEYS = {"summary", "chars", "prompt_tokens", "cached_prefix_tokens", "page_tokens", "truncated", "decode_steps", "ms"}
ANSWER = {"summary": "A shop page with earbuds on sale.", "chars": 33, "prompt_tokens": 410, "cached_prefix_tokens": 64,
          "page_tokens": 320, "truncated": False, "decode_steps": 9, "ms": 41.5}


class SummaryEngine(FakeIntentEngine):
    """The keyword engine plus a scripted ``summary_async``."""

    def __init__(self, answer=None, fail=None):
        super().__init__(fn=keyword_intents)
        self.answer, self.summary_fail, self.summary_calls = answer or ANSWER, fail, []
        self.summary_stats = dict(summaries=0, summary_tokens=0, n_kept_sum=0, nucleus_launches=0)

    def summary_async(self, text, title=None, url=None, **kw):
        self.summary_calls.append((text, title, url, kw))
        fut: Future = Future()
        if self.summary_fail is not None:
            fut.set_exception(self.summary_fail)
        else:
            self.summary_stats["summaries"] += 1
            self.summary_stats["summary_tokens"] += 9
            self.summary_stats["n_kept_sum"] += 270
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


def test_summarize_answers_with_the_engines_dict():
    eng = SummaryEngine()
    st, j = call(eng, "POST", "/summarize", {"text": "Earbuds on sale.", "title": "Shop", "url": "https://shop.example"})
    assert (st, j) == (200, ANSWER) and set(j) == KEYS
    assert eng.summary_calls == [("Earbuds on sale.", "Shop", "https://shop.example", {})]
    assert call(eng, "POST", "/summarize", {"text": "Earbuds.", "max_chars": 120})[0] == 200
    assert eng.summary_calls[-1] == ("Earbuds.", None, None, {"max_chars": 120})


def test_summarize_rejects_a_bad_body():
    eng = SummaryEngine()
    for body in ({}, {"text": ""}, {"text": "  \n "}, {"text": 5}, {"text": None}, {"text": ["page"]}, [1], "page",
                 {"title": "no text"}, {"text": "page", "title": 3}, {"text": "page", "url": ["x"]},
                 {"text": "page", "max_chars": 0}, {"text": "page", "max_chars": 15}, {"text": "page", "max_chars": 4097},
                 {"text": "page", "max_chars": "100"}, {"text": "page", "max_chars": 100.5},
                 {"text": "page", "max_chars": True}):
        st, j = call(eng, "POST", "/summarize", body)
        assert st == 400 and j["error"] == "invalid_request" and j["detail"], body
    st, j = call(eng, "POST", "/summarize", data=b"{not json")
    assert st == 400 and j["error"] == "invalid_request"
    assert eng.summary_calls == [], "an empty page never reaches the engine"
    assert (brain_server.SUMMARY_MIN_CHARS, brain_server.SUMMARY_MAX_CHARS) == (16, 4096)


def test_summarize_is_unsupported_by_the_keyword_engine():
    for eng in (FakeIntentEngine(fn=keyword_intents), FakeIntentEngine({})):
        assert call(eng, "POST", "/summarize", {"text": "a page"}) == (501, {"error": "summarize_unsupported"})
    assert call(FakeIntentEngine({}), "POST", "/summarize", {"text": ""})[0] == 400  # a bad body is still a bad body


def test_summarize_reports_an_engine_error_as_parse_does():
    st, j = call(SummaryEngine(fail=RuntimeError("kv cache exhausted")), "POST", "/summarize", {"text": "a page"})
    assert (st, j) == (500, {"error": "llm_error", "detail": "kv cache exhausted"})

    class Raises(SummaryEngine):
        def summary_async(self, text, title=None, url=None, **kw):
            raise ValueError("boom")

    assert call(Raises(), "POST", "/summarize", {"text": "a page"}) == (500, {"error": "llm_error", "detail": "boom"})


def test_metrics_count_summaries_tokens_and_the_mean_n_kept():
    async def fn(app, c):
        before = await (await c.get("/metrics")).json()
        async with app["lock"]:  # a serial engine's /parse in flight: /summarize does not wait for it
            for _ in range(2):
                r = await asyncio.wait_for(c.post("/summarize", json={"text": "a page"}), 10)
                assert r.status == 200
        await c.post("/summarize", json={"text": ""})
        assert (await c.post("/parse", json={"text": "scroll down"})).status == 200
        return before, await (await c.get("/metrics")).json()

    before, snap = session(SummaryEngine(), fn)
    assert (before["summaries"], before["summary_tokens"], before["summary_mean_n_kept"]) == (0, 0, 0.0)
    assert (snap["summaries"], snap["summary_tokens"], snap["summary_mean_n_kept"]) == (2, 18, 30.0)
    assert snap["counters"]["summarize_ok"] == 2 and snap["counters"]["ok"] == 1 and "summarize_ms" in str(snap)
    plain = session(FakeIntentEngine(fn=keyword_intents), lambda app, c: _metrics(c))
    assert "summaries" not in plain


async def _metrics(c):
    return await (await c.get("/metrics")).json()


def test_parse_and_health_are_unaffected():
    eng = SummaryEngine()
    assert call(eng, "GET", "/health") == (200, {"status": "ok", "service": "brain-ts"})
    plain = FakeIntentEngine(fn=keyword_intents)
    for body in ({"text": "scroll down"}, {"text": "summarize this page"}, {"text": ""}, {}):
        assert call(eng, "POST", "/parse", body) == call(plain, "POST", "/parse", body), body
    assert eng.summary_calls == []


def test_the_summary_defaults_come_from_the_settings(monkeypatch):
    class E:
        class engine:
            max_model_len = 4096

    assert brain_server.summary_defaults_from_env(E()).summary_defaults == \
        dict(max_chars=400, temperature=0.7, top_p=0.9, top_k=50, penalty=1.1)
    monkeypatch.setenv("VWA_SUMMARY_TOP_K", "20")
    monkeypatch.setenv("VWA_SUMMARY_MAX_CHARS", "300")
    E.engine.max_model_len = 1024  # GPT-2's window: the default length is lowered to fit
    d = brain_server.summary_defaults_from_env(E()).summary_defaults
    assert d["top_k"] == 20 and d["max_chars"] == 124


def test_summarize_through_the_llm_engine_on_cpu():
    from voice_enabled_browser_automation_amd.brain.intent_engine import LLMIntentEngine
    from voice_enabled_browser_automation_amd.models.config import LLAMA_PRESETS
    from voice_enabled_browser_automation_amd.models.llama import LlamaModel
    from voice_enabled_browser_automation_amd.runtime.engine import LLMEngine
    from voice_enabled_browser_automation_amd.tokenizer import load_tokenizer

    eng = LLMEngine(LlamaModel(LLAMA_PRESETS["llama-tiny"], device="cpu", seed=1), max_seqs=4, max_model_len=2048,
                    kv_blocks=800)
    ie = LLMIntentEngine(eng, load_tokenizer("llama3"), budget_chars=160)

    async def fn(_app, c):
        a = await c.post("/summarize", json={"text": "Earbuds are on sale this week. " * 8, "title": "Shop",
                                             "max_chars": 48})
        p = await c.post("/parse", json={"text": "scroll down"})
        big = await c.post("/summarize", json={"text": "page", "max_chars": 4096})  # no room in a 2048-token window
        m = await (await c.get("/metrics")).json()
        return a.status, await a.json(), p.status, big.status, (await big.json())["error"], m

    st, a, parse_status, big_status, big_error, m = session(ie, fn)
    assert st == 200 and set(a) == KEYS and isinstance(a["summary"], str) and a["chars"] == len(a["summary"]) <= 48
    assert parse_status == 200 and (big_status, big_error) == (500, "llm_error")
    assert m["summaries"] == 1 and m["summary_tokens"] == a["decode_steps"] and 1 <= m["summary_mean_n_kept"] <= 50
    assert not eng.seqs
