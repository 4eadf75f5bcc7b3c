"""Keyterms on the wire: ``/stream?keyterm=...`` (repeated, ``:boost``, at most 100), the
``keyterms`` control frame, ``warn`` frames for bad input, factories that take no keyterms, the
``/metrics`` counter, and the DP router forwarding the query string to its worker."""
import asyncio
import json

import aiohttp
import pytest
from aiohttp import web
from aiohttp.test_utils import TestClient, TestServer

from voice_enabled_browser_automation_amd.voice import server as vs
from voice_enabled_browser_automation_amd.voice.router import build_router
from voice_enabled_browser_automation_amd.voice.server import build_app


def test_parsing_one_term():
    assert vs.parse_keyterm("Grafana", 2.0) == ("Grafana", 2.0)
    assert vs.parse_keyterm("pull request:3", 2.0) == ("pull request", 3.0)
    assert vs.parse_keyterm(" Browserbase : 0.5 ", 2.0) == ("Browserbase", 0.5)
    assert vs.parse_keyterm("C: drive", 2.0) == ("C: drive", 2.0)  # a colon inside the term
    assert vs.parse_keyterm({"term": "Grafana", "boost": 20}, 2.0) == ("Grafana", 20.0)
    # a trailing :number is always the boost; a term that ends that way names its boost after it,
    # and the {"term", "boost"} form takes the term literally
    assert vs.parse_keyterm("10:30:2", 1.0) == ("10:30", 2.0) and vs.parse_keyterm("route:66:0.5", 1.0) == ("route:66", 0.5)
    assert vs.parse_keyterm({"term": "10:30"}, 1.5) == ("10:30", 1.5)
    assert vs.parse_keyterm({"term": "route:66", "boost": 3}, 1.5) == ("route:66", 3.0)
    with pytest.raises(ValueError, match="route.*66"):
        vs.parse_keyterm("route:66", 1.0)
    assert vs.parse_keyterm("Grafana")[1] == vs.knob("VWA_ASR_KEYTERM_BOOST")
    for bad in ("", "  ", ":3", "x:0", "x:-1", "x:20.5", "x:nan", "x:inf", 7, None, {"boost": 2}, {"term": "x", "boost": "a"}):
        with pytest.raises(ValueError):
            vs.parse_keyterm(bad, 2.0)
    with pytest.raises(ValueError):
        vs.parse_keyterm("x", 25.0)


def test_parsing_a_list_keeps_what_is_usable():
    terms, warns = vs.parse_keyterms(["Grafana", "pull request:3", "Grafana", "", "x:99"], 2.0)
    assert terms == [("Grafana", 2.0), ("pull request", 3.0)] and len(warns) == 2
    terms, warns = vs.parse_keyterms([f"term{i}" for i in range(130)], 1.0)
    assert len(terms) == 100 and terms[-1] == ("term99", 1.0) and len(warns) == 1 and "100" in warns[0]


def test_default_terms_come_from_the_knob(monkeypatch):
    assert vs.default_keyterms() == []
    monkeypatch.setenv("VWA_ASR_KEYTERMS", "Grafana, pull request:3 ,")
    monkeypatch.setenv("VWA_ASR_KEYTERM_BOOST", "1.5")
    assert vs.default_keyterms() == [("Grafana", 1.5), ("pull request", 3.0)]
    monkeypatch.setenv("VWA_ASR_KEYTERMS", "x:99")
    with pytest.raises(ValueError):
        vs.default_keyterms()


class Session:
    """An ASR session double that records its keyterms and counts boosted passes."""

    made = []

    def __init__(self, keyterms=None):
        self.keyterms = keyterms
        self.stats = {"boosted_passes": 0}
        Session.made.append(self)

    def set_keyterms(self, terms):
        if any(t[0] == "untokenizable" for t in terms or []):
            raise ValueError("keyterm 'untokenizable': 17 tokens")
        self.keyterms = terms or None

    def push(self, data):
        if self.keyterms:
            self.stats["boosted_passes"] += 1
        return [{"type": "Results", "is_final": False, "channel": {"alternatives": [{"transcript": "x"}]}}]

    def flush(self):
        return []


async def _frames(ws, n, timeout=5.0):
    return [json.loads((await ws.receive(timeout=timeout)).data) for _ in range(n)]


def _app(factory):
    return build_app(factory, brain_url="http://127.0.0.1:9/parse", executor_url="http://127.0.0.1:9", debounce_ms=60000)


def test_query_terms_reach_the_factory_and_bad_ones_warn():
    async def go():
        Session.made.clear()
        async with TestClient(TestServer(_app(lambda keyterms=None: Session(keyterms)))) as c:
            ws = await c.ws_connect("/stream?keyterm=Grafana&keyterm=pull+request:3&keyterm=x:99&keyterm=")
            fr = await _frames(ws, 4)
            assert [f["type"] for f in fr] == ["info", "info", "warn", "warn"]
            assert all(f["payload"].startswith("keyterm: ") for f in fr[2:])
            assert Session.made[-1].keyterms == [("Grafana", vs.knob("VWA_ASR_KEYTERM_BOOST")), ("pull request", 3.0)]
            await ws.send_bytes(b"\0" * 320)
            assert (await _frames(ws, 1))[0]["type"] == "transcript_partial"  # the socket is still served
            snap = await (await c.get("/metrics")).json()
            assert snap["counters"]["asr_boosted_passes"] == 1 and snap["counters"]["keyterm_warnings"] == 2
            await ws.close()
            # more than 100 terms: the first hundred, and one warn
            ws = await c.ws_connect("/stream?" + "&".join(f"keyterm=t{i}" for i in range(120)))
            fr = await _frames(ws, 3)
            assert fr[2]["type"] == "warn" and "100" in fr[2]["payload"] and len(Session.made[-1].keyterms) == 100
            await ws.close()
            # no terms: the factory is called as before, and nothing is counted
            ws = await c.ws_connect("/stream")
            await _frames(ws, 2)
            assert Session.made[-1].keyterms is None
            await ws.send_bytes(b"\0" * 320)
            await _frames(ws, 1)
            snap = await (await c.get("/metrics")).json()
            assert snap["counters"]["asr_boosted_passes"] == 1
            await ws.close()

    asyncio.run(go())


def test_the_control_frame_replaces_the_set():
    async def go():
        Session.made.clear()
        async with TestClient(TestServer(_app(lambda keyterms=None: Session(keyterms)))) as c:
            ws = await c.ws_connect("/stream?keyterm=Grafana:1")
            await _frames(ws, 2)
            s = Session.made[-1]
            await ws.send_str(json.dumps({"type": "keyterms", "payload": {"terms": ["Browserbase", "click:4"], "boost": 1.5}}))
            await ws.send_bytes(b"\0" * 320)
            assert (await _frames(ws, 1))[0]["type"] == "transcript_partial"
            assert s.keyterms == [("Browserbase", 1.5), ("click", 4.0)]
            for payload in ({"terms": "Grafana"}, None, {"terms": ["ok"], "boost": 50}, {"terms": ["untokenizable"]},
                            {"terms": ["fine", 7]}):
                await ws.send_str(json.dumps({"type": "keyterms", "payload": payload}))
                fr = (await _frames(ws, 1))[0]
                assert fr["type"] == "warn" and fr["payload"].startswith("keyterm: "), fr
            assert s.keyterms == [("fine", vs.knob("VWA_ASR_KEYTERM_BOOST"))]  # the usable part of the last frame
            await ws.send_str(json.dumps({"type": "keyterms", "payload": {"terms": []}}))  # an empty list: off
            await ws.send_bytes(b"\0" * 320)
            await _frames(ws, 1)
            assert s.keyterms is None and not ws.closed
            snap = await (await c.get("/metrics")).json()
            assert snap["counters"]["keyterm_updates"] == 3
            await ws.close()

    asyncio.run(go())


def test_a_zero_argument_factory_is_still_served():
    async def go():
        class Plain:
            def push(self, data):
                return [{"type": "Results", "is_final": False, "channel": {"alternatives": [{"transcript": "y"}]}}]

            def flush(self):
                return []

        async with TestClient(TestServer(_app(lambda: Plain()))) as c:
            ws = await c.ws_connect("/stream?keyterm=Grafana")
            fr = await _frames(ws, 3)
            assert [f["type"] for f in fr] == ["info", "info", "warn"] and "not supported" in fr[2]["payload"]
            await ws.send_str(json.dumps({"type": "keyterms", "payload": {"terms": ["x"]}}))
            assert "not supported" in (await _frames(ws, 1))[0]["payload"]
            await ws.send_bytes(b"\0" * 320)
            assert (await _frames(ws, 1))[0]["type"] == "transcript_partial"
            await ws.close()
            ws = await c.ws_connect("/stream")  # and without terms: exactly the frames of before
            assert [f["type"] for f in await _frames(ws, 2)] == ["info", "info"]
            await ws.close()

    asyncio.run(go())


def test_the_router_forwards_the_query_string_to_its_worker():
    async def go():
        seen = []

        async def stream(req):
            seen.append((req.query_string, req.query.getall("keyterm", [])))
            ws = web.WebSocketResponse()
            await ws.prepare(req)
            await ws.send_json({"type": "info", "payload": "stub"})
            async for _ in ws:
                pass
            return ws

        async def health(_req):
            return web.json_response({"status": "ok"})

        async def metrics(_req):
            return web.json_response({})

        stub = web.Application()
        stub.router.add_get("/stream", stream)
        stub.router.add_get("/health", health)
        stub.router.add_get("/metrics", metrics)
        worker = TestServer(stub)
        await worker.start_server()
        router = TestServer(build_router([str(worker.make_url(""))], probe_s=0.2, max_fails=1))
        await router.start_server()
        try:
            async with aiohttp.ClientSession() as http:
                ws = await http.ws_connect(str(router.make_url("/stream")) + "?keyterm=Grafana&keyterm=pull+request:3")
                assert json.loads((await ws.receive(timeout=10)).data)["payload"] == "stub"
                await ws.close()
                ws = await http.ws_connect(router.make_url("/stream"))
                await ws.receive(timeout=10)
                await ws.close()
        finally:
            await router.close()
            await worker.close()
        assert seen[0][1] == ["Grafana", "pull request:3"]
        assert seen[1] == ("", [])

    asyncio.run(go())
