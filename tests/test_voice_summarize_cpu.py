"""Voice service: an executor reply whose steps carry a summary (the summarize intent with
VWA_SUMMARIZE) is spoken -- one ``tts`` frame per such step, after the ``execution_result`` -- and a
reply without one produces no extra frame: the frame sequence is what it was."""
import asyncio
import json

from aiohttp import web
from aiohttp.test_utils import TestClient, TestServer

from voice_enabled_browser_automation_amd.asr.streaming import results_event
from voice_enabled_browser_automation_amd.voice.server import build_app, spoken_summaries

SUMMARY = "This page sells wireless earbuds. They are on sale this week."


class FakeAsr:
    def push(self, data):
        return []

    def flush(self):
        return [results_event("summarize this page", is_final=True, start=0, duration=1.0, model="fake")]


def frames_after_flush(results, tts_summary=None):
    """One utterance through the voice service with a fake brain (a summarize intent) and a fake
    executor answering ``results``.  Returns the frames from the intent on, up to a marker frame sent
    after the execution result (so that a frame that should NOT come would have been seen)."""
    async def brain(req):
        await req.json()
        out = {"version": "1.0", "intents": [{"type": "summarize", "args": {}, "priority": 0,
                                              "requires_confirmation": False}],
               "context_updates": {}, "confidence": 0.9}
        if tts_summary:
            out["tts_summary"] = tts_summary
        return web.json_response(out)

    async def execute(req):
        await req.json()
        return web.json_response({"session_id": "sess-1", "results": results, "artifacts": {"dir": "x"}})

    async def go():
        bapp, eapp = web.Application(), web.Application()
        bapp.router.add_post("/parse", brain)
        eapp.router.add_post("/execute", execute)
        async with TestServer(bapp) as bs, TestServer(eapp) as es:
            vapp = build_app(lambda: FakeAsr(), brain_url=str(bs.make_url("/parse")),
                             executor_url=str(es.make_url("")).rstrip("/"), debounce_ms=5)
            async with TestClient(TestServer(vapp)) as c:
                ws = await c.ws_connect("/stream")
                await ws.send_str(json.dumps({"type": "flush"}))
                got = []
                while not any(g["type"] in ("execution_result", "execution_error") for g in got):
                    got.append(json.loads((await asyncio.wait_for(ws.receive(), 10)).data))
                # whatever follows the result is already queued on the socket in order: a second
                # utterance's intent frame marks the end of the first one's frames
                await ws.send_str(json.dumps({"type": "flush"}))
                while sum(g["type"] == "intent" for g in got) < 2:
                    got.append(json.loads((await asyncio.wait_for(ws.receive(), 10)).data))
                await ws.close()
                m = await (await c.get("/metrics")).json()
                return got, m

    got, m = asyncio.run(go())
    types = [g["type"] for g in got]
    first = types.index("intent")
    return got[first : first + 1 + types[first + 1:].index("intent")], m


def step(data=None, ok=True):
    s = {"intent": {"type": "summarize"}, "ok": ok, "attempts": 1}
    if data is not None:
        s["data"] = data
    return s


def test_a_summary_step_is_spoken_after_the_execution_result():
    frames, m = frames_after_flush([step({"summary": SUMMARY, "chars": len(SUMMARY), "truncated": False,
                                          "source_chars": 900})], tts_summary="Summarising the page.")
    kinds = [(f["type"], f["payload"]) for f in frames if f["type"] in ("tts", "execution_result")]
    assert kinds == [("tts", "Summarising the page."),
                     ("execution_result", "Executed 1 actions successfully. Session: sess-1"), ("tts", SUMMARY)]
    assert m["counters"]["summaries_spoken"] >= 1  # (the marker utterance may have been executed, too)


def test_results_without_a_summary_produce_no_extra_frame():
    note = {"note": "summarize should be handled by the brain"}
    for results in ([step(note)], [], [step()], [step({"summary": ""})], [step({"summary": "   "})],
                    [step({"summary": 7})], [step({"summary": None})], [step("text")]):
        frames, m = frames_after_flush(results)
        assert [f["type"] for f in frames if f["type"] in ("tts", "execution_result", "execution_error")] == \
            ["execution_result"], results
        assert "summaries_spoken" not in m["counters"]


def test_every_summary_step_is_spoken_in_step_order():
    frames, _ = frames_after_flush([step({"summary": "First."}), step({"rows": 3}), step({"summary": "Second."}, ok=False)])
    assert [f["payload"] for f in frames if f["type"] == "tts"] == ["First.", "Second."]


def test_spoken_summaries_reads_only_the_reply_shape_it_knows():
    assert spoken_summaries({"results": [step({"summary": SUMMARY})]}) == [SUMMARY]
    for resp in (None, {"ok": False}, {"results": None}, {"results": "x"}, {"results": [None, 3, "s", {"data": []}]},
                 [step({"summary": SUMMARY})]):
        assert spoken_summaries(resp) == []
