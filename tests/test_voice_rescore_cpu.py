"""The voice service's n-best rescoring policy (VWA_RESCORE): a scripted recogniser, a fake brain with
``/rescore``, commit and debounce 0 (a final commits at once).  The alternative with the best
``logprob + weight x score`` reaches ``/parse``; the ``info`` frame appears only on a change; any
error, a timeout, a 501 and equal totals keep the recogniser's first; with the flag off no request is
made and the frames are what they were."""
import asyncio
import contextlib
import json

from aiohttp import web
from aiohttp.test_utils import TestClient, TestServer

from voice_enabled_browser_automation_amd.asr.streaming import results_event
from voice_enabled_browser_automation_amd.voice.server import build_app

SORT = [["sore by price", -3.0], ["sort by price", -3.5], ["sort by rice", -4.0]]


def beam_final(alts, logprobs=True):
    return results_event(alts[0][0], is_final=True, start=0, duration=1.0, model="fake", confidence=0.5,
                         alternatives=[dict(transcript=t, confidence=0.25) for t, _ in alts[1:]],
                         logprobs=[lp for _, lp in alts] if logprobs else None)


class ScriptedAsr:
    """Each binary frame is a script, its commands separated by ``|``: ``B:<json [[text, logprob], ...]>``
    a beam final with its alternatives' logprobs, ``N:<json>`` the same without logprobs (a session that
    does not rescore), ``F:<text>`` a greedy final, ``I:<text>`` a partial, ``P:<text>`` the speculative
    final pass finished with <text>."""

    def __init__(self):
        self.vad_events = False
        self.on_speculative = None

    def push(self, data):
        out = []
        for d in bytes(data).decode().split("|"):
            if d.startswith("B:") or d.startswith("N:"):
                out.append(beam_final(json.loads(d[2:]), logprobs=d[0] == "B"))
            elif d.startswith("F:") or d.startswith("I:"):
                out.append(results_event(d[2:], is_final=d[0] == "F", start=0, duration=1.0, model="fake"))
            elif d.startswith("P:") and self.on_speculative is not None:
                self.on_speculative(d[2:])
        return out

    def flush(self):
        return []


class Rig:
    """The voice app between a fake brain (/parse, /rescore) and a fake executor, one /stream client."""

    def __init__(self, rescore_fn=None, **kw):
        self.rescore_fn = rescore_fn    # alternatives -> (status, body, delay seconds; None: hangs)
        self.kw = kw
        self.parse_calls, self.rescore_calls = [], []

    @contextlib.asynccontextmanager
    async def open(self):
        release = asyncio.Event()

        async def parse(req):
            body = await req.json()
            self.parse_calls.append(body["text"])
            return web.json_response({"version": "1.0", "intents": [
                {"type": "search", "args": {"query": body["text"]}, "priority": 0, "requires_confirmation": False,
                 "retries": 1}], "context_updates": {}, "confidence": 0.9})

        async def rescore(req):
            body = await req.json()
            self.rescore_calls.append(body["alternatives"])
            status, payload, delay = self.rescore_fn(body["alternatives"])
            if delay is None:  # hung: answers only when the test is over
                await release.wait()
            if isinstance(payload, (dict, list)):
                return web.json_response(payload, status=status)
            return web.Response(text=payload, status=status)

        async def execute(_req):
            return web.json_response({"session_id": "s", "results": [], "artifacts": {}})

        bapp, eapp = web.Application(), web.Application()
        bapp.router.add_post("/parse", parse)
        if self.rescore_fn is not None:
            bapp.router.add_post("/rescore", rescore)
        eapp.router.add_post("/execute", execute)
        async with TestServer(bapp) as bs, TestServer(eapp) as es:
            args = dict(brain_url=str(bs.make_url("/parse")), executor_url=str(es.make_url("")).rstrip("/"),
                        debounce_ms=0, commit_ms=0, spec_brain=False)
            args.update(self.kw)
            async with TestClient(TestServer(build_app(lambda: ScriptedAsr(), **args))) as c:
                self.client = c
                self.ws = await c.ws_connect("/stream")
                await self.ws.receive()
                await self.ws.receive()
                try:
                    yield self
                finally:
                    release.set()
                    await self.ws.close()

    async def say(self, script: str):
        await self.ws.send_bytes(script.encode())

    async def until_intent(self, timeout=3.0):
        """(the frames up to the next intent frame as raw text, the intent's query = the committed text)."""
        async def go():
            raw = []
            while True:
                msg = await self.ws.receive()
                raw.append(msg.data)
                j = json.loads(msg.data)
                if j["type"] == "intent":
                    return raw, j["payload"]["intents"][0]["args"]["query"]

        return await asyncio.wait_for(go(), timeout)

    async def counters(self):
        return (await (await self.client.get("/metrics")).json())["counters"]


def scores(table, delay=0.0):
    """A /rescore that answers by text (default -20)."""
    return lambda alts: (200, {"scores": [table.get(a, -20.0) for a in alts], "scored_tokens": [1] * len(alts),
                               "common_prefix_tokens": 998, "prompt_tokens": [1000] * len(alts),
                               "cached_prefix_tokens": 976, "ms": 2.0}, delay)


def run(coro_fn):
    asyncio.run(coro_fn())


def infos(raw):
    return [json.loads(f)["payload"] for f in raw if json.loads(f)["type"] == "info"]


def test_the_chosen_text_reaches_parse_and_the_info_frame_tells_of_the_change():
    async def go():
        # totals at weight 0.5: -3 - 5 = -8, -3.5 - 1 = -4.5, -4 - 10 = -14
        rig = Rig(scores({"sore by price": -10.0, "sort by price": -2.0}), rescore=True, rescore_weight=0.5)
        async with rig.open():
            await rig.say("I:sore by|B:" + json.dumps(SORT))
            raw, text = await rig.until_intent()
            assert text == "sort by price" and rig.parse_calls == ["sort by price"]
            assert rig.rescore_calls == [[t for t, _ in SORT]]
            frames = [json.loads(f) for f in raw]
            # the final's frame goes out first, in the recogniser's order, then the one info frame
            fin = [f for f in frames if f["type"] == "transcript_final"]
            assert len(fin) == 1 and fin[0]["payload"] == beam_final(SORT)
            assert infos(raw) == [{"rescored": {"from": "sore by price", "to": "sort by price",
                                                "scores": [-8.0, -4.5, -14.0]}}]
            assert [f["type"] for f in frames].index("transcript_final") < [f["type"] for f in frames].index("info")
            # the recogniser's first is also the model's: no info frame; the pending text merges as ever
            await rig.say("B:" + json.dumps([["scroll down", -1.0], ["scroll town", -1.2]]))
            raw, text = await rig.until_intent()
            assert text == "scroll down" and infos(raw) == []
            m = await rig.counters()
            assert (m["rescore_asked"], m["rescore_changed"], m["commands"]) == (2, 1, 2) and "rescore_failed" not in m

    run(go)


def test_equal_totals_and_infinities_keep_the_recognisers_order():
    async def go():
        table = {}
        rig = Rig(lambda alts: scores(table)(alts), rescore=True, rescore_weight=1.0)
        async with rig.open():
            for tab, alts, want in (
                    ({"a b": -2.0, "a p": -1.0}, [["a b", -1.0], ["a p", -2.0]], "a b"),            # a tie: the lowest i
                    ({"a b": None, "a p": -50.0}, [["a b", -1.0], ["a p", -2.0]], "a p"),           # -inf loses to finite
                    ({"a b": None, "a p": None}, [["a b", -1.0], ["a p", -2.0]], "a b"),            # all -inf: the order
                    ({"a b": -1.0, "a p": -1.0, "a d": 0.0}, [["a b", -1.0], ["a p", -1.5], ["a d", -1.5]], "a d")):
                table.clear()
                table.update(tab)
                await rig.say("B:" + json.dumps(alts))
                assert (await rig.until_intent())[1] == want, (tab, alts)
        # weight 0 and a score at -inf: no NaN, the alternative at -inf still loses
        rig = Rig(scores({"a b": None, "a p": -3.0}), rescore=True, rescore_weight=0.0)
        async with rig.open():
            await rig.say("B:" + json.dumps([["a b", -1.0], ["a p", -2.0]]))
            raw, text = await rig.until_intent()
            assert text == "a p" and infos(raw)[0]["rescored"]["scores"] == [None, -2.0]

    run(go)


def test_errors_a_timeout_and_garbage_keep_alternative_0():
    async def go():
        bad = [(500, {"error": "llm_error"}, 0.0), (200, "not json", 0.0), (200, [1, 2], 0.0), (200, {"scores": [-1.0]}, 0.0),
               (200, {"scores": [-1.0, "x", -2.0]}, 0.0), (200, {"scores": [-1.0, True, -2.0]}, 0.0), (200, {}, 0.0),
               (404, "no", 0.0), (200, {"scores": [0.0, 0.0, 0.0]}, None)]  # the last one hangs: the client times out
        it = iter(bad)
        rig = Rig(lambda alts: next(it), rescore=True, rescore_timeout_s=0.2)
        async with rig.open():
            for _ in bad:
                await rig.say("B:" + json.dumps(SORT))
                raw, text = await rig.until_intent()
                assert text == "sore by price" and infos(raw) == []
            m = await rig.counters()
            assert (m["rescore_asked"], m["rescore_failed"], m["commands"]) == (len(bad), len(bad), len(bad))
            assert "rescore_changed" not in m
        # a brain that refuses the connection
        rig = Rig(None, rescore=True, rescore_url="http://127.0.0.1:1/rescore")
        async with rig.open():
            await rig.say("B:" + json.dumps(SORT))
            assert (await rig.until_intent())[1] == "sore by price"
            assert (await rig.counters())["rescore_failed"] == 1

    run(go)


def test_a_501_ends_the_asking_for_the_app():
    async def go():
        rig = Rig(lambda alts: (501, {"error": "rescore_unsupported"}, 0.0), rescore=True)
        async with rig.open():
            for _ in range(3):
                await rig.say("B:" + json.dumps(SORT))
                assert (await rig.until_intent())[1] == "sore by price"
            assert len(rig.rescore_calls) == 1
            m = await rig.counters()
            assert (m["rescore_asked"], m["rescore_failed"], m["commands"]) == (1, 1, 3)

    run(go)


def test_partials_greedy_finals_and_single_alternatives_never_ask():
    async def go():
        rig = Rig(scores({}), rescore=True, spec_brain=True)
        async with rig.open():
            await rig.say("I:scroll|P:scroll down|F:scroll down")          # greedy: no alternatives
            assert (await rig.until_intent())[1] == "scroll down"
            await rig.say("B:" + json.dumps([["go back", -1.0]]))          # one alternative
            assert (await rig.until_intent())[1] == "go back"
            await rig.say("N:" + json.dumps(SORT))                         # alternatives without logprob
            assert (await rig.until_intent())[1] == "sore by price"
            assert rig.rescore_calls == [] and "rescore_asked" not in await rig.counters()
            # a speculative brain answer is used only for exactly the chosen text
            rig.rescore_fn = scores({"sort by price": -1.0})
            await rig.say("P:sore by price|B:" + json.dumps(SORT))
            assert (await rig.until_intent())[1] == "sort by price"
            assert rig.parse_calls[-2:] == ["sore by price", "sort by price"]

    run(go)


# the frames of "I:sore by|B:<SORT>" with the flag off, as recorded before the feature existed
RECORDED = [
    '{"type": "transcript_partial", "payload": {"type": "Results", "channel_index": [0, 1], "duration": 1.0, "start": 0, '
    '"is_final": false, "speech_final": false, "channel": {"alternatives": [{"transcript": "sore by", "confidence": 0.0, '
    '"words": []}]}, "metadata": {"model_info": {"name": "fake"}}}}',
    '{"type": "transcript_final", "payload": {"type": "Results", "channel_index": [0, 1], "duration": 1.0, "start": 0, '
    '"is_final": true, "speech_final": true, "channel": {"alternatives": [{"transcript": "sore by price", "confidence": 0.5, '
    '"words": []}, {"transcript": "sort by price", "confidence": 0.25, "words": []}, {"transcript": "sort by rice", '
    '"confidence": 0.25, "words": []}]}, "metadata": {"model_info": {"name": "fake"}}}}',
]


def test_with_the_flag_off_no_request_is_made_and_the_frames_are_the_recorded_ones():
    async def go():
        rig = Rig(scores({"sort by price": 0.0}))
        async with rig.open():
            await rig.say("I:sore by|N:" + json.dumps(SORT))
            raw, text = await rig.until_intent()
            assert text == "sore by price" and raw[:2] == RECORDED
            assert [json.loads(f)["type"] for f in raw[2:]] == ["intent"]
            await rig.say("B:" + json.dumps(SORT))                          # even if an event carried logprobs
            assert (await rig.until_intent())[1] == "sore by price"
            assert rig.rescore_calls == []
            assert not any(k.startswith("rescore") for k in await rig.counters())

    run(go)
