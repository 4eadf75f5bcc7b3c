"""The voice service's turn-completion commit policy (VWA_TURN): a scripted recogniser, a fake brain
with ``/turn``, commit 700 and debounce 0 -- the ASR endpoint is 300 ms, so the full hold after a
final is 400 ms.  A complete verdict for exactly the pending text commits early; everything else
leaves the fixed window standing; SpeechStarted cancels whatever the verdict was."""
import asyncio
import contextlib

from aiohttp import web
from aiohttp.test_utils import TestClient, TestServer

from voice_enabled_browser_automation_amd.asr.streaming import results_event
from voice_enabled_browser_automation_amd.voice.server import build_app

FULL_HOLD = 0.4


class ScriptedAsr:
    """Each binary frame is a script, its commands separated by ``|`` and their events returned in
    one batch: ``S`` speech (re)starts, ``P:<text>`` the speculative final pass finished with <text>
    (the on_speculative callback), ``F:<text>`` a final, ``L:<text>`` a long-form final
    (speech_final false)."""

    def __init__(self):
        self.vad_events = False
        self.on_speculative = None

    def push(self, data):
        out = []
        for d in bytes(data).decode().split("|"):
            if d == "S" and self.vad_events:
                out.append({"type": "SpeechStarted", "channel": [0, 1], "timestamp": 0.0})
            elif d.startswith("P:") and self.on_speculative is not None:
                self.on_speculative(d[2:])
            elif d.startswith("F:"):
                out.append(results_event(d[2:], is_final=True, start=0, duration=1.0, model="fake"))
            elif d.startswith("L:"):
                out.append(dict(results_event(d[2:], is_final=True, start=0, duration=1.0, model="fake"),
                                speech_final=False))
        return out

    def flush(self):
        return []


class Rig:
    """The voice app between a fake brain (/parse, /turn) and a fake executor, one /stream client."""

    def __init__(self, turn_fn=None, **kw):
        self.turn_fn = turn_fn          # text -> (status, body, delay seconds); None: the brain has no /turn route
        self.kw = kw
        self.parse_calls, self.turn_calls, self.parse_at = [], [], []
        self.release = None

    @contextlib.asynccontextmanager
    async def open(self):
        self.release = asyncio.Event()
        loop = asyncio.get_running_loop()

        async def parse(req):
            body = await req.json()
            self.parse_calls.append(body["text"])
            self.parse_at.append(loop.time())
            return web.json_response({"version": "1.0", "intents": [
                {"type": "search", "args": {"query": body["text"]}, "priority": 0, "requires_confirmation": False,
                 "retries": 1}], "context_updates": {}, "confidence": 0.9})

        async def turn(req):
            body = await req.json()
            self.turn_calls.append(body["text"])
            status, payload, delay = self.turn_fn(body["text"])
            if delay is None:  # hung: answers only when the test is over
                await self.release.wait()
            elif delay:
                await asyncio.sleep(delay)
            if isinstance(payload, (dict, list)):
                return web.json_response(payload, status=status)
            return web.Response(text=payload, status=status)

        async def execute(_req):
            return web.json_response({"session_id": "s", "results": [], "artifacts": {}})

        bapp, eapp = web.Application(), web.Application()
        bapp.router.add_post("/parse", parse)
        bapp.router.add_post("/turn", turn)
        eapp.router.add_post("/execute", execute)
        async with TestServer(bapp) as bs, TestServer(eapp) as es:
            args = dict(brain_url=str(bs.make_url("/parse")), executor_url=str(es.make_url("")).rstrip("/"),
                        debounce_ms=0, commit_ms=700, spec_brain=False)
            args.update(self.kw)
            async with TestClient(TestServer(build_app(lambda: ScriptedAsr(), **args))) as c:
                self.client = c
                self.ws = await c.ws_connect("/stream")
                await self.ws.receive()
                await self.ws.receive()
                try:
                    yield self
                finally:
                    self.release.set()
                    await self.ws.close()

    async def say(self, script: str) -> float:
        await self.ws.send_bytes(script.encode())
        return asyncio.get_running_loop().time()

    async def intent(self, timeout=3.0):
        """The next intent frame's query (the committed text)."""
        async def go():
            while True:
                msg = await self.ws.receive_json()
                if msg["type"] == "intent":
                    return msg["payload"]["intents"][0]["args"]["query"]

        return await asyncio.wait_for(go(), timeout)

    async def counters(self):
        return (await (await self.client.get("/metrics")).json())["counters"]


def verdicts(table, delay=0.0):
    """A /turn that answers p_end by text (default 0.1)."""
    return lambda text: (200, {"p_end": table.get(text, 0.1), "logprob": -1.0, "prompt_tokens": 1000,
                               "cached_prefix_tokens": 976, "ms": 2.0}, delay)


def run(coro_fn):
    asyncio.run(coro_fn())


def test_a_complete_verdict_commits_within_200_ms_of_the_final():
    async def go():
        rig = Rig(verdicts({"scroll down": 0.9, "go back.": 0.5}), turn=True)
        async with rig.open():
            await rig.say("S")
            await rig.say("P:scroll down")           # the verdict is there before the final
            await asyncio.sleep(0.1)
            t0 = await rig.say("F:scroll down")
            assert await rig.intent() == "scroll down"
            assert rig.parse_at[0] - t0 < 0.2
            # no speculative pass: the final itself asks; p_end == threshold counts as complete
            await rig.say("S")
            t0 = await rig.say("F:go back.")
            assert await rig.intent() == "go back."
            assert rig.parse_at[1] - t0 < 0.2
            assert rig.turn_calls == ["scroll down", "go back."] and rig.parse_calls == ["scroll down", "go back."]
            m = await rig.counters()
            assert (m["turn_probes"], m["turn_complete"], m["turn_early_commits"], m["commands"]) == (2, 2, 2, 2)
            assert "turn_incomplete" not in m and "turn_unknown" not in m
            lat = (await (await rig.client.get("/metrics")).json())["latency"]
            assert lat["turn_ms"]["n"] == 2

    run(go)


def test_an_incomplete_verdict_keeps_the_window_and_the_pause_merges():
    async def go():
        rig = Rig(verdicts({"search for wireless earbuds": 0.8}), turn=True)
        async with rig.open():
            await rig.say("S")
            await rig.say("P:search for")
            await rig.say("F:search for")
            await asyncio.sleep(0.3)
            assert rig.parse_calls == [], "an incomplete command was committed inside the window"
            await rig.say("S")                          # ... the user goes on, inside the 400 ms
            await asyncio.sleep(0.3)
            assert rig.parse_calls == []
            t0 = await rig.say("F:wireless earbuds")
            assert await rig.intent() == "search for wireless earbuds"
            assert rig.parse_at[0] - t0 < 0.2           # the merged command is complete: early
            assert rig.turn_calls == ["search for", "search for wireless earbuds"]
            m = await rig.counters()
            assert (m["turn_incomplete"], m["turn_complete"], m["commits_held"], m["commands"]) == (1, 1, 1, 1)

    run(go)


def test_an_incomplete_verdict_commits_after_the_full_window():
    async def go():
        rig = Rig(verdicts({}), turn=True)
        async with rig.open():
            await rig.say("S")
            t0 = await rig.say("F:search for")
            assert await rig.intent() == "search for"
            assert rig.parse_at[0] - t0 >= FULL_HOLD - 0.02
            m = await rig.counters()
            assert m["turn_incomplete"] == 1 and "turn_early_commits" not in m

    run(go)


def test_a_verdict_delayed_150_ms_commits_on_arrival():
    async def go():
        rig = Rig(verdicts({"scroll down": 0.9}, delay=0.15), turn=True)
        async with rig.open():
            await rig.say("S")
            t0 = await rig.say("F:scroll down")
            assert await rig.intent() == "scroll down"
            assert 0.14 <= rig.parse_at[0] - t0 < 0.3, "well before the 400 ms window, not before the verdict"
            assert (await rig.counters())["turn_early_commits"] == 1

    run(go)


def test_errors_garbage_and_a_hung_probe_give_the_full_window():
    for turn_fn in (lambda t: (500, {"error": "llm_error", "detail": "x"}, 0.0),
                    lambda t: (200, "<html>not json</html>", 0.0),
                    lambda t: (200, {"p_end": "high"}, 0.0),
                    lambda t: (200, {"p_end": 7.0}, 0.0),
                    lambda t: (200, [0.9], 0.0),
                    lambda t: (200, {"p_end": 0.9}, None)):      # hung
        async def go():
            rig = Rig(turn_fn, turn=True)
            async with rig.open():
                await rig.say("S")
                await rig.say("P:scroll down")
                t0 = await rig.say("F:scroll down")
                assert await rig.intent() == "scroll down"
                assert rig.parse_at[0] - t0 >= FULL_HOLD - 0.02
                assert rig.turn_calls == ["scroll down"]
                m = await rig.counters()
                assert m["turn_unknown"] == 1 and m["turn_probes"] == 1
                assert "turn_early_commits" not in m and "turn_complete" not in m

        run(go)


def test_an_answer_after_the_commit_changes_nothing():
    async def go():
        rig = Rig(verdicts({"scroll down": 0.9}, delay=0.6), turn=True)
        async with rig.open():
            await rig.say("S")
            t0 = await rig.say("F:scroll down")
            assert await rig.intent() == "scroll down"
            assert rig.parse_at[0] - t0 >= FULL_HOLD - 0.02
            await asyncio.sleep(0.4)
            m = await rig.counters()
            assert m["commands"] == 1 and rig.parse_calls == ["scroll down"] and "turn_early_commits" not in m

    run(go)


def test_after_a_501_no_further_probe_is_sent(capsys):
    async def go():
        rig = Rig(lambda t: (501, {"error": "turn_unsupported"}, 0.0), turn=True)
        async with rig.open():
            for text in ("scroll down", "go back"):
                await rig.say("S")
                await rig.say(f"P:{text}")
                t0 = await rig.say(f"F:{text}")
                assert await rig.intent() == text
                assert rig.parse_at[-1] - t0 >= FULL_HOLD - 0.02
            assert rig.turn_calls == ["scroll down"]
            m = await rig.counters()
            assert m["turn_probes"] == 1 and m["turn_unknown"] == 1 and m["commands"] == 2

    run(go)
    assert capsys.readouterr().out.count("has no turn probe") == 1


def test_a_stale_verdict_for_other_text_is_ignored():
    async def go():
        rig = Rig(verdicts({"go": 0.95}), turn=True)
        async with rig.open():
            await rig.say("S")
            await rig.say("P:go")                      # complete -- for "go"
            await asyncio.sleep(0.1)
            t0 = await rig.say("F:go back to the")     # not the text the verdict is for
            assert await rig.intent() == "go back to the"
            assert rig.parse_at[0] - t0 >= FULL_HOLD - 0.02
            assert rig.turn_calls == ["go", "go back to the"]
            m = await rig.counters()
            assert (m["turn_complete"], m["turn_incomplete"]) == (1, 1) and "turn_early_commits" not in m

    run(go)


def test_speech_started_after_a_complete_verdict_still_cancels():
    async def go():
        # COMMIT_MIN 300 is the endpoint itself: the early commit is armed for "now" -- and the
        # SpeechStarted in the same batch of events still cancels it
        rig = Rig(verdicts({"search for": 0.9, "search for shoes": 0.9}), turn=True, commit_min_ms=300)
        async with rig.open():
            await rig.say("S")
            await rig.say("P:search for")
            await asyncio.sleep(0.1)
            await rig.say("F:search for|S")
            await asyncio.sleep(0.6)
            assert rig.parse_calls == []
            await rig.say("F:shoes")
            assert await rig.intent() == "search for shoes"
            m = await rig.counters()
            assert m["commits_held"] == 1 and m["commands"] == 1 and m["turn_early_commits"] == 1

    run(go)

    async def later():
        # COMMIT_MIN 500: the early commit waits 200 ms after the final; speech at 100 ms cancels it
        rig = Rig(verdicts({"search for": 0.9}), turn=True, commit_min_ms=500)
        async with rig.open():
            await rig.say("S")
            await rig.say("P:search for")
            await asyncio.sleep(0.1)
            await rig.say("F:search for")
            await asyncio.sleep(0.1)
            await rig.say("S")
            await asyncio.sleep(0.6)
            assert rig.parse_calls == []
            m = await rig.counters()
            assert m["commits_held"] == 1 and m["turn_complete"] == 1 and "turn_early_commits" not in m

    run(later)


def test_commit_min_ms_holds_a_complete_command_that_long():
    async def go():
        rig = Rig(verdicts({"scroll down": 0.9}), turn=True, commit_min_ms=500)
        async with rig.open():
            await rig.say("S")
            await rig.say("P:scroll down")
            await asyncio.sleep(0.05)
            t0 = await rig.say("F:scroll down")
            assert await rig.intent() == "scroll down"
            assert 0.18 <= rig.parse_at[0] - t0 < 0.35

    run(go)


def test_a_long_form_final_is_never_probed():
    async def go():
        rig = Rig(verdicts({}), turn=True)
        async with rig.open():
            await rig.say("S")
            await rig.say("L:open the settings page and then")
            await asyncio.sleep(0.2)
            assert rig.turn_calls == [] and rig.parse_calls == []
            await rig.say("F:scroll down")
            assert await rig.intent() == "open the settings page and then scroll down"
            assert rig.turn_calls == ["open the settings page and then scroll down"]

    run(go)


def test_the_probe_is_independent_of_the_speculative_brain_and_of_its_lock():
    async def go():
        rig = Rig(verdicts({"scroll down": 0.9}), turn=True, spec_brain=True)
        async with rig.open():
            await rig.say("S")
            await rig.say("P:scroll down")
            await asyncio.sleep(0.1)
            t0 = await rig.say("F:scroll down")
            assert await rig.intent() == "scroll down"
            assert asyncio.get_running_loop().time() - t0 < 0.2
            m = await rig.counters()
            assert m["spec_brain_used"] == 1 and m["turn_early_commits"] == 1 and rig.parse_calls == ["scroll down"]

    run(go)


def test_with_the_feature_off_turn_is_never_requested():
    async def go():
        rig = Rig(verdicts({"scroll down": 0.99}))      # (build_app's default: VWA_TURN off)
        async with rig.open():
            await rig.say("S")
            await rig.say("P:scroll down")
            t0 = await rig.say("F:scroll down")
            assert await rig.intent() == "scroll down"
            assert rig.parse_at[0] - t0 >= FULL_HOLD - 0.02
            assert rig.turn_calls == []
            assert not [k for k in await rig.counters() if k.startswith("turn_")]

    run(go)


def test_the_turn_url_defaults_to_the_brain_url_with_turn_for_parse(monkeypatch):
    from voice_enabled_browser_automation_amd.utils.env import knob

    assert knob("VWA_TURN") is False and knob("VWA_TURN_THRESHOLD") == 0.5 and knob("VWA_COMMIT_MIN_MS") == 0.0
    assert knob("VWA_TURN_URL") is None
    for bad in (dict(turn_threshold=0.0), dict(turn_threshold=1.5), dict(commit_min_ms=-1)):
        try:
            build_app(None, **bad)
        except ValueError:
            continue
        raise AssertionError(f"build_app accepted {bad}")
