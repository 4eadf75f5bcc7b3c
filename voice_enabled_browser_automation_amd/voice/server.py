"""Voice service: ``GET /health``, ``GET /metrics``, WebSocket ``/stream`` (parity with
apps/voice/src/server.ts:60-304).

Per connection:
  * binary frames = raw PCM16 LE 16 kHz mono -> on-node streaming ASR (asr/streaming.py) ->
    ``transcript_partial`` / ``transcript_final`` frames carrying Deepgram-shaped payloads;
  * final transcripts are aggregated and debounced (``VWA_DEBOUNCE_MS``, reference fixed 1000 ms:
    :229) before ``POST BRAIN_URL`` {text, context};
  * commit policy for pauses (the reference only merges finals that land inside its debounce):
    the recognizer's VAD events (``SpeechStarted``) hold the pending text while the user speaks
    again -- a pause longer than the ASR endpoint is not a command boundary until ``VWA_COMMIT_MS``
    of silence have passed since the speech end; the brain is started SPECULATIVELY on the
    speculative final pass (``VWA_SPEC_BRAIN``), so its latency hides in the endpoint / commit
    wait, and its answer is used only if the committed text is exactly the text it parsed (and
    the context did not change meanwhile) -- otherwise it is dropped and the merged text parsed;
  * n-best rescoring (``VWA_RESCORE``, off by default): a beam final carries ranked alternatives with
    their acoustic log-probabilities; before its text joins the pending command the transcripts go to
    the brain (``POST /rescore``: the language model's log-probability that the user's text is exactly
    each alternative, behind the same few-shot commands) and the alternative with the best
    ``logprob + VWA_RESCORE_WEIGHT x score`` is the final's text -- "sort by price", not "sore by
    price".  The ``transcript_final`` frame is sent first, unchanged; a changed choice is followed by
    one ``info`` frame ``{"rescored": {"from", "to", "scores"}}``.  Any error, a timeout or a malformed
    answer keeps the recogniser's first; a 501 ends the asking.  Partials, speculative finals and
    finals with one alternative never ask;
  * turn-completion probe (``VWA_TURN``, off by default): a fixed silence timer cannot tell "search
    for" + pause from "scroll down" + pause; the brain can (``POST /turn``: the probability that the
    pending text is a finished command).  The connection asks on the speculative final pass and,
    if it then has no verdict for exactly the pending text, on the committing final.  The final
    arms the full hold as ever; a verdict ``p_end >= VWA_TURN_THRESHOLD`` for exactly the pending
    text, arriving while that commit is still armed, re-arms it to ``VWA_COMMIT_MIN_MS`` after the
    speech end (not before the debounce).  Anything else -- a lower ``p_end``, an HTTP error,
    garbage, no answer yet, another text -- leaves the full window standing, and ``SpeechStarted``
    cancels as before whatever the verdict was;
  * brain reply -> ``intent`` frame, ``tts`` frame (tts_summary), context merge of
    ``context_updates``, safe/risky split: safe intents go to ``POST EXECUTOR_URL/execute`` with
    the connection's executor session id (``execution_result`` / ``execution_error``), risky
    ones produce ``confirmation_required``;
  * JSON control frames: ``{"type":"close"}``, ``{"type":"context_update","payload":{...}}``,
    ``{"type":"flush"}`` (end of utterance: finalise without waiting for silence) and
    ``{"type":"keyterms","payload":{"terms":[...],"boost":x}}`` (replaces the session's keyterms);
  * keyterm prompting as Deepgram's ``keyterm`` option: ``/stream?keyterm=Grafana&keyterm=pull+request:3``
    -- repeated parameters, an optional ``:boost`` suffix in (0, 20] (a trailing ``:number`` is always
    the boost: the term "10:30" is written ``10:30:2``), at most 100 terms -- names words
    the recogniser should prefer (asr/keyterms.py); ``VWA_ASR_KEYTERMS`` gives every session default
    terms.  Bad input is answered with a ``warn`` frame and the connection goes on;
  * the wire format as Deepgram's ``encoding`` / ``sample_rate`` / ``channels`` options:
    ``/stream?encoding=mulaw&sample_rate=8000``, ``?encoding=linear16&sample_rate=48000&channels=2``
    -- linear16 | mulaw | alaw, 8000..48000 Hz (asr/wire.py SAMPLE_RATES), 1..8 interleaved channels
    whose mean is recognised, or the one channel an optional ``channel=i`` names.  Without them the
    binary frames are PCM16 LE 16 kHz mono as ever.  An unsupported value, or ``multichannel=true``
    (per-channel transcripts are not served), is refused with HTTP 400 before the upgrade:
    ``{"error": "unsupported_audio_format", "param": <the parameter>, "message": ...}``.

Races of the reference fixed here: brain calls of one connection are serialised
by a per-connection lock (context updates apply in utterance order), and its executor calls run
one at a time from a per-connection queue, so the executor session id is assigned in order; sends
after a client disconnect are dropped.  As in the reference (server.ts:186-224) the execution is
NOT awaited on the brain path: ``intent``, ``tts`` and ``confirmation_required`` go out as soon as
the brain answers, and the next utterance's brain call does not wait for a browser run.
"""
from __future__ import annotations

import asyncio
import json
import os
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Any, Callable, Dict, List, Optional

import aiohttp
from aiohttp import WSMsgType, web

from ..asr.wire import FormatError, format_from_query
from ..utils.context import merge_context
from ..utils.metrics import Metrics
from ..utils.env import knob

VERSION = "0.1.0"


MAX_KEYTERMS = 100      # Deepgram's limit on keyterms per request
MAX_KEYTERM_BOOST = 20.0


def parse_keyterm(raw: Any, default_boost: Optional[float] = None):
    """One wire keyterm -> (text, boost): ``"pull request:3"``, ``"Grafana"`` (the default boost),
    or {"term", "boost"}.  The boost is in (0, 20].  ValueError names what is wrong.

    In the string form a trailing ``:number`` is ALWAYS the boost, so a term whose own text ends that
    way ("10:30", "route:66") must name its boost after it -- ``"10:30:2"`` is the term "10:30" with
    boost 2.  The {"term", "boost"} form takes ``term`` literally, colon and all."""
    import math

    if default_boost is None:
        default_boost = knob("VWA_ASR_KEYTERM_BOOST")
    boost: Any = None
    literal = isinstance(raw, dict)
    if literal:
        raw, boost = raw.get("term", raw.get("text")), raw.get("boost")
    if not isinstance(raw, str):
        raise ValueError(f"keyterm {raw!r} is not a string")
    text = raw.strip()
    if not literal and ":" in text:
        head, _, tail = text.rpartition(":")
        try:
            boost, text = float(tail), head.strip()
        except ValueError:
            pass  # (a colon inside the term itself)
    if not text:
        raise ValueError(f"keyterm {raw!r} is empty")
    try:
        b = float(default_boost if boost is None else boost)
    except (TypeError, ValueError):
        raise ValueError(f"keyterm {text!r}: boost {boost!r} is not a number") from None
    if not math.isfinite(b) or not 0.0 < b <= MAX_KEYTERM_BOOST:
        raise ValueError(f"keyterm {text!r}: boost {boost!r} outside (0, {MAX_KEYTERM_BOOST:g}]")
    return text, b


def parse_keyterms(raws, default_boost: Optional[float] = None):
    """([(text, boost)], [warnings]): every usable term of the list, at most MAX_KEYTERMS."""
    terms, warns = [], []
    for raw in raws:
        try:
            t = parse_keyterm(raw, default_boost)
        except ValueError as e:
            warns.append(str(e))
            continue
        if len(terms) >= MAX_KEYTERMS:
            warns.append(f"more than {MAX_KEYTERMS} keyterms: the rest are ignored")
            break
        if t not in terms:
            terms.append(t)
    return terms, warns


def default_keyterms():
    """The VWA_ASR_KEYTERMS terms (a comma list; a bad entry is an error at startup)."""
    raw = knob("VWA_ASR_KEYTERMS") or ""
    return [parse_keyterm(x) for x in raw.split(",") if x.strip()][:MAX_KEYTERMS]


def _takes(factory, keyword: str) -> bool:
    import inspect

    try:
        ps = inspect.signature(factory).parameters
    except (TypeError, ValueError):
        return False
    return keyword in ps or any(p.kind is inspect.Parameter.VAR_KEYWORD for p in ps.values())


def _takes_keyterms(factory) -> bool:
    return _takes(factory, "keyterms")


async def post_json_and_return(session: aiohttp.ClientSession, url: str, body: Any) -> Any:
    """postJsonAndReturn parity (apps/voice/src/server.ts:15-52): non-JSON reply -> {ok: False}."""
    async with session.post(url, json=body) as resp:
        text = await resp.text()
    try:
        return json.loads(text)
    except ValueError:
        return {"ok": False}


def spoken_summaries(resp: Any) -> List[str]:
    """The summaries in an executor /execute reply: ``data.summary`` of every step where it is a
    non-empty string, in step order (anything else -- another reply shape, no such step -- gives none)."""
    results = resp.get("results") if isinstance(resp, dict) else None
    out = []
    for step in results if isinstance(results, list) else ():
        data = step.get("data") if isinstance(step, dict) else None
        s = data.get("summary") if isinstance(data, dict) else None
        if isinstance(s, str) and s.strip():
            out.append(s)
    return out


def build_app(asr_factory: Optional[Callable[[], Any]] = None, *, brain_url: Optional[str] = None,
              executor_url: Optional[str] = None, debounce_ms: Optional[float] = None,
              commit_ms: Optional[float] = None, spec_brain: Optional[bool] = None, turn: Optional[bool] = None,
              turn_url: Optional[str] = None, turn_threshold: Optional[float] = None,
              commit_min_ms: Optional[float] = None, rescore: Optional[bool] = None,
              rescore_url: Optional[str] = None, rescore_weight: Optional[float] = None,
              rescore_timeout_s: float = 5.0) -> web.Application:
    """asr_factory() -> a StreamingAsrSession-like object (push(bytes)->events, flush()->events);
    None = passthrough mode (no recognizer, as the reference without DEEPGRAM_API_KEY)."""
    app = web.Application()
    app["metrics"] = Metrics("voice")
    app["live"] = 0  # open /stream sessions (reported to the DP router's metrics gather)
    # one worker per live session pass: a session's recognition pass blocks its worker inside the
    # recognizer (asr/streaming.py AsrBatcher), whose single scheduler thread batches the passes
    # of all sessions onto the GPU -- so the pool only needs to be as wide as the session count
    app["asr_pool"] = ThreadPoolExecutor(max_workers=knob("VWA_MAX_SESSIONS") + 4,
                                         thread_name_prefix="asr")
    app["asr_factory"] = asr_factory
    app["exec_tasks"] = set()  # executor queues still draining after their connection closed
    brain_url = brain_url or knob("BRAIN_URL")
    executor_url = executor_url or knob("EXECUTOR_URL")
    if debounce_ms is None:
        debounce_ms = knob("VWA_DEBOUNCE_MS")
    commit_ms = knob("VWA_COMMIT_MS") if commit_ms is None else commit_ms
    spec_brain = knob("VWA_SPEC_BRAIN") if spec_brain is None else spec_brain
    # the ASR final fires endpoint_ms after the speech end: the commit window's rest comes after it
    hold_s = max(debounce_ms, commit_ms - knob("VWA_ENDPOINT_MS")) / 1000.0
    # turn-completion probe (module docstring): off unless VWA_TURN; the hold of a command it judged complete
    turn_on = bool(knob("VWA_TURN") if turn is None else turn)
    if turn_url is None:
        turn_url = knob("VWA_TURN_URL")
    if not turn_url:
        base, sep, rest = brain_url.rpartition("/parse")
        turn_url = base + "/turn" + rest if sep else brain_url.rstrip("/") + "/turn"
    turn_threshold = float(knob("VWA_TURN_THRESHOLD") if turn_threshold is None else turn_threshold)
    if not 0.0 < turn_threshold <= 1.0:
        raise ValueError(f"turn_threshold = {turn_threshold} outside (0, 1]")
    commit_min_ms = float(knob("VWA_COMMIT_MIN_MS") if commit_min_ms is None else commit_min_ms)
    if commit_min_ms < 0:
        raise ValueError(f"commit_min_ms = {commit_min_ms} is negative")
    early_s = max(debounce_ms, commit_min_ms - knob("VWA_ENDPOINT_MS")) / 1000.0
    turn_state = {"unsupported": False}  # set by the brain's first 501: the app stops asking
    # n-best rescoring (module docstring): off unless VWA_RESCORE
    rescore_on = bool(knob("VWA_RESCORE") if rescore is None else rescore)
    if rescore_url is None:
        rescore_url = knob("VWA_RESCORE_URL")
    if not rescore_url:
        base, sep, rest = brain_url.rpartition("/parse")
        rescore_url = base + "/rescore" + rest if sep else brain_url.rstrip("/") + "/rescore"
    rescore_weight = float(knob("VWA_RESCORE_WEIGHT") if rescore_weight is None else rescore_weight)
    if not rescore_weight >= 0.0:
        raise ValueError(f"rescore_weight = {rescore_weight} is negative")
    rescore_state = {"unsupported": False}  # likewise

    async def on_startup(app_):
        app_["http"] = aiohttp.ClientSession(timeout=aiohttp.ClientTimeout(total=120))

    async def on_cleanup(app_):
        for t in list(app_["exec_tasks"]):
            t.cancel()
        await app_["http"].close()
        app_["asr_pool"].shutdown(wait=False)

    app.on_startup.append(on_startup)
    app.on_cleanup.append(on_cleanup)

    async def health(_req):
        return web.json_response({"status": "ok", "service": "voice", "version": VERSION})

    async def metrics(_req):
        snap = app["metrics"].snapshot()
        batcher = getattr(asr_factory, "batcher", None)
        if batcher is not None:  # cross-session ASR batching: passes per GPU batch
            snap["asr_batcher"] = dict(batcher.stats, rows_per_batch=round(batcher.rows_per_batch(), 3),
                                       queue_depth=batcher.queue_depth())
        snap["live_sessions"] = app["live"]
        return web.json_response(snap)

    async def stream(req: web.Request) -> web.WebSocketResponse:
        m: Metrics = app["metrics"]
        # the wire format (Deepgram's encoding / sample_rate / channels, and our channel=i): refused
        # before the upgrade when it is not served -- a client must not stream audio nobody decodes
        try:
            fmt = format_from_query(req.query)
            if fmt is not None and asr_factory is not None and not _takes(asr_factory, "fmt"):
                raise FormatError("encoding", "this recognizer takes mono linear16 at 16000 Hz only")
        except FormatError as e:
            m.inc("asr_wire_rejected")
            return web.json_response({"error": "unsupported_audio_format", "param": e.param, "message": str(e)},
                                     status=400)
        ws = web.WebSocketResponse()
        await ws.prepare(req)
        m.inc("connections")
        fmt_kw = {} if fmt is None else {"fmt": fmt}
        if fmt is not None:
            m.inc(f'asr_wire_sessions{{encoding="{fmt.encoding}",sample_rate="{fmt.sample_rate}"}}')
        loop = asyncio.get_running_loop()
        # per-utterance span (monotonic): first audio -> final transcript -> brain reply
        # pending: final text not yet sent to the brain; spec: a speculative brain call {text, ctx,
        # task}; ctx: context version (a speculative answer is only used for the context it saw)
        st: Dict[str, Any] = {"context": {}, "pending": "", "debounce": None, "session_id": None, "closed": False,
                              "t_final": None, "t_utt": None, "spec": None, "ctx": 0, "procs": set(),
                              "turn": None}  # turn: the latest probe {text, task, done, complete}
        lock = asyncio.Lock()

        async def send(obj):
            if st["closed"] or ws.closed:
                return
            try:
                await ws.send_str(json.dumps(obj))
            except (ConnectionResetError, RuntimeError):
                st["closed"] = True

        # connection-state frames as the reference sends them for its Deepgram socket
        # (apps/voice/src/server.ts:233-250): "deepgram_connected" once the recognizer exists, then
        # the recognizer's own state events {state: open|close|error, info}; a recognizer that
        # cannot be created -> error "deepgram_connect_failed" and the connection stays up
        # without transcription (as the reference, whose audio then goes nowhere)
        # the session's keyterms: the query's, else the VWA_ASR_KEYTERMS defaults; what is wrong with
        # them is reported once the recognizer frames are out
        kt_warns: list = []
        try:
            keyterms, kt_warns = parse_keyterms(req.query.getall("keyterm", []))
            keyterms = keyterms or default_keyterms()
        except ValueError as e:
            keyterms, kt_warns = [], [str(e)]
        asr = None
        if asr_factory is not None:
            try:
                if keyterms and _takes_keyterms(asr_factory):
                    try:
                        asr = asr_factory(keyterms=keyterms, **fmt_kw)
                    except ValueError as e:  # (a term the tokenizer cannot take: serve without)
                        kt_warns.append(str(e))
                        asr = asr_factory(**fmt_kw)
                else:
                    if keyterms:
                        kt_warns.append("keyterms are not supported by this recognizer")
                    asr = asr_factory(**fmt_kw)
            except Exception as e:  # noqa: BLE001
                print(f"[voice] recognizer start failed: {e}", flush=True)
                m.inc("asr_connect_failed")
                await send({"type": "error", "payload": "deepgram_connect_failed"})
            else:
                await send({"type": "info", "payload": "deepgram_connected"})
                await send({"type": "info", "payload": {"state": "open"}})
                if hasattr(asr, "vad_events"):
                    asr.vad_events = True
                    asr.on_speculative = lambda text: loop.call_soon_threadsafe(on_speculative_final, text)
        else:
            await send({"type": "warn", "payload": "no_api_key; running in passthrough"})
        for w in kt_warns:
            m.inc("keyterm_warnings")
            await send({"type": "warn", "payload": f"keyterm: {w}"})
        seen = {"boosted_passes": 0, "fallback_passes": 0, "fallback_retries": 0, "fallback_rejected": 0}

        def count_boosted():
            """The session's recognition passes that carried keyterms -> the asr_boosted_passes counter;
            its final passes under the quality gate, their retried attempts and the finals the gate
            emptied -> asr_fallback_passes / asr_fallback_retries / asr_fallback_rejected."""
            stats = getattr(asr, "stats", None) or {}
            for k in seen:
                n = int(stats.get(k, 0))
                if n > seen[k]:
                    m.inc("asr_" + k, n - seen[k])
                    seen[k] = n

        async def set_keyterms(payload):
            """The ``keyterms`` control frame: replaces the session's set from the next pass on."""
            if not isinstance(payload, dict) or not isinstance(payload.get("terms"), list):
                await send({"type": "warn", "payload": "keyterm: payload must be {terms: [...], boost?: x}"})
                return
            try:
                dflt = payload.get("boost")
                if dflt is not None:
                    dflt = parse_keyterm("x", dflt)[1]
                terms, warns = parse_keyterms(payload["terms"], dflt)
                if asr is None or not hasattr(asr, "set_keyterms"):
                    warns.append("keyterms are not supported by this recognizer")
                else:
                    asr.set_keyterms(terms)
                    m.inc("keyterm_updates")
            except ValueError as e:
                warns = [str(e)]
            for w in warns:
                m.inc("keyterm_warnings")
                await send({"type": "warn", "payload": f"keyterm: {w}"})

        async def asr_call(fn, *a):
            """One recognizer call on the worker pool; an engine failure is reported as the
            reference reports a Deepgram socket error ({state: "error", info}) and the session
            continues (the next audio retries)."""
            try:
                return await loop.run_in_executor(app["asr_pool"], fn, *a)
            except Exception as e:  # noqa: BLE001
                m.inc("asr_errors")
                await send({"type": "info", "payload": {"state": "error", "info": str(e) or e.__class__.__name__}})
                return []

        async def run_executor(safe):
            try:
                resp = await post_json_and_return(app["http"], f"{executor_url}/execute",
                                                  {**({"session_id": st["session_id"]} if st["session_id"] else {}),
                                                   "intents": safe})
                st["session_id"] = resp.get("session_id", st["session_id"]) if isinstance(resp, dict) else st["session_id"]
                await send({"type": "execution_result",
                            "payload": f"Executed {len(safe)} actions successfully. Session: {st['session_id']}"})
                m.inc("executions")
                # a step that carries a summary (the executor's summarize intent with VWA_SUMMARIZE) is
                # spoken: one tts frame each, after the result
                for summary in spoken_summaries(resp):
                    await send({"type": "tts", "payload": summary})
                    m.inc("summaries_spoken")
            except Exception as e:  # noqa: BLE001
                await send({"type": "execution_error", "payload": f"Execution failed: {e}"})
                m.inc("execution_errors")

        # executor calls of this connection, in order, off the brain path (the reference fires
        # /execute without awaiting it, server.ts:186-219; one at a time here so session ids chain)
        exec_q: asyncio.Queue = asyncio.Queue()

        async def exec_worker():
            while True:
                safe = await exec_q.get()
                if safe is None:
                    return
                await run_executor(safe)

        exec_task = asyncio.ensure_future(exec_worker())

        async def call_brain(text: str):
            """One /parse call (serialised per connection: context updates apply in order)."""
            async with lock:
                t0 = time.perf_counter()
                try:
                    resp = await post_json_and_return(app["http"], brain_url, {"text": text, "context": st["context"]})
                except Exception as e:  # noqa: BLE001
                    m.inc("brain_errors")
                    print(f"[voice] brain post failed: {e}", flush=True)
                    return None
                m.observe("brain_ms", (time.perf_counter() - t0) * 1e3)
                return resp

        async def process(combined: str):
            """Commit one command: the speculative answer if it parsed exactly this text under the
            current context, else a fresh brain call; then deliver it."""
            sp, st["spec"] = st["spec"], None
            if sp is not None and sp["text"] == combined and sp["ctx"] == st["ctx"]:
                resp = await sp["task"]
                m.inc("spec_brain_used")
                if resp is None:
                    resp = await call_brain(combined)
            else:
                if sp is not None:
                    m.inc("spec_brain_dropped")
                resp = await call_brain(combined)
            if resp is not None:
                await deliver(resp)

        async def deliver(resp):
            async with lock:
                await send({"type": "intent", "payload": resp})
                now = time.perf_counter()
                m.inc("commands")
                if st["t_final"] is not None:
                    m.observe("final_to_intent_ms", (now - st["t_final"]) * 1e3)
                if st["t_utt"] is not None:
                    m.observe("utterance_to_intent_ms", (now - st["t_utt"]) * 1e3)
                    st["t_utt"] = None
                if isinstance(resp, dict) and resp.get("tts_summary"):
                    await send({"type": "tts", "payload": resp["tts_summary"]})
                if isinstance(resp, dict) and isinstance(resp.get("context_updates"), dict):
                    st["context"] = merge_context(st["context"], resp["context_updates"])
                    st["ctx"] += 1
                intents = resp.get("intents") if isinstance(resp, dict) else None
                if isinstance(intents, list):
                    safe = [i for i in intents if not (isinstance(i, dict) and i.get("requires_confirmation"))]
                    risky = [i for i in intents if isinstance(i, dict) and i.get("requires_confirmation")]
                    if safe:
                        exec_q.put_nowait(safe)
                    if risky:
                        await send({"type": "confirmation_required",
                                    "payload": f"{len(risky)} risky actions require manual confirmation"})

        async def debounced(delay: float = hold_s, early: bool = False):
            try:
                await asyncio.sleep(delay)
            except asyncio.CancelledError:
                return
            combined = st["pending"].strip()
            st["pending"] = ""
            st["debounce"] = None
            rec = st["turn"]
            if rec is not None and not rec["done"]:
                rec["task"].cancel()  # an answer after the commit changes nothing: counted unknown
            if early:
                m.inc("turn_early_commits")
            if combined:
                await process(combined)

        def start_debounce(delay: float = hold_s, early: bool = False):
            t = asyncio.ensure_future(debounced(delay, early))
            st["debounce"] = t
            st["procs"].add(t)  # (tracked until done: a disconnect lets a committing call finish)
            t.add_done_callback(st["procs"].discard)

        async def run_turn(rec):
            """One /turn call (NOT under the per-connection brain lock: it changes no context) and
            its verdict: complete, incomplete, or unknown for anything but a well-formed answer."""
            t0 = time.perf_counter()
            p_end = None
            try:
                async with app["http"].post(turn_url, json={"text": rec["text"], "context": st["context"]},
                                            timeout=aiohttp.ClientTimeout(total=5)) as resp:
                    status, body = resp.status, await resp.text()
                if status == 501:
                    if not turn_state["unsupported"]:
                        turn_state["unsupported"] = True
                        print(f"[voice] the brain at {turn_url} has no turn probe (501): VWA_TURN is ignored from "
                              "here on", flush=True)
                elif status == 200:
                    p = json.loads(body).get("p_end")
                    if isinstance(p, (int, float)) and not isinstance(p, bool) and 0.0 <= p <= 1.0:
                        p_end = float(p)
            except asyncio.CancelledError:
                pass
            except Exception:  # noqa: BLE001  (refused, timed out, not JSON, not an object)
                pass
            rec["done"] = True
            if p_end is None:
                m.inc("turn_unknown")
                return
            m.observe("turn_ms", (time.perf_counter() - t0) * 1e3)
            rec["complete"] = p_end >= turn_threshold
            m.inc("turn_complete" if rec["complete"] else "turn_incomplete")
            if rec["complete"]:
                commit_early(rec)

        def ask_turn(cand: str):
            """Ask the brain whether ``cand`` is a finished command, once per text."""
            rec = st["turn"]
            if not turn_on or turn_state["unsupported"] or st["closed"] or (rec is not None and rec["text"] == cand):
                return
            if rec is not None and not rec["done"]:
                rec["task"].cancel()  # superseded: its text is no longer what is pending
            m.inc("turn_probes")
            rec = st["turn"] = {"text": cand, "done": False, "complete": False, "task": None}
            rec["task"] = asyncio.ensure_future(run_turn(rec))

        def commit_early(rec):
            """Re-arm the commit of a command judged complete -- only if the verdict is the latest,
            is for exactly the pending text, and the commit the final armed is still armed (not
            cancelled by SpeechStarted, not fired)."""
            if rec is not st["turn"] or not rec["complete"] or st["debounce"] is None or st["t_final"] is None \
                    or st["pending"].strip() != rec["text"]:
                return
            st["debounce"].cancel()
            start_debounce(max(0.0, st["t_final"] + early_s - time.perf_counter()), early=True)

        async def rescore_final(alts, text: str) -> str:
            """The text of a beam final after n-best rescoring: the alternative with the best acoustic +
            weight x language-model score (one /rescore call, NOT under the brain lock: it changes no
            context).  Ties go to the recogniser's order; an alternative at -inf loses to any finite
            one; anything but a well-formed answer keeps the recogniser's first."""
            cands = [a for a in alts if isinstance(a, dict) and isinstance(a.get("transcript"), str)
                     and isinstance(a.get("logprob"), (int, float)) and not isinstance(a.get("logprob"), bool)]
            if len(cands) < 2 or cands[0] is not alts[0]:
                return text
            m.inc("rescore_asked")
            t0 = time.perf_counter()
            lm = None
            try:
                async with app["http"].post(rescore_url, json={"alternatives": [a["transcript"] for a in cands]},
                                            timeout=aiohttp.ClientTimeout(total=rescore_timeout_s)) as resp:
                    status, body = resp.status, await resp.text()
                if status == 501:
                    if not rescore_state["unsupported"]:
                        rescore_state["unsupported"] = True
                        print(f"[voice] the brain at {rescore_url} does not rescore (501): VWA_RESCORE is ignored "
                              "from here on", flush=True)
                elif status == 200:
                    sc = json.loads(body).get("scores")
                    if isinstance(sc, list) and len(sc) == len(cands) and all(
                            s is None or (isinstance(s, (int, float)) and not isinstance(s, bool) and s == s)
                            for s in sc):
                        lm = [float("-inf") if s is None else float(s) for s in sc]
            except Exception:  # noqa: BLE001  (refused, timed out, not JSON, not an object)
                pass
            if lm is None:
                m.inc("rescore_failed")
                return text
            m.observe("rescore_ms", (time.perf_counter() - t0) * 1e3)
            ninf = float("-inf")
            totals = []
            for a, s in zip(cands, lm):
                ac = float(a["logprob"])
                # (never NaN: an infinite term decides before the weight, which may be 0, multiplies it)
                totals.append(ninf if not (s > ninf and ac > ninf) else
                              (ac + rescore_weight * s if s < float("inf") and ac < float("inf") else float("inf")))
            best = 0
            for i, t in enumerate(totals):
                if t > totals[best]:
                    best = i
            chosen = cands[best]["transcript"].strip()
            if best == 0 or not chosen or chosen == text:
                return text
            m.inc("rescore_changed")
            await send({"type": "info", "payload": {"rescored": {
                "from": text, "to": chosen, "scores": [t if abs(t) != float("inf") else None for t in totals]}}})
            return chosen

        def on_speculative_final(text: str):
            """The ASR's speculative final pass finished (the user has been silent for
            VWA_SPEC_FINAL_MS): parse pending + it now, commit later (process); with VWA_TURN, ask
            whether pending + it is a finished command (independent of VWA_SPEC_BRAIN)."""
            text = (text or "").strip()
            if not text or st["closed"]:
                return
            cand = f"{st['pending']} {text}" if st["pending"] else text
            ask_turn(cand.strip())
            if not spec_brain:
                return
            sp = st["spec"]
            if sp is not None and sp["text"] == cand and sp["ctx"] == st["ctx"]:
                return
            m.inc("spec_brain_started")
            st["spec"] = {"text": cand, "ctx": st["ctx"], "task": asyncio.ensure_future(call_brain(cand))}

        async def handle_events(events):
            for ev in events:
                if ev.get("type") == "SpeechStarted":
                    # the user speaks (again): nothing pending is a finished command yet
                    if st["debounce"] is not None:
                        st["debounce"].cancel()
                        st["debounce"] = None
                        m.inc("commits_held")
                    continue
                is_final = bool(ev.get("is_final") or (ev.get("channel") or {}).get("is_final"))
                await send({"type": "transcript_final" if is_final else "transcript_partial", "payload": ev})
                if not is_final:
                    continue
                alt = ((ev.get("channel") or {}).get("alternatives") or [{}])[0]
                text = (alt.get("transcript") or "").strip()
                if not text:
                    continue
                m.inc("finals")
                st["t_final"] = time.perf_counter()
                if st["t_utt"] is not None:
                    m.observe("speech_to_final_ms", (st["t_final"] - st["t_utt"]) * 1e3)
                if rescore_on and not rescore_state["unsupported"]:
                    # (the frame above went out in the recogniser's order; only the command's text changes)
                    text = await rescore_final((ev.get("channel") or {}).get("alternatives") or [], text)
                st["pending"] = f"{st['pending']} {text}" if st["pending"] else text
                if st["debounce"] is not None:
                    st["debounce"].cancel()
                if ev.get("speech_final") is False:
                    # a long utterance cut at a segment end (asr/streaming.py long-form): the speaker
                    # is still talking, so the text waits for the final that ends the utterance
                    st["debounce"] = None
                    m.inc("longform_finals")
                    continue
                start_debounce()
                if turn_on:
                    # the full hold is armed; a verdict for exactly this text shortens it, now or
                    # when it arrives; without one (no speculative pass, or another text) ask now
                    rec, pend = st["turn"], st["pending"].strip()
                    if rec is not None and rec["text"] == pend:
                        commit_early(rec)
                    else:
                        ask_turn(pend)

        app["live"] += 1
        try:
            async for msg in ws:
                if msg.type == WSMsgType.BINARY:
                    m.inc("audio_frames")
                    if fmt is not None:
                        m.inc("asr_wire_bytes", len(msg.data))
                    if st["t_utt"] is None:
                        st["t_utt"] = time.perf_counter()
                    if asr is not None:
                        t_push = time.perf_counter()
                        events = await asr_call(asr.push, msg.data)
                        count_boosted()
                        dt = time.perf_counter() - t_push
                        m.observe("asr_push_ms", dt * 1e3)
                        # a recognition pass ran: real-time factor = pass time over the seconds of
                        # audio that pass recognised (the utterance buffer it covered)
                        covered = max((float(ev.get("duration") or 0.0) for ev in events), default=0.0)
                        if covered > 0:
                            m.observe("asr_rtf", dt / covered)
                        await handle_events(events)
                elif msg.type == WSMsgType.TEXT:
                    try:
                        ctl = json.loads(msg.data)
                    except ValueError:
                        continue
                    if not isinstance(ctl, dict):
                        continue
                    if ctl.get("type") == "close":
                        await ws.close()
                        break
                    if ctl.get("type") == "context_update" and isinstance(ctl.get("payload"), dict):
                        st["context"] = merge_context(st["context"], ctl["payload"])
                        st["ctx"] += 1
                    elif ctl.get("type") == "flush" and asr is not None:
                        events = await asr_call(asr.flush)
                        count_boosted()
                        await handle_events(events)
                    elif ctl.get("type") == "keyterms":
                        await set_keyterms(ctl.get("payload"))
                elif msg.type in (WSMsgType.ERROR, WSMsgType.CLOSE):
                    break
        finally:
            app["live"] -= 1
            st["closed"] = True
            if st["debounce"] is not None:
                st["debounce"].cancel()  # (still sleeping: a command nobody finished saying)
            if st["turn"] is not None and not st["turn"]["done"]:
                st["turn"]["task"].cancel()
            if asr is not None and hasattr(asr, "close"):
                asr.close()
            # queued executions still run (the reference's fire-and-forget promises do); their
            # frames are dropped once the socket is closed.  A command already committing (its
            # brain call in flight) still enqueues its safe intents: the sentinel goes in after it
            # (ADVICE r5 -- enqueued behind the sentinel they were silently dropped)
            inflight = [t for t in st["procs"] if not t.done()]

            async def close_exec():
                if inflight:
                    await asyncio.gather(*inflight, return_exceptions=True)
                exec_q.put_nowait(None)

            closer = asyncio.ensure_future(close_exec())
            for t in (closer, exec_task):
                app["exec_tasks"].add(t)
                t.add_done_callback(app["exec_tasks"].discard)
        return ws

    app.router.add_get("/health", health)
    app.router.add_get("/metrics", metrics)
    app.router.add_get("/stream", stream)
    return app


def asr_factory_from_env() -> Optional[Callable[[], Any]]:
    kind = knob("VWA_ASR_ENGINE")
    if kind == "none":
        return None
    import torch

    from ..asr.engine import AsrEngine
    from ..asr.streaming import AsrBatcher, StreamingAsrSession
    from ..models.config import get_config
    from ..models.whisper import WhisperModel
    from ..tokenizer import load_tokenizer

    name = knob("VWA_ASR_MODEL")
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    wpath = knob("VWA_ASR_WEIGHTS")
    if wpath:
        from ..runtime.weights import LazySafetensors

    model = WhisperModel(get_config(name), device=dev, weights=LazySafetensors(wpath) if wpath else None)
    from ..utils.env import asr_beam_knobs

    beam, n_alt = asr_beam_knobs()  # (a bad VWA_ASR_BEAM / VWA_ASR_ALTERNATIVES stops the worker here)
    eng = AsrEngine(model, load_tokenizer("whisper"),
                    max_sessions=max(knob("VWA_MAX_SESSIONS"), beam))  # a beam pass takes `beam` slots
    # VWA_ASR_TOKENS_PER_S: fixed-work transcripts for benchmarks on random-init weights
    tps = knob("VWA_ASR_TOKENS_PER_S") or None
    batcher = AsrBatcher(eng, tokens_per_s=tps)
    every = knob("VWA_PARTIAL_EVERY_S")

    default_keyterms()  # (a bad VWA_ASR_KEYTERMS stops the worker here)

    def factory(keyterms=None, fmt=None):
        return StreamingAsrSession(batcher, model_name=name, partial_every_s=every, beam=beam, alternatives=n_alt,
                                   keyterms=keyterms, fmt=fmt)

    factory.batcher = batcher
    return factory


def main():
    from ..utils.env import load_dotenv

    load_dotenv()
    port = knob("VOICE_PORT")
    print(f"[voice] http/ws listening on http://127.0.0.1:{port}", flush=True)
    # binds all interfaces, as the reference (apps/voice/src/server.ts:80)
    web.run_app(build_app(asr_factory_from_env()), host="0.0.0.0", port=port, print=None)


if __name__ == "__main__":
    main()
