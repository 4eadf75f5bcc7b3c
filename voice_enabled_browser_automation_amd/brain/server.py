"""Brain service: ``GET /health``, ``POST /parse``, ``GET /metrics`` (parity with apps/brain/src/server.ts),
and ``POST /turn``, ``POST /summarize`` and ``POST /rescore``, this project's own: the turn-completion
probe, the page summary behind the ``summarize`` intent, and the language-model scores of the
recogniser's n-best alternatives.

Request flow (apps/brain/src/server.ts:89-139):
  ParseRequest validation -> 400 {error:"invalid_request", detail}
  prompt (system + few-shots + user JSON) -> intent engine
     engine raises            -> 500 {error:"llm_error", detail}
     reply fails ParseResponse -> ONE repair call with the repair system note
  final validation fails      -> 422 {error:"schema_validation_failed", detail}
  200 -> ParseResponse with zod-style defaults filled.

``POST /turn`` {"text", "context"?}: 400 invalid_request for a missing, empty or non-string text;
501 {error:"turn_unsupported"} for an engine without ``turn_async`` (keyword, TP); 500 llm_error as
``/parse``; 200 {p_end, logprob, prompt_tokens, cached_prefix_tokens, ms}.

``POST /summarize`` {"text", "title"?, "url"?, "max_chars"?}: 400 invalid_request for a missing, empty
or non-string text, a non-string title or url, or a max_chars that is not an integer in [16, 4096];
501 {error:"summarize_unsupported"} for an engine without ``summary_async`` (keyword, TP); 500 llm_error
as ``/parse``; 200 {summary, chars, prompt_tokens, cached_prefix_tokens, page_tokens, truncated,
decode_steps, ms}.  ``/metrics`` counts ``summaries`` and ``summary_tokens`` and gives the mean ``n_kept``
(ids the nucleus step left per sampled token).

``POST /rescore`` {"alternatives": [1..8 strings]}: 400 {error:"bad_request"} for anything else; 501
{error:"rescore_unsupported"} for an engine without ``rescore_async`` (keyword, TP); 500 llm_error as
``/parse``; 200 {scores, scored_tokens, common_prefix_tokens, prompt_tokens, cached_prefix_tokens, ms}
(LLMIntentEngine.rescore: the scores of one answer are comparable with each other and only with each
other; a score at -inf is null, JSON has no -inf).  ``/metrics`` counts ``rescore_requests`` and
observes ``rescore_ms``.

With the LLM engine the grammar makes the first answer schema-valid, so the repair path only
runs for engines without constrained decoding (or injected faults in tests).

Engines (VWA_BRAIN_ENGINE): ``llm`` (on-GPU Llama + constrained decoding; VWA_LLM_MODEL, VWA_TP),
``keyword`` (rule-based, CPU), or any object passed to ``build_app(engine=...)``.
"""
from __future__ import annotations

import asyncio
import json
import os
import time
from typing import Any, Optional

from aiohttp import web

from ..contracts import ParseRequest, ParseResponse, safe_parse
from ..utils.context import cap_context
from ..utils.metrics import Metrics
from .prompt import messages_for
from .tp_engine import TPIntentEngine  # noqa: F401  (re-exported: the TP control plane)
from ..utils.env import knob

SUMMARY_MIN_CHARS, SUMMARY_MAX_CHARS = 16, 4096  # a request's max_chars

SERVICE_NAME = "brain-ts"  # byte-compatible /health payload (apps/brain/src/server.ts:87)


def build_app(engine: Any = None) -> web.Application:
    if engine is None:
        engine = make_engine_from_env()
    app = web.Application()
    app["engine"] = engine
    app["lock"] = asyncio.Lock()
    app["metrics"] = Metrics("brain")

    async def health(_req: web.Request) -> web.Response:
        failed = getattr(app["engine"], "failed", None)
        if failed is not None:  # a TP group that lost lockstep: the process is about to exit
            return web.json_response({"status": "error", "service": SERVICE_NAME, "detail": str(failed)}, status=503)
        return web.json_response({"status": "ok", "service": SERVICE_NAME})

    async def metrics(_req: web.Request) -> web.Response:
        snap = app["metrics"].snapshot()
        eng = app["engine"]
        st = getattr(eng, "last_stats", None)
        if st:
            snap["last_request"] = st
        if hasattr(eng, "engine_stats"):
            snap["engine"] = eng.engine_stats()
        ss = getattr(eng, "summary_stats", None)
        if ss is not None:
            snap["summaries"] = ss["summaries"]
            snap["summary_tokens"] = ss["summary_tokens"]
            snap["summary_mean_n_kept"] = round(ss["n_kept_sum"] / ss["summary_tokens"], 3) if ss["summary_tokens"] else 0.0
        return web.json_response(snap)

    async def call(eng, messages):
        if hasattr(eng, "submit_async"):
            # continuous batching: concurrent requests decode together on the scheduler thread
            eng.start()
            return json.loads(await asyncio.wrap_future(eng.submit_async(messages)))
        async with app["lock"]:  # engines without a scheduler: serial requests
            return await asyncio.get_running_loop().run_in_executor(None, eng, messages)

    async def on_cleanup(_app):
        if hasattr(app["engine"], "stop"):
            app["engine"].stop()

    async def parse(req: web.Request) -> web.Response:
        m: Metrics = app["metrics"]
        t0 = time.perf_counter()
        try:
            body = await req.json()
        except Exception:  # noqa: BLE001
            body = None
        pr = safe_parse(ParseRequest, body)
        if not pr.success:
            m.inc("invalid_request")
            return web.json_response({"error": "invalid_request", "detail": pr.format_error()}, status=400)
        request = pr.data
        # bounded context: whatever a client accumulated, the prompt stays
        # inside the model's window (oldest keys evicted first)
        if isinstance(request.get("context"), dict):
            request = {**request, "context": cap_context(request["context"])}
        eng = app["engine"]
        try:
            out = await call(eng, messages_for(request))
            first = safe_parse(ParseResponse, out)
            if not first.success:
                m.inc("repairs")
                out = await call(eng, messages_for(request, repair=True))
        except Exception as e:  # noqa: BLE001
            m.inc("llm_error")
            return web.json_response({"error": "llm_error", "detail": str(e) or e.__class__.__name__}, status=500)
        final = safe_parse(ParseResponse, out)
        if not final.success:
            m.inc("schema_validation_failed")
            return web.json_response({"error": "schema_validation_failed", "detail": final.format_error()}, status=422)
        m.observe("parse_ms", (time.perf_counter() - t0) * 1e3)
        m.inc("ok")
        st = getattr(eng, "last_stats", None) or {}
        if "prefill_ms" in st:  # engine-side request spans (TTFT ~ queue + prefill; decode rate)
            m.observe("ttft_ms", st.get("queue_ms", 0.0) + st["prefill_ms"])
            m.observe("decode_ms", st["decode_ms"])
            if st.get("decode_ms", 0) > 0:
                toks = st.get("decode_steps", 0) + st.get("forced_tokens", 0)
                m.observe("decode_tok_per_s", toks / (st["decode_ms"] / 1e3))
        return web.json_response(final.data)

    async def turn(req: web.Request) -> web.Response:
        """How likely the transcript is a finished command (LLMIntentEngine.turn).  The probe reads
        only the text: a ``context`` is accepted, as ``/parse`` clients send one, and ignored."""
        m: Metrics = app["metrics"]
        t0 = time.perf_counter()
        try:
            body = await req.json()
        except Exception:  # noqa: BLE001
            body = None
        text = body.get("text") if isinstance(body, dict) else None
        if not isinstance(text, str) or not text.strip() \
                or not isinstance(body.get("context", {}), dict):
            m.inc("invalid_request")
            return web.json_response({"error": "invalid_request",
                                      "detail": "body must be {\"text\": non-empty string, \"context\"?: object}"},
                                     status=400)
        eng = app["engine"]
        if not hasattr(eng, "turn_async"):
            m.inc("turn_unsupported")
            return web.json_response({"error": "turn_unsupported"}, status=501)
        try:
            # a scheduler engine: the probe joins the running batch (no serial lock)
            if hasattr(eng, "start"):
                eng.start()
            out = dict(await asyncio.wrap_future(eng.turn_async(text)))
        except Exception as e:  # noqa: BLE001
            m.inc("llm_error")
            return web.json_response({"error": "llm_error", "detail": str(e) or e.__class__.__name__}, status=500)
        for k in ("p_end", "logprob"):  # (JSON has no -inf: an end set at -inf reads p_end 0, logprob null)
            if not isinstance(out.get(k), (int, float)) or out[k] != out[k] or out[k] in (float("inf"), float("-inf")):
                out[k] = 0.0 if k == "p_end" else None
        m.observe("turn_ms", (time.perf_counter() - t0) * 1e3)
        m.inc("turn_ok")
        return web.json_response(out)

    async def summarize(req: web.Request) -> web.Response:
        """A spoken-style summary of a page's text (LLMIntentEngine.summary): what the executor's
        summarize intent asks for."""
        m: Metrics = app["metrics"]
        t0 = time.perf_counter()
        try:
            body = await req.json()
        except Exception:  # noqa: BLE001
            body = None
        body = body if isinstance(body, dict) else {}
        text, max_chars = body.get("text"), body.get("max_chars")
        ok = isinstance(text, str) and bool(text.strip()) \
            and all(body.get(k) is None or isinstance(body.get(k), str) for k in ("title", "url")) \
            and (max_chars is None or (isinstance(max_chars, int) and not isinstance(max_chars, bool)
                                       and SUMMARY_MIN_CHARS <= max_chars <= SUMMARY_MAX_CHARS))
        if not ok:
            m.inc("invalid_request")
            return web.json_response({"error": "invalid_request",
                                      "detail": "body must be {\"text\": non-empty string, \"title\"?: string, "
                                                f"\"url\"?: string, \"max_chars\"?: integer in [{SUMMARY_MIN_CHARS}, "
                                                f"{SUMMARY_MAX_CHARS}]}}"}, status=400)
        eng = app["engine"]
        if not hasattr(eng, "summary_async"):
            m.inc("summarize_unsupported")
            return web.json_response({"error": "summarize_unsupported"}, status=501)
        try:
            if hasattr(eng, "start"):
                eng.start()
            kw = {} if max_chars is None else {"max_chars": max_chars}
            out = dict(await asyncio.wrap_future(eng.summary_async(text, body.get("title"), body.get("url"), **kw)))
        except Exception as e:  # noqa: BLE001
            m.inc("llm_error")
            return web.json_response({"error": "llm_error", "detail": str(e) or e.__class__.__name__}, status=500)
        m.observe("summarize_ms", (time.perf_counter() - t0) * 1e3)
        m.inc("summarize_ok")
        return web.json_response(out)

    async def rescore(req: web.Request) -> web.Response:
        """Language-model scores of the recogniser's alternatives (LLMIntentEngine.rescore)."""
        m: Metrics = app["metrics"]
        t0 = time.perf_counter()
        try:
            body = await req.json()
        except Exception:  # noqa: BLE001
            body = None
        alts = body.get("alternatives") if isinstance(body, dict) else None
        if not isinstance(alts, list) or not 1 <= len(alts) <= 8 or not all(isinstance(a, str) for a in alts):
            m.inc("bad_request")
            return web.json_response({"error": "bad_request",
                                      "detail": "body must be {\"alternatives\": [1..8 strings]}"}, status=400)
        eng = app["engine"]
        if not hasattr(eng, "rescore_async"):
            m.inc("rescore_unsupported")
            return web.json_response({"error": "rescore_unsupported"}, status=501)
        m.inc("rescore_requests")
        try:
            # a scheduler engine: the alternatives join the running batch (no serial lock)
            if hasattr(eng, "start"):
                eng.start()
            out = dict(await asyncio.wrap_future(eng.rescore_async(alts)))
        except Exception as e:  # noqa: BLE001
            m.inc("llm_error")
            return web.json_response({"error": "llm_error", "detail": str(e) or e.__class__.__name__}, status=500)
        # (JSON has no -inf: an alternative the model gives no mass reads null)
        out["scores"] = [s if isinstance(s, (int, float)) and s == s and abs(s) != float("inf") else None
                         for s in out.get("scores", [])]
        m.observe("rescore_ms", (time.perf_counter() - t0) * 1e3)
        return web.json_response(out)

    app.on_cleanup.append(on_cleanup)
    app.router.add_get("/health", health)
    app.router.add_get("/metrics", metrics)
    app.router.add_post("/parse", parse)
    app.router.add_post("/turn", turn)
    app.router.add_post("/summarize", summarize)
    app.router.add_post("/rescore", rescore)
    return app


def make_engine_from_env():
    kind = knob("VWA_BRAIN_ENGINE")
    if kind == "keyword":
        from .intent_engine import FakeIntentEngine, keyword_intents

        return FakeIntentEngine(fn=keyword_intents)
    if kind == "llm":
        return build_llm_engine()
    raise ValueError(f"unknown VWA_BRAIN_ENGINE={kind!r}")


def summary_defaults_from_env(ie):
    """The summary defaults of an LLMIntentEngine from the summary knobs (VWA_SUMMARY_MAX_CHARS, _TEMPERATURE, _TOP_P, _TOP_K, _PENALTY); the default length is
    lowered where it would take more than half of the model's window (GPT-2's 1024 tokens)."""
    fit = max(SUMMARY_MIN_CHARS, (ie.engine.max_model_len // 2 - 16) // 4)
    ie.summary_defaults = dict(max_chars=min(knob("VWA_SUMMARY_MAX_CHARS"), fit),
                               temperature=knob("VWA_SUMMARY_TEMPERATURE"), top_p=knob("VWA_SUMMARY_TOP_P"),
                               top_k=knob("VWA_SUMMARY_TOP_K"), penalty=knob("VWA_SUMMARY_PENALTY"))
    return ie


def build_llm_engine(model_name: Optional[str] = None, device: Optional[str] = None):
    """Intent LLM from env: VWA_LLM_MODEL (llama3-8b | llama3-70b | llama3.2-1b | llama-tiny |
    gpt2-small | gpt2-tiny), VWA_LLM_WEIGHTS (safetensors dir; random init if unset), VWA_DTYPE
    (bf16 | fp8 weights for Llama), VWA_TP,
    VWA_MAX_SESSIONS, VWA_BUDGET_CHARS, VWA_SEED.  GPT-2 is the
    CPU config (BASELINE.json config 1): plain-text prompt layout, GPT-2 vocabulary."""
    import torch

    from ..models.config import GPT2Config, get_config
    from ..parallel.tp import init_distributed
    from ..runtime.engine import LLMEngine
    from ..runtime.weights import load_llm
    from ..tokenizer import load_tokenizer
    from .intent_engine import LLMIntentEngine
    from .prompt import llama3_chat, plain_chat

    name = model_name or knob("VWA_LLM_MODEL")
    cfg = get_config(name)
    seed = knob("VWA_SEED")
    dev = device or ("cuda" if torch.cuda.is_available() else "cpu")
    sessions = knob("VWA_MAX_SESSIONS")
    budget = knob("VWA_BUDGET_CHARS")
    wpath = knob("VWA_LLM_WEIGHTS") or None  # safetensors checkpoint (HF names)
    if isinstance(cfg, GPT2Config):
        model = load_llm(name, device=dev, seed=seed, weights_path=wpath)
        eng = LLMEngine(model, max_seqs=sessions, max_model_len=cfg.max_pos)
        eng.capture_all()
        return summary_defaults_from_env(
            LLMIntentEngine(eng, load_tokenizer("gpt2"), budget_chars=budget, chat_format=plain_chat))
    tp = init_distributed(tp_size=knob("VWA_TP"))
    model = load_llm(name, device=dev, tp=tp, seed=seed, weights_path=wpath,
                     wdtype=knob("VWA_DTYPE"))
    eng = LLMEngine(model, max_seqs=sessions, max_model_len=4096)
    from ..utils.busy_flag import from_env

    flag = from_env(create=True)  # shared-GPU deployment: no chained launch while the ASR runs
    if flag is not None and tp.size == 1:
        hold = knob("VWA_ASR_BUSY_HOLD_MS")
        eng.chain_gate = lambda: flag.busy(hold)
    eng.capture_all()
    ie = summary_defaults_from_env(
        LLMIntentEngine(eng, load_tokenizer("llama3"), budget_chars=budget, chat_format=llama3_chat))
    return TPIntentEngine(ie, tp) if tp.size > 1 else ie


def main():
    from ..utils.env import load_dotenv

    load_dotenv()
    port = knob("BRAIN_PORT")
    engine = make_engine_from_env()
    if isinstance(engine, TPIntentEngine) and engine.tp.rank != 0:
        engine.worker_loop()  # TP worker: no HTTP, follows rank 0's requests
        return
    print(f"[brain] listening on http://127.0.0.1:{port}", flush=True)
    web.run_app(build_app(engine), host="127.0.0.1", port=port, print=None)


if __name__ == "__main__":
    main()
