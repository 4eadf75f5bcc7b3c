"""Config / flag system: ONE typed settings object for every knob.

* ``load_dotenv()`` mirrors the reference's two dotenv loads (app ``.env`` then repo-root
  ``.env``; the first value wins and real environment variables are never overridden:
  apps/brain/src/server.ts:10-11).
* ``Settings`` declares every knob -- the reference's variable names verbatim (drop-in parity:
  apps/brain/src/llm.ts:7-9, apps/voice/src/server.ts:64-72, apps/executor/src/*.ts) plus the
  engine's ``VWA_*`` flags -- with its type, default and meaning.
* ``knob(name)`` is how code reads a knob: the environment value parsed with the declared type, or
  the declared default.  An undeclared name raises (a typo or an undocumented knob fails loudly;
  ``tests/test_settings_cpu.py`` also checks that every ``VWA_*`` name in the sources is declared).
  It reads the environment at call time, so a process (or a test) that changes a variable sees the
  change; ``settings()`` is the parsed snapshot a service takes at startup.
"""
from __future__ import annotations

import os
from typing import Any, Optional

from pydantic import BaseModel, Field, model_validator


def _parse_env_file(path: str) -> dict:
    out = {}
    try:
        with open(path, "r", encoding="utf-8") as fh:
            for line in fh:
                line = line.strip()
                if not line or line.startswith("#") or "=" not in line:
                    continue
                k, v = line.split("=", 1)
                k = k.strip()
                if k.startswith("export "):
                    k = k[7:].strip()
                v = v.strip()
                if len(v) >= 2 and v[0] == v[-1] and v[0] in "\"'":
                    v = v[1:-1]
                out[k] = v
    except OSError:
        pass
    return out


def load_dotenv(app_dir: Optional[str] = None) -> None:
    cwd = app_dir or os.getcwd()
    for path in (os.path.join(cwd, ".env"), os.path.join(cwd, "..", "..", ".env")):
        for k, v in _parse_env_file(path).items():
            os.environ.setdefault(k, v)


class Settings(BaseModel):
    # ---- reference variables (names kept)
    LLM_BASE_URL: str = Field("https://api.openai.com", description="reference brain LLM endpoint (unused on-node)")
    LLM_API_KEY: str = Field("", description="reference brain LLM key (unused on-node)")
    LLM_MODEL: str = Field("gpt-4o-mini", description="reference brain model name (reported in /health)")
    BRAIN_PORT: int = Field(8090, description="brain HTTP port")
    VOICE_PORT: int = Field(7072, description="voice HTTP/WS port (the DP router's port with several workers)")
    WEB_PORT: int = Field(5173, description="web UI port")
    EXECUTOR_PORT: int = Field(7081, description="executor HTTP port")
    DEEPGRAM_API_KEY: Optional[str] = Field(None, description="reference STT key (unused: on-node ASR)")
    DEEPGRAM_MODEL: str = Field("nova-3", description="reference STT model name (unused)")
    BRAIN_URL: str = Field("http://127.0.0.1:8090/parse", description="voice -> brain /parse URL")
    EXECUTOR_URL: str = Field("http://127.0.0.1:7081", description="voice -> executor base URL")
    ARTIFACTS_DIR: str = Field(".artifacts", description="executor screenshots / extracts")
    UPLOAD_DIR: str = Field(".uploads", description="executor file uploads")
    EXECUTOR_HEADLESS: bool = Field(False, description="launch the local browser headless")
    CDP_URL: Optional[str] = Field(None, description="attach the executor to a running browser's DevTools endpoint")
    CHROME_PATH: Optional[str] = Field(None, description="browser binary for the local session")
    BROWSERBASE_API_KEY: Optional[str] = Field(None, description="Browserbase cloud sessions")
    BROWSERBASE_PROJECT_ID: Optional[str] = Field(None, description="Browserbase project")
    BROWSERBASE_API_BASE: str = Field("https://api.browserbase.com/v1", description="Browserbase REST base")
    # ---- services / deployment
    VWA_BRAIN_ENGINE: str = Field("keyword", description="brain engine: keyword | llm | gpt2")
    VWA_ASR_ENGINE: str = Field("none", description="voice recognizer: none (passthrough) | whisper")
    VWA_ASR_MODEL: str = Field("whisper-tiny", description="Whisper config name (models/config.py)")
    VWA_ASR_WEIGHTS: Optional[str] = Field(None, description="safetensors checkpoint for the ASR (random init otherwise)")
    VWA_LLM_MODEL: str = Field("llama3-8b", description="Llama config name (models/config.py)")
    VWA_LLM_WEIGHTS: Optional[str] = Field(None, description="safetensors checkpoint for the LLM (random init otherwise)")
    VWA_DTYPE: str = Field("bf16", description="LLM weight dtype: bf16 | fp8")
    VWA_SEED: int = Field(0, description="random-init seed / sampling seed")
    VWA_TP: int = Field(1, description="tensor-parallel degree of the brain")
    VWA_DP: int = Field(1, description="voice workers behind the session router")
    VWA_MAX_SESSIONS: int = Field(8, description="concurrent sessions per engine (ASR slots, LLM sequences)")
    VWA_BUDGET_CHARS: int = Field(512, description="intent JSON character budget (grammar closes within it)")
    VWA_BRAIN_GPUS: str = Field("", description="launch.py: brain GPU list override")
    VWA_VOICE_GPUS: str = Field("", description="launch.py: voice GPU list override")
    VWA_VOICE_BASE_PORT: int = Field(7100, description="first port of the per-GPU voice workers")
    VWA_BRAIN_MAX_RESTARTS: int = Field(5, description="brain (TP group) restarts per 10 min before giving up")
    VWA_MASTER_PORT: Optional[str] = Field(None, description="TP rendezvous port of the first brain start")
    VWA_SHARED_CHAIN: str = Field("0", description="brain sharing its GPU with a voice worker keeps the chained decode")
    VWA_SHARED_CHAIN_GRID_DIV: Optional[str] = Field(None, description="that chained launch on CUs / k workgroups")
    VWA_SHARED_GB: float = Field(0.0, description="HBM a co-located service keeps (KV auto-sizing leaves it free)")
    VWA_WATCHDOG_S: float = Field(2.0, description="DP router: health poll period")
    VWA_WATCHDOG_FAILS: int = Field(2, description="DP router: failed polls before a worker is declared dead")
    VWA_TP_HEARTBEAT_S: float = Field(5.0, description="idle TP leader control heartbeat")
    VWA_TP_CONTROL: str = Field("shm", description="TP brain per-iteration control channel: shm (/dev/shm ring, parallel/control.py) or gloo (broadcast)")
    VWA_TP_DEAD_S: float = Field(60.0, description="TP worker: the leader counts as dead after this long without a control message or heartbeat (shm channel)")
    VWA_DIST_BACKEND: Optional[str] = Field(None, description="torch.distributed backend override (nccl = RCCL)")
    VWA_CUSTOM_AR: bool = Field(True, description="one-shot IPC all-reduce for small TP messages (else RCCL)")
    VWA_BROWSER_DRIVER: str = Field("auto", description="executor browser driver: auto | cdp | playwright")
    VWA_LLAMA_TOKENIZER: Optional[str] = Field(None, description="tokenizer.json for the Llama brain (bundled otherwise)")
    VWA_WHISPER_TOKENIZER: Optional[str] = Field(None, description="tokenizer.json for Whisper (bundled otherwise)")
    VWA_GPT2_TOKENIZER: Optional[str] = Field(None, description="tokenizer.json for the GPT-2 brain (bundled otherwise)")
    # ---- voice path (streaming ASR / debounce)
    VWA_DEBOUNCE_MS: float = Field(1000.0, description="final transcript -> brain call debounce (reference: 1000)")
    VWA_COMMIT_MS: float = Field(0.0, description="voice: silence after the speech end before pending finals are a command (0: the ASR endpoint; speech resuming earlier holds them -- voice/server.py commit policy)")
    VWA_SPEC_BRAIN: bool = Field(True, description="voice: start the brain on the ASR's speculative final pass (its answer is used only for exactly that text)")
    VWA_TURN: bool = Field(False, description="voice: ask the brain's turn-completion probe (POST /turn) whether the pending text is a finished command and, if it says so, commit without waiting out VWA_COMMIT_MS (0, the default: no request is ever made to /turn and every timing is the fixed timer's)")
    VWA_TURN_URL: Optional[str] = Field(None, description="voice -> brain /turn URL (default: BRAIN_URL with /parse replaced by /turn)")
    VWA_TURN_THRESHOLD: float = Field(0.5, gt=0.0, le=1.0, description="voice: a pending text whose probe answers p_end >= this is a finished command. In (0, 1]; 1.0 never commits early. 0.5 is a policy default and is NOT tuned on real speech or real weights")
    VWA_COMMIT_MIN_MS: float = Field(0.0, ge=0.0, description="voice: silence after the speech end before a command the turn probe judged complete is committed (0: as soon as the verdict and the ASR final are both there)")
    VWA_RESCORE: bool = Field(False, description="voice: rescore a beam final's n-best alternatives with the brain's language model (POST /rescore) before the text joins the pending command, and take the alternative with the best acoustic + VWA_RESCORE_WEIGHT x language-model score; the recogniser's final events then carry every alternative's logprob. Needs VWA_ASR_BEAM and VWA_ASR_ALTERNATIVES >= 2 (0, the default: no request is ever made to /rescore and every event and frame is what it was)")
    VWA_RESCORE_URL: Optional[str] = Field(None, description="voice -> brain /rescore URL (default: BRAIN_URL with /parse replaced by /rescore)")
    VWA_RESCORE_WEIGHT: float = Field(0.5, ge=0.0, description="voice: weight of the language-model score against the recogniser's acoustic sum log-probability in n-best rescoring (0: the recogniser's order stands). >= 0; 0.5 lies in the range n-best rescoring commonly uses and is NOT tuned on real speech or real weights")
    VWA_SUMMARIZE: bool = Field(False, description="executor: the summarize intent reads the page's title, url and visible text and asks the brain (POST /summarize) for a spoken-style summary (0, the default: the step answers the fixed note it always did and no request is made)")
    VWA_SUMMARIZE_URL: Optional[str] = Field(None, description="executor -> brain /summarize URL (default: BRAIN_URL with /parse replaced by /summarize)")
    VWA_SUMMARY_PAGE_CHARS: int = Field(20000, ge=1, description="executor: at most this many characters of the page's visible text are sent to /summarize (the brain cuts further, by tokens, to its context window)")
    VWA_SUMMARY_MAX_CHARS: int = Field(400, ge=1, le=4096, description="brain: default upper bound of a summary's length in characters (a request's max_chars overrides it; lowered where the model's window leaves no room for it)")
    VWA_SUMMARY_TEMPERATURE: float = Field(0.7, gt=0.0, description="brain: sampling temperature of summaries. The four summary sampling defaults are the values common for free text; they are policy defaults and are NOT tuned on real weights or real pages")
    VWA_SUMMARY_TOP_P: float = Field(0.9, gt=0.0, description="brain: nucleus (top-p) mass of summaries, taken over the renormalised top-k (>= 1: no cut)")
    VWA_SUMMARY_TOP_K: int = Field(50, ge=1, le=1024, description="brain: top-k of summaries (the nucleus kernel sorts at most 1024 candidates)")
    VWA_SUMMARY_PENALTY: float = Field(1.1, gt=0.0, description="brain: repetition penalty of summaries over the last 64 sampled answer tokens (1: none)")
    VWA_ASR_BUSY_FILE: Optional[str] = Field(None, description="/dev/shm word the voice worker's ASR batcher marks busy while recognition runs (shared-GPU deployment: the brain's decode uses the chained launch only while it is idle; launch.py sets it)")
    VWA_ASR_BUSY_HOLD_MS: float = Field(20.0, description="brain: keep the per-kernel decode form this long after the last ASR pass ended")
    VWA_ENDPOINT_MS: float = Field(300.0, description="trailing silence that ends an utterance (VAD endpoint)")
    VWA_SPEC_FINAL_MS: float = Field(120.0, description="trailing silence that starts the speculative final pass (0: off)")
    VWA_VAD_THRESHOLD: float = Field(300.0, description="speech frame RMS floor (PCM16 units)")
    VWA_VAD_NOISE_MULT: float = Field(3.0, description="speech frame RMS >= this x the tracked noise floor")
    VWA_PARTIAL_EVERY_S: float = Field(1.0, description="interim result period during speech")
    VWA_ASR_TOKENS_PER_S: float = Field(0.0, description="fixed-work transcripts (benchmarks on random weights; 0: off)")
    VWA_ASR_WORDS: bool = Field(False, description="final transcript events carry per-word start / end / confidence and the transcript confidence (an alignment pass after each final recognition pass: csrc/align)")
    VWA_ASR_LANGUAGE: str = Field("en", description="spoken language of the recognizer: a Whisper language code, or auto (detected per utterance from the logits at the start-of-transcript position: csrc/sot; one extra one-row decoder step per pass)")
    VWA_ASR_LANGUAGES: Optional[str] = Field(None, description="comma list of language codes that detection may report (unset: every language of the model)")
    VWA_ASR_TASK: str = Field("transcribe", description="Whisper task: transcribe | translate (to English)")
    VWA_ASR_NO_SPEECH: float = Field(0.0, description="no-speech gate: a window whose no-speech probability exceeds this yields an empty final and no partial (0: off; Whisper's customary threshold is 0.6)")
    VWA_ASR_BEAM: int = Field(1, ge=1, le=8, description="beam width of the final recognition passes (1: greedy, the default; 2-8: beam search, csrc/beam -- a final pass then takes this many ASR session slots; partials and speculative passes stay greedy)")
    VWA_ASR_ALTERNATIVES: int = Field(1, ge=1, le=8, description="ranked alternatives a final transcript event carries (Deepgram's alternatives; 1..VWA_ASR_BEAM)")
    VWA_ASR_LONGFORM: bool = Field(False, description="long utterances: when the 30 s window fills while the speaker is still talking, cut it at the end of the last segment a timestamp pass closes (csrc/tsrules, asr/segments.py) and carry the rest of the audio over, instead of finalising the whole window at an arbitrary sample (0, the default: today's whole-window final)")
    VWA_ASR_LONGFORM_MIN_S: float = Field(10.0, ge=0.0, le=30.0, description="the earliest segment end, in seconds from the window's start, a long-form cut is taken at; an earlier one is ignored (the window would refill almost at once) and the whole window is finalised. 10 s is a policy default and is NOT tuned on real speech")
    VWA_ASR_FALLBACK: bool = Field(False, description="Whisper's quality gate and temperature fallback on the final recognition passes: a final whose average token log-probability is below VWA_ASR_LOGPROB_THRESHOLD or whose text compresses better than VWA_ASR_COMPRESSION_RATIO is decoded again at the next of VWA_ASR_TEMPERATURES, on the kept encoder output (csrc/score, asr/fallback.py); a greedy final's confidence is then exp(average log-probability). 0, the default: off, nothing of it is loaded or launched")
    VWA_ASR_TEMPERATURES: str = Field("0,0.2,0.4,0.6,0.8,1.0", description="the fallback's temperature schedule: a comma list, non-decreasing, each in [0, 2], at most 8 (Whisper's published default)")
    VWA_ASR_LOGPROB_THRESHOLD: float = Field(-1.0, le=0.0, description="a final whose average token log-probability is below this is rejected. -1.0 is Whisper's published default and is NOT tuned here on real speech")
    VWA_ASR_COMPRESSION_RATIO: float = Field(2.4, gt=0.0, description="a final whose text's zlib compression ratio exceeds this (a transcript that loops) is rejected. 2.4 is Whisper's published default and is NOT tuned here on real speech")
    VWA_ASR_FALLBACK_REJECT: bool = Field(False, description="1: a final whose last fallback attempt still fails the quality gate is emitted empty, like a no-speech-gated final, so a hallucinated command never reaches the brain (0, the default: the last attempt is emitted, as Whisper does)")
    VWA_ASR_KEYTERMS: str = Field("", description="default keyterms of every voice session: a comma list of words or phrases the recogniser should prefer, each with an optional :boost (Deepgram's keyterm; csrc/boost); empty, the default: keyterm boosting is off unless a client names terms (/stream?keyterm=...)")
    VWA_ASR_KEYTERM_BOOST: float = Field(2.0, gt=0.0, le=20.0, description="boost, in logit units (nats), of a keyterm that names none: the odds of its tokens are multiplied by e^boost. In (0, 20]; 2.0 is in the range the shallow-fusion literature commonly uses and is NOT tuned on real speech")
    VWA_CONTEXT_MAX_BYTES: int = Field(2048, description="per-session context cap sent to the brain")
    # ---- engine
    VWA_HIPGRAPH: bool = Field(True, description="replay decode steps from captured hipGraphs")
    VWA_KV_GB: str = Field("0", description="paged-KV budget in GB, 0: per max_seqs x max_len, auto: HBM plan")
    VWA_ROW_BUCKETS: str = Field("1,2,4,8,12,16,32,48,64", description="decode row buckets of the captured graphs")
    VWA_SHARED_ATTN: bool = Field(True, description="decode attention reads a shared prompt prefix once per row group")
    VWA_PREFILL_FLASH: bool = Field(True, description="batched admission prefill through one causal flash launch")
    VWA_RMS_HANDOFF: bool = Field(True, description="> 16-row steps: residual GEMMs hand the next RMSNorm its row statistics (no row_rstd launches)")
    VWA_FP8_A16_ROWS: int = Field(64, description="fp8 weights: rows up to which the > 16-row GEMM runs W8A16 (no activation quantisation)")
    VWA_PREFILL_DECODE_ATTN: bool = Field(True, description="cached-prefix prompt suffix through the decode attention")
    VWA_TILED_WEIGHTS: bool = Field(True, description="keep projection weights only in the MFMA-tiled layout")
    VWA_MASKED_HEAD: bool = Field(True, description="LM head computes only the vocab tiles the grammar admits")
    VWA_SPIN_WAIT: bool = Field(True, description="wait for a step's tokens by polling the pinned readback")
    VWA_ZERO_COPY: bool = Field(True, description="grammar masks written straight into pinned step memory")
    VWA_ASR_DEVICE_LOOP: bool = Field(True, description="single-session Whisper greedy loop resident on the GPU")
    VWA_CHAIN: bool = Field(True, description="chained Llama decode layer (skinny_stream.hip chain_kernel)")
    VWA_CHAIN_ATTN: bool = Field(True, description="decode attention as the chained launch's phase 0")
    VWA_CHAIN_MAX_ROWS: int = Field(4, description="rows per step the chained launch takes")
    VWA_CHAIN_TP: bool = Field(True, description="chained launch with in-launch TP all-reduce rounds")
    VWA_CHAIN_RETRY: bool = Field(True, description="re-arm the chain after a barrier-timeout fallback")
    VWA_CHAIN_ASR: bool = Field(False, description="chained Whisper decoder launches (measured slower; off)")
    VWA_WDEC_OPT: int = Field(0, description="diagnostic: schedule option bits of the persistent Whisper decoder (whisper_dec.hip kOpt*; 0 = the measured defaults)")
    VWA_ASR_PERSIST: bool = Field(True, description="one-row Whisper decode steps (every width, tiny .. large) as ONE persistent launch: embedding, every decoder layer, LM head and, in the device loop, argmax + advance (csrc/kernels/whisper_dec.hip); needs every CU free: off when the GPU is shared with a persistent brain launch")
    VWA_CHAIN_GRID_DIV: Optional[str] = Field(None, description="chained launch on CUs / k workgroups (shared GPU)")
    VWA_CHAIN_PLAN: bool = Field(True, description="chained attention: layer 0 writes the step's work plan, layers 1.. read it")
    VWA_CHAIN_MULTI: bool = Field(True, description="chained decode: all layers in ONE launch (skinny_stream.hip chain_kernel MULTI)")
    VWA_CHAIN_PACK: bool = Field(True, description="chained decode (bf16, one rank, <= 4 rows): stream a lossless 13-bit form of the layer weights (ops.pack_weight; 0.81 x the bytes, the same output bits) kept next to the tiled bf16 copy, about 0.8 x the layer weights' size in extra memory")
    VWA_CHAIN_WNT: bool = Field(True, description="chained decode with the attention phase (packed, bf16, fp8): load the pre-tiled weight stream non-temporally (skinny_stream.hip chain_wnt_kernel; the same output bits)")
    VWA_STREAM_WNT: bool = Field(True, description="Llama <= 16-row streaming GEMMs (LM head, 5..16-row steps): load the pre-tiled layer and LM-head weights non-temporally (SkinnyParams::w_nt; the same output bits)")
    VWA_CHAIN_BAR_MODE: int = Field(2, description="chained launches' grid barrier: 2 two-level tickets + scalar polls (default), 4 no-return arrivals + polled sum of the 8 group counters")
    VWA_CHAIN_SCHED: Optional[str] = Field(None, description="DIAGNOSTIC: chained schedule override name=value,...")
    VWA_GEMM_QKV: bool = Field(True, description="> 16-row QKV: rotary + KV write in the tiled GEMM epilogue")
    VWA_GEMM_P8: Optional[str] = Field(None, description="DIAGNOSTIC: 256x256 8-phase GEMM eligibility override")
    VWA_GEMM_SPLIT_FILL: Optional[str] = Field(None, description="DIAGNOSTIC: split-K fill target (% of CUs)")
    VWA_SKINNY_X_SKEW: Optional[str] = Field(None, description="DIAGNOSTIC: LDS X-row skew of the streaming GEMM")
    VWA_ATTN_IMPL: Optional[str] = Field(None, description="DIAGNOSTIC: decode attention implementation")
    VWA_KERNEL_SO: Optional[str] = Field(None, description="DIAGNOSTIC: another build of the kernel library (A/B)")
    VWA_STRICT_NATIVE: bool = Field(False, description="vendor-library fallbacks in the op layer raise (tests, bench)")
    VWA_BENCH_CONCURRENT: int = Field(0, description="bench.py --full: concurrent sessions (0: the headline only)")
    # ---- build
    VWA_FORCE_BUILD: bool = Field(False, description="__graft_entry__.build(): recompile every source")
    VWA_HIPCC_EXTRA: str = Field("", description="extra hipcc flags (experiments)")

    @model_validator(mode="after")
    def _alternatives_within_beam(self):
        if self.VWA_ASR_ALTERNATIVES > self.VWA_ASR_BEAM:
            raise ValueError(f"VWA_ASR_ALTERNATIVES={self.VWA_ASR_ALTERNATIVES} exceeds VWA_ASR_BEAM={self.VWA_ASR_BEAM}: "
                             "a beam of W hypotheses has no more than W alternatives")
        if self.VWA_RESCORE and self.VWA_ASR_ALTERNATIVES < 2:
            raise ValueError("VWA_RESCORE=1 needs alternatives to rescore: set VWA_ASR_BEAM and VWA_ASR_ALTERNATIVES "
                             f"to 2..8 (VWA_ASR_ALTERNATIVES={self.VWA_ASR_ALTERNATIVES})")
        return self

    @classmethod
    def from_env(cls) -> "Settings":
        return cls(**{name: knob(name) for name in cls.model_fields})


_TRUE = ("1", "true", "yes", "on")


def _parse(name: str, raw: str) -> Any:
    ann = Settings.model_fields[name].annotation
    raw = raw.strip()
    if ann is bool:
        return raw.lower() in _TRUE
    if ann is int:
        return int(raw) if raw else Settings.model_fields[name].default
    if ann is float:
        return float(raw) if raw else Settings.model_fields[name].default
    return raw


def knob(name: str) -> Any:
    """The typed value of a declared knob: the environment's (parsed with the declared type) or the
    declared default.  Raises KeyError for an undeclared name and ValueError for an unparsable
    value (a bad setting is an error, not a silent default)."""
    field = Settings.model_fields.get(name)
    if field is None:
        raise KeyError(f"undeclared knob {name!r}: add it to utils/env.py Settings")
    raw = os.environ.get(name)
    if raw is None:
        return field.default
    try:
        return _parse(name, raw)
    except ValueError as e:
        raise ValueError(f"{name}={raw!r}: {e}") from e


def asr_beam_knobs(beam: Optional[int] = None, alternatives: Optional[int] = None) -> tuple:
    """(beam width, alternatives) of the final recognition passes: the arguments, else VWA_ASR_BEAM /
    VWA_ASR_ALTERNATIVES.  A width outside 1-8 or alternatives outside 1..width is an error (at
    startup: the voice worker reads them when it builds its engine)."""
    b = int(knob("VWA_ASR_BEAM") if beam is None else beam)
    a = int(knob("VWA_ASR_ALTERNATIVES") if alternatives is None else alternatives)
    if not 1 <= b <= 8:
        raise ValueError(f"VWA_ASR_BEAM={b}: the beam width must be in 1..8")
    if not 1 <= a <= b:
        raise ValueError(f"VWA_ASR_ALTERNATIVES={a}: must be in 1..VWA_ASR_BEAM={b}")
    return b, a


def settings() -> Settings:
    """A parsed snapshot of every knob (services take one at startup)."""
    return Settings.from_env()
