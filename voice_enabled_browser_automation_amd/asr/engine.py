"""ASR engine: on-node Whisper transcription (replaces the Deepgram live socket,
apps/voice/src/deepgram.ts:21-67).

`WhisperRunner` owns static decoder buffers for up to ``max_sessions`` concurrent utterances
(one row per session per step -> continuous batching across voice sessions, the DP unit of a
GPU) and captures one hipGraph per row bucket.  `AsrEngine.transcribe` runs
PCM16 -> f32 (HIP) -> log-mel (HIP) -> encoder -> cross K/V -> greedy constrained decode.
"""
from __future__ import annotations

import time
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import ops
from ..models.whisper import WhisperModel
from ..tokenizer.languages import language_code, language_index, language_token
from . import beam as beam_rule
from .logit_steps import (TS_MAX_INITIAL, BoostBuffers, BoostRun, LogitSteps, ScoreBuffers,  # noqa: F401
                          ScoreRun, TsBuffers, TsRun, ts_state)  # (TS_MAX_INITIAL, ts_state: also read from here)
from .segments import segments
from .words import Alignment, group_words

BUCKETS = (1, 2, 4, 8, 16, 32, 64)


class RunnerBuffers(SimpleNamespace):
    """The decoder step's fixed-address buffers.  Hashable by identity and weak-referenceable:
    the model's chained-launch descriptors (raw pointers into these buffers) are cached per
    buffers object in a WeakKeyDictionary (models/whisper.py _chain_descs)."""

    __hash__ = object.__hash__

    def __eq__(self, other):
        return self is other

class WhisperRunner:
    def __init__(self, model: WhisperModel, *, max_sessions: int = 4, block_size: int = 16,
                 use_graphs: Optional[bool] = None):
        cfg = model.cfg
        self.model = model
        dev = model.device
        self.device = dev
        self.max_sessions = max_sessions
        self.bs = block_size
        self.bps = (cfg.n_text_ctx + block_size - 1) // block_size  # blocks per session
        n_blocks = max_sessions * self.bps + 1
        H, hd, d = model.H, model.hd, cfg.d_model
        R = max(BUCKETS)
        i32 = dict(dtype=torch.int32, device=dev)
        b = RunnerBuffers()
        # one device block for a step's inputs (tokens | positions | seq_ids | ctx_lens | slots as
        # int64) and its pinned mirror: ONE host->device copy per step (five separate copies were
        # 7 % of the 32-session batched decode's GPU time, profiles/r4_asr_tiny_batch32_kernel_stats.md)
        b.step_in = torch.zeros(6 * R, **i32)
        b.tokens, b.positions, b.seq_ids, b.ctx_lens = (b.step_in[i * R : (i + 1) * R] for i in range(4))
        b.slots = b.step_in[4 * R :].view(torch.int64)
        b.ctx_lens.fill_(1)
        b.slots.fill_(-1)
        b.block_table = torch.zeros(max_sessions, self.bps, **i32)
        for s in range(max_sessions):
            b.block_table[s] = torch.arange(1 + s * self.bps, 1 + (s + 1) * self.bps, dtype=torch.int32)
        L = cfg.n_dec_layers
        b.k_cache = torch.zeros(L, n_blocks, H, block_size, hd, dtype=model.dtype, device=dev)
        b.v_cache = torch.zeros_like(b.k_cache)
        b.max_ctx = self.bps * block_size
        b.hidden = torch.zeros(R, d, dtype=model.dtype, device=dev)
        b.h = torch.zeros_like(b.hidden)
        b.q = torch.zeros(R, d, dtype=model.dtype, device=dev)
        b.att = torch.zeros_like(b.q)
        b.f = torch.zeros(R, cfg.ffn, dtype=model.dtype, device=dev)
        b.logits = torch.zeros(R, model.vocab_padded, dtype=torch.float32, device=dev)
        ns = max(ops.decode_n_splits(b.max_ctx), ops.decode_n_splits(cfg.n_audio_ctx))
        b.part_o = torch.zeros(R * ns * H * hd, dtype=torch.float32, device=dev)
        b.part_ml = torch.zeros(R * ns * H * 2, dtype=torch.float32, device=dev)
        b.attn_cnt = torch.zeros(R * H, dtype=torch.int32, device=dev)
        b.cross = [(torch.zeros(max_sessions, cfg.n_audio_ctx, H, hd, dtype=model.dtype, device=dev),
                    torch.zeros(max_sessions, cfg.n_audio_ctx, H, hd, dtype=model.dtype, device=dev)) for _ in range(L)]
        b.cross_table = torch.arange(max_sessions, dtype=torch.int32, device=dev)[:, None].contiguous()
        b.cross_lens = torch.full((R,), cfg.n_audio_ctx, dtype=torch.int32, device=dev)
        self.b = b
        pin = dev.type == "cuda"
        self.h_in = torch.zeros(6 * R, dtype=torch.int32, pin_memory=pin)
        self.h_i32 = self.h_in[: 4 * R].view(4, R)
        self.h_slots = self.h_in[4 * R :].view(torch.int64)
        self.h_i32[3].fill_(1)
        self.h_slots.fill_(-1)
        if use_graphs is None:
            use_graphs = ops.env_flag("VWA_HIPGRAPH")
        self.use_graphs = bool(use_graphs) and dev.type == "cuda"
        self.graphs: Dict[int, Tuple[torch.cuda.CUDAGraph, torch.Tensor]] = {}
        self.pool = None
        self._copy_done: Optional["torch.cuda.Event"] = None  # the last step's staging copy (step())

    def set_cross(self, slot: int, enc_states: torch.Tensor) -> None:
        """Compute this session's cross-attention K/V from encoder states [1, T, d]."""
        kvs = self.model.cross_kv(enc_states)
        for li, (k, v) in enumerate(kvs):
            self.b.cross[li][0][slot].copy_(k[0])
            self.b.cross[li][1][slot].copy_(v[0])

    def _fwd(self, M: int) -> torch.Tensor:
        return self.model.decode_step(self.b, M)

    def _capture(self, M: int):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self._fwd(M)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        if self.pool is None:
            self.pool = torch.cuda.graph_pool_handle()
        with torch.cuda.graph(g, pool=self.pool):
            out = self._fwd(M)
        self.graphs[M] = (g, out)
        return self.graphs[M]

    def step(self, rows: Sequence[Tuple[int, int, int]], fwd=None, pre=None) -> torch.Tensor:
        """rows: (session slot, token, position). Returns f32 logits [len(rows), vocab_padded].
        ``fwd``: the forward to run on the staged rows instead of the (graph-replayed) decode step --
        ``fwd(M) -> logits`` (the word-alignment pass, never captured).
        ``pre``: called between the staging copy and the forward / graph replay -- stream-ordered
        work that rewrites staged rows on the device (the SOT probe putting a detected language
        token into ``b.tokens``: AsrEngine._prompt_auto)."""
        n = len(rows)
        M = next(bk for bk in BUCKETS if bk >= n)
        if self._copy_done is not None:
            # the previous step's pinned -> device copy may still be queued behind its forward:
            # rewriting the pinned rows before it ran would feed that step the NEXT step's tokens /
            # positions / slots (back-to-back step() calls with no host sync in between; the
            # one-launch decoder leaves the host far ahead of the GPU)
            self._copy_done.synchronize()
        hi = self.h_i32
        for i, (slot, tok, pos) in enumerate(rows):
            hi[0, i], hi[1, i], hi[2, i], hi[3, i] = tok, pos, slot, pos + 1
            blk = 1 + slot * self.bps + pos // self.bs
            self.h_slots[i] = blk * self.bs + pos % self.bs
        for i in range(n, M):
            hi[0, i], hi[1, i], hi[2, i], hi[3, i] = 0, 0, 0, 1
            self.h_slots[i] = -1
        b = self.b
        b.step_in.copy_(self.h_in, non_blocking=True)
        if self.device.type == "cuda":
            if self._copy_done is None:
                self._copy_done = torch.cuda.Event()
            self._copy_done.record()
        if pre is not None:
            pre()
        if fwd is not None:
            out = fwd(M)
        elif self.use_graphs:
            g, out = self.graphs.get(M) or self._capture(M)
            g.replay()
        else:
            out = self._fwd(M)
        return out[:n]


class AsrEngine:
    """Whisper transcription with fixed-work decoding options for benchmarking."""

    def __init__(self, model: WhisperModel, tokenizer, *, max_sessions: int = 4, use_graphs: Optional[bool] = None,
                 language: Optional[str] = None, task: Optional[str] = None,
                 languages_allowed: Optional[Sequence[str]] = None, no_speech_threshold: Optional[float] = None):
        """language: the default language code of a session, or "auto" (detect per pass);
        task: "transcribe" | "translate"; languages_allowed: codes detection may report (None: all
        the model has); no_speech_threshold: a session whose no-speech probability exceeds it is
        reported as gated (0: the probability is not computed).  None: the VWA_ASR_LANGUAGE /
        VWA_ASR_TASK / VWA_ASR_LANGUAGES / VWA_ASR_NO_SPEECH settings."""
        from ..utils.env import knob

        self.model = model
        self.tok = tokenizer
        cfg = model.cfg
        self.runner = WhisperRunner(model, max_sessions=max_sessions, use_graphs=use_graphs)
        dev = model.device
        W = (model.vocab_padded + 31) // 32
        text_ids = np.arange(model.vocab_padded) < cfg.eot
        self.mask_text = torch.from_numpy(self._pack(text_ids)).to(dev)[None]
        with_eot = text_ids.copy()
        with_eot[cfg.eot] = True
        self.mask_text_eot = torch.from_numpy(self._pack(with_eot)).to(dev)[None]
        self.d_seed = torch.zeros(1, dtype=torch.int64, device=dev)
        self.d_step = torch.zeros(1, dtype=torch.int32, device=dev)
        # the sampler's tokens, one per row of the largest step: ONE buffer for the engine's life --
        # captured loop graphs read it, and eager code hands them a token through it
        self.d_tok = torch.zeros(max(max_sessions, max(BUCKETS)), dtype=torch.int32, device=dev)
        self.part_val = torch.zeros(64, dtype=torch.float32, device=dev)
        self.part_idx = torch.zeros(64, dtype=torch.int32, device=dev)
        self.language = str(knob("VWA_ASR_LANGUAGE") if language is None else language).strip().lower()
        self.task = str(knob("VWA_ASR_TASK") if task is None else task).strip().lower()
        if languages_allowed is None:
            languages_allowed = knob("VWA_ASR_LANGUAGES") or None
        if isinstance(languages_allowed, str):
            languages_allowed = [c for c in (x.strip() for x in languages_allowed.split(",")) if c]
        self.allow = (1 << cfg.n_langs) - 1  # bit i: detection may report language i
        if languages_allowed:
            self.allow = sum({1 << language_index(cfg, c) for c in languages_allowed})
        self.no_speech_threshold = float(knob("VWA_ASR_NO_SPEECH") if no_speech_threshold is None
                                         else no_speech_threshold)
        # an "auto" session's language row until the probe patches it: the lowest allowed language
        self._lang_placeholder = cfg.lang_en + (self.allow & -self.allow).bit_length() - 1
        # the default session's SOT sequence (an "auto" default: the placeholder language)
        self.prompt = [cfg.sot,
                       self._lang_placeholder if self.language == "auto" else language_token(cfg, self.language),
                       self._task_id(self.task), cfg.no_timestamps]
        # decode_many: one entry per utterance of the last call -- language (code), language_confidence,
        # no_speech_prob, gated; with keep_sot also "logits" (the SOT row, host) and "lang_probs"
        self.last_sot: List[Dict] = []
        # device-resident single-session decode loop (graphs keyed by (slot, eot allowed))
        self.loop_out = torch.zeros(max(448, cfg.n_text_ctx), dtype=torch.int32, device=dev)
        self.loop_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        self.loop_graphs: Dict[Tuple[int, bool, int, bool, bool], torch.cuda.CUDAGraph] = {}
        self.device_loop = self.runner.use_graphs and ops.env_flag("VWA_ASR_DEVICE_LOOP")
        self.last_stats: Dict[str, float] = {}
        # decode_many(words=True): one entry per utterance of the last call (asr/words.py Alignment)
        self.last_alignments: List[Alignment] = []
        # decode_many(beam_size >= 2): per utterance its ranked hypotheses {tokens, sum_logprob, avg_logprob};
        # with keep_beam_trace also one entry per step of the last call (_decode_beams)
        self.last_beams: List[List[Dict]] = []
        self.last_beam_trace: List[Dict] = []
        # decode_many(keyterms=...): the keyterm tables' device memory (BoostBuffers), built by the first
        # boosted call; with keep_boost_trace one entry per boosting launch of the last call (BoostRun)
        self._boost_bufs: Optional[BoostBuffers] = None
        self.last_boost_trace: List[Dict] = []
        # decode_many(timestamps=...): the rules' device memory (TsBuffers) and the two masks (text and
        # timestamps, without / with EOT), built by the first timestamp call; per utterance of the last
        # call its segments (asr/segments.py; None: decoded without timestamps); with keep_ts_trace one
        # entry per rules launch of the last call (TsRun)
        self._ts_bufs: Optional[TsBuffers] = None
        self.mask_ts: Optional[torch.Tensor] = None
        self.mask_ts_eot: Optional[torch.Tensor] = None
        self.last_segments: List[Optional[List[Dict]]] = []
        self.last_ts_trace: List[Dict] = []
        # decode_many(score=True / fallback=...): the scores' device memory (ScoreBuffers), built by the
        # first scored call; per utterance of the last scored call its score entry (asr/fallback.py
        # score_entry); with keep_score_trace one entry per score launch of the last call (ScoreRun)
        self._score_bufs: Optional[ScoreBuffers] = None
        self.last_scores: List[Dict] = []
        self.last_score_trace: List[Dict] = []
        self.sample_seed = 0  # a scored call's Gumbel noise: a function of this seed, the attempt and the step
        self.free_slots = list(range(max_sessions - 1, -1, -1))

    keep_sot = False  # decode_many: always probe; keep host copies of the SOT logits and language probabilities
    keep_beam_trace = False  # decode_many with beams: keep host copies of every step's select inputs and outputs
    # decode_many with keyterms: keep, per step, each live row's history, the logits before and after
    # boosting, the automaton state and the chosen token (host copies); the call then steps from the
    # host -- a single session does not take the device loop
    keep_boost_trace = False
    # decode_many with timestamps: keep, per step, each live row's sampled tokens, the logits before
    # and after the rules, the rows' masks and the chosen tokens (host copies); the call then steps
    # from the host, as with keep_boost_trace
    keep_ts_trace = False
    # decode_many with score / fallback: keep, per step, the logits the sampler read, the rows' mask,
    # the chosen tokens and their log-probabilities (host copies); the call then steps from the host
    keep_score_trace = False

    def compile_keyterms(self, terms, boost: Optional[float] = None):
        """Text terms (strings, (text, boost) pairs) compiled for this engine's tokenizer: the
        object ``decode_many(keyterms=[...])`` takes per utterance (asr/keyterms.py; None: no terms)."""
        from . import keyterms as kt

        return kt.compile_keyterms(terms, self.tok, self.model.cfg.eot, boost)

    def _persistent_loop_ok(self, boost, ts=None, score=None) -> bool:
        """The one routing decision for the persistent one-launch decoder (wdec_loop_step): its
        argmax runs inside the kernel, before anything could bias or ban the logits, so a boosted
        call and a timestamp call never take it; nor does a scored call -- the logits never leave
        the kernel for the score launch to read, and it draws no temperature."""
        return boost is None and ts is None and score is None

    def _ts_setup(self) -> None:
        """The timestamp masks and buffers, on the first timestamp call."""
        if self._ts_bufs is not None:
            return
        m = self.model
        cfg = m.cfg
        ids = np.arange(m.vocab_padded)
        allowed = (ids < cfg.eot) | ((ids > cfg.no_timestamps) & (ids < cfg.vocab_size))
        self.mask_ts = torch.from_numpy(self._pack(allowed)).to(m.device)[None]
        allowed[cfg.eot] = True
        self.mask_ts_eot = torch.from_numpy(self._pack(allowed)).to(m.device)[None]
        self._ts_bufs = TsBuffers(m.device)

    def _mask(self, allow_eot: bool, ts: bool = False) -> torch.Tensor:
        if ts:
            return self.mask_ts_eot if allow_eot else self.mask_ts
        return self.mask_text_eot if allow_eot else self.mask_text

    def _task_id(self, task: str) -> int:
        cfg = self.model.cfg
        if task not in ("transcribe", "translate"):
            raise ValueError(f"unknown ASR task {task!r}: transcribe | translate")
        return cfg.transcribe if task == "transcribe" else cfg.translate

    @staticmethod
    def _pack(bits: np.ndarray) -> np.ndarray:
        n = (len(bits) + 31) // 32 * 32
        b = np.zeros(n, dtype=np.uint8)
        b[: len(bits)] = bits
        return np.packbits(b, bitorder="little").view(np.uint32).view(np.int32).copy()

    def pcm_to_audio(self, pcm: np.ndarray, rate: int = 16000) -> torch.Tensor:
        t = torch.from_numpy(np.ascontiguousarray(pcm, dtype=np.int16)).to(self.model.device, non_blocking=True)
        return ops.pcm16_to_f32(t, in_rate=rate)

    def wire_to_audio(self, raw, fmt) -> torch.Tensor:
        """A window of wire frames (bytes or a uint8 array, whole frames of ``fmt``: asr/wire.py
        AudioFormat) -> the 16 kHz f32 samples decode_many takes: one ops.ingest launch (G.711 / PCM16
        decode, downmix, band-limited resampling)."""
        a = np.frombuffer(raw, dtype=np.uint8).copy() if isinstance(raw, (bytes, bytearray, memoryview)) else raw
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)).to(self.model.device,
                                                                                      non_blocking=True)
        out = ops.ingest(t, fmt)
        if self.ingest_hook is not None:
            self.ingest_hook(t, fmt, out)
        return out

    # test hook: called with (raw tensor, fmt, the audio) after every wire_to_audio
    ingest_hook = None

    # ---- device-resident greedy decode (one session): step graph = forward -> masked argmax ->
    # decode_advance (sampled token becomes the next input, position / context / KV slot move on),
    # replayed back to back; the host reads the tokens once per chunk instead of once per token
    # (measured per token before: 5 metadata copies + a host round trip, ~80 us of GPU idle)
    def _loop_step(self, slot: int, allow_eot: bool, steps: LogitSteps) -> None:
        r = self.runner
        b = r.b
        # whisper-large persistent decoder: embedding, layers, LM head, argmax and advance are ONE
        # launch (models/whisper.py wdec_loop_step)
        if self._persistent_loop_ok(steps.boost, steps.ts, steps.score) and self.model.wdec_loop_step(
                b, self.mask_text_eot if allow_eot else self.mask_text, self.d_tok, self.d_step, self.loop_out,
                self.loop_cnt, 1 + slot * r.bps):
            return
        logits = r._fwd(1)
        self._advance(logits, slot, allow_eot, steps)

    def _advance(self, logits: torch.Tensor, slot: int, allow_eot: bool, steps: LogitSteps, first=False) -> None:
        """steps: the session's staged runs (row 0) launch around the sampler -- from the staged states
        at the ``first`` step (after the prompt), afterwards moving on by the token the previous step
        left in ``d_tok``, on the device (no host wait).  A scored sampler reads the row's temperature
        from the score buffers (0: the greedy path of sample.hip, the same as no temperature at all)."""
        b = self.runner.b
        x = logits[:1]
        mask, temperature = steps.before_sample(x, self.d_tok, allow_eot, first)
        ops.sample(x, mask=mask, temperature=temperature, seed=self.d_seed, step=self.d_step, out_tokens=self.d_tok,
                   part_val=self.part_val, part_idx=self.part_idx)
        steps.after_sample(x, mask, self.d_tok, first)
        ops.ext().decode_advance(b.tokens, b.positions, b.ctx_lens, b.slots, self.d_tok, self.loop_out,
                                 self.loop_cnt, 1 + slot * self.runner.bps, self.runner.bs)

    LOOP_STEPS = 4  # decode steps per replayed loop graph (graph-to-graph launch gap ~10 us per replay)

    def _loop_graph(self, slot: int, allow_eot: bool, steps: LogitSteps, n: int = 1) -> "torch.cuda.CUDAGraph":
        # (a loop with boost, rules or score is a graph of its own: it holds those launches and not the
        # persistent decoder; it addresses the engine's fixed buffers and masks -- a scored sampler reads
        # the row's temperature there -- so one graph serves every such call, attempt and temperature)
        key = (slot, allow_eot, n) + steps.graph_key
        g = self.loop_graphs.get(key)
        if g is None:
            r = self.runner
            b = r.b
            # one warm-up step with no KV write (slot -1): the session's cache holds the prompt
            b.seq_ids[:1].fill_(slot)
            b.positions[:1].fill_(0)
            b.ctx_lens[:1].fill_(1)
            b.slots[:1].fill_(-1)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self._loop_step(slot, allow_eot, steps)
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            if r.pool is None:
                r.pool = torch.cuda.graph_pool_handle()
            with torch.cuda.graph(g, pool=r.pool):
                for _ in range(n):  # identical steps: each reads what the previous advanced
                    self._loop_step(slot, allow_eot, steps)
            self.loop_graphs[key] = g
        return g

    def _decode_device(self, slot: int, first_logits: torch.Tensor, n_max: int, exact: bool, steps: LogitSteps,
                       P: Optional[int] = None, step0: int = 0) -> List[int]:
        """P: the session's prompt length (SOT sequence + any forced prefix) -- the first sampled
        token sits at position P.  steps: the session's staged runs (row 0); the graphs' warm-up
        step moves their work states, which the first advance sets again from the staged ones.  It
        also moves the sampler's step counter, which a scored call therefore sets (``step0``) once
        the graphs exist."""
        cfg = self.model.cfg
        r = self.runner
        b = r.b
        P = len(self.prompt) if P is None else P
        n_max = min(n_max, self.loop_out.numel(), r.bps * r.bs - P)
        if n_max <= 0:
            return []
        g = self._loop_graph(slot, not exact, steps)
        K = self.LOOP_STEPS
        gk = self._loop_graph(slot, not exact, steps, K) if K > 1 else None
        if steps.score is not None:
            self.d_step.fill_(step0)
        # row 0 = this session at the last prompt position; the first advance moves it to P
        b.seq_ids[:1].fill_(slot)
        b.positions[:1].fill_(P - 1)
        self.loop_cnt.zero_()
        self._advance(first_logits, slot, not exact, steps, first=True)
        out: List[int] = []
        done = 1
        chunk = n_max if exact else 8
        while True:
            todo = min(chunk, n_max - done)
            while gk is not None and todo >= K:  # K steps per replay (never past n_max)
                gk.replay()
                done += K
                todo -= K
            for _ in range(todo):
                g.replay()
                done += 1
            toks = self.loop_out[:done].tolist()
            if not exact and cfg.eot in toks:
                return toks[: toks.index(cfg.eot)]
            if done >= n_max:
                return toks[:n_max]

    def set_cross_batch(self, slots: List[int], enc_states: torch.Tensor) -> None:
        cross = self.runner.b.cross
        s0 = slots[0]
        if list(slots) == list(range(s0, s0 + len(slots))):  # a run of slots: projected in place
            self.model.cross_kv(enc_states, out=[(k[s0 : s0 + len(slots)], v[s0 : s0 + len(slots)]) for k, v in cross])
            return
        kvs = self.model.cross_kv(enc_states)
        for li, (k, v) in enumerate(kvs):
            for i, slot in enumerate(slots):
                self.runner.b.cross[li][0][slot].copy_(k[i])
                self.runner.b.cross[li][1][slot].copy_(v[i])

    def transcribe(self, audio: torch.Tensor, *, max_tokens: int = 96, min_tokens: int = 0,
                   exact_tokens: Optional[int] = None) -> str:
        """audio: f32 16 kHz on the model device (<= 30 s).

        exact_tokens: decode exactly this many text tokens (EOT suppressed) -- fixed-work mode
        used by the benchmark so random-init weights do the same work as a real transcript.
        """
        return self.transcribe_many([audio], max_tokens=max_tokens, min_tokens=min_tokens,
                                    exact_tokens=exact_tokens)[0]

    def transcribe_many(self, audios: List[torch.Tensor], *, max_tokens: int = 96, min_tokens: int = 0,
                        exact_tokens: Optional[int] = None) -> List[str]:
        """Batch of utterances (concurrent voice sessions on this GPU): one batched encoder pass
        ([B, 3000, mels] through conv/flash-attention/GEMMs), then every decode step is one
        ragged row-per-session graph replay with one masked-argmax launch for all sessions."""
        toks = self.decode_many(audios, max_tokens=max_tokens, min_tokens=min_tokens, exact_tokens=exact_tokens)
        return [self.tok.decode(o) for o in toks]

    def max_prefix(self) -> int:
        """Longest forced text prefix decode_many keeps (the decoder's position cap minus the SOT
        prompt and one decoded token); longer prefixes are cut to this length."""
        r = self.runner
        return max(0, r.bps * r.bs - len(self.prompt) - 1)

    def decode_many(self, audios: List[torch.Tensor], prefixes: Optional[Sequence[Sequence[int]]] = None, *,
                    max_tokens: int = 96, min_tokens: int = 0, exact_tokens: Optional[int] = None,
                    words: bool = False, languages: Optional[Sequence[Optional[str]]] = None,
                    task: Optional[str] = None, beam_size: int = 1,
                    keyterms: Optional[Sequence] = None,
                    timestamps: Optional[Sequence[bool]] = None, score: bool = False,
                    temperatures: Optional[Sequence[float]] = None, fallback=None) -> List[List[int]]:
        """Token ids decoded for each utterance.  ``prefixes[i]``: text tokens forced after the
        SOT sequence (a streaming session's committed transcript -- asr/streaming.py local
        agreement): they are prefilled in the same ragged prompt step as the SOT tokens and only
        the continuation is decoded; the result EXCLUDES the prefix.  A prefix longer than
        ``max_prefix()`` is cut to that length (callers build hypotheses from the cut prefix).

        ``words``: also align the transcript (prefix + decoded tokens) to the audio and score its
        tokens, before the session slots are released -- ``self.last_alignments[i]`` then holds
        utterance i's token ids, first / last 20 ms frame per token and token log-probabilities
        (``_align``).  Off: nothing is allocated or launched for it.

        ``languages[i]``: utterance i's language code, "auto" (detected from the logits at the SOT
        position, restricted to the engine's allowed languages) or None (the engine's default);
        ``task``: "transcribe" | "translate" (None: the engine's).  ``self.last_sot[i]`` reports the
        language used, and -- when a session is "auto", the no-speech gate is on or ``keep_sot`` is
        set -- its confidence and the no-speech probability (``_probe``).  With every language fixed
        and the gate off nothing is launched for it; a gated session is still decoded (skipping it
        would take a host wait on every un-gated call).

        ``beam_size`` W >= 2 (<= 8): every utterance is decoded with W beams (_decode_beams) and the
        best hypothesis' tokens are returned; ``self.last_beams[i]`` holds utterance i's ranked
        hypotheses.  An utterance takes W session slots for the call -- the encoder and the cross K/V
        are computed once, into the first; the others' ``cross_table`` rows point at it and are
        restored when the call ends -- so B * W free slots (<= 64) are needed.  1: the greedy path,
        and nothing of the beam library is loaded or launched.

        ``keyterms[i]``: utterance i's compiled keyterm set (``compile_keyterms``; asr/keyterms.py) or
        None.  Every step's logits of a boosted row get ``bias(h, v)`` added (h: the forced prefix and
        the tokens decoded so far -- a term may straddle the prefix boundary) by one launch
        (ops.boost_step) before the argmax or the beam selection reads them, so the beams' scores and
        ``last_beams`` log-probabilities are those of the biased distribution; ``_align`` keeps scoring
        the model's own logits.  Identical sets share one automaton; the call's distinct automata
        must fit the engine's tables (ops.BOOST_CAP_STATES / BOOST_CAP_EDGES) or the call raises
        before anything is launched.  Host-to-device copies: one at the first step (the rows' roots and
        initial states, with the tables when the device holds others), and -- batched rows and beams
        only -- one more small one (roots and states, 512 bytes) at each step where a row or an
        utterance has dropped out and the rows have moved up: the states are then staged again from
        the histories the host holds, not compacted on the device.  A boosted call does not take the persistent one-launch decoder.
        None, or a list of None: nothing of the boosting library is loaded, allocated or launched.

        ``timestamps[i]`` true: utterance i is decoded with timestamp tokens.  Its SOT sequence has no
        ``<|notimestamps|>``, its masks allow text and timestamps, and one launch per step
        (ops.ts_rules_step; csrc/tsrules/tsrules.h has Whisper's rules) bans what the rules forbid
        after the tokens sampled so far -- after the boost, so the rules compare the biased logits, and
        before the sampler.  Its tokens come back with the timestamp tokens among them and
        ``self.last_segments[i]`` holds its segments (asr/segments.py; None for the other utterances).
        Greedy only: with ``beam_size > 1``, ``words`` or a prefix on such an utterance the call raises
        ValueError before anything is launched.  The rules' states advance on the device from the
        sampler's tokens and are staged again from the host's histories when the rows move up; a
        single session runs the captured device loop with the rules launch in its graph, and does
        not take the persistent one-launch decoder.  None or all false: nothing of the rules library
        is loaded, allocated or launched.

        ``score``: every utterance's running score is kept on the device -- one launch per step
        (ops.score_step; csrc/score/score.h) right after the sampler adds the chosen token's
        log-probability under the distribution it was drawn from: the logits after the boost and the
        rules, restricted to the sampler's mask.  ``self.last_scores[i]`` = {sum_logprob, tokens,
        avg_logprob (Whisper's: sum / (tokens + 1), the EOT's log-probability is in the sum),
        temperature, attempts, passed, failed_on}.  ``temperatures[i]`` (implies ``score``): utterance
        i is sampled at that temperature (0: greedy) -- the sampler reads a device tensor of the rows'
        temperatures; its Gumbel noise is a function of ``self.sample_seed``, the attempt and the step.
        ``fallback`` (a FallbackPolicy, asr/fallback.py; implies ``score``, excludes ``temperatures``):
        after a decode the utterances its rule rejects are decoded again at the schedule's next
        temperature, within this call and on the same slots -- the encoder ran once, the cross K/V
        stay, only the prompt step and the token loop run again -- until they pass or the schedule
        ends (the last attempt then stands, ``passed`` false).  An utterance the no-speech gate
        rejects is not retried.  The sums advance on the device and are staged again from the host's
        copies when the rows move up (one small copy each way at such a step); a single session runs
        the captured device loop with the score launch in its graph.  It composes with prefixes,
        keyterms, timestamps and words (``_align`` runs once, on the returned attempt); with
        ``beam_size > 1`` the call raises ValueError before anything is launched (the beams carry
        their own scores: ``last_beams``).  A scored call does not take the persistent one-launch
        decoder: its logits never leave the kernel -- the same trade as boost and rules.  All off:
        nothing of the score library is loaded, allocated or launched."""
        t0 = time.perf_counter()
        kw = dict(max_tokens=max_tokens, min_tokens=min_tokens, exact_tokens=exact_tokens, words=words,
                  languages=languages, task=task, beam_size=beam_size, keyterms=keyterms, timestamps=timestamps,
                  score=score, temperatures=temperatures, fallback=fallback)
        c = self._call(audios, prefixes, **kw)
        m, r, cfg, B, W, steps, outs = self.model, self.runner, self.model.cfg, c.B, c.W, c.steps, c.outs
        c.slots = slots = [self.free_slots.pop() for _ in range(B)]
        # beams: utterance i's beams sit in slots[i] (beam 0: prompt, encoder K/V, alignment) and W - 1 more
        c.beam_slots = beam_slots = ([[s] + [self.free_slots.pop() for _ in range(W - 1)] for s in slots]
                                     if W > 1 else None)
        cross_saved = None
        try:
            if beam_slots is not None:
                ct = r.b.cross_table
                cross_saved = ct.clone()
                extra = torch.tensor([s for bs_ in beam_slots for s in bs_[1:]], dtype=torch.long, device=ct.device)
                first = torch.tensor([bs_[0] for bs_ in beam_slots for _ in bs_[1:]], dtype=torch.long, device=ct.device)
                ct[extra] = ct[first]  # every beam reads the utterance's one cross K/V
            mel = m.mel_batch(audios)
            enc = m.encode(mel)
            self.set_cross_batch(slots, enc)
            t_enc = time.perf_counter()
            # GPU-side decode time (prompt step + token loop): the host stamps above are taken when
            # the encoder and the cross K/V projections are LAUNCHED, so decode_ms also holds
            # whatever of them was still running; events bracket the decoder's own stream time
            ev = None
            if m.device.type == "cuda":
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            beam_ms = None
            if steps.score is None:
                beam_ms = self._decode_pass(c, list(range(B)), True)
            else:
                from . import fallback as fb

                if c.policy is None:
                    res = self._attempt(c, list(range(B)), None)
                    scores = [fb.score_entry(s_, n_, c.temps[j], 1, tx) for j, (s_, n_, tx) in enumerate(res)]
                else:
                    scores = fb.run(lambda utts, T: self._attempt(c, utts, T), B, c.policy,
                                    gated=lambda j: bool(c.sot_read[j]["gated"]))
            retry = self._chain_failed()  # (results of a timed-out chained launch are invalid: redo)
            t_end = time.perf_counter()
            dec_gpu = None
            if ev is not None:
                ev[1].record()
                ev[1].synchronize()  # (the tokens were read back: the stream is already there)
                dec_gpu = ev[0].elapsed_time(ev[1])
            self.last_stats = dict(encode_ms=(t_enc - t0) * 1e3, decode_ms=(t_end - t_enc) * 1e3,
                                   decode_gpu_ms=dec_gpu, total_ms=(t_end - t0) * 1e3,
                                   tokens=sum(len(o) for o in outs), batch=B,
                                   prefix_tokens=sum(len(f) for f in c.forced))
            if steps.boost is not None:
                self.last_stats["boosted"] = sum(k is not None for k in keyterms)
            if steps.ts is not None:
                self.last_stats["timestamps"] = sum(c.ts_flags)
            if steps.score is not None:
                self.last_stats.update(scored=B, attempts=c.attempts, retried=c.retried)
            if beam_slots is not None:
                self.last_stats["beam_size"] = W
                if beam_ms is not None:
                    self.last_stats["beam_ms"] = beam_ms()
            if not retry:
                # (fills in the detected language tokens; a fallback call has read it after its first attempt)
                self.last_sot = c.sot_read if c.sot_read is not None else self._read_sot(c.sot, c.langs, c.prompts)
                if steps.score is not None:
                    self.last_scores = scores
                self.last_segments = [segments(o, cfg.no_timestamps + 1, cfg.eot, self.tok) if f else None
                                      for o, f in zip(outs, c.ts_flags)]
                if words:
                    self.last_alignments = self._align(slots, audios, c.prompts, outs, c.exact, min_tokens)
                    self.last_stats["align_ms"] = (time.perf_counter() - t_end) * 1e3
                return outs
        finally:
            if beam_slots is None:
                self.free_slots.extend(slots)
            else:
                if cross_saved is not None:
                    r.b.cross_table.copy_(cross_saved)
                # (in reverse: the free list is what it was before the call)
                self.free_slots.extend(reversed(slots + [s for bs_ in beam_slots for s in bs_[1:]]))
        return self.decode_many(audios, prefixes, **kw)

    def _call(self, audios, prefixes, *, max_tokens, min_tokens, exact_tokens, words, languages, task, beam_size,
              keyterms, timestamps, score, temperatures, fallback) -> SimpleNamespace:
        """Every check of a decode_many call's arguments, and what the call then works on: its
        prompts, forced prefixes, limits, flags and LogitSteps.  It raises before a slot is taken or
        anything is launched; a feature's buffers are built here, on its first call."""
        m = self.model
        B = len(audios)
        W = int(beam_size)
        if W != 1 and not 2 <= W <= ops.BEAM_MAX_WIDTH:
            raise ValueError(f"beam_size = {beam_size} outside [1, {ops.BEAM_MAX_WIDTH}]")
        if B > len(self.free_slots):
            raise RuntimeError(f"{B} utterances exceed the {len(self.free_slots)} free ASR session slots")
        if W > 1 and (B * W > len(self.free_slots) or B * W > ops.BEAM_MAX_ROWS):
            raise RuntimeError(f"{B} utterances of {W} beams exceed the {min(len(self.free_slots), ops.BEAM_MAX_ROWS)} "
                               "free ASR session slots")
        policy, sc, temps = fallback, None, [0.0] * B
        scored = bool(score) or temperatures is not None or policy is not None
        if scored:
            from .fallback import FallbackPolicy

            if W > 1:
                raise ValueError("score / temperatures / fallback: not with beam_size > 1 (the beams carry their own "
                                 "scores: last_beams)")
            if policy is not None and not isinstance(policy, FallbackPolicy):
                raise TypeError(f"fallback: {type(policy).__name__} is not a FallbackPolicy (asr/fallback.py)")
            if temperatures is not None:
                if policy is not None:
                    raise ValueError("temperatures: not with fallback (its schedule sets them)")
                if len(temperatures) != B:
                    raise ValueError(f"temperatures: {len(temperatures)} entries for {B} utterances")
                temps = [float(t) for t in temperatures]
                if any(not 0.0 <= t <= 2.0 for t in temps):
                    raise ValueError(f"temperatures: {temps} not all in [0, 2]")
            if B > ops.SCORE_MAX_ROWS:
                raise RuntimeError(f"{B} scored utterances exceed {ops.SCORE_MAX_ROWS} rows")
        prefixes = [list(p) for p in prefixes] if prefixes is not None else [[] for _ in range(B)]
        assert len(prefixes) == B
        ts, ts_flags = None, [False] * B
        if timestamps is not None and any(timestamps):
            if len(timestamps) != B:
                raise ValueError(f"timestamps: {len(timestamps)} entries for {B} utterances")
            ts_flags = [bool(f) for f in timestamps]
            if W > 1:
                raise ValueError("timestamps: not with beam_size > 1 (the rules' state would have to follow the parents)")
            if words:
                raise ValueError("timestamps: not with words=True")
            if any(f and p for f, p in zip(ts_flags, prefixes)):
                raise ValueError("timestamps: an utterance decoded with timestamps takes no prefix")
            if B > ops.TS_MAX_ROWS:
                raise RuntimeError(f"{B} utterances with timestamps exceed {ops.TS_MAX_ROWS} rows")
            self._ts_setup()
            if self.keep_ts_trace:
                self.last_ts_trace = []
            ts = TsRun(self._ts_bufs, ts_flags, m.cfg, self.last_ts_trace if self.keep_ts_trace else None)
        boost: Optional[BoostRun] = None
        if keyterms is not None and any(k is not None for k in keyterms):
            if len(keyterms) != B:
                raise ValueError(f"keyterms: {len(keyterms)} entries for {B} utterances")
            if B * W > ops.BOOST_MAX_ROWS:
                raise RuntimeError(f"{B} boosted utterances of {W} rows exceed {ops.BOOST_MAX_ROWS} rows")
            if self._boost_bufs is None:
                self._boost_bufs = BoostBuffers(m.device)
            if self.keep_boost_trace:
                self.last_boost_trace = []
            # (raises when the call's automata do not fit the tables: nothing is launched yet)
            boost = BoostRun(self._boost_bufs, keyterms, m.cfg.vocab_size,
                             self.last_boost_trace if self.keep_boost_trace else None)
            boost.load()
        if scored:  # (built only now: every check of the call's arguments has passed)
            if self._score_bufs is None:
                self._score_bufs = ScoreBuffers(m.device)
            if self.keep_score_trace:
                self.last_score_trace = []
            sc = ScoreRun(self._score_bufs, B, m.cfg, self.last_score_trace if self.keep_score_trace else None)
            self.d_seed.fill_(int(self.sample_seed))
        cfg, cap = m.cfg, self.runner.bps * self.runner.bs  # (cap: decoder positions per session)
        langs = [self.language if l is None else str(l).strip().lower()
                 for l in (languages if languages is not None else [None] * B)]
        assert len(langs) == B
        auto = [l == "auto" for l in langs]
        task_id = self._task_id(self.task if task is None else str(task).strip().lower())
        heads = [[cfg.sot, self._lang_placeholder if a else language_token(cfg, l), task_id, cfg.no_timestamps]
                 for l, a in zip(langs, auto)]
        if ts is not None:  # (an utterance decoded with timestamps: no <|notimestamps|>)
            heads = [h[:3] if f else h for h, f in zip(heads, ts_flags)]
        prompts = [h + p[: max(0, cap - len(h) - 1)] for h, p in zip(heads, prefixes)]
        forced = [p[len(h):] for h, p in zip(heads, prompts)]  # the text prefix each decoder really gets
        n_max = exact_tokens if exact_tokens is not None else max_tokens
        return SimpleNamespace(
            B=B, W=W, policy=policy, temps=temps, ts_flags=ts_flags, langs=langs, auto=auto, prompts=prompts,
            forced=forced, steps=LogitSteps(self._mask, forced, boost, ts, sc),
            probe=any(auto) or self.no_speech_threshold > 0.0 or self.keep_sot, sot=None, sot_read=None,
            n_max=n_max, min_tokens=min_tokens, exact=exact_tokens is not None, outs=[[] for _ in range(B)],
            pos=[len(p) for p in prompts], limit=[min(n_max, cap - len(p)) for p in prompts], attempts=0, retried=0)

    def _decode_pass(self, c: SimpleNamespace, utts: List[int], first_pass: bool, step0: int = 0):
        """The prompt step and the token loop of the utterances ``utts`` of the call ``c`` (ascending;
        every utterance at the first pass, the rejected ones at a fallback pass), on their own
        slots: the encoder's output and the cross K/V stay.  Fills ``c.outs``."""
        steps, outs, limit = c.steps, c.outs, c.limit
        sl, pr = [c.slots[j] for j in utts], [c.prompts[j] for j in utts]
        if not (first_pass and c.probe):
            logits = self._prompt_logits(sl, pr)
        elif not any(c.auto):
            # the SOT row's logits do not depend on the rows after it: the one prompt step serves
            logits, sot_logits = self._prompt_logits(sl, pr, first=True)
            c.sot = self._probe(sot_logits)
        else:
            logits, c.sot = self._prompt_auto(sl, pr, c.auto)
        live, ms = list(utts), None
        if steps.score is not None:
            self.d_step.fill_(step0)
        if c.beam_slots is not None:
            res, ms = self._decode_beams(c.beam_slots, logits, c.pos, limit, c.n_max, c.min_tokens, c.exact,
                                         steps.boost, c.forced)
            outs[:] = res
            live = []
        elif (c.B == 1 and self.device_loop and (c.exact or c.min_tokens == 0) and c.n_max > 0
              and not steps.traced):  # (a trace steps from the host)
            steps.restage([0], outs)
            outs[0] = self._decode_device(c.slots[0], logits, limit[0], c.exact, steps, P=c.pos[0], step0=step0)
            live = []
        for i in range(c.n_max if live else 0):
            allow_eot = not c.exact and i >= c.min_tokens
            first = steps.restage(live, outs)
            mask, temperature = steps.before_sample(logits, self.d_tok, allow_eot, first)
            toks = self._sample_rows(logits, mask, temperature)
            steps.after_sample(logits, mask, self.d_tok, first)
            steps.note(tokens=list(toks), allow_eot=allow_eot)
            nxt = []
            for j, tok in zip(live, toks):
                if tok == self.model.cfg.eot or tok < 0:
                    continue
                outs[j].append(tok)
                if len(outs[j]) < limit[j]:
                    nxt.append(j)
            live = nxt
            if not live or i + 1 >= c.n_max:
                break
            logits = self.runner.step([(c.slots[j], outs[j][-1], c.pos[j] + len(outs[j]) - 1) for j in live])
        steps.finish()
        return ms

    def _attempt(self, c: SimpleNamespace, utts: List[int], T: Optional[float]):
        """One scored decode of the utterances ``utts`` at the temperature T (None: each its own):
        (sum of log-probabilities, tokens, text) per utterance -- what asr/fallback.py run asks for."""
        k = c.attempts
        c.attempts += 1
        sc = c.steps.score
        sc.begin(utts, [c.temps[j] if T is None else T for j in utts], k)
        for j in utts:
            c.outs[j] = []
        self._decode_pass(c, utts, k == 0, k << 16)
        if k == 0 and c.policy is not None:
            # (the gate's verdicts, and an auto session's detected language token in its prompt)
            c.sot_read = self._read_sot(c.sot, c.langs, c.prompts)
        if k > 0:
            c.retried += len(utts)
        eot = self.model.cfg.eot
        return [(sc.sums[j], len(c.outs[j]), self.tok.decode([t for t in c.outs[j] if t < eot])) for j in utts]

    def _decode_beams(self, beam_slots: List[List[int]], logits: torch.Tensor, pos: List[int], limit: List[int],
                      n_max: int, min_tokens: int, exact: bool, boost: Optional[BoostRun] = None,
                      forced: Optional[List[List[int]]] = None):
        """Beam search over every utterance of the call in one batch.  ``logits``: each utterance's
        last prompt row (the prompt is prefilled on beam 0's slot only); ``pos[i]``: utterance i's
        prompt length.  Per token step:

        1. ops.beam_select over the W rows of every live utterance (the first step with cum =
           [0, -inf, ...]: only beam 0's row counts);
        2. ONE device-to-host copy of the packed candidates;
        3. the bookkeeping (asr/beam.py advance) -- a finished utterance drops out;
        4. ONE host-to-device copy: the live groups' slots, parents, context lengths and new cum;
        5. ops.kv_beam_gather over the positions below the current one (the first one, with every
           parent 0, fans the prompt's K/V out to all beams);
        6. runner.step with W rows per live utterance.

        Returns (the best hypothesis' tokens per utterance, a callable giving the event-timed
        milliseconds of select, gather and the copies -- None on the CPU); fills ``last_beams`` and,
        with ``keep_beam_trace``, ``last_beam_trace``: per step ``utts`` (the live utterances, in row
        order), ``logits`` [G W, vocab_padded] and ``cum`` [G, W] the select read, ``allow_eot`` (the
        mask: text ids with or without EOT), ``cand_score`` / ``cand_beam`` / ``cand_tok`` [G, 2 W],
        and ``parents`` / ``tokens`` [G, W] chosen.

        ``boost`` (``forced``: every utterance's text prefix): before each select the rows' keyterm
        biases go onto ``x``.  The automaton states live on the device in two buffers and follow the
        beams: row r starts from its parent's state and moves on by its token (the staging copy
        carries the tokens too).  At the first step, and when an utterance has dropped out and the
        rows have moved up, the states are staged from the beams' histories instead."""
        m = self.model
        cfg = m.cfg
        r = self.runner
        b = r.b
        dev = m.device
        cuda = dev.type == "cuda"
        B, W = len(beam_slots), len(beam_slots[0])
        K = 2 * W
        states = [beam_rule.BeamState(W, cfg.eot, limit[i]) for i in range(B)]
        live = [i for i in range(B) if not states[i].done]
        x = torch.zeros(B * W, logits.shape[1], dtype=torch.float32, device=dev)
        x[0::W] = logits  # (the dead rows are never read into a result: any finite filler serves)
        if live != list(range(B)):
            x = x.view(B, W, -1)[live].reshape(len(live) * W, -1)
        res = torch.empty(3 * B * K, dtype=torch.float32, device=dev)  # score | beam | token, per step [3, G, K]
        n_stage = B * (3 * W + 1 + (W if boost is not None else 0))  # (boosted: the rows' tokens too)
        h_stage = torch.zeros(n_stage, dtype=torch.int32, pin_memory=cuda)  # slots | parents | cum bits | n_ctx
        d_stage = torch.zeros(n_stage, dtype=torch.int32, device=dev)
        timed: List[Tuple["torch.cuda.Event", "torch.cuda.Event"]] = []

        def mark():
            if not cuda:
                return None
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            return e

        def stage(groups: List[int], parents: List[List[int]], n_ctx: List[int],
                  tokens: Optional[List[List[int]]] = None):
            G = len(groups)
            n = G * (3 * W + 1)
            hs = h_stage[:n]
            hs[: G * W] = torch.tensor([s for j in groups for s in beam_slots[j]], dtype=torch.int32)
            hs[G * W : 2 * G * W] = torch.tensor(parents, dtype=torch.int32).reshape(-1)
            hs[2 * G * W : 3 * G * W] = torch.tensor([c for j in groups for c in states[j].cum],
                                                     dtype=torch.float32).view(torch.int32)
            hs[3 * G * W :] = torch.tensor(n_ctx, dtype=torch.int32)
            tok_d = None
            if boost is not None:  # the rows' tokens ride in the same copy
                h_stage[n : n + G * W] = torch.tensor(tokens if tokens is not None else [[0] * W] * G,
                                                      dtype=torch.int32).reshape(-1)
                tok_d = d_stage[n : n + G * W]
                n += G * W
            d_stage[:n].copy_(h_stage[:n], non_blocking=True)
            ds = d_stage
            return (ds[: G * W].view(G, W), ds[G * W : 2 * G * W].view(G, W),
                    ds[2 * G * W : 3 * G * W].view(torch.float32), ds[3 * G * W : G * (3 * W + 1)], tok_d)

        trace: List[Dict] = []
        self.last_beam_trace = trace
        t_a = mark()  # (the first select's bracket holds the first staging copy)
        _, _, cum_d, _, _ = stage(live, [[0] * W for _ in live], [0] * len(live)) if live else (None,) * 5
        par_d = tok_d = None
        for i in range(n_max):
            if not live:
                break
            G = len(live)
            allow_eot = not exact and i >= min_tokens
            cs, cb, ct = (res[k * G * K : (k + 1) * G * K].view(G, K) for k in range(3))
            if boost is not None:
                if boost.restage([j for j in live for _ in range(W)],
                                 lambda: [forced[j] + states[j].tokens[w] for j in live for w in range(W)]):
                    boost.step(x, None, True)
                else:
                    boost.follow(x, tok_d, par_d.reshape(-1), W)
                boost.note(alive=[c != beam_rule.NEG_INF for j in live for c in states[j].cum], allow_eot=allow_eot)
            ops.beam_select(x, cum_d, self.mask_text_eot if allow_eot else self.mask_text, cfg.vocab_size, W,
                            cand_score=cs, cand_beam=cb.view(torch.int32), cand_tok=ct.view(torch.int32))
            h = res[: 3 * G * K].cpu()  # the one copy (it also waits for the step)
            if cuda:
                timed.append((t_a, mark()))
            hs = h[: G * K].view(G, K).tolist()
            hb = h[G * K : 2 * G * K].view(torch.int32).view(G, K).tolist()
            ht = h[2 * G * K :].view(torch.int32).view(G, K).tolist()
            step = None
            if self.keep_beam_trace:
                step = dict(step=i, utts=list(live), logits=x.cpu().clone(), cum=[list(states[j].cum) for j in live],
                            allow_eot=allow_eot, cand_score=h[: G * K].view(G, K).clone(),
                            cand_beam=h[G * K : 2 * G * K].view(torch.int32).view(G, K).clone(),
                            cand_tok=h[2 * G * K :].view(torch.int32).view(G, K).clone(), parents=[], tokens=[])
                trace.append(step)
            nxt, parents, tokens = [], [], []
            for g, j in enumerate(live):
                par, tok = beam_rule.advance(states[j], list(zip(hs[g], hb[g], ht[g])))
                if step is not None:
                    step["parents"].append(par)
                    step["tokens"].append(tok)
                if boost is not None and boost.trace:
                    boost.trace[-1].setdefault("parents", []).append(par)
                    boost.trace[-1].setdefault("tokens", []).append(tok)
                if not states[j].done:
                    nxt.append(j)
                    parents.append(par)
                    tokens.append(tok)
            live = nxt
            if not live:
                break
            t_c = mark()
            n_ctx = [pos[j] + i for j in live]
            slots_d, par_d, cum_d, ctx_d, tok_d = stage(live, parents, n_ctx, tokens)
            ops.kv_beam_gather(b.k_cache, b.v_cache, b.block_table, slots_d, par_d, ctx_d, max_ctx=max(n_ctx))
            if cuda:
                timed.append((t_c, mark()))  # (the forward that follows is not counted)
            x = r.step([(beam_slots[j][w], tokens[g][w], pos[j] + i) for g, j in enumerate(live) for w in range(W)])
            t_a = mark()
        self.last_beams = [beam_rule.ranked(st) for st in states]
        outs = [list(hyps[0]["tokens"]) for hyps in self.last_beams]

        def beam_ms() -> float:
            return float(sum(a.elapsed_time(z) for a, z in timed))

        return outs, (beam_ms if cuda else None)

    keep_costs = False  # _align: also keep each utterance's cost matrix (host copy) in its Alignment

    def _align(self, slots: List[int], audios: List[torch.Tensor], prompts: List[List[int]], outs: List[List[int]],
               exact: bool, min_tokens: int) -> List[Alignment]:
        """Word alignment and token scores of every session, while it still holds its slot:

        1. a teacher-forced decoder pass over SOT prompt + forced prefix + decoded tokens (<= 64 rows
           per step, a session's rows in order) that records the alignment heads' cross-attention
           probabilities over the audio's frames (models/whisper.py align_step) and scores each
           step's logits (row p scores token p + 1, under the mask the sampler used there);
        2. per session the alignment cost over its text-token rows and the DTW path;
        3. ONE device -> host copy of every session's frames and log-probabilities."""
        m = self.model
        cfg = m.cfg
        dev = m.device
        r = self.runner
        R = max(BUCKETS)
        S = cfg.n_audio_ctx
        P0 = len(self.prompt)
        n_heads = m.align_layers()[1]
        seqs = [p + o for p, o in zip(prompts, outs)]
        n_keys = [min(S, max(1, -(-int(a.numel()) // 320))) for a in audios]
        n_text = [len(s) - P0 for s in seqs]
        live = [i for i in range(len(seqs)) if n_text[i] > 0]
        result = [Alignment(n_keys=n_keys[i]) for i in range(len(seqs))]
        if not live:
            return result
        rows: List[Tuple[int, int, int]] = []   # (slot, token, position) of every row, session by session
        owner: List[int] = []                   # the row's session
        targets: List[int] = []
        sel: List[int] = []                     # 0: text ids only, 1: text ids + EOT (the sampler's two masks)
        base: Dict[int, int] = {}
        for i in live:
            base[i] = len(rows)
            seq = seqs[i]
            for p, t in enumerate(seq):
                rows.append((slots[i], t, p))
                owner.append(i)
                scored = P0 - 1 <= p < len(seq) - 1
                tgt = seq[p + 1] if scored else 0
                k = p + 1 - len(prompts[i])     # index among the decoded tokens (< 0: forced prefix)
                only_text = exact or 0 <= k < min_tokens
                if scored and not (0 <= tgt < cfg.eot):
                    raise ValueError(f"token {tgt} of utterance {i} is not a text token: the sampler's mask forbids it")
                targets.append(tgt)
                sel.append(0 if only_text else 1)
        G = len(rows)
        n_tot = sum(n_text[i] for i in live)
        host = torch.tensor(targets + sel, dtype=torch.int32)
        d_in = host.to(dev)
        tgt_d, sel_d = d_in[:G], d_in[G:]
        masks = (self.mask_text, self.mask_text_eot)
        uniform = masks[sel[0]] if len(set(sel)) == 1 else None
        both = None if uniform is not None else torch.cat(masks)
        # frames and log-probabilities of every session in one buffer: [first | last | log-prob bits]
        res = torch.zeros(2 * n_tot + G, dtype=torch.int32, device=dev)
        lp = res[2 * n_tot :].view(torch.float32)
        probs = {i: torch.empty(n_heads, len(seqs[i]), S, dtype=torch.float32, device=dev) for i in live}
        for g0 in range(0, G, R):
            g1 = min(G, g0 + R)
            segs = []
            a = g0
            while a < g1:
                i = owner[a]
                e = a
                while e < g1 and owner[e] == i:
                    e += 1
                segs.append((a - g0, e - a, slots[i], probs[i], rows[a][2], n_keys[i]))
                a = e
            logits = r.step(rows[g0:g1], fwd=lambda M, segs=segs: m.align_step(r.b, M, segs))
            mask = uniform if uniform is not None else both[sel_d[g0:g1].long()]
            ops.token_logprob(logits, tgt_d[g0:g1], mask, cfg.vocab_size, out=lp[g0:g1])
        off = {}
        o = 0
        costs = {}
        for i in live:
            n = n_text[i]
            cost = ops.align_cost(probs[i][:, P0:], n, n_keys[i])
            ops.dtw_path(cost, n, n_keys[i], res[o : o + n], res[n_tot + o : n_tot + o + n])
            if self.keep_costs:
                costs[i] = cost[:n, : n_keys[i]]
            off[i] = o
            o += n
        h = res.cpu()  # the one copy (it also waits for the pass)
        h_lp = h[2 * n_tot :].view(torch.float32)
        for i in live:
            n, o = n_text[i], off[i]
            b0 = base[i] + P0 - 1  # the row that scores the first text token
            result[i] = Alignment(tokens=list(seqs[i][P0:]), first_frame=h[o : o + n].tolist(),
                                  last_frame=h[n_tot + o : n_tot + o + n].tolist(),
                                  logprobs=h_lp[b0 : b0 + n].tolist(), n_keys=n_keys[i],
                                  cost=costs[i].cpu() if i in costs else None)
        return result

    def words_of(self, al: Alignment, *, duration: Optional[float] = None) -> List[Dict]:
        """The Deepgram ``words`` list of one aligned utterance, on the utterance's own clock."""
        tb = self.tok.token_bytes()
        return group_words(al, lambda t: tb[t] if 0 <= t < len(tb) else b"", duration=duration)

    def _prompt_logits(self, slots: List[int], prompts: List[List[int]], *, first: bool = False, start: int = 0,
                       pre=None):
        """Prefill every session's prompt (ragged rows, <= 64 per step; a session's rows stay in
        order) and return the logits of each session's LAST prompt row, in session order.
        ``first``: return (those, the logits of each session's position-0 row) -- the SOT row the
        probe reads.  ``start``: the prompts' first ``start`` tokens are prefilled already.
        ``pre(rows)``: run between a step's staging copy and its forward (WhisperRunner.step)."""
        R = max(BUCKETS)
        rows: List[Tuple[int, int, int]] = []
        want: List[int] = []   # row index (within the pending step) of a session's last prompt token
        want0: List[int] = []  # ... of a session's position-0 row (first)
        got: List[torch.Tensor] = []
        got0: List[torch.Tensor] = []

        def run():
            nonlocal rows, want, want0
            if rows:
                out = self.runner.step(rows, pre=None if pre is None else (lambda r=rows: pre(r)))
                if want:
                    # (clone: the logits live in the replayed graph's static output buffer)
                    got.append(out[torch.tensor(want, device=out.device)].clone())
                if want0:
                    got0.append(out[torch.tensor(want0, device=out.device)].clone())
            rows, want, want0 = [], [], []

        for slot, prompt in zip(slots, prompts):
            n = len(prompt) - start
            if len(rows) + n > R and n <= R:
                run()
            for p in range(start, len(prompt)):
                if len(rows) == R:
                    run()
                rows.append((slot, prompt[p], p))
                if first and p == 0:
                    want0.append(len(rows) - 1)
            want.append(len(rows) - 1)
        run()
        return (torch.cat(got), torch.cat(got0)) if first else torch.cat(got)

    def _probe(self, sot_logits: torch.Tensor, tok_dst: Optional[torch.Tensor] = None,
               dst_rows: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None):
        """ops.sot_probe on the sessions' SOT-row logits [B, vocab_padded].  Every output lives in
        one f32 buffer ``res`` = [B x n_langs probabilities | B language ids (int32 bits) | B
        confidences | B no-speech probabilities]: one device-to-host copy reads it (_read_sot).
        Returns (res, sot_logits)."""
        cfg = self.model.cfg
        B, n = sot_logits.shape[0], cfg.n_langs
        if res is None:
            res = torch.empty(B * (n + 3), dtype=torch.float32, device=sot_logits.device)
        o = B * n
        ops.sot_probe(sot_logits, cfg.vocab_size, cfg.lang_en, n, cfg.no_speech, self.allow,
                      lang_probs=res[:o].view(B, n), lang_tok=res[o : o + B].view(torch.int32),
                      lang_conf=res[o + B : o + 2 * B], no_speech=res[o + 2 * B :], tok_dst=tok_dst, dst_rows=dst_rows)
        return res, sot_logits

    def _prompt_auto(self, slots: List[int], prompts: List[List[int]], auto: List[bool]):
        """The prompt with language detection, in two decoder steps and no host wait between them:
        step 1 is every session's SOT row alone; step 2 the rest of every prompt from position 1,
        the auto sessions with a placeholder language token.  Between step 2's staging copy and its
        forward (or graph replay) the probe reads step 1's logits and writes each auto session's
        detected language id over the placeholder in the staged token rows (``b.tokens``) -- so the
        language row is embedded from the detected id, stream-ordered, on the device.  Fixed
        sessions get no patch (dst_rows -1) and still get their probabilities."""
        b = self.runner.b
        dev = self.model.device
        B = len(slots)
        R = max(BUCKETS)
        sot_rows = [(s, p[0], 0) for s, p in zip(slots, prompts)]
        # (clone: the logits live in the replayed graph's static output buffer, which step 2 rewrites)
        parts = [self.runner.step(sot_rows[a : a + R]).clone() for a in range(0, B, R)]
        sot_logits = parts[0] if len(parts) == 1 else torch.cat(parts)
        where = {s: i for i, s in enumerate(slots) if auto[i]}
        state: Dict[str, torch.Tensor] = {}

        def pre(rows):
            dst = [-1] * B
            for k, (slot, _tok, pos) in enumerate(rows):
                if pos == 1 and slot in where:
                    dst[where[slot]] = k
            h = torch.tensor(dst, dtype=torch.int32)
            if dev.type == "cuda":  # (pinned + non-blocking: the host does not wait for step 1)
                h = h.pin_memory()
            state["res"], _ = self._probe(sot_logits, b.tokens, h.to(dev, non_blocking=True), state.get("res"))

        logits = self._prompt_logits(slots, prompts, start=1, pre=pre)
        return logits, (state["res"], sot_logits)

    def _read_sot(self, sot, langs: List[str], prompts: List[List[int]]) -> List[Dict]:
        """last_sot of a call: the probe's outputs in ONE device-to-host copy (after the tokens were
        read: the stream is already there).  An auto session's detected token replaces the
        placeholder in its prompt (``_align`` teacher-forces the prompt the decoder really saw)."""
        cfg = self.model.cfg
        B = len(langs)
        if sot is None:
            return [dict(language=l, language_confidence=None, no_speech_prob=None, gated=False) for l in langs]
        res, sot_logits = sot
        n = cfg.n_langs
        h = res.cpu()
        probs = h[: B * n].view(B, n)
        tok = h[B * n : B * n + B].view(torch.int32).tolist()
        conf = h[B * n + B : B * n + 2 * B].tolist()
        nsp = h[B * n + 2 * B :].tolist()
        h_logits = sot_logits.cpu() if self.keep_sot else None
        thr = self.no_speech_threshold
        out = []
        for i, l in enumerate(langs):
            if l == "auto":
                prompts[i][1] = tok[i]
                d = dict(language=language_code(cfg, tok[i]), language_confidence=conf[i])
            else:
                d = dict(language=l, language_confidence=float(probs[i, language_index(cfg, l)]))
            d.update(no_speech_prob=nsp[i], gated=thr > 0.0 and nsp[i] > thr)
            if self.keep_sot:
                d.update(logits=h_logits[i], lang_probs=probs[i].clone())
            out.append(d)
        return out

    def _chain_failed(self) -> bool:
        """Health check of the chained decoder launches (models/whisper.py): a grid barrier that
        timed out (workgroups not co-resident) leaves an error word; the model then falls back to
        per-kernel launches and every captured graph is dropped."""
        m = self.model
        if getattr(m, "chain_error", None) is None or getattr(m, "_chain_disabled", False) or not m.chain_error():
            return False
        import warnings

        warnings.warn("chained Whisper decode launch timed out at a grid barrier; using per-kernel launches")
        m.disable_chain()
        self.runner.graphs.clear()
        self.loop_graphs.clear()
        return True

    def _sample_rows(self, logits: torch.Tensor, mask: torch.Tensor, temperature: Optional[torch.Tensor]) -> List[int]:
        """mask: the rows' own allow-bits [n, words] (a call with timestamp rows) or one shared row.
        temperature: the rows' temperatures, f32 [n] on the device (a scored call); None: greedy."""
        n = logits.shape[0]
        part_val, part_idx = self.part_val, self.part_idx
        if n > 1:
            logits = logits.contiguous()
            if mask.shape[0] == 1:
                mask = mask.expand(n, -1).contiguous()
            assert n <= self.d_tok.numel()  # (a step has at most max(BUCKETS) rows; d_tok is never replaced)
            part_val = torch.empty(n * 64, dtype=torch.float32, device=logits.device)
            part_idx = torch.empty(n * 64, dtype=torch.int32, device=logits.device)
        ops.sample(logits, mask=mask, temperature=temperature, seed=self.d_seed, step=self.d_step,
                   out_tokens=self.d_tok, part_val=part_val, part_idx=part_idx)
        return self.d_tok[:n].tolist()
