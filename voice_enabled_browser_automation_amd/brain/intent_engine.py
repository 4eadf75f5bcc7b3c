"""Intent engines: the on-node replacement of `callLLMJSON` (apps/brain/src/llm.ts:19-30).

`LLMIntentEngine` runs the Llama-class model through runtime.engine.LLMEngine with
grammar-constrained decoding:

* the static prompt prefix is served from the paged-KV prefix cache; only the request suffix is
  prefilled;
* **jump-forward**: whenever the grammar admits exactly one continuation (keys, punctuation,
  closing brackets, budget-forced closes) those bytes are tokenised and appended in the SAME
  forward as the previously sampled token (one ragged step of 1 + k rows), so forced JSON
  structure costs no extra decode steps;
* the token mask for step t is computed on the CPU (native grammar engine, GIL released) while
  the GPU runs step t's forward; the mask upload + sampling kernel follow on the same stream;
* a character budget (``budget_chars``) guarantees the JSON can always be closed, so every
  request terminates with a schema-valid ParseResponse;
* **continuous batching**: concurrent requests (voice sessions) decode together, one ragged
  forward + one masked-sampling launch per iteration for all of them;
* **turn probes** (``turn`` / ``turn_async`` / ``submit_turn``): a request of another kind that asks
  how likely the transcript is a finished command.  Its prompt is the ``/parse`` prompt cut inside
  the user turn's ``{"text":"...`` (prompt.turn_tail); it is prefilled behind the same cached prefix,
  its last prompt token joins one ragged step, and the probability that the next token closes the
  string is read off its logits row by one ``ops.set_logprob`` launch -- nothing is decoded;
* **summaries** (``summary`` / ``summary_async`` / ``submit_summary``): a request of a third kind, free
  text inside ``{"summary":"..."}``.  It has its own prompt head, its own grammar and its own sampling
  parameters (temperature, top-p, top-k, repetition penalty over its own sampled tokens).  Its rows
  are sampled rows after the parse rows; an iteration that holds one runs one ``ops.nucleus_step``
  launch over all sampled rows in front of the sampler (parse rows pass through), an iteration
  without one launches exactly what it did before;
* **rescoring** (``rescore`` / ``rescore_async`` / ``submit_rescore``): a request of a fourth kind that
  scores the recogniser's n-best alternatives.  Each distinct alternative is one sequence whose prompt
  is the turn probe's; the ids all alternatives share are prefilled, every id after them rides in the
  ragged step as a row with a logits row, and one ``ops.seq_logprob`` call per iteration turns those
  rows into per-sequence running sums on the device -- nothing is decoded, nothing is sampled.

`FakeIntentEngine` is the test double (the reference mocks callLLMJSON with vi.spyOn,
apps/brain/test/parse.test.ts:7-21).
"""
from __future__ import annotations

import json
import threading
import time
from collections import deque
from concurrent.futures import Future
from dataclasses import dataclass, field
from typing import Any, Callable, Deque, Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import ops
from ..grammar import CompiledGrammar, intent_grammar, summary_grammar
from .prompt import llama3_chat, messages_for, summary_messages, turn_tail, turn_text


class IntentEngineError(RuntimeError):
    pass


@dataclass
class IntentRequest:
    """One in-flight parse: prompt -> sequence -> grammar matcher -> JSON bytes."""

    messages: List[Dict[str, str]]
    ids: List[int] = field(default_factory=list)
    seq: Any = None
    matcher: Any = None
    out: bytearray = field(default_factory=bytearray)
    feed: List[int] = field(default_factory=list)   # tokens to append before the next sample
    steps: int = 0
    forced: int = 0
    cached: int = 0
    t_submit: float = 0.0
    t_start: float = 0.0
    t_first: float = 0.0
    t_end: float = 0.0
    done: bool = False
    text: Optional[str] = None
    error: Optional[BaseException] = None
    future: Any = None
    diag: Optional[str] = None
    kind: str = "parse"                 # "turn": a turn-completion probe (no matcher, nothing sampled)
                                        # "score": one alternative of a rescore (the same, many rows)
    probe_text: Optional[str] = None    # "summary": free text under the summary grammar
    result: Optional[Dict[str, Any]] = None
    head_len: int = 0                   # tokens of this request's static head: what _finish publishes
    # summaries: the page, the sampling parameters (temperature, top_p, top_k, penalty), the ids of
    # the answer tokens the sampler drew (not the forced ones) -- the repetition penalty's history
    page: Optional[Dict[str, Any]] = None
    max_chars: int = 0
    sampling: Tuple[float, float, int, float] = (0.0, 1.0, 0, 1.0)
    sampled: List[int] = field(default_factory=list)
    page_tokens: int = 0
    truncated: bool = False
    n_kept: int = 0
    # rescoring: a "score" request is one distinct alternative of its parent (kind "rescore", never
    # queued itself); its slot in the running-sum buffers, the rows of it scored so far
    parent: Any = None
    alt: int = 0
    slot: int = -1
    n_scored: int = 0
    texts: Optional[List[str]] = None       # parent: the texts as given, their normalised forms,
    norm: Optional[List[str]] = None        # the distinct ones' ids, the common prefix length,
    alt_ids: Optional[List[List[int]]] = None   # the children and how many are still to retire
    common: int = 0
    children: Optional[List["IntentRequest"]] = None
    left: int = 0

    def stats(self, t_end: float) -> Dict[str, Any]:
        return dict(prompt_tokens=len(self.ids), cached_prefix_tokens=self.cached,
                    prefill_tokens=len(self.ids) - self.cached, decode_steps=self.steps, forced_tokens=self.forced,
                    output_chars=len(self.out), queue_ms=(self.t_start - self.t_submit) * 1e3,
                    prefill_ms=(self.t_first - self.t_start) * 1e3, decode_ms=(t_end - self.t_first) * 1e3,
                    total_ms=(t_end - self.t_start) * 1e3)


_TOK_PENDING = -0x7A7A7A7A  # never a token id nor the sampler's -1 failure code


def end_set_ids(tokenizer) -> List[int]:
    """The ids that close a JSON string -- the turn probe's end set: every non-special id whose
    bytes begin with ``"`` (``token_bytes()`` gives special and unused ids no bytes)."""
    return [i for i, b in enumerate(tokenizer.token_bytes()) if b[:1] == b'"']


class LLMIntentEngine:
    """Grammar-constrained intent decoding with continuous batching.

    Every scheduler iteration (``step``) runs ONE ragged forward over all active requests --
    each contributes its pending rows (last sampled token + jump-forward tokens) and gets its
    logits row back (the LM head runs on one row per request) -- then one masked sampling
    launch for all of them.  New requests are admitted between iterations (prefix-cached
    prompt, prefill of all but the last prompt token, which joins the batched forward), and
    finished ones leave immediately, so a burst of voice sessions shares every weight read.
    """

    name = "llm"

    def __init__(self, engine, tokenizer, grammar: Optional[CompiledGrammar] = None, *, budget_chars: int = 512,
                 temperature: float = 0.1, max_steps: int = 400, seed: int = 0, max_active: Optional[int] = None,
                 chat_format: Callable[[List[Dict[str, str]]], Tuple[str, str]] = llama3_chat):
        self.engine = engine
        self.chat_format = chat_format
        self.tok = tokenizer
        self.grammar = grammar or intent_grammar(tokenizer)
        self.budget_chars = budget_chars
        self.temperature = temperature
        self.max_steps = max_steps
        self.max_active = max_active or engine.max_seqs
        self.max_rows = engine.bufs.max_rows
        dev = engine.device
        self.dev = dev
        pin = dev.type == "cuda"
        self._cuda_index = (dev.index if dev.index is not None else torch.cuda.current_device()) if pin else None
        R, W = self.max_active, self.grammar.words
        # (one mask row per sampled request and probe, and one per row of a rescored alternative)
        self.h_mask = torch.zeros(R + self.max_rows, W, dtype=torch.int32, pin_memory=pin)
        self.h_mask_np = self.h_mask.numpy()
        self.d_mask = torch.zeros(R + self.max_rows, W, dtype=torch.int32, device=dev)
        self.d_temp = torch.full((R,), float(temperature), dtype=torch.float32, device=dev)
        self.d_seed = torch.tensor([seed], dtype=torch.int64, device=dev)
        self.d_step = torch.zeros(1, dtype=torch.int32, device=dev)
        self.d_tok = torch.zeros(R, dtype=torch.int32, device=dev)
        self.h_tok = torch.zeros(R, dtype=torch.int32, pin_memory=pin)
        self.h_tok_np = self.h_tok.numpy()
        # wait for the sampled tokens by polling the pinned readback buffer (sentinel -> token)
        # instead of a stream synchronize: the GPU idles from the sampler's end until the host
        # has posted the next step, so the wake-up latency is on the critical path
        self.spin_wait = pin and ops.env_flag("VWA_SPIN_WAIT")
        # LM head under the grammar mask (LLMEngine.head_logits): the vocab tiles no row may sample
        # are skipped -- 42 % of the tiles live per step on average on the intent grammar
        self.masked_head = ops.env_flag("VWA_MASKED_HEAD")
        # zero-copy host buffers (GPU): the LM head and the sampler read the grammar masks straight
        # from the pinned host rows and the sampler stores the tokens into pinned host memory -- no
        # H2D mask copy and no D2H token copy per step (each a DMA start on the critical path)
        self.zero_copy = pin and ops.env_flag("VWA_ZERO_COPY")
        self.part_val = torch.zeros(R * 64, dtype=torch.float32, device=dev)
        self.part_idx = torch.zeros(R * 64, dtype=torch.int32, device=dev)
        self.last_stats: Dict[str, Any] = {}
        self.last_batch: List[Dict[str, Any]] = []
        self.batch_stats = dict(iterations=0, rows=0, sampled=0, max_active=0)
        # host-side time per scheduler phase (where a decode step's wall time goes)
        self.timing = dict(build_launch_ms=0.0, mask_ms=0.0, sample_launch_ms=0.0, gpu_wait_ms=0.0, post_ms=0.0,
                           admit_prefill_ms=0.0)
        self._prefix_ids: Dict[str, List[int]] = {}
        self._head_len = 0
        # turn probes: the ids that close a JSON string, as packed allow-bits (one shared row); one
        # (log p, log-sum-exp) pair per probe row, read back through pinned memory after a stream
        # synchronise; the traced-run record of the ASR logit steps (off by default)
        self._end_set: Optional[torch.Tensor] = None
        self.d_turn = torch.zeros(R, 2, dtype=torch.float32, device=dev)
        self.h_turn = torch.zeros(R, 2, dtype=torch.float32, pin_memory=pin)
        self.keep_turn_trace = False
        self.last_turn_trace: List[Dict[str, Any]] = []
        self.last_turn_stats: Dict[str, Any] = {}
        # summaries: per-row sampling parameters and history for ops.nucleus_step, staged in one pinned
        # buffer ([temperature | top_p | top_k | penalty] x R, then R x H history ids) and copied in one
        # piece; the narrowed masks and the kept counts it writes; the traced-run record (off by default)
        H = self.summary_history = 64
        self.summary_max_steps = 2048
        self.summary_defaults = dict(max_chars=400, temperature=0.7, top_p=0.9, top_k=50, penalty=1.1)
        self.h_nuc = torch.zeros(4 * R + R * H, dtype=torch.int32, pin_memory=pin)
        self.d_nuc = torch.zeros(4 * R + R * H, dtype=torch.int32, device=dev)
        self.h_nuc_np = self.h_nuc.numpy()
        self.d_nuc_mask = torch.zeros(R, W, dtype=torch.int32, device=dev)
        self.d_nkept = torch.zeros(R, dtype=torch.int32, device=dev)
        self.keep_summary_trace = False
        self._nuc_traced = 0
        self.last_summary_trace: List[Dict[str, Any]] = []
        self.last_summary_stats: Dict[str, Any] = {}
        self.summary_stats = dict(summaries=0, summary_tokens=0, n_kept_sum=0, nucleus_launches=0)
        # rescoring: (target, seq) per scored row staged in pinned memory; the rows' log-probabilities;
        # three buffers of running sums, one slot per sequence being scored -- d_acc[0] holds the verified
        # sums, an iteration's calls write the other two in turn and the last one written becomes d_acc[0]
        # once the step is verified; the traced-run record (off by default)
        S = ops.RESCORE_MAX_SEQ
        self.h_score = torch.zeros(2, self.max_rows, dtype=torch.int32, pin_memory=pin)
        self.d_score = torch.zeros(2, self.max_rows, dtype=torch.int32, device=dev)
        self.h_score_np = self.h_score.numpy()
        self.d_lp = torch.zeros(self.max_rows, dtype=torch.float32, device=dev)
        self.d_acc = [torch.zeros(S, dtype=torch.float32, device=dev) for _ in range(3)]
        self.h_acc = torch.zeros(S, dtype=torch.float32, pin_memory=pin)
        self._score_free = list(range(S - 1, -1, -1))
        self._score_last = 0
        self.keep_rescore_trace = False
        self._score_traced = 0
        self.last_rescore_trace: List[Dict[str, Any]] = []
        self.last_rescore_stats: Dict[str, Any] = {}
        self.waiting: Deque[IntentRequest] = deque()
        self.active: List[IntentRequest] = []
        self._lock = threading.Lock()
        self._wake = threading.Condition(self._lock)
        self._thread: Optional[threading.Thread] = None
        self._stop = False

    # ------------------------------------------------------------------ helpers
    def _encode_prompt(self, messages) -> List[int]:
        return self._encode_head_tail(*self.chat_format(messages))

    def _encode_head_tail(self, head: str, tail: str) -> List[int]:
        ids = self._prefix_ids.get(head)
        if ids is None:
            ids = self.tok.encode(head)
            if len(self._prefix_ids) >= 4:  # the parse head and the summary head, with room for a changed one
                self._prefix_ids.pop(next(iter(self._prefix_ids)))
            self._prefix_ids[head] = ids
        self._head_len = len(ids)  # of the prompt encoded last: a request keeps its own (head_len)
        return ids + self.tok.encode(tail)

    def grammar_bytes(self, tok: int) -> bytes:
        return self.tok.token_bytes()[tok]

    def _jump_forward(self, r: IntentRequest) -> None:
        forced = r.matcher.forced_prefix()
        if forced:
            r.matcher.accept_bytes(forced)
            r.out += forced
            # the grammar forces a small set of strings (JSON syntax, keys, enum values): their
            # standalone encodings are cached (a tokenizer call is ~9 us, 1-2 per sampled token)
            cache = self.__dict__.setdefault("_forced_ids", {})
            ftoks = cache.get(forced)
            if ftoks is None:
                ftoks = self.tok.encode(forced.decode("ascii"))
                if len(cache) < 8192:
                    cache[forced] = ftoks
            r.forced += len(ftoks)
            r.feed += ftoks

    def _admit(self, r: IntentRequest) -> None:
        """Admit one request on its own (prefill included)."""
        self._admit_begin(r)
        self.engine.prefill(r.seq, upto=self._prefill_upto(r))
        self._admit_end(r)

    def _admit_begin(self, r: IntentRequest) -> None:
        """Prompt -> sequence (prefix-cache match) + grammar matcher; the prefill is left to the
        caller (batched over every request admitted in the same iteration).  A turn probe has no
        matcher and no budget: nothing of it is decoded."""
        eng = self.engine
        r.t_start = time.perf_counter()
        if r.kind == "turn":
            r.ids = self._encode_head_tail(*turn_tail(r.probe_text, self.chat_format))
        elif r.kind == "score":
            if r.parent.alt_ids is None:
                self._rescore_prepare(r.parent)
            r.ids = r.parent.alt_ids[r.alt]
            self._head_len = r.parent.head_len
        elif r.kind == "summary":
            self._encode_summary(r)
        else:
            r.ids = self._encode_prompt(r.messages)
            r.matcher = self.grammar.matcher(self.budget_chars)
            if r.matcher.min_completion() > self.budget_chars:
                raise IntentEngineError(f"budget_chars={self.budget_chars} is below the shortest schema-valid "
                                        f"answer ({r.matcher.min_completion()} chars)")
        r.head_len = self._head_len
        r.seq = eng.new_sequence(r.ids)
        r.cached = r.seq.n_computed
        if r.cached >= self._prefill_upto(r) + 1:  # whole prompt cached: recompute its last token for logits
            r.seq.n_computed = r.cached = self._prefill_upto(r)
        if r.kind == "score":
            r.slot = self._score_free.pop()
            self.d_acc[0][r.slot : r.slot + 1].zero_()  # (on the step's stream, before any call reads it)

    def _prefill_upto(self, r: IntentRequest) -> int:
        """How many of the prompt's tokens the admission prefill computes: all but the last -- of a
        rescored alternative, all but the last one it shares with the others (the rest are scored rows)."""
        return (r.parent.common if r.kind == "score" else len(r.ids)) - 1

    def _admit_end(self, r: IntentRequest) -> None:
        r.t_first = time.perf_counter()
        if r.kind == "score":
            r.feed = list(r.ids[r.parent.common - 1 :])  # every one of them is a scored row
            return
        r.feed = [r.ids[-1]]  # the last prompt token joins the batched step
        if r.kind != "turn":
            self._jump_forward(r)

    def _finish(self, r: IntentRequest, error: Optional[BaseException] = None) -> None:
        r.done = True
        r.error = error
        if error is None and r.kind not in ("turn", "score"):
            r.text = r.out.decode("utf-8")
        if r.seq is not None:
            # only the static system + few-shot prefix is shared across requests; the request's
            # own suffix and answer are never served from cache (no replay of repeated commands)
            self.engine.free_sequence(r.seq, publish_upto=r.head_len)
            r.seq = None
        r.t_end = time.perf_counter()
        if r.kind == "score":
            self._rescore_retired(r, error)  # the parent holds the future
            return
        if r.kind == "turn":
            if r.result is not None:
                r.result["ms"] = (r.t_end - r.t_submit) * 1e3
                self.last_turn_stats = r.result
        elif r.kind == "summary":
            if error is None:
                text = json.loads(r.text)["summary"]
                r.result = dict(summary=text, chars=len(text), prompt_tokens=len(r.ids),
                                cached_prefix_tokens=r.cached, page_tokens=r.page_tokens, truncated=r.truncated,
                                decode_steps=r.steps, ms=(r.t_end - r.t_submit) * 1e3)
                self.last_summary_stats = dict(r.result, **r.stats(r.t_end))
                self.summary_stats["summaries"] += 1
                self.summary_stats["summary_tokens"] += r.steps
                self.summary_stats["n_kept_sum"] += r.n_kept
        else:
            self.last_stats = r.stats(r.t_end)
        if r.future is not None:
            if error is None:
                r.future.set_result(r.result if r.kind in ("turn", "summary") else r.text)
            else:
                r.future.set_exception(error)

    # ------------------------------------------------------------------ scheduler
    def submit(self, messages: List[Dict[str, str]], future=None) -> IntentRequest:
        r = IntentRequest(messages=messages, t_submit=time.perf_counter(), future=future)
        with self._lock:
            self.waiting.append(r)
            self._wake.notify()
        return r

    def has_work(self) -> bool:
        return bool(self.active or self.waiting)

    def step(self) -> List[IntentRequest]:
        """One scheduler iteration; returns the requests that finished in it."""
        finished: List[IntentRequest] = []
        admitted: List[IntentRequest] = []
        while len(self.active) + len(admitted) < self.max_active:
            with self._lock:
                if not self.waiting:
                    break
                if self.waiting[0].kind == "score" and not self._score_free:
                    break  # every running-sum slot is taken: it waits for a sequence to retire
                r = self.waiting.popleft()
            try:
                self._admit_begin(r)
                admitted.append(r)
            except Exception as e:  # noqa: BLE001
                self._finish(r, e)
                finished.append(r)
        if admitted:
            # ONE batched prefill of every admitted request's prompt suffix (all but its last
            # token, which joins the decode step below)
            ta = time.perf_counter()
            try:
                self.engine.prefill_batch([(r.seq, self._prefill_upto(r)) for r in admitted])
                self.timing["admit_prefill_ms"] += (time.perf_counter() - ta) * 1e3
            except Exception as e:  # noqa: BLE001
                if getattr(getattr(self.engine.model, "tp", None), "size", 1) > 1:
                    raise  # TP: lockstep is lost -- brain/tp_engine.py ends the group
                for r in admitted:
                    self._finish(r, e)
                    finished.append(r)
                admitted = []
            for r in admitted:
                self._admit_end(r)
                self.active.append(r)
        if not self.active:
            return finished
        # rows: each request's pending tokens; requests that do not fit wait one iteration, a
        # feed longer than the row cap is consumed in pieces (sampled once it is exhausted)
        rows, last, batch, budget = [], [], [], self.max_rows
        # turn probes go after the sampled requests, rows and logits rows alike, and are never
        # given to the sampler: the sampled requests' row indices, their mask rows and the
        # sampler's step counter are what they would be without the probes
        probes: List[IntentRequest] = []
        # summaries are sampled rows after the parse rows: the parse rows keep their row indices, mask
        # rows and (with the one sampler launch per iteration) the sampler's step counter
        # rescored alternatives go last: every row of theirs is a logits row (it is scored, not
        # sampled), after the probes', so that parse, summary and probe rows keep the indices, mask rows
        # and sampler step counter they would have had without them.  (request, first row, rows) each.
        pieces: List[Tuple[IntentRequest, int, int]] = []
        order = self.active
        if any(r.kind != "parse" for r in order):
            order = [r for k in ("parse", "summary", "turn", "score") for r in order if r.kind == k]
        for r in order:
            if not r.feed or budget <= 0:
                continue
            take = r.feed[:budget]
            if len(take) < len(r.feed) and rows:
                continue
            rows += [(r.seq, t) for t in take]
            budget -= len(take)
            r.feed = r.feed[len(take):]
            if r.kind == "score":
                pieces.append((r, len(rows) - len(take), len(take)))
            elif not r.feed:
                last.append(len(rows) - 1)
                (probes if r.kind == "turn" else batch).append(r)
        if not rows:
            return finished
        q = sum(k for _, _, k in pieces)
        sel = last + [i for _, at, k in pieces for i in range(at, at + k)] if pieces else last
        tm = self.timing
        t0 = time.perf_counter()
        if sel and not batch:
            # probes (and scored rows) only: no sampler runs, so no fail word reports a chained launch
            # that timed out -- the step is verified (and, if need be, re-run) synchronously
            self.engine.run_rows(rows, logits_for=sel, check=True, defer_head=True)
        elif sel:
            self.engine.run_rows(rows, logits_for=sel, check=False, defer_head=True)
        else:
            # only part of one long feed fits this iteration: its rows still have to reach the KV
            # cache (nothing is sampled -- no LM head -- so the step is verified synchronously)
            self.engine.run_rows(rows, logits_for=[len(rows) - 1], check=True, defer_head=True)
        t1 = time.perf_counter()
        tm["build_launch_ms"] += (t1 - t0) * 1e3
        self.batch_stats["iterations"] += 1
        self.batch_stats["rows"] += len(rows)
        self.batch_stats["max_active"] = max(self.batch_stats["max_active"], len(self.active))
        if not batch and not probes and not pieces:
            return finished
        n, p = len(batch), len(probes)
        for i, r in enumerate(batch):  # CPU grammar masks overlap the in-flight forward
            r.matcher.fill_mask(self.h_mask_np[i])
        if p + q:
            # a probe reads every column of its row, and so does a scored row: its mask row is all ones
            # and counts in mask_rows, so the masked LM head skips no vocab tile (a skipped tile's
            # logits are stale)
            self.h_mask_np[n : n + p + q] = -1
        t2 = time.perf_counter()
        if not self.zero_copy:
            self.d_mask[: n + p + q].copy_(self.h_mask[: n + p + q], non_blocking=True)
        mask = self.h_mask if self.zero_copy else self.d_mask
        # the LM head under the same masks: only vocab tiles some row may sample are computed
        logits = self.engine.head_logits(col_mask=mask if self.masked_head else None, mask_rows=n + p + q,
                                         gather=False)
        if p:
            self._probe_launch(logits, n, p)  # (before the sampler, on the same stream)
        if q:
            self._score_launch(logits, n + p, pieces)  # (likewise; from the verified sums, out of place)
        ns = sum(r.kind == "summary" for r in batch)
        if ns:
            # one nucleus launch over all sampled rows, in front of the sampler (parse rows pass
            # through): the sampler then reads the narrowed device masks and per-row temperatures
            self._nucleus_launch(logits, batch, n, mask)
            toks = self._sample(logits[:n], n, self.engine.step_fail_word(), narrowed=True)
        elif n:
            toks = self._sample(logits[:n], n, self.engine.step_fail_word())
        else:  # probes only: no sampler launch, the sampler's step counter does not move
            toks = []
            self._t3 = time.perf_counter()
        if any(t == -2 for t in toks):
            # the forward's chained launch timed out at a grid barrier (tokens -2 from the
            # sampler's fail word): re-run the step on the per-kernel path and sample again
            self.engine.host_synced()
            logits = self.engine.recover_step()
            if ns:
                # the re-run logits are fresh (unpenalised): the step runs on them once more, penalty
                # included -- the rows the failed launch penalised are not read again
                self._nucleus_launch(logits, batch, n, mask, rerun=True)
            toks = self._sample(logits[:n], n, None, narrowed=bool(ns))
            if p:
                self._probe_launch(logits, n, p)  # the probes too, from the re-run logits
            if q:
                # and the scored rows, from the same sums the failed launch started from: nothing of
                # it is kept, nothing counts twice
                self._score_launch(logits, n + p, pieces, rerun=True)
        if p:
            self._probe_finish(probes, logits, n, finished)
        if q:
            self._score_finish(pieces, finished)  # the step is verified: its sums become the sums
        self.engine.host_synced()  # the sampled tokens are back: the step's staging copy has run
        t4 = time.perf_counter()
        tm["mask_ms"] += (t2 - t1) * 1e3
        tm["sample_launch_ms"] += (self._t3 - t2) * 1e3
        tm["gpu_wait_ms"] += (t4 - self._t3) * 1e3
        self.batch_stats["sampled"] += n
        if ns:
            self._nucleus_finish(batch, toks, n)
        if any(t == -1 for t in toks):
            self._diagnose(batch, toks, logits, n)
        self._accept(batch, toks, finished)
        if finished:
            self.active = [r for r in self.active if not r.done]
        tm["post_ms"] += (time.perf_counter() - t4) * 1e3
        return finished

    def _sample(self, logits: torch.Tensor, n: int, fail_word: Optional[torch.Tensor],
                narrowed: bool = False) -> List[int]:
        """Masked sampling of the n logits rows (masks already in d_mask) and the token readback.
        ``narrowed``: an iteration with summary rows -- the masks are the nucleus step's output and the
        temperatures the per-row ones it was given."""
        zc = self.zero_copy
        if zc and self.spin_wait:
            self.h_tok_np[:n] = _TOK_PENDING  # before the launch: the sampler stores into it directly
        if narrowed:
            mask, temperature = self.d_nuc_mask, self._nuc_views()[0]
        else:
            mask, temperature = self.h_mask if zc else self.d_mask, self.d_temp if self.temperature > 0 else None
        self.engine.sample(logits, mask=mask, temperature=temperature, seed=self.d_seed,
                           step=self.d_step, out_tokens=self.h_tok if zc else self.d_tok,
                           part_val=self.part_val[: n * 64], part_idx=self.part_idx[: n * 64], fail_word=fail_word)
        if self.dev.type == "cuda" and zc and self.spin_wait:
            t3 = time.perf_counter()
            hv = self.h_tok_np[:n]
            deadline = t3 + 0.05
            while (hv == _TOK_PENDING).any():
                if time.perf_counter() > deadline:  # long step: block on the stream instead
                    torch.cuda.current_stream().synchronize()
                    break
            # (the sampler's system-scope int32 stores land whole; the masks it and the LM head
            # read are done by then -- the host may overwrite them for the next step)
            toks = hv.tolist()
        elif self.dev.type == "cuda":
            if self.spin_wait:
                self.h_tok_np[:n] = _TOK_PENDING
            if zc:
                t3 = time.perf_counter()
                torch.cuda.current_stream().synchronize()
                self._t3 = t3
                return self.h_tok[:n].tolist()
            self.h_tok[:n].copy_(self.d_tok[:n], non_blocking=True)
            t3 = time.perf_counter()
            if self.spin_wait:
                hv = self.h_tok_np[:n]
                deadline = t3 + 0.05
                while (hv == _TOK_PENDING).any():
                    if time.perf_counter() > deadline:  # long step (or none in flight): block instead
                        break
            # always end on the stream: the spin only sees the copy START landing -- its bytes are
            # not written atomically per int32 (seen with two processes on one GPU: the low byte
            # of a token over the sentinel's upper bytes, 0x85858561), so the values are read
            # only after the copy completed.  Polled with stream queries (a blocking synchronize
            # measured +38 us per iteration: its wake-up, not the copy)
            st = torch.cuda.current_stream()
            if self.spin_wait:
                while not st.query():
                    if time.perf_counter() > deadline:
                        break
            st.synchronize()
            toks = self.h_tok[:n].tolist()
        else:
            t3 = time.perf_counter()
            toks = self.d_tok[:n].tolist()
        self._t3 = t3
        return toks

    # ------------------------------------------------------------------ summaries
    def _nuc_views(self, host: bool = False):
        """(temperature f32, top_p f32, top_k i32, penalty f32, history i32 [R, H]) views of the staged
        parameter buffer, on the device (or the host copy)."""
        R, H = self.max_active, self.summary_history
        b = self.h_nuc if host else self.d_nuc
        return (b[:R].view(torch.float32), b[R : 2 * R].view(torch.float32), b[2 * R : 3 * R],
                b[3 * R : 4 * R].view(torch.float32), b[4 * R :].view(R, H))

    def _encode_summary(self, r: IntentRequest) -> None:
        """The summary prompt, the page text cut by tokens so that prompt + worst-case answer (every
        byte of the matcher's budget a token) fits max_model_len; the request's matcher."""
        g = summary_grammar(self.tok, r.max_chars)
        if g.words != self.grammar.words:
            raise IntentEngineError("the summary grammar's mask width differs from the intent grammar's")
        budget = 4 * r.max_chars + 16  # bytes: UTF-8 at its widest, the JSON around the string
        r.matcher = g.matcher(budget)
        room = self.engine.max_model_len - budget - 2
        page = r.page
        text = page["text"].strip()
        ids = self._encode_head_tail(*self.chat_format(summary_messages(text, page.get("title"), page.get("url"))))
        page_ids = self.tok.encode(text)
        keep = len(page_ids)
        while len(ids) > room:
            keep = min(keep - 1, keep - (len(ids) - room))
            if keep < 1:
                raise IntentEngineError(f"max_chars={r.max_chars} leaves no room for the page within "
                                        f"max_model_len={self.engine.max_model_len}")
            r.truncated = True
            text = self.tok.decode(page_ids[:keep]).strip()
            ids = self._encode_head_tail(*self.chat_format(summary_messages(text, page.get("title"), page.get("url"))))
        r.page_tokens = len(self.tok.encode(text)) if r.truncated else len(page_ids)
        r.ids = ids

    def _nucleus_launch(self, logits: torch.Tensor, batch: List[IntentRequest], n: int, mask: torch.Tensor,
                        rerun: bool = False) -> None:
        """One ops.nucleus_step launch over the n sampled rows (64 per launch at most): parse rows get
        pass-through parameters (top_k 0, top_p 1, penalty 1), summary rows their own and the ids they
        sampled last.  The narrowed masks land in d_nuc_mask, the kept counts in d_nkept."""
        R, H = self.max_active, self.summary_history
        hv = self.h_nuc_np
        fv = hv.view(np.float32)
        hist = hv[4 * R :].reshape(R, H)
        for i, r in enumerate(batch):
            if r.kind == "summary":
                T, p, k, th = r.sampling
                h = r.sampled[-H:]
            else:
                T, p, k, th, h = max(float(self.temperature), 0.0), 1.0, 0, 1.0, ()
            fv[i], fv[R + i], hv[2 * R + i], fv[3 * R + i] = T, p, k, th
            hist[i, : len(h)] = h
            hist[i, len(h) :] = -1
        self.d_nuc.copy_(self.h_nuc, non_blocking=True)
        dT, dp, dk, dth, dh = self._nuc_views()
        trace = self.keep_summary_trace
        pre = logits[:n].clone() if trace else None
        V = logits.shape[1]
        for i in range(0, n, ops.NUCLEUS_MAX_ROWS):
            j = min(n, i + ops.NUCLEUS_MAX_ROWS)
            ops.nucleus_step(logits[i:j], mask[i:j], self.d_nuc_mask[i:j], self.d_nkept[i:j], dT[i:j], dp[i:j],
                             dk[i:j], dth[i:j], dh[i:j], vocab=V)
            self.summary_stats["nucleus_launches"] += 1
        if trace:
            if rerun and self._nuc_traced:  # the failed launch's records describe logits nobody sampled from
                del self.last_summary_trace[-self._nuc_traced :]
            self._nuc_traced = 0
            hT, hp, hk, hth, hh = self._nuc_views(host=True)
            for i, r in enumerate(batch):
                if r.kind == "summary":
                    self.last_summary_trace.append(dict(
                        request=r, row=i, step=r.steps, rows=n, logits=pre[i].detach().cpu(),
                        mask_in=mask[i].detach().cpu().clone(), temperature=float(hT[i]), top_p=float(hp[i]),
                        top_k=int(hk[i]), penalty=float(hth[i]), history=hh[i].clone()))
                    self._nuc_traced += 1

    def _nucleus_finish(self, batch: List[IntentRequest], toks: List[int], n: int) -> None:
        """After the tokens are back: the summary rows' kept counts (read after a stream synchronise, as
        the probes' results are) into the requests' statistics, and the traced rows' outputs."""
        if self.dev.type == "cuda":
            torch.cuda.current_stream().synchronize()
        kept = self.d_nkept[:n].tolist()
        for i, r in enumerate(batch):
            if r.kind == "summary":
                r.n_kept += kept[i]
        if self.keep_summary_trace:
            out = self.d_nuc_mask[:n].cpu()
            for tr in self.last_summary_trace[-self._nuc_traced :]:
                i = tr["row"]
                tr.update(mask_out=out[i].clone(), n_kept=kept[i], token=toks[i])

    def submit_summary(self, text: str, title: Optional[str] = None, url: Optional[str] = None, *,
                       max_chars: Optional[int] = None, temperature: Optional[float] = None,
                       top_p: Optional[float] = None, top_k: Optional[int] = None, penalty: Optional[float] = None,
                       future=None) -> IntentRequest:
        """Queue a summary of the page ``text`` (admitted like any request)."""
        if getattr(getattr(self.engine.model, "tp", None), "size", 1) > 1:
            raise IntentEngineError("summaries are not supported under tensor parallelism (vocab-parallel logits)")
        if not isinstance(text, str) or not text.strip():
            raise IntentEngineError("summary: text must be a non-empty string")
        d = self.summary_defaults
        pick = lambda v, k: d[k] if v is None else v  # noqa: E731
        max_chars = int(pick(max_chars, "max_chars"))
        T, p, k, th = (float(pick(temperature, "temperature")), float(pick(top_p, "top_p")), int(pick(top_k, "top_k")),
                       float(pick(penalty, "penalty")))
        if not 1 <= max_chars <= 4096:
            raise IntentEngineError("summary: max_chars must be in [1, 4096]")
        if not 0 <= k <= ops.NUCLEUS_MAX_TOP_K or (p < 1.0 and k < 1) or not p > 0.0 or not th > 0.0:
            raise IntentEngineError("summary: top_k must be in [0, 1024] (>= 1 with top_p < 1), top_p and penalty > 0")
        r = IntentRequest(messages=[], t_submit=time.perf_counter(), future=future, kind="summary",
                          page=dict(text=text, title=title, url=url), max_chars=max_chars, sampling=(T, p, k, th))
        with self._lock:
            self.waiting.append(r)
            self._wake.notify()
        return r

    def summary_async(self, text: str, title: Optional[str] = None, url: Optional[str] = None, **kw):
        """concurrent.futures.Future resolved with the summary's dict (requires start())."""
        fut: Future = Future()
        self.submit_summary(text, title, url, future=fut, **kw)
        return fut

    def summary(self, text: str, title: Optional[str] = None, url: Optional[str] = None, **kw) -> Dict[str, Any]:
        """A spoken-style summary of a page: ``{"summary", "chars", "prompt_tokens", "cached_prefix_tokens",
        "page_tokens", "truncated", "decode_steps", "ms"}``.  Through the background scheduler when it
        runs, otherwise by stepping here."""
        if self._thread is not None:
            return self.summary_async(text, title, url, **kw).result()
        r = self.submit_summary(text, title, url, **kw)
        while not r.done:
            self.step()
        if r.error is not None:
            raise r.error
        return r.result

    # ------------------------------------------------------------------ turn probes
    def end_set_ids(self) -> List[int]:
        return end_set_ids(self.tok)

    def end_set(self) -> torch.Tensor:
        """``end_set_ids`` as packed allow-bits, int32 [1, words], like the grammar masks and as
        wide as the model's padded vocabulary; built once per engine (per tokenizer)."""
        if self._end_set is None:
            words = max(self.grammar.words, (self.engine.model.cfg.vocab_size + 31) // 32)
            bits = np.zeros(words * 32, dtype=np.uint8)
            bits[self.end_set_ids()] = 1
            packed = np.packbits(bits, bitorder="little").view(np.int32).reshape(1, words)
            self._end_set = torch.from_numpy(packed.copy()).to(self.dev)
        return self._end_set

    def _probe_launch(self, logits: torch.Tensor, n: int, p: int) -> None:
        """One set_logprob launch over the probes' logits rows [n, n + p): (log p(end set), log-sum-exp)
        per row into d_turn, and their copy to pinned memory, both on the step's stream."""
        for i in range(0, p, ops.TURN_MAX_ROWS):
            rows = logits[n + i : n + min(p, i + ops.TURN_MAX_ROWS)]
            ops.set_logprob(rows, rows.shape[1], self.end_set(), out=self.d_turn[i : i + rows.shape[0]])
        if self.dev.type == "cuda":
            self.h_turn[:p].copy_(self.d_turn[:p], non_blocking=True)

    def _probe_finish(self, probes: List[IntentRequest], logits: torch.Tensor, n: int,
                      finished: List[IntentRequest]) -> None:
        """Read the probes' results and retire them in this iteration.  The host reads only after the
        stream is synchronised: seeing the sampler's tokens land (the pinned-buffer spin wait, the
        zero-copy tokens) proves nothing about another kernel's output or its copy (the torn read
        recorded at ``_sample``)."""
        p = len(probes)
        if self.dev.type == "cuda":
            torch.cuda.current_stream().synchronize()
            out = self.h_turn[:p].clone()
        else:
            out = self.d_turn[:p].clone()
        for j, r in enumerate(probes):
            lp = float(out[j, 0])
            r.result = dict(p_end=float(np.exp(lp)), logprob=lp, prompt_tokens=len(r.ids),
                            cached_prefix_tokens=r.cached, ms=0.0)
            if self.keep_turn_trace:
                self.last_turn_trace.append(dict(
                    text=r.probe_text, ids=list(r.ids), row=n + j, logits=logits[n + j].detach().cpu().clone(),
                    set=self.end_set().cpu().clone(), out=out[j].clone()))
            self.batch_stats["probes"] = self.batch_stats.get("probes", 0) + 1
            self._finish(r)  # frees the sequence; only the static head is published
            finished.append(r)

    def submit_turn(self, text: str, future=None) -> IntentRequest:
        """Queue a turn-completion probe of ``text`` (admitted like any request)."""
        if getattr(getattr(self.engine.model, "tp", None), "size", 1) > 1:
            raise IntentEngineError("turn probes are not supported under tensor parallelism (vocab-parallel logits)")
        if not isinstance(text, str):
            raise IntentEngineError("turn: text must be a string")
        r = IntentRequest(messages=[], t_submit=time.perf_counter(), future=future, kind="turn", probe_text=text)
        with self._lock:
            self.waiting.append(r)
            self._wake.notify()
        return r

    def turn_async(self, text: str):
        """concurrent.futures.Future resolved with the probe's dict (requires start())."""
        fut: Future = Future()
        self.submit_turn(text, future=fut)
        return fut

    def turn(self, text: str) -> Dict[str, Any]:
        """How likely ``text`` is a finished command: ``{"p_end", "logprob", "prompt_tokens",
        "cached_prefix_tokens", "ms"}`` -- the probability (and its log) that the token after
        ``{"text":"<text>`` closes the string.  Through the background scheduler when it runs,
        otherwise by stepping here."""
        if self._thread is not None:
            return self.turn_async(text).result()
        r = self.submit_turn(text)
        while not r.done:
            self.step()
        if r.error is not None:
            raise r.error
        return r.result

    # ------------------------------------------------------------------ n-best rescoring
    def _rescore_prepare(self, par: IntentRequest) -> None:
        """The ids of every distinct alternative -- exactly a turn probe's -- and the length of their
        longest common prefix (at most the shortest): what lies inside it has the same probability
        under every alternative and is not scored."""
        ids = [self._encode_head_tail(*turn_tail(c.probe_text, self.chat_format)) for c in par.children]
        par.head_len = self._head_len
        c, m = 0, min(len(x) for x in ids)
        while c < m and all(x[c] == ids[0][c] for x in ids):
            c += 1
        par.alt_ids, par.common = ids, c

    def _score_launch(self, logits: torch.Tensor, base: int, pieces: List[Tuple[IntentRequest, int, int]],
                      rerun: bool = False) -> None:
        """One ops.seq_logprob call (256 rows per piece at most) over the scored rows' logits rows
        [base, base + q): row p of a sequence carries target ids[p + 1], its last row -1 (the end set);
        seq is the sequence's slot.  The sums start from d_acc[0], the verified ones, and land in another
        buffer (``_score_last``): a re-run after a failed chained launch starts from d_acc[0] again."""
        hv = self.h_score_np
        j = 0
        for r, _, k in pieces:
            pos = r.parent.common - 1 + r.n_scored  # the position of this piece's first row
            nxt = r.ids[pos + 1 : pos + 1 + k]
            hv[0, j : j + k] = nxt + [-1] * (k - len(nxt))
            hv[1, j : j + k] = r.slot
            j += k
        q = j
        self.d_score.copy_(self.h_score, non_blocking=True)
        V, S, step = logits.shape[1], ops.RESCORE_MAX_SEQ, ops.RESCORE_MAX_ROWS
        trace = self.keep_rescore_trace
        if trace and rerun and self._score_traced:  # the failed launch's records describe logits nobody kept
            del self.last_rescore_trace[-self._score_traced :]
        self._score_traced = 0
        src = 0
        for n_call, i in enumerate(range(0, q, step)):
            e = min(q, i + step)
            dst = 1 + (n_call & 1)
            ops.seq_logprob(logits[base + i : base + e], V, self.d_score[0, i:e], self.end_set(), self.d_score[1, i:e],
                            S, acc_in=self.d_acc[src], lp=self.d_lp[i:e], acc_out=self.d_acc[dst])
            if trace:
                reqs = [r for r, _, _ in pieces]
                self.last_rescore_trace.append(dict(
                    texts=[r.probe_text for r in reqs], ids=[list(r.ids) for r in reqs], slots=[r.slot for r in reqs],
                    first_pos=[r.parent.common - 1 + r.n_scored for r in reqs], counts=[k for _, _, k in pieces],
                    rows=list(range(base + i, base + e)), target=self.h_score[0, i:e].clone(),
                    seq=self.h_score[1, i:e].clone(), logits=logits[base + i : base + e].detach().cpu().clone(),
                    set=self.end_set().cpu().clone(), acc_in=self.d_acc[src].cpu().clone(),
                    lp=self.d_lp[i:e].cpu().clone(), acc_out=self.d_acc[dst].cpu().clone()))
                self._score_traced += 1
            src = dst
        self._score_last = src

    def _score_finish(self, pieces: List[Tuple[IntentRequest, int, int]], finished: List[IntentRequest]) -> None:
        """The step is verified: the sums it wrote become the verified ones, and the sequences whose last
        row it scored retire in this iteration.  The host reads only after the stream is synchronised
        (see ``_probe_finish``); the synchronise also frees the pinned (target, seq) rows for the next
        iteration."""
        a = self.d_acc
        a[0], a[self._score_last] = a[self._score_last], a[0]
        done = []
        for r, _, k in pieces:
            r.n_scored += k
            self.batch_stats["rescore_rows"] = self.batch_stats.get("rescore_rows", 0) + k
            if not r.feed:
                done.append(r)
        if self.dev.type == "cuda":
            if done:
                self.h_acc.copy_(a[0], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            out = self.h_acc
        else:
            out = a[0]
        for r in done:
            r.result = float(out[r.slot])
            self._finish(r)  # frees the sequence; only the static head is published
            finished.append(r)

    def _rescore_retired(self, r: IntentRequest, error: Optional[BaseException]) -> None:
        """A scored sequence left (``_finish``): its slot is free again; the parent resolves with its last."""
        if r.slot >= 0:
            self._score_free.append(r.slot)
            r.slot = -1
        par = r.parent
        par.left -= 1
        if error is not None and par.error is None:
            par.error = error
        if par.left:
            return
        par.done = True
        par.t_end = time.perf_counter()
        if par.error is None:
            by = {c.probe_text: c for c in par.children}
            of = [by[t] for t in par.norm]
            par.result = dict(scores=[c.result for c in of], scored_tokens=[c.n_scored for c in of],
                              common_prefix_tokens=par.common, prompt_tokens=[len(c.ids) for c in of],
                              cached_prefix_tokens=min(c.cached for c in par.children),
                              ms=(par.t_end - par.t_submit) * 1e3)
            self.last_rescore_stats = par.result
            self.batch_stats["rescores"] = self.batch_stats.get("rescores", 0) + 1
        if par.future is not None:
            if par.error is None:
                par.future.set_result(par.result)
            else:
                par.future.set_exception(par.error)

    def submit_rescore(self, texts: List[str], future=None) -> IntentRequest:
        """Queue the rescoring of 1..8 alternatives: one sequence per distinct normalised text, admitted
        like any request.  Returns the parent request (done when its last sequence has retired)."""
        if getattr(getattr(self.engine.model, "tp", None), "size", 1) > 1:
            raise IntentEngineError("rescoring is not supported under tensor parallelism (vocab-parallel logits)")
        if not isinstance(texts, (list, tuple)) or not 1 <= len(texts) <= 8 \
                or not all(isinstance(t, str) for t in texts):
            raise IntentEngineError("rescore: texts must be a list of 1..8 strings")
        norm = [turn_text(t) for t in texts]
        now = time.perf_counter()
        par = IntentRequest(messages=[], t_submit=now, future=future, kind="rescore", texts=list(texts), norm=norm)
        par.children = [IntentRequest(messages=[], t_submit=now, kind="score", probe_text=t, parent=par, alt=i)
                        for i, t in enumerate(dict.fromkeys(norm))]
        par.left = len(par.children)
        with self._lock:
            self.waiting.extend(par.children)
            self._wake.notify()
        return par

    def rescore_async(self, texts: List[str]):
        """concurrent.futures.Future resolved with the rescoring's dict (requires start())."""
        fut: Future = Future()
        self.submit_rescore(texts, future=fut)
        return fut

    def rescore(self, texts: List[str]) -> Dict[str, Any]:
        """Language-model scores of the recogniser's alternatives: ``{"scores", "scored_tokens",
        "common_prefix_tokens", "prompt_tokens", "cached_prefix_tokens", "ms"}``.  ``scores[i]`` is the
        log-probability, given the ids all alternatives share, that the user's text is exactly
        ``turn_text(texts[i])``: the sum over the ids after the common prefix plus the turn probe's
        ``logprob`` (the string closes).  Alternatives that normalise to the same string are scored once
        and share the value.  The scores of ONE call are comparable with each other and only with each
        other: another call has another common prefix.  Through the background scheduler when it runs,
        otherwise by stepping here."""
        if self._thread is not None:
            return self.rescore_async(texts).result()
        r = self.submit_rescore(texts)
        while not r.done:
            self.step()
        if r.error is not None:
            raise r.error
        return r.result

    def _diagnose(self, batch, toks, logits, n) -> None:
        """A -1 token means no admissible token had a finite logit: record what the row looked like
        (mask population, finite admissible logits) in the request's error for the logs."""
        for i, (r, t) in enumerate(zip(batch, toks)):
            if t != -1:
                continue
            words = torch.from_numpy(self.h_mask_np[i].copy()).to(torch.int64) & 0xFFFFFFFF
            bits = ((words[:, None] >> torch.arange(32)[None, :]) & 1).reshape(-1).bool()
            row = logits[i].float().cpu()
            lo = self.engine.model.v_start if getattr(self.engine.model, "tp", None) and self.engine.model.tp.size > 1 else 0
            adm = bits[lo : lo + row.shape[0]]
            vals = row[adm[: row.shape[0]]]
            r.diag = (f"row {i}/{n}: {int(bits.sum())} admissible tokens, {int(torch.isfinite(vals).sum())} finite "
                      f"admissible logits, row finite {int(torch.isfinite(row).sum())}/{row.numel()}, step {r.steps}, "
                      f"out {bytes(r.out[-40:])!r}")

    def _accept(self, batch: List[IntentRequest], toks: List[int], finished: List[IntentRequest]) -> None:
        for r, tok in zip(batch, toks):
            r.steps += 1
            m = r.matcher
            if tok < 0 or not m.accept_token(tok):
                self.batch_stats["rejects"] = self.batch_stats.get("rejects", 0) + 1
                self._finish(r, IntentEngineError(f"sampler returned a token the grammar rejects ({tok})"
                                                  + (f": {r.diag}" if getattr(r, "diag", None) else "")))
            else:
                r.out += self.grammar_bytes(tok)
                if r.kind == "summary":
                    r.sampled.append(tok)
                if m.is_accept():
                    r.seq.tokens.append(tok)
                    self._finish(r)
                elif r.steps >= (self.summary_max_steps if r.kind == "summary" else self.max_steps):
                    self._finish(r, IntentEngineError("decode step limit reached"))
                else:
                    r.feed = [tok]
                    self._jump_forward(r)
            if r.done:
                finished.append(r)

    def engine_stats(self) -> Dict[str, Any]:
        """Scheduler + KV-cache state for /metrics (batch size, KV utilisation, grammar cache)."""
        eng = self.engine
        bm = eng.blocks
        used = bm.num_blocks - bm.n_free()
        it = max(1, self.batch_stats["iterations"])
        out = {"active": len(self.active), "waiting": len(self.waiting),
               "kv_blocks_used": used, "kv_blocks_total": bm.num_blocks,
               "kv_utilisation": round(used / max(1, bm.num_blocks), 4),
               "rows_per_iteration": round(self.batch_stats["rows"] / it, 3),
               "samples_per_iteration": round(self.batch_stats["sampled"] / it, 3),
               "grammar_rejects": self.batch_stats.get("rejects", 0),
               "rescores": self.batch_stats.get("rescores", 0),
               "rescore_rows": self.batch_stats.get("rescore_rows", 0),
               "host_ms": {k: round(v, 1) for k, v in self.timing.items()}}
        out.update(self.grammar.stats())
        out.update({k: v for k, v in eng.stats.items()})
        return out

    def run_until_idle(self) -> None:
        while self.has_work():
            self.step()

    def generate_many(self, messages_list: List[List[Dict[str, str]]]) -> List[str]:
        """Decode a batch of requests together (continuous batching); raises the first error."""
        reqs = [self.submit(m) for m in messages_list]
        while not all(r.done for r in reqs):
            self.step()
        self.last_batch = [dict(r.stats(r.t_end), latency_ms=(r.t_end - r.t_submit) * 1e3) for r in reqs]
        for r in reqs:
            if r.error is not None:
                raise r.error
        return [r.text for r in reqs]

    def generate(self, messages: List[Dict[str, str]]) -> str:
        return self.generate_many([messages])[0]

    def __call__(self, messages: List[Dict[str, str]]) -> Any:
        """callLLMJSON parity: returns the parsed JSON object."""
        return json.loads(self.generate(messages))

    def parse(self, request: Dict[str, Any], repair: bool = False) -> Any:
        return self(messages_for(request, repair=repair))

    def parse_many(self, requests: List[Dict[str, Any]]) -> List[Any]:
        return [json.loads(t) for t in self.generate_many([messages_for(r) for r in requests])]

    # ------------------------------------------------------------------ background serving
    def start(self) -> None:
        """Run the scheduler on a background thread (the brain service submits into it)."""
        if self._thread is not None:
            return
        self._stop = False
        self._thread = threading.Thread(target=self._loop, name="intent-scheduler", daemon=True)
        self._thread.start()

    def stop(self) -> None:
        with self._lock:
            self._stop = True
            self._wake.notify()
        if self._thread is not None:
            self._thread.join(timeout=30)
            self._thread = None

    def _loop(self) -> None:
        if self.dev.type == "cuda":
            # the scheduler thread inherits no current device: use the model's ("cuda" with no
            # index means the device that was current when the engine was built)
            torch.cuda.set_device(self._cuda_index)
        while True:
            with self._lock:
                while not self._stop and not self.waiting and not self.active:
                    self._wake.wait()
                if self._stop:
                    return
            try:
                self.step()
            except Exception as e:  # noqa: BLE001  (fail every in-flight request, keep serving)
                for r in self.active:
                    self._finish(r, e)
                self.active = []

    def submit_async(self, messages: List[Dict[str, str]]):
        """concurrent.futures.Future resolved with the JSON text (requires start())."""
        fut: Future = Future()
        self.submit(messages, future=fut)
        return fut


class FakeIntentEngine:
    """Deterministic stand-in (tests / CPU-only service runs): returns a canned or computed reply."""

    name = "fake"

    def __init__(self, reply: Optional[Any] = None, fn: Optional[Callable[[List[Dict[str, str]]], Any]] = None,
                 fail: Optional[BaseException] = None):
        self.reply = reply
        self.fn = fn
        self.fail = fail
        self.calls: List[List[Dict[str, str]]] = []

    def __call__(self, messages):
        self.calls.append(messages)
        if self.fail is not None:
            raise self.fail
        if self.fn is not None:
            return self.fn(messages)
        if isinstance(self.reply, list):  # sequence of replies (first call, repair call, ...)
            return self.reply[min(len(self.calls) - 1, len(self.reply) - 1)]
        return self.reply

    def parse(self, request, repair=False):
        return self(messages_for(request, repair=repair))


def keyword_intents(messages) -> Dict[str, Any]:
    """Rule-based fallback engine used when no model is configured (keeps /parse usable on CPU)."""
    req = json.loads(messages[-1]["content"]) if messages[-1]["role"] == "user" else json.loads(messages[-2]["content"])
    text = req.get("text", "").lower()
    it: Dict[str, Any]
    if text.startswith("search") or "search for" in text:
        q = text.split("search", 1)[1].replace("for ", "", 1).strip()
        it = {"type": "search", "args": {"query": q}, "priority": 0, "requires_confirmation": False}
    elif text.startswith(("go to", "open ", "navigate")) and "." in text:
        url = text.split()[-1]
        it = {"type": "navigate", "args": {"url": url if url.startswith("http") else "https://" + url}, "priority": 0,
              "requires_confirmation": False}
    elif "scroll" in text:
        it = {"type": "scroll", "args": {"direction": "up" if "up" in text else "down"}, "priority": 0,
              "requires_confirmation": False}
    elif "back" in text:
        it = {"type": "back", "args": {}, "priority": 0, "requires_confirmation": False}
    elif "screenshot" in text:
        it = {"type": "screenshot", "args": {"label": "voice"}, "priority": 0, "requires_confirmation": False}
    else:
        return {"version": "1.0", "intents": [{"type": "unknown", "args": {}, "priority": 0,
                                               "requires_confirmation": False}],
                "context_updates": {}, "confidence": 0.4, "follow_up_question": "What should I do on the page?"}
    return {"version": "1.0", "intents": [it], "context_updates": {}, "confidence": 0.7,
            "tts_summary": f"Running {it['type']}."}
