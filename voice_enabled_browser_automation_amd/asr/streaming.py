"""Streaming recognition with Deepgram-compatible events (replaces the Deepgram live connection,
apps/voice/src/deepgram.ts:33-51).

The voice server feeds raw PCM16 LE 16 kHz mono frames (the UI sends ~60 ms packets,
apps/web/src/App.tsx:279-288) -- or, to a session made with a wire format (``fmt=``: asr/wire.py
AudioFormat, Deepgram's encoding / sample_rate / channels), frames of that format: the window then
holds the wire bytes, the VAD reads a mono int16 view decoded here, every time below is counted at
the format's own rate, and the recogniser turns the window into 16 kHz samples on the GPU
(AsrEngine.wire_to_audio).  A session keeps the current utterance buffer and:

* energy VAD on 20 ms frames tracks speech start and trailing silence;
* every ``partial_every_s`` of new speech it runs a recognition pass and emits an interim result
  (``is_final: false``), like Deepgram's interim_results;
* **local agreement**: the token prefix on which the last two interim hypotheses agree is
  *committed* -- later passes force it as the decoder prefix (prefilled in one ragged step with
  the SOT tokens) and decode only the continuation, so a long utterance does not re-decode its
  whole transcript at every partial, and the committed words never flicker;
* on an endpoint (``endpoint_silence_s`` of silence after speech, ``VWA_ENDPOINT_MS``), on
  ``flush()`` (client end-of-utterance) or when the 30 s Whisper window is full, it emits a final
  result (``is_final: true, speech_final: true``) and starts a new utterance;
* **long-form** (``VWA_ASR_LONGFORM``, off by default): a full window is not finalised whole.  One
  boundary pass decodes it with timestamp tokens (asr/segments.py); the window is cut at the end
  of the last segment that pass closes, the audio before the cut gets the normal final pass and
  its final says ``speech_final: false`` (the speaker is still talking), and the audio after the
  cut opens the next window of the same utterance -- no word is split by the cut;
* **speculative final**: once the trailing silence reaches ``spec_silence_s``
  (``VWA_SPEC_FINAL_MS``, shorter than the endpoint) the final recognition pass is started in the
  background on the utterance so far; if the silence lasts to the endpoint its result IS the final
  (no pass after the endpoint), if speech resumes it is discarded -- so the final costs the
  endpoint wait alone, not endpoint + a recognition pass (Deepgram's live endpointing finalises
  without a client-side wait, deepgram.ts:36-45);
* the VAD threshold adapts to the noise floor (``max(energy_threshold, noise_mult x floor)``; the
  floor is bootstrapped from a stationary mic-open period and kept by the non-speech frames), so a
  noisy microphone still endpoints.

Recognition passes go through a *recognizer* (``recognize(pcm, prefix) -> Hypothesis``).
``AsrBatcher`` is the serving recognizer: one scheduler thread per GPU engine that gathers the
pending passes of ALL live sessions and runs them as one batch (``AsrEngine.decode_many``: one
batched encoder pass, then one ragged decode step per token for every session) -- the
session-DP unit of a GPU.

Events use the Deepgram ``Results`` shape that the unchanged UI and voice logic read
(``payload.is_final``, ``payload.channel.alternatives[0].transcript``; apps/voice/src/server.ts:112,123).
"""
from __future__ import annotations

import math
import threading
import time
from concurrent.futures import Future
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, List, Optional, Sequence

import numpy as np

from .segments import cut_index, ts_time
from .words import confidence as _confidence
from .wire import AudioFormat, WireAudio, mono_int16
from .words import shift_words


def results_event(text: str, *, is_final: bool, start: float, duration: float, model: str,
                  confidence: float = 0.0, words: Optional[List[Dict]] = None, language: Optional[str] = None,
                  language_confidence: Optional[float] = None, no_speech_prob: Optional[float] = None,
                  alternatives: Optional[List[Dict]] = None, speech_final: Optional[bool] = None,
                  logprobs: Optional[List[float]] = None) -> Dict:
    """``words``: the alternative's Deepgram word list ({"word", "punctuated_word", "start", "end",
    "confidence"}, stream-clock seconds); None: the empty list.  ``language``: the detected (or
    set) language code -- Deepgram's ``channel.detected_language`` / ``language_confidence`` and
    the alternative's ``languages``.  ``no_speech_prob``: of a final the no-speech gate emptied
    (``metadata.no_speech_prob``).  ``alternatives``: the ranked hypotheses after the first
    ({"transcript", "confidence"}, from a beam pass) -- ``channel.alternatives[1:]`` in Deepgram's
    shape, with no words.  ``speech_final``: a final of a long utterance cut at a segment end says
    False -- the speaker has not stopped (None: as ``is_final``).  ``logprobs``: the acoustic sum
    log-probability of every alternative, the first included (a beam final of a session that rescores:
    the brain's n-best rescoring weighs it against its own score) -- alternative i then carries
    ``"logprob"``.  Without them the event is unchanged."""
    ev = {
        "type": "Results",
        "channel_index": [0, 1],
        "duration": round(duration, 3),
        "start": round(start, 3),
        "is_final": is_final,
        "speech_final": is_final if speech_final is None else bool(speech_final),
        "channel": {"alternatives": [{"transcript": text, "confidence": confidence,
                                      "words": list(words) if words else []}]},
        "metadata": {"model_info": {"name": model}},
    }
    if language is not None:
        ev["channel"]["detected_language"] = language
        ev["channel"]["language_confidence"] = 0.0 if language_confidence is None else language_confidence
        ev["channel"]["alternatives"][0]["languages"] = [language]
    if no_speech_prob is not None:
        ev["metadata"]["no_speech_prob"] = no_speech_prob
    for alt in alternatives or []:
        ev["channel"]["alternatives"].append({"transcript": alt["transcript"], "confidence": alt["confidence"],
                                              "words": []})
    if logprobs is not None:
        for alt, lp in zip(ev["channel"]["alternatives"], logprobs):
            alt["logprob"] = float(lp)
    return ev


@dataclass
class Hypothesis:
    """One recognition pass: the full transcript's token ids (forced prefix included) and text;
    from a pass that was asked for them, the words (asr/words.py, seconds from the utterance's
    start) and the transcript's confidence; from an engine that analysed the start-of-transcript
    logits, the language the pass decoded under, its probability and the probability that the
    window holds no speech; from a beam pass, the ranked hypotheses after the first
    (``alternatives``: {"transcript", "confidence" = exp(avg_logprob)}) -- ``confidence`` is then
    the best hypothesis' exp(avg_logprob) unless the words pass set it, and ``beam_logprobs`` the
    ranked hypotheses' sum log-probabilities, the first included; from a timestamp pass,
    ``tokens`` holds the timestamp tokens too and ``segments`` the transcript's segments
    (asr/segments.py: {start, end, tokens, text}, seconds from the window's start); from a pass under
    the quality gate (``fallback=``), ``score``: the engine's score entry of the returned attempt
    (asr/fallback.py score_entry) -- ``confidence`` is then exp(avg_logprob) unless the words pass set it."""

    tokens: List[int] = field(default_factory=list)
    text: str = ""
    words: List[Dict] = field(default_factory=list)
    confidence: float = 0.0
    language: Optional[str] = None
    language_confidence: Optional[float] = None
    no_speech_prob: Optional[float] = None
    alternatives: List[Dict] = field(default_factory=list)
    beam_logprobs: List[float] = field(default_factory=list)
    segments: List[Dict] = field(default_factory=list)
    score: Optional[Dict] = None


class TextRecognizer:
    """Adapter for a plain ``transcribe(pcm) -> str`` callable (tests, CPU stand-ins): no token
    ids, so no committed prefix (local agreement is a no-op)."""

    def __init__(self, fn: Callable[[np.ndarray], str]):
        self.fn = fn

    def recognize(self, pcm: np.ndarray, prefix: Sequence[int] = ()) -> Hypothesis:
        return Hypothesis([], self.fn(pcm).strip())


def _as_recognizer(r: Any):
    return r if hasattr(r, "recognize") else TextRecognizer(r)


def recognize_async(rec: Any, pcm: np.ndarray, prefix: Sequence[int] = (), **kw) -> Future:
    """A recognition pass that runs in the background when the recognizer can (AsrBatcher: queued
    for the next GPU batch), else synchronously into an already completed Future.  ``kw``: passed
    on (``words=True``: a final pass of a session that wants word timestamps)."""
    if hasattr(rec, "recognize_async"):
        return rec.recognize_async(pcm, prefix, **kw)
    fut: Future = Future()
    try:
        fut.set_result(rec.recognize(pcm, prefix, **kw))
    except BaseException as e:  # noqa: BLE001
        fut.set_exception(e)
    return fut


def common_prefix(a: Sequence[int], b: Sequence[int]) -> int:
    n = min(len(a), len(b))
    i = 0
    while i < n and a[i] == b[i]:
        i += 1
    return i


class StreamingAsrSession:
    def __init__(self, recognizer: Any, *, rate: int = 16000, model_name: str = "whisper",
                 partial_every_s: float = 1.0, endpoint_silence_s: Optional[float] = None,
                 energy_threshold: Optional[float] = None, max_window_s: float = 30.0, min_speech_s: float = 0.2,
                 local_agreement: bool = True, spec_silence_s: Optional[float] = None,
                 noise_mult: Optional[float] = None, words: Optional[bool] = None, language: Optional[str] = None,
                 no_speech_threshold: Optional[float] = None, beam: Optional[int] = None,
                 alternatives: Optional[int] = None, keyterms=None, longform: Optional[bool] = None,
                 fallback=None, fallback_reject: Optional[bool] = None, fmt: Optional[AudioFormat] = None,
                 rescore: Optional[bool] = None):
        from ..utils.env import asr_beam_knobs, knob

        # the wire format (asr/wire.py; None: mono PCM16 at ``rate``, the session as it always was).
        # With one, the window buffer holds wire frames and the recogniser gets them as a WireAudio
        # (decoded, mixed and resampled on the GPU: ops.ingest); the session's clock -- start, duration,
        # endpointing, the window, the long-form cut -- counts frames of the format's own rate
        self.fmt = fmt
        if fmt is not None:
            rate = fmt.sample_rate

        # the quality gate and temperature fallback (VWA_ASR_FALLBACK, off by default; asr/fallback.py):
        # a FallbackPolicy, True (the policy of the VWA_ASR_TEMPERATURES / _LOGPROB_THRESHOLD /
        # _COMPRESSION_RATIO settings -- Whisper's published defaults, not tuned here on real speech),
        # False, or None (the VWA_ASR_FALLBACK setting).  Greedy final passes only: partials stay
        # greedy and unscored, and a beam final carries its beams' own scores
        if fallback is None:
            fallback = bool(knob("VWA_ASR_FALLBACK"))
        if fallback is True:
            from .fallback import FallbackPolicy, parse_temperatures

            fallback = FallbackPolicy(temperatures=parse_temperatures(knob("VWA_ASR_TEMPERATURES")),
                                      logprob_threshold=float(knob("VWA_ASR_LOGPROB_THRESHOLD")),
                                      compression_ratio_threshold=float(knob("VWA_ASR_COMPRESSION_RATIO")))
        self.fallback = fallback or None
        self._spec_policy = None
        if self.fallback is not None:
            from dataclasses import replace

            # a speculative final gets one attempt, at the schedule's first temperature
            self._spec_policy = replace(self.fallback, temperatures=self.fallback.temperatures[:1])
        # VWA_ASR_FALLBACK_REJECT: a final whose last attempt still fails is emitted empty
        self.fallback_reject = bool(knob("VWA_ASR_FALLBACK_REJECT")) if fallback_reject is None else bool(fallback_reject)

        # long utterances (VWA_ASR_LONGFORM, off by default): a full window is cut at the end of the
        # last segment a timestamp pass closes, if that lies at or after VWA_ASR_LONGFORM_MIN_S (a
        # policy default, not tuned on real speech: an earlier cut would refill the window at once)
        self.longform = bool(knob("VWA_ASR_LONGFORM")) if longform is None else bool(longform)
        self.longform_min = int(float(knob("VWA_ASR_LONGFORM_MIN_S")) * rate)

        # keyterm boosting (asr/keyterms.py): the session's terms -- text terms or a compiled set --
        # go with EVERY pass, partial, speculative and final (recognize(..., keyterms=...)), so the
        # hypotheses local agreement compares are decoded under one bias.  None: no pass carries
        # the keyword (recognizers with the old signature keep working)
        self.keyterms = None

        # beam search on the final passes (VWA_ASR_BEAM; 1: greedy) and the ranked alternatives a
        # final event carries (VWA_ASR_ALTERNATIVES, 1..beam): the final pass and the speculative
        # final pass are asked for recognize(..., beam=W); partials never are
        self.beam, self.n_alternatives = asr_beam_knobs(beam, alternatives)
        # n-best rescoring (VWA_RESCORE, off by default): only then does every alternative of a beam
        # final, the first included, carry "logprob", its sum log-probability -- what the voice service
        # weighs against the brain's language-model score.  Off: the events are what they always were
        self.rescore = bool(knob("VWA_RESCORE")) if rescore is None else bool(rescore)

        # language (VWA_ASR_LANGUAGE): a code, or "auto" -- then the passes of an utterance ask the
        # recognizer for "auto" until the first pass that commits tokens by local agreement; that
        # pass's language is locked for the rest of the utterance, so a forced prefix is never
        # decoded under another language token.  Set (by argument, or a knob other than "en"), the
        # passes carry language= and the events the language; unset, neither (recognizers with the
        # old signature keep working).
        lang = str(knob("VWA_ASR_LANGUAGE") if language is None else language).strip().lower()
        self.language: Optional[str] = lang if (language is not None or lang != "en") else None
        self._lang_lock: Optional[str] = None
        # no-speech gate (VWA_ASR_NO_SPEECH; 0: off): a pass whose no-speech probability exceeds it
        # commits nothing and shows nothing -- its final is an empty transcript
        self.no_speech_threshold = float(knob("VWA_ASR_NO_SPEECH") if no_speech_threshold is None
                                         else no_speech_threshold)

        # word timestamps + confidences on final results (VWA_ASR_WORDS): the final pass and the
        # speculative final pass -- whose hypothesis becomes the final -- are asked for them
        # (recognize(..., words=True)); partials never are
        self.words = bool(knob("VWA_ASR_WORDS")) if words is None else bool(words)

        self.rec = _as_recognizer(recognizer)
        self.rate = rate
        self.model_name = model_name
        self.partial_every = int(partial_every_s * rate)
        if endpoint_silence_s is None:
            endpoint_silence_s = knob("VWA_ENDPOINT_MS") / 1000.0
        if spec_silence_s is None:
            spec_silence_s = knob("VWA_SPEC_FINAL_MS") / 1000.0
        self.endpoint = int(endpoint_silence_s * rate)
        # speculative final pass after this much trailing silence (0: off; never later than the endpoint)
        self.spec_at = min(int(spec_silence_s * rate), self.endpoint) if spec_silence_s > 0 else 0
        self.thresh = knob("VWA_VAD_THRESHOLD") if energy_threshold is None else energy_threshold
        self.noise_mult = knob("VWA_VAD_NOISE_MULT") if noise_mult is None else noise_mult
        self.noise_floor = 0.0  # tracked non-speech frame RMS (0: not known)
        self._boot: Optional[List[float]] = []  # frame RMS of the stream's first 300 ms
        self._spec: Optional[Future] = None  # the speculative final pass in flight
        self.max_window = int(max_window_s * rate)
        self.min_speech = int(min_speech_s * rate)
        self.local_agreement = local_agreement
        self.frame = rate // 50  # 20 ms
        # the utterance buffer: preallocated to the window (+ one packet), appended in place --
        # no per-frame re-concatenation of the whole utterance
        # (with a wire format: one row of frame bytes per frame, so every index stays a frame count)
        self._frame_bytes = 2 if fmt is None else fmt.frame_bytes
        self._pcm = (np.zeros(self.max_window + 4 * rate, dtype=np.int16) if fmt is None
                     else np.zeros((self.max_window + 4 * rate, fmt.frame_bytes), dtype=np.uint8))
        self._n = 0
        self._carry = b""
        self.t_offset = 0.0          # stream time of buf[0]
        self.speech = 0              # speech samples in the utterance
        self.trailing_silence = 0
        self.since_partial = 0
        self.last_partial = ""
        self.committed: List[int] = []   # agreed token prefix of the current utterance
        self.prev_tokens: List[int] = []  # previous interim hypothesis
        self.stats: Dict[str, float] = {"partials": 0, "finals": 0, "asr_ms": 0.0, "passes": 0,
                                        "committed_tokens": 0, "spec_started": 0, "spec_used": 0,
                                        "spec_discarded": 0, "no_speech": 0, "boosted_passes": 0,
                                        "longform_cuts": 0, "longform_fallbacks": 0, "fallback_passes": 0,
                                        "fallback_retries": 0, "fallback_rejected": 0, "spec_rejected": 0}
        # on_speculative(text): called (from the recognizer's thread) when a speculative final pass
        # finishes while it still covers the utterance -- the voice server starts the brain on it
        # (voice/server.py: the brain's latency then overlaps the rest of the endpoint wait)
        self.on_speculative: Optional[Callable[[str], None]] = None
        # vad_events (Deepgram's live option of that name, off by default there too): push() also
        # returns {"type": "SpeechStarted"} when speech begins or resumes after a speculative final
        self.vad_events = False
        if keyterms:
            self.set_keyterms(keyterms)

    # ------------------------------------------------------------------ internals
    @property
    def buf(self):
        """The current utterance's samples (a view of the preallocated buffer); with a wire format,
        its frames as the WireAudio a recogniser takes."""
        if self.fmt is not None:
            return WireAudio(self._pcm[: self._n].reshape(-1), self.fmt)
        return self._pcm[: self._n]

    def _append(self, fr: np.ndarray) -> None:
        if self._n + len(fr) > len(self._pcm):  # (never with the window cut; a safety net)
            more = np.zeros((max(len(fr), len(self._pcm) // 2),) + self._pcm.shape[1:], dtype=self._pcm.dtype)
            self._pcm = np.concatenate([self._pcm, more])
        self._pcm[self._n : self._n + len(fr)] = fr
        self._n += len(fr)

    def _pass_kw(self, final: bool, spec: bool = False) -> Dict:
        """Keywords of a recognition pass: only those of the features that are on.  ``spec``: the
        speculative final pass -- under the quality gate it gets one scored attempt, no retries."""
        kw: Dict[str, Any] = {"words": True} if final and self.words else {}
        if final and self.beam > 1:
            kw["beam"] = self.beam
        elif final and self.fallback is not None:
            kw["fallback"] = self._spec_policy if spec else self.fallback
        if self.language is not None:
            kw["language"] = self._lang_lock or self.language
        if self.keyterms is not None:
            kw["keyterms"] = self.keyterms
            self.stats["boosted_passes"] += 1
        return kw

    def set_keyterms(self, keyterms) -> None:
        """Replace the session's keyterms (None or empty: none); in effect from the next pass.  A
        recognizer that compiles terms (``compile_keyterms``: EngineRecognizer, AsrBatcher) does so
        here, so a term it cannot take raises ValueError now and the old set stays."""
        if not keyterms:
            self.keyterms = None
            return
        comp = getattr(getattr(self, "rec", None), "compile_keyterms", None)
        self.keyterms = comp(keyterms) if comp is not None else keyterms

    def _gated(self, hyp: Hypothesis) -> bool:
        p = getattr(hyp, "no_speech_prob", None)
        return self.no_speech_threshold > 0.0 and p is not None and p > self.no_speech_threshold

    def _failed(self, hyp: Hypothesis) -> bool:
        """The quality gate rejects the pass's returned attempt."""
        sc = getattr(hyp, "score", None)
        return self.fallback is not None and sc is not None and not sc.get("passed", True)

    def _lang_kw(self, hyp: Hypothesis) -> Dict:
        lang = getattr(hyp, "language", None) if self.language is not None else None
        if lang is None:
            return {}
        return dict(language=lang, language_confidence=getattr(hyp, "language_confidence", None))

    def _run(self, final: bool = False) -> Hypothesis:
        t0 = time.perf_counter()
        kw = self._pass_kw(final)
        hyp = self.rec.recognize(self.buf, self.committed if self.local_agreement else (), **kw)
        self.stats["asr_ms"] += (time.perf_counter() - t0) * 1e3
        self.stats["passes"] += 1
        return hyp

    def _track_floor(self, rms: float) -> None:
        """Bootstrap the noise floor from the stream's first 300 ms (the mic-open moment) when that
        audio is stationary (frame RMS within 2x: hiss, hum -- not a speech onset) and quiet enough
        (mult x level <= 10 x the fixed threshold); afterwards the non-speech frames maintain it."""
        if self._boot is None or self.noise_mult <= 0.0:
            return
        self._boot.append(rms)
        if len(self._boot) < 15:
            return
        lo, hi = min(self._boot), max(self._boot)
        med = float(np.median(self._boot))
        if hi <= 2.0 * max(lo, 1e-6) and self.noise_mult * med <= 10.0 * self.thresh:
            self.noise_floor = max(self.noise_floor, med)
        self._boot = None

    def _floor_cap(self) -> float:
        """The highest noise floor the VAD tracks: the bootstrap's own ceiling (mult x floor <= 10 x
        the fixed threshold)."""
        return 10.0 * self.thresh / self.noise_mult if self.noise_mult > 0.0 else 0.0

    def _reset_utterance(self) -> None:
        self.t_offset += self._n / self.rate
        self._n = 0
        self.speech = self.trailing_silence = self.since_partial = 0
        self.last_partial = ""
        self.committed = []
        self.prev_tokens = []
        self._lang_lock = None
        self._drop_spec()

    def _drop_spec(self) -> None:
        if self._spec is not None:
            self.stats["spec_discarded"] += 1
            self._spec = None

    def _start_spec(self) -> None:
        """The final pass, started during the trailing silence (see module docstring)."""
        self.stats["spec_started"] += 1
        self._spec_t0 = time.perf_counter()
        fut = recognize_async(self.rec, self.buf.copy(), self.committed if self.local_agreement else (),
                              **self._pass_kw(True, spec=True))
        self._spec = fut
        if self.on_speculative is not None:
            fut.add_done_callback(self._spec_ready)

    def _spec_ready(self, fut: Future) -> None:
        if self._spec is not fut or fut.cancelled() or fut.exception() is not None:
            return  # (speech resumed meanwhile, or a failed pass: the endpoint runs the final itself)
        try:
            if self._gated(fut.result()) or self._failed(fut.result()):
                return  # (no speech in the window, or the quality gate rejects it: nothing to start the brain on)
            self.on_speculative(fut.result().text)
        except Exception:  # noqa: BLE001  (a listener failure must not break recognition)
            pass

    def _cut_sample(self) -> Optional[int]:
        """Long-form: the sample a full window is cut at, or None.  One boundary pass with
        timestamps (the session's language and keyterms; no prefix, words or beam); the cut is the
        end of the last segment it closes (asr/segments.py cut_index), when that lies at or after
        the minimum and inside the window."""
        t0 = time.perf_counter()
        kw = {k: v for k, v in self._pass_kw(False).items() if k in ("language", "keyterms")}
        hyp = self.rec.recognize(self.buf, (), timestamps=True, **kw)
        self.stats["asr_ms"] += (time.perf_counter() - t0) * 1e3
        self.stats["passes"] += 1
        tsb = getattr(self.rec, "ts_begin", None)
        if tsb is not None:
            c = cut_index(hyp.tokens, tsb)
            t = None if c is None else ts_time(hyp.tokens[c], tsb)
        else:  # (a recognizer that reports segments only)
            ends = [sg["end"] for sg in getattr(hyp, "segments", None) or [] if sg.get("end") is not None]
            t = ends[-1] if ends else None
        if t is None:
            return None
        cut = int(round(t * self.rate))
        return cut if max(self.longform_min, 1) <= cut <= self._n else None

    def _window_full(self) -> List[Dict]:
        """The 30 s window filled while the speaker is still talking."""
        cut = self._cut_sample() if self.longform and self.speech >= self.min_speech else None
        if cut is None:
            if self.longform:
                self.stats["longform_fallbacks"] += 1
            return self._final(use_spec=False)
        n, speech, silence, lock = self._n, self.speech, self.trailing_silence, self._lang_lock
        tail = self._pcm[cut:n].copy()
        # the normal final pass on the audio before the cut; the committed prefix was agreed on the
        # whole window and may reach past the cut, so this pass forces none
        self._n = cut
        self.committed = []
        out = self._final(use_spec=False, speech_final=False)  # (t_offset moves on by the cut; the rest is cleared)
        self._pcm[: len(tail)] = tail
        self._n = len(tail)
        # the utterance stays open: the endpoint, a flush or the next full window ends it
        self.speech = max(min(speech, len(tail)), self.min_speech)
        self.trailing_silence = min(silence, len(tail))
        self._lang_lock = lock
        self.stats["longform_cuts"] += 1
        return out

    def _final(self, use_spec: bool = True, speech_final: Optional[bool] = None) -> List[Dict]:
        out: List[Dict] = []
        if self.speech >= self.min_speech and self._n:
            hyp = None
            if use_spec and self._spec is not None:
                try:
                    hyp = self._spec.result()
                    self.stats["spec_used"] += 1
                    self.stats["asr_ms"] += (time.perf_counter() - self._spec_t0) * 1e3
                    self.stats["passes"] += 1
                    self._spec = None
                    if self._failed(hyp) and not self._gated(hyp):
                        # its one greedy attempt fails the quality gate: the real final pass runs, with the retries
                        self.stats["spec_rejected"] += 1
                        hyp = None
                except Exception:  # noqa: BLE001  (a failed background pass: run the final now)
                    self._drop_spec()
            if hyp is None:
                hyp = self._run(final=True)
            kw = {}
            text = hyp.text
            sc = getattr(hyp, "score", None) if self.fallback is not None else None
            if sc is not None:
                self.stats["fallback_passes"] += 1
                self.stats["fallback_retries"] += max(0, int(sc.get("attempts", 1)) - 1)
            if self._gated(hyp):
                # Deepgram emits empty finals for noise too; the voice server drops an empty transcript
                text, kw = "", dict(no_speech_prob=hyp.no_speech_prob)
                self.stats["no_speech"] += 1
            elif self.fallback_reject and self._failed(hyp):
                # every temperature failed the gate: an empty final, so a hallucinated command never reaches the brain
                text = ""
                self.stats["fallback_rejected"] += 1
            elif self.words:
                kw = dict(confidence=getattr(hyp, "confidence", 0.0),
                          words=shift_words(getattr(hyp, "words", None) or [], self.t_offset))
            if sc is not None and not self.words and text:
                kw["confidence"] = math.exp(sc["avg_logprob"])  # of the returned attempt
            if self.beam > 1 and not self._gated(hyp):
                if not self.words:
                    kw["confidence"] = getattr(hyp, "confidence", 0.0)  # exp(avg_logprob) of the best hypothesis
                alts = list(getattr(hyp, "alternatives", None) or [])[: self.n_alternatives - 1]
                if alts:
                    kw["alternatives"] = alts
                    lps = list(getattr(hyp, "beam_logprobs", None) or [])[: len(alts) + 1]
                    if self.rescore and len(lps) == len(alts) + 1:
                        kw["logprobs"] = lps
            if speech_final is not None:
                kw["speech_final"] = speech_final
            out.append(results_event(text, is_final=True, start=self.t_offset, duration=self._n / self.rate,
                                     model=self.model_name, **kw, **self._lang_kw(hyp)))
            self.stats["finals"] += 1
        self._reset_utterance()
        return out

    def _partial(self) -> List[Dict]:
        hyp = self._run()
        if self._gated(hyp):
            return []  # (not speech: no event, nothing committed)
        if self.local_agreement and hyp.tokens:
            # LocalAgreement-2: what two consecutive hypotheses agree on is stable
            n = common_prefix(self.prev_tokens, hyp.tokens)
            if n > len(self.committed):
                self.stats["committed_tokens"] += n - len(self.committed)
                self.committed = list(hyp.tokens[:n])
                if self.language == "auto" and self._lang_lock is None and getattr(hyp, "language", None):
                    self._lang_lock = hyp.language  # the utterance's language from here on
            self.prev_tokens = list(hyp.tokens)
        if hyp.text == self.last_partial:
            return []
        self.last_partial = hyp.text
        self.stats["partials"] += 1
        return [results_event(hyp.text, is_final=False, start=self.t_offset, duration=self._n / self.rate,
                              model=self.model_name, **self._lang_kw(hyp))]

    # ------------------------------------------------------------------ API
    def push(self, data: bytes) -> List[Dict]:
        data = self._carry + bytes(data)
        odd = len(data) % self._frame_bytes  # a packet that ends inside a frame: its bytes wait for the next
        if odd:
            self._carry, data = data[-odd:], data[:-odd]
        else:
            self._carry = b""
        if self.fmt is None:
            pcm = wire = np.frombuffer(data, dtype="<i2")
        else:
            # the VAD reads a mono int16 view decoded here; the window keeps the wire frames themselves
            wire = np.frombuffer(data, dtype=np.uint8).reshape(-1, self._frame_bytes)
            pcm = mono_int16(data, self.fmt)
        events: List[Dict] = []
        for i in range(0, len(pcm), self.frame):
            fr = pcm[i : i + self.frame]
            if len(fr) == 0:
                continue
            self._append(wire[i : i + self.frame])
            rms = float(np.sqrt(np.mean(fr.astype(np.float32) ** 2)))
            self._track_floor(rms)
            if rms >= max(self.thresh, self.noise_mult * self.noise_floor):
                if self.vad_events and (self.speech == 0 or self._spec is not None):
                    # Deepgram's VAD event (vad_events): speech begins -- a new utterance, or the
                    # speaker resumed after a speculative final (the voice server holds / drops
                    # what it started on the previous words: voice/server.py commit policy)
                    events.append({"type": "SpeechStarted", "channel": [0, 1],
                                   "timestamp": round(self.t_offset + self._n / self.rate, 3)})
                self.speech += len(fr)
                self.trailing_silence = 0
                self._drop_spec()  # speech resumed: the speculative final no longer covers the utterance
            else:
                self.trailing_silence += len(fr)
                # non-speech frames: the floor falls fast to quieter frames, rises slowly (0.3 % /
                # frame) and only between utterances (never from an utterance's own pauses), capped
                # at the bootstrap's ceiling -- steady soft speech or a TV in the background cannot
                # walk the threshold up until quiet speakers stop being detected
                if self.noise_floor > 0.0:
                    if rms < self.noise_floor:
                        self.noise_floor = 0.8 * self.noise_floor + 0.2 * rms
                    elif self.speech == 0:
                        self.noise_floor = min(rms, self.noise_floor * 1.003, self._floor_cap())
            if self.speech > 0:
                self.since_partial += len(fr)
            if self.speech >= self.min_speech and self.trailing_silence >= self.endpoint:
                events += self._final()
            elif self._n >= self.max_window:
                events += self._window_full() if self.longform else self._final(use_spec=False)
            elif (self.spec_at and self._spec is None and self.speech >= self.min_speech
                  and self.trailing_silence >= self.spec_at):
                self._start_spec()
            elif self.speech == 0 and self.trailing_silence >= self.endpoint:
                # leading silence: drop it, keep the stream clock
                self.t_offset += self._n / self.rate
                self._n = 0
                self.trailing_silence = 0
        if self.speech >= self.min_speech and self.since_partial >= self.partial_every:
            self.since_partial = 0
            events += self._partial()
        return events

    def flush(self) -> List[Dict]:
        return self._final()  # (a speculative pass in flight covers the utterance: speech since would have dropped it)

    def close(self) -> None:
        pass


# ---------------------------------------------------------------------------------- recognizers
def _words_knob(words: Optional[bool]) -> bool:
    from ..utils.env import knob

    return bool(knob("VWA_ASR_WORDS")) if words is None else bool(words)


def _hypothesis(eng, full: List[int], n_samples: int, al=None, sot: Optional[Dict] = None,
                beams: Optional[List[Dict]] = None, prefix: Sequence[int] = (),
                score: Optional[Dict] = None) -> Hypothesis:
    """The pass's hypothesis; with its alignment (a words pass) also the words, on the utterance's
    own clock, and the transcript confidence (exp of the mean log-probability of its text tokens);
    with its ``last_sot`` entry the language and the no-speech probability; with its ``last_beams``
    entry (a beam pass: ranked {tokens, sum_logprob, avg_logprob}, ``prefix`` the forced tokens
    before them) the alternatives after the first and the confidence exp(avg_logprob) of the best.
    In a pass with keyterms the beams are scored on the biased logits, so these confidences are
    those of the biased distribution; the words pass scores the model's own logits.  With its
    ``last_scores`` entry (a pass under the quality gate) the score and the confidence
    exp(avg_logprob) of the returned attempt."""
    text = eng.tok.decode(full).strip()
    hyp = Hypothesis(full, text)
    if score is not None:
        hyp.score, hyp.confidence = dict(score), math.exp(score["avg_logprob"])
    if beams:
        hyp.confidence = math.exp(beams[0]["avg_logprob"])
        hyp.alternatives = [dict(transcript=eng.tok.decode(list(prefix) + list(h["tokens"])).strip(),
                                 confidence=math.exp(h["avg_logprob"])) for h in beams[1:]]
        hyp.beam_logprobs = [float(h["sum_logprob"]) for h in beams]
    if al is not None:
        hyp.words, hyp.confidence = eng.words_of(al, duration=n_samples / 16000.0), _confidence(al.logprobs)
    if sot is not None:
        hyp.language, hyp.language_confidence = sot.get("language"), sot.get("language_confidence")
        hyp.no_speech_prob = sot.get("no_speech_prob")
    return hyp


def _ts_hypothesis(eng, toks: List[int], i: int) -> Hypothesis:
    """The hypothesis of a timestamp pass: every decoded token (the timestamp tokens among them),
    the text of the text tokens alone, and utterance i's segments of the engine's last call."""
    eot = eng.model.cfg.eot
    hyp = Hypothesis(list(toks), eng.tok.decode([t for t in toks if t < eot]).strip())
    segs = getattr(eng, "last_segments", None)
    hyp.segments = list(segs[i]) if segs and i < len(segs) and segs[i] else []
    sot = _sot_of(eng, i)
    if sot is not None:
        hyp.language, hyp.language_confidence = sot.get("language"), sot.get("language_confidence")
        hyp.no_speech_prob = sot.get("no_speech_prob")
    return hyp


def _ts_tokens(eng) -> int:
    """Tokens a timestamp pass may decode: half the decoder's context (Whisper's own sample length)."""
    return eng.model.cfg.n_text_ctx // 2


def _sot_of(eng, i: int) -> Optional[Dict]:
    """Utterance i's start-of-transcript report of the engine's last call (engines without: None)."""
    sots = getattr(eng, "last_sot", None)
    return sots[i] if sots and i < len(sots) else None


def _to_audio(eng, pcm):
    """A pass's window as the 16 kHz f32 tensor decode_many takes: int16 samples at 16 kHz, or the
    wire frames of a session with a format (any format: they differ only up to here)."""
    if isinstance(pcm, WireAudio):
        return eng.wire_to_audio(pcm.raw, pcm.fmt)
    return eng.pcm_to_audio(pcm)


def _compile_keyterms(eng, keyterms):
    """A pass's ``keyterms=`` as the engine takes it: a compiled set stays, text terms are compiled
    with the engine's tokenizer (cached by content), None or empty is None."""
    if not keyterms:
        return None
    from .keyterms import as_set

    return as_set(keyterms, eng.tok, eng.model.cfg.eot)


class EngineRecognizer:
    """Serial recognizer on an AsrEngine (one pass at a time, caller's thread)."""

    def __init__(self, asr_engine, *, max_tokens: int = 96, words: Optional[bool] = None):
        """words: serve passes that ask for word timestamps (None: the VWA_ASR_WORDS knob); off,
        such a pass gets the plain hypothesis."""
        self.eng = asr_engine
        self.max_tokens = max_tokens
        self.words = _words_knob(words)

    @property
    def ts_begin(self) -> int:
        """The id of ``<|0.00|>``: what a session reads a timestamp pass's tokens with."""
        return self.eng.model.cfg.no_timestamps + 1

    def compile_keyterms(self, keyterms):
        return _compile_keyterms(self.eng, keyterms)

    def recognize(self, pcm: np.ndarray, prefix: Sequence[int] = (), words: bool = False,
                  language: Optional[str] = None, beam: int = 1, keyterms=None,
                  timestamps: bool = False, fallback=None) -> Hypothesis:
        """fallback: the pass's FallbackPolicy (greedy passes; None: unscored) -- its hypothesis
        carries the returned attempt's score.
        language: this pass's language code or "auto" (None: the engine's default); beam: the
        pass's beam width (1: greedy) -- it then takes that many of the engine's session slots;
        keyterms: this pass's keyterms, text terms or a compiled set (None: not boosted);
        timestamps: decode with timestamp tokens, up to half the decoder's context whatever
        ``max_tokens`` is -- such a pass carries no prefix, words or beam, and its hypothesis the
        segments."""
        kw: Dict[str, Any] = {}
        if language is not None:
            kw["languages"] = [language]
        ks = _compile_keyterms(self.eng, keyterms)
        if ks is not None:
            kw["keyterms"] = [ks]
        if timestamps:
            toks = self.eng.decode_many([_to_audio(self.eng, pcm)], max_tokens=_ts_tokens(self.eng),
                                        timestamps=[True], **kw)[0]
            return _ts_hypothesis(self.eng, toks, 0)
        prefix = list(prefix)[: self.eng.max_prefix()]  # the prefix the decoder actually forces
        words = bool(words) and self.words
        if words:
            kw["words"] = True
        if beam > 1:
            kw["beam_size"] = int(beam)
        elif fallback is not None:
            kw["fallback"] = fallback
        toks = self.eng.decode_many([_to_audio(self.eng, pcm)], [prefix], max_tokens=self.max_tokens, **kw)[0]
        return _hypothesis(self.eng, prefix + toks, len(pcm), self.eng.last_alignments[0] if words else None,
                           _sot_of(self.eng, 0), self.eng.last_beams[0] if beam > 1 else None, prefix,
                           self.eng.last_scores[0] if "fallback" in kw else None)


class AsrBatcher:
    """Cross-session batching of recognition passes on one ASR engine (one GPU).

    ``recognize`` is called from the voice server's worker threads (one blocking call per session
    pass); the scheduler thread takes EVERY pass queued since its last batch -- up to the
    engine's free session slots -- and runs them as one ``decode_many`` batch.  While a batch is
    on the GPU the next one accumulates, so under load each GPU pass serves many sessions."""

    def __init__(self, asr_engine, *, max_tokens: int = 96, max_batch: Optional[int] = None,
                 tokens_per_s: Optional[float] = None, words: Optional[bool] = None):
        """tokens_per_s: fixed-work mode for benchmarks on random-init weights (which emit EOT at
        random): every pass decodes exactly round(audio seconds x tokens_per_s) transcript tokens
        in all (committed prefix included), as bench.py's ``exact_tokens``."""
        self.eng = asr_engine
        self.max_tokens = max_tokens
        self.tokens_per_s = tokens_per_s
        # serve passes that ask for word timestamps (None: the VWA_ASR_WORDS knob): a batch with
        # such a pass runs decode_many(words=True)
        self.words = _words_knob(words)
        self.max_batch = max_batch or len(asr_engine.free_slots)
        from .. import ops

        # what one call's distinct keyterm automata may hold together (the engine's tables)
        self.cap_states, self.cap_edges = ops.BOOST_CAP_STATES, ops.BOOST_CAP_EDGES
        self._q: List[tuple] = []
        self._cv = threading.Condition()
        self._stop = False
        self.stats = {"batches": 0, "passes": 0, "max_batch": 0, "gpu_ms": 0.0, "boosted_passes": 0}
        # shared-GPU deployment: the brain reads this to keep its persistent chained decode launch
        # off the GPU while recognition runs (utils/busy_flag.py; launch.py sets the path)
        from ..utils.busy_flag import from_env

        self.busy = from_env(create=True)
        dev = getattr(asr_engine.model, "device", None)
        self._cuda_index = None
        if dev is not None and getattr(dev, "type", "cpu") == "cuda":
            import torch

            self._cuda_index = dev.index if dev.index is not None else torch.cuda.current_device()
        self._thread = threading.Thread(target=self._loop, name="asr-batcher", daemon=True)
        self._thread.start()

    @property
    def ts_begin(self) -> int:
        """The id of ``<|0.00|>``: what a session reads a timestamp pass's tokens with."""
        return self.eng.model.cfg.no_timestamps + 1

    def compile_keyterms(self, keyterms):
        return _compile_keyterms(self.eng, keyterms)

    def recognize(self, pcm: np.ndarray, prefix: Sequence[int] = (), words: bool = False,
                  language: Optional[str] = None, beam: int = 1, keyterms=None,
                  timestamps: bool = False, fallback=None) -> Hypothesis:
        return self.recognize_async(pcm, prefix, words=words, language=language, beam=beam,
                                    keyterms=keyterms, timestamps=timestamps, fallback=fallback).result()

    def recognize_async(self, pcm: np.ndarray, prefix: Sequence[int] = (), words: bool = False,
                        language: Optional[str] = None, beam: int = 1, keyterms=None,
                        timestamps: bool = False, fallback=None) -> Future:
        """Queue a pass for the next GPU batch; the Future resolves to its Hypothesis.  language:
        this pass's code or "auto" (None: the engine's default); a batch may mix them.  beam: the
        pass's beam width (1: greedy).  A beam pass counts ``beam`` session slots; greedy passes and
        the beam passes of each width run as decode_many calls of their own, and a beam pass that
        does not fit a round's slots stays queued for the next (it is never failed for that).  A
        width the engine's slots can never hold is refused here.  keyterms: this pass's keyterms
        (text terms or a compiled set; None: not boosted); a batch may mix boosted and plain passes
        and different sets.  A round whose distinct sets would not fit the engine's keyterm tables is
        split -- the passes past the capacity stay queued; a set that alone exceeds it is refused here.
        timestamps: decode with timestamp tokens (up to half the decoder's context; the hypothesis
        carries the segments).  Such a pass is greedy and carries no prefix or words, and such
        passes are batched among themselves: a decode_many call of their own.
        fallback: the pass's FallbackPolicy (None: unscored).  Greedy passes only (a beam or timestamp
        pass drops it); the passes under one policy are batched among themselves, a decode_many call
        of their own (<= 64 rows), and their hypotheses carry the returned attempts' scores."""
        beam = int(beam)
        if timestamps:
            prefix, words, beam = (), False, 1
        if timestamps or beam > 1:
            fallback = None
        if beam < 1 or beam > min(8, self.max_batch):
            raise ValueError(f"beam = {beam} outside 1..{min(8, self.max_batch)} (the engine's session slots)")
        ks = _compile_keyterms(self.eng, keyterms)
        if ks is not None and (ks.n_states > self.cap_states or ks.n_edges > self.cap_edges):
            raise ValueError(f"keyterms: {ks.n_states} states / {ks.n_edges} edges exceed the engine's tables "
                             f"({self.cap_states} / {self.cap_edges})")
        fut: Future = Future()
        with self._cv:
            if self._stop:
                raise RuntimeError("ASR batcher stopped")
            # (cut to what the decoder forces: the hypothesis is built on the prefix it really used)
            own = pcm.copy() if isinstance(pcm, WireAudio) else np.array(pcm, dtype=np.int16, copy=True)
            self._q.append((own, list(prefix)[: self.eng.max_prefix()], fut,
                            bool(words) and self.words, language, beam, ks, bool(timestamps), fallback))
            self._cv.notify()
        return fut

    def _take(self) -> Dict[tuple, List[tuple]]:
        """(under the lock) The queued passes of this round by (beam width, timestamps, fallback
        policy), in queue order: of each kind as many as the slots hold (a pass of width W counts W; a beam call and a
        timestamp call hold <= 64 rows); the rest stays queued."""
        groups: Dict[tuple, List[tuple]] = {}
        used: Dict[tuple, int] = {}
        sets: Dict[tuple, Dict] = {}  # per kind: the distinct keyterm sets of its call, by key
        rest: List[tuple] = []
        for item in self._q:
            w, ks = item[5], item[6]
            g = (w, item[7], item[8])
            cap = self.max_batch if g == (1, False, None) else min(self.max_batch, 64)
            fits = used.get(g, 0) + w <= cap
            if fits and ks is not None and ks.key not in sets.setdefault(g, {}):
                # a set the call does not hold yet: the call's automata must still fit the tables
                mine = list(sets[g].values()) + [ks]
                fits = (sum(k.n_states for k in mine) <= self.cap_states
                        and sum(k.n_edges for k in mine) <= self.cap_edges)
                if fits:
                    sets[g][ks.key] = ks
            if fits:
                groups.setdefault(g, []).append(item)
                used[g] = used.get(g, 0) + w
            else:
                rest.append(item)
        self._q = rest
        return groups

    def rows_per_batch(self) -> float:
        return self.stats["passes"] / max(1, self.stats["batches"])

    def queue_depth(self) -> int:
        """Recognition passes waiting for the next GPU batch (the router's load signal)."""
        with self._cv:
            return len(self._q)

    def _loop(self) -> None:
        if self._cuda_index is not None:
            import torch

            torch.cuda.set_device(self._cuda_index)
        while True:
            with self._cv:
                while not self._q and not self._stop:
                    self._cv.wait()
                if self._stop and not self._q:
                    return
                groups = self._take()
            # greedy passes first, then the fallback passes (one call per policy), then the timestamp
            # passes, then one call per beam width
            for g in sorted(groups, key=lambda g: (g[0], g[1], g[2] is not None, repr(g[2]))):
                self._run_batch(groups[g], g[0], g[1], g[2])

    def _run_batch(self, batch: List[tuple], beam: int, timestamps: bool = False, fallback=None) -> None:
        """One decode_many call: the round's greedy passes (beam 1), its passes under one fallback
        policy, its timestamp passes, or its beam passes of one width."""
        t0 = time.perf_counter()
        if self.busy is not None:
            self.busy.enter()
        try:
            audios = [_to_audio(self.eng, item[0]) for item in batch]
            max_tokens = _ts_tokens(self.eng) if timestamps else self.max_tokens
            kw = dict(max_tokens=max_tokens)
            if self.tokens_per_s:
                kw = dict(exact_tokens=max(1, min(max_tokens, max(
                    int(round(len(item[0]) / 16000 * self.tokens_per_s)) - len(item[1]) for item in batch))))
            want = any(item[3] for item in batch)
            if want:
                kw["words"] = True
            if any(item[4] is not None for item in batch):
                kw["languages"] = [item[4] for item in batch]
            if beam > 1:
                kw["beam_size"] = beam
            if any(item[6] is not None for item in batch):
                kw["keyterms"] = [item[6] for item in batch]
                self.stats["boosted_passes"] += sum(item[6] is not None for item in batch)
            if timestamps:
                toks = self.eng.decode_many(audios, timestamps=[True] * len(batch), **kw)
                for i, (item, t) in enumerate(zip(batch, toks)):
                    item[2].set_result(_ts_hypothesis(self.eng, t, i))
            else:
                if fallback is not None:
                    kw["fallback"] = fallback
                    self.stats["fallback_passes"] = self.stats.get("fallback_passes", 0) + len(batch)
                toks = self.eng.decode_many(audios, [item[1] for item in batch], **kw)
                als = self.eng.last_alignments if want else [None] * len(batch)
                beams = self.eng.last_beams if beam > 1 else [None] * len(batch)
                scores = self.eng.last_scores if fallback is not None else [None] * len(batch)
                for i, (item, t, al) in enumerate(zip(batch, toks, als)):
                    p, pre, fut, w = item[:4]
                    fut.set_result(_hypothesis(self.eng, pre + t, len(p), al if w else None, _sot_of(self.eng, i),
                                               beams[i], pre, scores[i]))
        except BaseException as e:  # noqa: BLE001  (fail this batch's passes, keep serving)
            for item in batch:
                if not item[2].done():
                    item[2].set_exception(e)
        finally:
            if self.busy is not None:
                self.busy.leave()
        n = len(batch)
        self.stats["batches"] += 1
        self.stats["passes"] += n
        self.stats["max_batch"] = max(self.stats["max_batch"], n)
        self.stats["gpu_ms"] += (time.perf_counter() - t0) * 1e3

    def close(self) -> None:
        with self._cv:
            self._stop = True
            self._cv.notify_all()
        self._thread.join(timeout=30)


def make_asr_transcriber(asr_engine, *, tokens_per_s: Optional[float] = None) -> Callable[[np.ndarray], str]:
    """Adapter: AsrEngine -> transcribe(pcm int16) callable (fixed-work mode with tokens_per_s)."""

    def fn(pcm: np.ndarray) -> str:
        audio = asr_engine.pcm_to_audio(pcm)
        if tokens_per_s:
            n = max(1, int(round(len(pcm) / 16000 * tokens_per_s)))
            return asr_engine.transcribe(audio, exact_tokens=n)
        return asr_engine.transcribe(audio)

    return fn
