"""Whisper's quality gate and temperature fallback, the host's half (no torch).

A decode is rejected when its average token log-probability is below ``logprob_threshold`` or when
its text compresses better than ``compression_ratio_threshold`` under zlib (a transcript that
loops); a rejected decode is tried again at the next temperature of the schedule.  These are the
rule and the defaults of Whisper's published ``transcribe()``; the log-probabilities come from the
device (ops.score_step), and the engine's ``decode_many(fallback=...)`` runs ``run`` below with a
decoder that keeps the encoder's output."""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

MAX_TEMPERATURES = 8
DEFAULT_TEMPERATURES = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)


def compression_ratio(text: str) -> float:
    """len(utf8) / len(zlib.compress(utf8)): Whisper's definition."""
    raw = text.encode("utf-8")
    return len(raw) / len(zlib.compress(raw))


def avg_logprob(sum_logprob: float, n_text_tokens: int) -> float:
    """Whisper's average: the sum (which holds the EOT's log-probability) over the text tokens + 1."""
    return float(sum_logprob) / (int(n_text_tokens) + 1)


@dataclass(frozen=True)
class FallbackPolicy:
    """temperatures: the schedule, non-decreasing, in [0, 2], at most 8 (0: greedy);
    logprob_threshold / compression_ratio_threshold: None disables that test."""

    temperatures: Tuple[float, ...] = DEFAULT_TEMPERATURES
    logprob_threshold: Optional[float] = -1.0
    compression_ratio_threshold: Optional[float] = 2.4

    def __post_init__(self):
        try:
            ts = tuple(float(t) for t in self.temperatures)
        except (TypeError, ValueError) as e:
            raise ValueError(f"temperatures: {self.temperatures!r} is not a sequence of numbers") from e
        if not 1 <= len(ts) <= MAX_TEMPERATURES:
            raise ValueError(f"temperatures: {len(ts)} entries outside [1, {MAX_TEMPERATURES}]")
        if any(not 0.0 <= t <= 2.0 for t in ts):  # (a NaN fails too)
            raise ValueError(f"temperatures: {ts} not all in [0, 2]")
        if any(b < a for a, b in zip(ts, ts[1:])):
            raise ValueError(f"temperatures: {ts} is not non-decreasing")
        object.__setattr__(self, "temperatures", ts)
        for name in ("logprob_threshold", "compression_ratio_threshold"):
            v = getattr(self, name)
            if v is not None:
                v = float(v)
                if v != v:
                    raise ValueError(f"{name} is NaN")
                object.__setattr__(self, name, v)
        if self.logprob_threshold is not None and self.logprob_threshold > 0.0:
            raise ValueError(f"logprob_threshold = {self.logprob_threshold} above 0: no log-probability passes")
        if self.compression_ratio_threshold is not None and self.compression_ratio_threshold <= 0.0:
            raise ValueError(f"compression_ratio_threshold = {self.compression_ratio_threshold} not above 0")


def parse_temperatures(spec) -> Tuple[float, ...]:
    """"0,0.2,0.4" (the VWA_ASR_TEMPERATURES setting) or a sequence -> the schedule."""
    if isinstance(spec, str):
        parts = [p.strip() for p in spec.split(",") if p.strip()]
        try:
            return tuple(float(p) for p in parts)
        except ValueError as e:
            raise ValueError(f"temperatures: {spec!r} is not a comma-separated list of numbers") from e
    return tuple(float(t) for t in spec)


def needs_fallback(avg_lp: float, text: str, policy: FallbackPolicy) -> Tuple[bool, Optional[str]]:
    """(rejected, which test failed: "compression_ratio" | "logprob" | None).  The compression test
    comes first, as in Whisper."""
    if policy.compression_ratio_threshold is not None and text \
            and compression_ratio(text) > policy.compression_ratio_threshold:
        return True, "compression_ratio"
    if policy.logprob_threshold is not None and not avg_lp >= policy.logprob_threshold:  # (NaN: rejected)
        return True, "logprob"
    return False, None


def score_entry(sum_logprob: float, n_text_tokens: int, temperature: float, attempts: int,
                text: Optional[str] = None, policy: Optional[FallbackPolicy] = None) -> Dict:
    """One utterance's ``last_scores`` entry; without a policy every decode passes."""
    avg = avg_logprob(sum_logprob, n_text_tokens)
    bad, why = needs_fallback(avg, text or "", policy) if policy is not None else (False, None)
    return dict(sum_logprob=float(sum_logprob), tokens=int(n_text_tokens), avg_logprob=avg,
                temperature=float(temperature), attempts=int(attempts), passed=not bad, failed_on=why)


def run(attempt: Callable[[List[int], float], Sequence[Tuple[float, int, str]]], n: int, policy: FallbackPolicy,
        gated: Optional[Callable[[int], bool]] = None) -> List[Dict]:
    """The retry loop over ``n`` utterances.  ``attempt(utts, temperature)`` decodes the utterances
    ``utts`` (ascending) at that temperature and returns (sum_logprob, n_text_tokens, text) for
    each; it is first called with all of them at the schedule's first temperature, then with those
    ``needs_fallback`` rejects at the next one, until none is left or the schedule ends -- the last
    attempt then stands with ``passed`` false.  ``gated(i)`` (asked after the first attempt): true
    for an utterance the no-speech gate rejects, which is not retried."""
    entries: List[Optional[Dict]] = [None] * n
    todo = list(range(n))
    for k, T in enumerate(policy.temperatures):
        if not todo:
            break
        res = attempt(list(todo), T)
        assert len(res) == len(todo)
        for i, (s, cnt, text) in zip(todo, res):
            entries[i] = score_entry(s, cnt, T, k + 1, text, policy)
        todo = [i for i in todo if not entries[i]["passed"] and not (gated is not None and gated(i))]
    return entries  # type: ignore[return-value]
