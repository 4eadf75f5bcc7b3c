"""Word timestamps and confidences from a token alignment (pure Python).

``AsrEngine.decode_many(words=True)`` aligns the transcript's tokens to 20 ms encoder frames
(cross-attention of the alignment heads -> DTW, csrc/align) and scores every token under the
distribution the sampler drew from.  This module turns one utterance's ``Alignment`` into the
Deepgram ``words`` list: ``{"word", "punctuated_word", "start", "end", "confidence"}``.
"""
from __future__ import annotations

import math
import string
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

FRAME_S = 0.02  # one encoder frame: 320 samples at 16 kHz

_EDGE = string.punctuation + "¿¡«»“”‘’…—–"


@dataclass
class Alignment:
    """One utterance: text token ids (forced prefix included), per token the first / last frame
    of its stretch of the DTW path and its log-probability, and the frames the audio covers."""

    tokens: List[int] = field(default_factory=list)
    first_frame: List[int] = field(default_factory=list)
    last_frame: List[int] = field(default_factory=list)
    logprobs: List[float] = field(default_factory=list)
    n_keys: int = 0
    cost: Any = None  # the device's cost matrix [tokens, n_keys] (AsrEngine.keep_costs; tests)


def confidence(logprobs: Sequence[float]) -> float:
    """exp(mean token log-probability), rounded to 4 places (0.0 for no tokens)."""
    if not logprobs:
        return 0.0
    return round(min(1.0, math.exp(sum(logprobs) / len(logprobs))), 4)


def _units(tokens: Sequence[int], token_bytes: Callable[[int], bytes]) -> List[Tuple[str, int, int]]:
    """Merge tokens until they decode to valid UTF-8: (text, first token index, last token index).
    Bytes that never complete (a transcript cut inside a character) decode with replacement."""
    out: List[Tuple[str, int, int]] = []
    buf, start = b"", 0
    for i, t in enumerate(tokens):
        if not buf:
            start = i
        buf += token_bytes(t)
        try:
            text = buf.decode("utf-8")
        except UnicodeDecodeError:
            continue
        out.append((text, start, i))
        buf = b""
    if buf:
        out.append((buf.decode("utf-8", errors="replace"), start, len(tokens) - 1))
    return out


def group_words(al: Alignment, token_bytes: Callable[[int], bytes], *, t_offset: float = 0.0,
                duration: Optional[float] = None) -> List[Dict]:
    """The utterance's words.  A word starts at unit 0 and at every unit whose text begins with a
    space; ``start`` = t_offset + 0.02 * first frame of its first token, ``end`` = t_offset + 0.02 *
    (last frame of its last token + 1), both clipped to the utterance (``duration`` seconds from
    t_offset, when given); ``confidence`` = exp(mean log-probability of its tokens)."""
    groups: List[List[Tuple[str, int, int]]] = []
    for u in _units(al.tokens, token_bytes):
        if not groups or u[0].startswith(" "):
            groups.append([])
        groups[-1].append(u)
    words: List[Dict] = []
    for g in groups:
        text = "".join(u[0] for u in g).strip()
        if not text:
            continue
        i0, i1 = g[0][1], g[-1][2]
        start = FRAME_S * al.first_frame[i0]
        end = FRAME_S * (al.last_frame[i1] + 1)
        if duration is not None:
            end = min(end, duration)
            start = min(start, end)
        words.append({
            "word": text.strip(_EDGE).lower() or text.lower(),
            "punctuated_word": text,
            "start": round(t_offset + start, 3),
            "end": round(t_offset + end, 3),
            "confidence": confidence(al.logprobs[i0 : i1 + 1]),
        })
    return words


def shift_words(words: Sequence[Dict], t_offset: float) -> List[Dict]:
    """The same words on a stream clock that started t_offset seconds before the utterance."""
    return [{**w, "start": round(w["start"] + t_offset, 3), "end": round(w["end"] + t_offset, 3)} for w in words]
