"""Segments of a transcript decoded with timestamp tokens (decode_many(timestamps=...)).

A timestamp token ``ts_begin + i`` stands for ``i * 0.02`` s from the start of the window.  Whisper
writes a segment as ``<|t0|> text ... <|t1|>``: the rules (csrc/tsrules/tsrules.h) make timestamps
come in pairs except the last, never decrease, and close a segment only after text.  Pure Python:
the streaming session cuts a full window at the last closed segment's end (``cut_index``).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

FRAME_S = 0.02  # one timestamp step


def ts_time(token: int, ts_begin: int) -> float:
    return round((token - ts_begin) * FRAME_S, 2)


def segments(tokens: Sequence[int], ts_begin: int, eot: int, tok=None) -> List[Dict]:
    """``[{start, end, tokens, text}]``: the text between an opening and a closing timestamp
    (``start`` None: the text had no opening timestamp); a trailing run the transcript did not
    close has ``end`` None.  Tokens from ``eot`` up that are no timestamps are dropped; ``tok``:
    the tokenizer ``text`` is decoded with (None: text stays None)."""
    out: List[Dict] = []
    start: Optional[float] = None
    cur: List[int] = []

    def close(end: Optional[float]) -> None:
        out.append(dict(start=start, end=end, tokens=list(cur), text=tok.decode(cur) if tok is not None else None))

    for t in tokens:
        if t >= ts_begin:
            if cur:  # a closing timestamp
                close(ts_time(t, ts_begin))
                cur = []
                start = None
            else:  # an opening one (of two in a row, the later counts)
                start = ts_time(t, ts_begin)
        elif t < eot:
            cur.append(t)
    if cur:
        close(None)
    return out


def cut_index(tokens: Sequence[int], ts_begin: int) -> Optional[int]:
    """Index in ``tokens`` of the last timestamp token that closes a segment -- one directly
    preceded by a text token -- or None."""
    for i in range(len(tokens) - 1, 0, -1):
        if tokens[i] >= ts_begin and tokens[i - 1] < ts_begin:
            return i
    return None
