"""Beam search bookkeeping on host data (asr/engine.py decode_many with ``beam_size`` >= 2).

The device picks a group's 2 W best continuations (ops.beam_select); what becomes of them is
decided here, by the standard Whisper rule with patience 1.  Walking the candidates in order:

* an end-of-text candidate goes to the utterance's finished list while that list holds fewer than
  W hypotheses;
* any other candidate becomes the next live beam, until there are W -- the walk stops there.

A beam gives at most one end-of-text candidate, so the 2 W best always hold W others: 2 W is a
derived number, not a tuned one.  The utterance is done when it has W finished hypotheses or its live
beams reach the token limit (they then fill the list up to W).  Hypotheses are ranked by
``sum_logprob / n_tokens``, the end-of-text token counted in both where it was emitted.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Sequence, Tuple

NEG_INF = float("-inf")


@dataclass
class BeamState:
    """One utterance's beams.  ``tokens[w]`` / ``cum[w]``: live beam w's text tokens and running
    log-probability (``cum`` -inf: a dead row -- at the first step every beam but 0)."""

    width: int
    eot: int
    limit: int                      # text tokens a hypothesis may hold
    tokens: List[List[int]] = field(default_factory=list)
    cum: List[float] = field(default_factory=list)
    finished: List[Dict] = field(default_factory=list)
    done: bool = False

    def __post_init__(self):
        if not self.tokens:
            self.tokens = [[] for _ in range(self.width)]
            self.cum = [0.0] + [NEG_INF] * (self.width - 1)
        if self.limit <= 0:
            self.finished.append(hypothesis([], 0.0, 0))
            self.done = True


def hypothesis(tokens: Sequence[int], sum_logprob: float, n_scored: int) -> Dict:
    """``n_scored``: the tokens ``sum_logprob`` sums over (the text tokens, and the end-of-text token
    where the hypothesis ended with one)."""
    return dict(tokens=list(tokens), sum_logprob=float(sum_logprob),
                avg_logprob=float(sum_logprob) / n_scored if n_scored else 0.0)


def advance(state: BeamState, cands: Sequence[Tuple[float, int, int]]) -> Tuple[List[int], List[int]]:
    """One step of one utterance: ``cands`` are its (score, beam, token) candidates in the device's
    order ((-inf, -1, -1): none).  Updates ``state`` and returns (parents, tokens) of the W rows of
    the next decoder step: row w continues beam ``parents[w]`` with ``tokens[w]``.  A row without a
    candidate stays dead (its own parent, token 0, cum -inf)."""
    W = state.width
    assert not state.done
    live: List[Tuple[int, int, float]] = []  # (parent, token, score)
    for score, beam, tok in cands:
        if beam < 0 or tok < 0 or score == NEG_INF:
            break
        if tok == state.eot:
            if len(state.finished) < W:
                state.finished.append(hypothesis(state.tokens[beam], score, len(state.tokens[beam]) + 1))
            continue
        live.append((int(beam), int(tok), float(score)))
        if len(live) == W:
            break
    old = state.tokens
    parents = [p for p, _, _ in live] + list(range(len(live), W))
    tokens = [t for _, t, _ in live] + [0] * (W - len(live))
    state.tokens = [old[p] + [t] for p, t, _ in live] + [[] for _ in range(len(live), W)]
    state.cum = [s for _, _, s in live] + [NEG_INF] * (W - len(live))
    if len(state.finished) >= W or not live:
        state.done = True
    elif len(state.tokens[0]) >= state.limit:
        for w in range(len(live)):  # the token limit: live beams fill the list, best first
            if len(state.finished) < W:
                state.finished.append(hypothesis(state.tokens[w], state.cum[w], len(state.tokens[w])))
        state.done = True
    return parents, tokens


def ranked(state: BeamState) -> List[Dict]:
    """The utterance's hypotheses, best first (a stable sort: equal averages keep the order found).
    An utterance that ran out of candidates before finishing any hypothesis has one empty one."""
    hyps = sorted(state.finished, key=lambda h: -h["avg_logprob"])
    return hyps or [hypothesis([], 0.0, 0)]
