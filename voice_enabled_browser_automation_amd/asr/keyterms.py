"""Keyterm boosting: the host side (the device step is csrc/boost, ops.boost_step).

A caller names words the recogniser should prefer (Deepgram's ``keyterm``), each with a boost
``b > 0`` in logit units: the token's odds are multiplied by ``e^b``.  A term is expanded into token
sequences with the engine's tokenizer -- as written, with a leading space, lower-cased and
first-letter-capitalised, de-duplicated -- and the set of sequences is compiled into an
Aho-Corasick automaton over token ids.

With ``h`` a row's text-token history (forced prefix + decoded tokens, no SOT sequence):

    bias(h, v) = max over (sequence q with boost b, 0 <= k < len(q))
                 with q[:k] a suffix of h and q[k] == v   of b        (0 if there is none)

The automaton's state is the deepest trie node whose path is a suffix of ``h``; the trie nodes that
are suffixes of ``h`` are exactly that node's failure chain, so ``bias(h, .)`` is the maximum of the
chain's child weights, a child's weight being the largest boost of the sequences through it.  There
is no penalty for a partial match that is abandoned, and a term is matched only through the
tokenisations enumerated here.

Device tables of a set (local state ids, root 0; ``concat`` offsets several sets into one table):
``edge_off`` int32 [S + 1], ``edge_tok`` / ``edge_next`` int32 [E] and ``edge_bias`` f32 [E] with
tokens strictly ascending within a state, ``state_root`` int32 [S].  A root's list holds its
children.  A non-root state's list holds the *resolved* edges of its own children and of the
non-root nodes on its failure chain: ``next`` from the deepest of them, ``bias`` the maximum over
the whole chain, the root included.  delta(s, v): v in L(s), else in L(root), else the root.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_TERM_TOKENS = 16
MAX_TERMS = 100


class KeytermSet:
    """A compiled set of (token sequence, boost).  ``key`` identifies it: equal keys, one automaton."""

    def __init__(self, seqs: Sequence[Tuple[Sequence[int], float]]):
        best: Dict[Tuple[int, ...], float] = {}
        for q, b in seqs:
            q = tuple(int(t) for t in q)
            best[q] = max(best.get(q, 0.0), float(b))
        self.key: Tuple = tuple(sorted(best.items()))
        if not self.key:
            raise ValueError("a keyterm set needs at least one sequence")
        # trie: children[n] = {token: node}, weight[n] = the largest boost of the sequences through n
        children: List[Dict[int, int]] = [{}]
        weight: List[float] = [0.0]
        for q, b in self.key:
            n = 0
            for t in q:
                c = children[n].get(t)
                if c is None:
                    c = len(children)
                    children[n][t] = c
                    children.append({})
                    weight.append(0.0)
                weight[c] = max(weight[c], b)
                n = c
        S = len(children)
        # failure links, breadth first; resolved[n]: token -> (next, bias) over n and its failure
        # chain (for the root: its children) -- a node's chain is its failure node's chain after it
        fail = [0] * S
        resolved: List[Dict[int, Tuple[int, float]]] = [dict() for _ in range(S)]
        resolved[0] = {t: (c, weight[c]) for t, c in children[0].items()}
        order = list(children[0].values())
        i = 0
        while i < len(order):
            n = order[i]
            i += 1
            for t, c in children[n].items():
                f = fail[n]
                while f and t not in children[f]:
                    f = fail[f]
                fail[c] = children[f].get(t, 0)  # (n is not the root, so this is never c itself)
                order.append(c)
        for n in order:  # (breadth first: fail[n] is shallower, so already resolved)
            res = dict(resolved[fail[n]]) if fail[n] else {}
            for t, c in children[n].items():
                res[t] = (c, max(weight[c], res[t][1] if t in res else 0.0))
            # the root's weight joins the maximum of every token the list holds
            for t in res:
                rc = children[0].get(t)
                if rc is not None:
                    res[t] = (res[t][0], max(res[t][1], weight[rc]))
            resolved[n] = res
        self.n_states = S
        self._resolved = resolved
        off = [0]
        tok: List[int] = []
        nxt: List[int] = []
        bias: List[float] = []
        for n in range(S):
            for t in sorted(resolved[n]):
                tok.append(t)
                nxt.append(resolved[n][t][0])
                bias.append(resolved[n][t][1])
            off.append(len(tok))
        self.edge_off = np.asarray(off, dtype=np.int32)
        self.edge_tok = np.asarray(tok, dtype=np.int32)
        self.edge_next = np.asarray(nxt, dtype=np.int32)
        self.edge_bias = np.asarray(bias, dtype=np.float32)
        self.n_edges = len(tok)

    def step(self, s: int, tok: int) -> int:
        """delta(s, tok) in local state ids (root 0)."""
        e = self._resolved[s].get(tok)
        if e is None and s:
            e = self._resolved[0].get(tok)
        return e[0] if e is not None else 0

    def run(self, history: Sequence[int], s: int = 0) -> int:
        for t in history:
            s = self.step(s, int(t))
        return s

    def bias(self, s: int) -> Dict[int, float]:
        """token -> bias in state s (the two-list rule: the state's list, then the root's)."""
        out = {t: b for t, (_, b) in self._resolved[0].items()}
        out.update({t: b for t, (_, b) in self._resolved[s].items()})
        return out


def validate_boost(boost, what: str = "boost") -> float:
    try:
        b = float(boost)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {boost!r} is not a number") from None
    if not math.isfinite(b) or b <= 0.0:
        raise ValueError(f"{what}: {boost!r} must be finite and positive")
    return b


def check_sequence(q: Sequence[int], limit: int, term) -> Tuple[int, ...]:
    q = tuple(int(t) for t in q)
    if not 1 <= len(q) <= MAX_TERM_TOKENS:
        raise ValueError(f"keyterm {term!r}: {len(q)} tokens, a sequence must have 1..{MAX_TERM_TOKENS}")
    if any(t < 0 or t >= limit for t in q):
        raise ValueError(f"keyterm {term!r}: token ids {list(q)} must all be text ids below {limit}")
    return q


def variants(text: str) -> List[str]:
    """The spellings a term is matched through: as written, with a leading space, lower-cased,
    first-letter-capitalised (each with and without the space), de-duplicated in that order."""
    t = text.strip()
    out: List[str] = []
    for base in (t, t.lower(), t[:1].upper() + t[1:]):
        for v in (base, " " + base):
            if base and v not in out:
                out.append(v)
    return out


_CACHE: "OrderedDict[Tuple, KeytermSet]" = OrderedDict()
_CACHE_MAX = 256


def compile_sequences(seqs: Sequence[Tuple[Sequence[int], float]], *, limit: Optional[int] = None) -> KeytermSet:
    """The automaton of (token sequence, boost) pairs; ``limit``: ids must be below it (``cfg.eot``).
    Cached by the set's key: identical sets are one object."""
    checked = []
    for q, b in seqs:
        b = validate_boost(b, f"keyterm {list(q)!r} boost")
        checked.append((check_sequence(q, limit if limit is not None else 1 << 30, list(q)), b))
    best: Dict[Tuple[int, ...], float] = {}
    for q, b in checked:
        best[q] = max(best.get(q, 0.0), b)
    key = tuple(sorted(best.items()))
    hit = _CACHE.get(key)
    if hit is not None:
        _CACHE.move_to_end(key)
        return hit
    ks = KeytermSet(checked)
    _CACHE[key] = ks
    if len(_CACHE) > _CACHE_MAX:
        _CACHE.popitem(last=False)
    return ks


def normalize_terms(terms, default_boost: Optional[float] = None) -> List[Tuple[str, float]]:
    """[(text, boost)] from strings, (text, boost) pairs or {"term"/"text", "boost"} dicts; a term
    that names no boost takes ``default_boost`` (None: VWA_ASR_KEYTERM_BOOST)."""
    if default_boost is None:
        from ..utils.env import knob

        default_boost = knob("VWA_ASR_KEYTERM_BOOST")
    out: List[Tuple[str, float]] = []
    for t in terms:
        b = None
        if isinstance(t, dict):
            t, b = t.get("term", t.get("text")), t.get("boost")
        elif isinstance(t, (tuple, list)) and len(t) == 2:
            t, b = t
        if not isinstance(t, str) or not t.strip():
            raise ValueError(f"keyterm {t!r}: a term is a non-empty string")
        out.append((t.strip(), validate_boost(default_boost if b is None else b, f"keyterm {t!r} boost")))
    return out


def compile_keyterms(terms, tokenizer, eot: int, default_boost: Optional[float] = None) -> Optional[KeytermSet]:
    """The automaton of text terms under ``tokenizer`` (None for no terms).  Every variant of every
    term must tokenise to 1..16 text ids (below ``eot``): anything else is a ValueError naming the term."""
    seqs = []
    for text, b in normalize_terms(terms, default_boost):
        for v in variants(text):
            seqs.append((check_sequence(tokenizer.encode(v), eot, text), b))
    return compile_sequences(seqs, limit=eot) if seqs else None


def as_set(keyterms, tokenizer, eot: int) -> Optional[KeytermSet]:
    """A recogniser's ``keyterms=`` argument: a compiled set, text terms, or None / empty."""
    if keyterms is None or isinstance(keyterms, KeytermSet):
        return keyterms
    return compile_keyterms(keyterms, tokenizer, eot) if len(keyterms) else None


def concat(sets: Sequence[KeytermSet]):
    """The sets' tables concatenated: (bases, edge_off [S + 1], edge_tok, edge_next, edge_bias [E],
    state_root [S]) -- ``bases[i]`` is set i's root (its local state 0) in the joint table."""
    bases, off, tok, nxt, bias, root = [], [np.zeros(1, np.int32)], [], [], [], []
    S = E = 0
    for ks in sets:
        bases.append(S)
        off.append(ks.edge_off[1:] + E)
        tok.append(ks.edge_tok)
        nxt.append(ks.edge_next + S)
        bias.append(ks.edge_bias)
        root.append(np.full(ks.n_states, S, np.int32))
        S += ks.n_states
        E += ks.n_edges
    return (bases, np.concatenate(off).astype(np.int32), np.concatenate(tok).astype(np.int32),
            np.concatenate(nxt).astype(np.int32), np.concatenate(bias).astype(np.float32),
            np.concatenate(root).astype(np.int32))
