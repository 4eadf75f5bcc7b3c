"""References for keyterm boosting (asr/keyterms.py, csrc/boost), written from the contract alone.

* ``bias_brute``: bias(h, v) straight from the definition -- suffix tests on Python lists, no
  automaton, no trie.
* ``table_step``: one launch of the step on host copies of the device tables, following delta and
  the two-list apply rule as the header states them (its own code: not ops.reference).

Every comparison made with these is exact: states and tokens as integers, logits bit for bit (a
boosted id gets ONE f32 add, so ``x + f32(b)`` in torch is the expected bit pattern)."""
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

SENTINEL = -7.25  # what the cells a launch must not touch are filled with


def bias_brute(seqs: Sequence[Tuple[Sequence[int], float]], h: Sequence[int]) -> Dict[int, float]:
    """{v: bias(h, v)} for the ids with a non-zero bias.  ``seqs``: (token sequence q, boost b)."""
    h = list(h)
    out: Dict[int, float] = {}
    for q, b in seqs:
        q = list(q)
        for k in range(len(q)):
            if k == 0 or (k <= len(h) and h[len(h) - k :] == q[:k]):
                out[q[k]] = max(out.get(q[k], 0.0), float(b))
    return out


def state_brute(seqs: Sequence[Tuple[Sequence[int], float]], h: Sequence[int]) -> Tuple[int, ...]:
    """The automaton state as the contract names it: the longest prefix of any sequence that is a
    suffix of h (a tuple of ids; () is the root)."""
    h = list(h)
    best: Tuple[int, ...] = ()
    for q, _ in seqs:
        for k in range(1, len(q) + 1):
            if k <= len(h) and h[len(h) - k :] == list(q[:k]) and k > len(best):
                best = tuple(q[:k])
    return best


def boosted(row: torch.Tensor, bias: Dict[int, float], vocab: int) -> torch.Tensor:
    """``row`` (f32) with one f32 add per boosted id below ``vocab``."""
    out = row.clone()
    for v, b in bias.items():
        if 0 <= v < vocab:
            out[v] = out[v] + torch.tensor(b, dtype=torch.float32)
    return out


def path_states(ks, seqs) -> Dict[Tuple[int, ...], int]:
    """{trie path: local state} of a compiled set: the state reached from the root along each
    prefix of each sequence.  Distinct paths must be distinct states, and there are no others."""
    out: Dict[Tuple[int, ...], int] = {(): 0}
    for q, _ in seqs:
        for k in range(1, len(q) + 1):
            out[tuple(q[:k])] = ks.run(q[:k])
    assert len(set(out.values())) == len(out) == ks.n_states, "paths and states are not one to one"
    return out


def table_step(tables, logits: torch.Tensor, vocab: int, roots, state_in, tokens=None, parents=None, W: int = 1):
    """(logits after, state_out) of one launch over rows = len(roots); ``tables`` = (edge_off,
    edge_tok, edge_next, edge_bias, state_root) as numpy arrays; inputs are not modified."""
    off, tok, nxt, bias, root_of = (np.asarray(t) for t in tables)
    S, E = len(root_of), len(tok)
    rows = len(roots)
    x = logits.clone()
    out = [int(s) for s in state_in[:rows]]

    def lst(s):
        lo, hi = int(off[s]), int(off[s + 1])
        return list(range(lo, hi)) if 0 <= lo <= hi <= E else []

    def lookup(s, v):
        for e in lst(s):
            if int(tok[e]) == v:
                return e
        return None

    for r in range(rows):
        root = int(roots[r])
        if root < 0 or root >= S or int(root_of[root]) != root:
            out[r] = int(state_in[r])
            continue
        s = root
        src = r
        if parents is not None:
            p = int(parents[r])
            src = (r // W) * W + p if 0 <= p < W else None
        if src is not None and src < rows:
            s = int(state_in[src])
            if s < 0 or s >= S or int(root_of[s]) != root:
                s = root
        if tokens is not None:
            t = int(tokens[r])
            if t < 0:
                out[r] = s
                continue
            e = lookup(s, t)
            if e is None and s != root:
                e = lookup(root, t)
            n = int(nxt[e]) if e is not None else root
            s = n if 0 <= n < S and int(root_of[n]) == root else root
        out[r] = s
        own = {int(tok[e]) for e in lst(s)}
        for e in lst(s):
            if 0 <= int(tok[e]) < vocab:
                x[r, int(tok[e])] = x[r, int(tok[e])] + torch.tensor(float(bias[e]), dtype=torch.float32)
        if s != root:
            for e in lst(root):
                if 0 <= int(tok[e]) < vocab and int(tok[e]) not in own:
                    x[r, int(tok[e])] = x[r, int(tok[e])] + torch.tensor(float(bias[e]), dtype=torch.float32)
    return x, out


def greedy_ref(row: torch.Tensor, eot: int, allow_eot: bool) -> int:
    """The sampler's greedy choice on a kept logits row: the largest allowed logit, the lowest id
    among equals (text ids below ``eot``, and ``eot`` itself when allowed)."""
    n = eot + 1 if allow_eot else eot
    return int(torch.argmax(row[:n].double()))


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
