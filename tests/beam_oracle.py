"""Float64 oracle of the beam selection (csrc/beam/beam.h), working from the very f32 inputs the
kernel read, and the comparison rule the kernel and engine tests share."""
from types import SimpleNamespace

import numpy as np
import torch

EXTRA = 8  # ranks the oracle lists beyond K (the comparison needs K + 1)


def _np(t, dtype=None):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a if dtype is None else a.astype(dtype)


def allowed_bits(mask, rows: int, vocab: int) -> np.ndarray:
    """bool [rows, vocab] of a packed allow-mask [rows or 1, words] (None: all)."""
    if mask is None:
        return np.ones((rows, vocab), dtype=bool)
    m = _np(mask).reshape(-1, _np(mask).shape[-1]).view(np.uint32)
    ids = np.arange(vocab)
    bits = ((m[:, ids // 32] >> (ids % 32).astype(np.uint32)) & 1).astype(bool)
    return np.broadcast_to(bits, (rows, vocab)) if bits.shape[0] == 1 else bits[:rows]


def score_bound(lse, logprob, score, vocab: int):
    """|kernel f32 score - f64 score| <= 2^-16 + 2^-23 (|lse| + |logprob| + |score|).

    The kernel computes score = cum (+) (x (-) lse), lse = M (+) logf(S), S = the f32 sum of
    expf(x - m) over <= vocab allowed ids ((+), (-): rounded f32 operations, u = 2^-24).
    * S: every term carries expf's error (<= 2 u relative) and the rounding of its argument x - m,
      u |x - m| relative, which for a term of weight e^-|x - m| is at most 0.37 u of the largest
      term; the terms are added 32 to a lane, then over 6 shuffle levels, 4 waves and T =
      ceil(vocab / 8192) <= 128 tiles, each tile rescaled by one more expf(m_t - M): a chain of at
      most 32 + 6 + 2 + T additions of positive terms, <= (40 + T) u relative, plus ~5 u for the
      expf's: <= (45 + T) u <= 173 u relative in S, the same absolute in ln S.
    * logf(S): S lies in [1, vocab], ln S <= 13.9 for vocab <= 2^20, so one ulp of the result is
      at most 2^-20 = 16 u.
    * the three roundings of M (+) ., x (-) lse and cum (+) .: u |lse|, u |logprob|, u |score|.
    Together <= 189 u + u (|lse| + |logprob| + |score|); 2^-16 = 256 u and a factor 2 on the last
    term (the quantities are the oracle's, not the kernel's rounded ones) bound it with room.  The
    bound does not come from measured kernel output."""
    assert vocab <= 1 << 20
    return 2.0 ** -16 + 2.0 ** -23 * (np.abs(lse) + np.abs(logprob) + np.abs(score))


def select64(logits, cum, mask, vocab: int, W: int):
    """Per group the fully sorted candidate list in float64, to K + EXTRA entries (fewer when the
    group has fewer finite candidates): descending score, equal scores by ascending beam * vocab +
    token.  Returns a namespace: ``score`` / ``beam`` / ``tok`` / ``bound`` (lists of arrays, one per
    group), ``K``, ``W``, ``vocab`` and ``at(g, b, v)`` -> (the f64 score of any candidate, its bound)."""
    x = _np(logits, np.float64)[:, :vocab]
    c = _np(cum, np.float64)
    N = x.shape[0]
    assert N % W == 0
    G, K = N // W, 2 * W
    ok = allowed_bits(mask, N, vocab)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        xm = np.where(ok, x, -np.inf)
        m = xm.max(axis=1, keepdims=True)
        lse = m + np.log(np.exp(xm - m).sum(axis=1, keepdims=True))
        lp = xm - lse
        s = c[:N, None] + lp
    s = np.where(np.isfinite(s), s, -np.inf)
    out = SimpleNamespace(score=[], beam=[], tok=[], bound=[], K=K, W=W, vocab=vocab, G=G)
    for g in range(G):
        flat = s[g * W : (g + 1) * W].reshape(-1)
        n = min(K + EXTRA, int(np.isfinite(flat).sum()))
        # the n best by (score descending, flat index ascending): a stable sort of the negated scores
        order = np.argsort(-flat, kind="stable")[:n]
        b, v = order // vocab, order % vocab
        out.score.append(flat[order])
        out.beam.append(b)
        out.tok.append(v)
        out.bound.append(score_bound(lse[g * W + b, 0], lp[g * W + b, v], flat[order], vocab))

    def at(g, b, v):
        r = g * W + b
        return s[r, v], score_bound(lse[r, 0], lp[r, v], s[r, v], vocab)

    out.at = at
    return out


def near_ties(ref) -> int:
    """Neighbouring ranks among 1 .. K + 1 of any group whose oracle scores differ by less than twice
    the bound (the kernel tests choose inputs where this is 0, so no rank is excused there)."""
    n = 0
    for s, bd in zip(ref.score, ref.bound):
        top = min(len(s), ref.K + 1)
        for r in range(top - 1):
            n += bool(s[r] - s[r + 1] < 2 * max(bd[r], bd[r + 1]))
    return n


def check_select(got, ref, what: str = "") -> int:
    """got: (cand_score [G, >= K], cand_beam, cand_tok) of the written region; ref: select64's.
    Every returned score is within the bound of the oracle's score of that (beam, token); the
    returned (beam, token) sequence equals the oracle's, except that ranks whose neighbouring oracle
    scores differ by less than twice the bound are compared as a set; ranks past the group's
    candidates hold (-inf, -1, -1).  Returns the number of ranks that needed the exception."""
    gs, gb, gt = (_np(t) for t in got)
    K, excused = ref.K, 0
    worst = 0.0
    for g in range(ref.G):
        rs, rb, rt, bd = ref.score[g], ref.beam[g], ref.tok[g], ref.bound[g]
        n = min(K, len(rs))
        for r in range(n, K):
            assert gs[g, r] == -np.inf and gb[g, r] == -1 and gt[g, r] == -1, \
                f"{what}: group {g} rank {r} is ({gs[g, r]}, {gb[g, r]}, {gt[g, r]}), not the (-inf, -1, -1) tail"
        for r in range(n):
            b, v = int(gb[g, r]), int(gt[g, r])
            assert 0 <= b < ref.W and 0 <= v < ref.vocab, f"{what}: group {g} rank {r} is ({b}, {v})"
            s64, bound = ref.at(g, b, v)
            assert np.isfinite(gs[g, r]) and np.isfinite(s64), f"{what}: group {g} rank {r}: ({b}, {v}) is no candidate"
            err = abs(float(gs[g, r]) - s64)
            worst = max(worst, err / bound)
            assert err <= bound, f"{what}: group {g} rank {r} ({b}, {v}): score {gs[g, r]} vs {s64}, bound {bound}"
        # clusters of ranks joined by near-ties, over the listed ranks (K + 1 and beyond included)
        r = 0
        while r < n:
            e = r
            while e + 1 < len(rs) and rs[e] - rs[e + 1] < 2 * max(bd[e], bd[e + 1]):
                e += 1
            hi = min(e, n - 1)
            got_set = {(int(gb[g, i]), int(gt[g, i])) for i in range(r, hi + 1)}
            assert len(got_set) == hi + 1 - r, f"{what}: group {g} ranks {r}..{hi} repeat a candidate"
            if e == r:
                assert (int(gb[g, r]), int(gt[g, r])) == (int(rb[r]), int(rt[r])), \
                    f"{what}: group {g} rank {r}: ({gb[g, r]}, {gt[g, r]}) != oracle ({rb[r]}, {rt[r]})"
            else:
                ref_set = {(int(rb[i]), int(rt[i])) for i in range(r, e + 1)}
                open_end = e == len(rs) - 1 and len(rs) == K + EXTRA  # the cluster may go on past the list
                if e < n:  # wholly inside the returned ranks: the same set
                    assert got_set == ref_set, f"{what}: group {g} ranks {r}..{e}: {got_set} != oracle {ref_set}"
                elif not open_end:
                    assert got_set <= ref_set, f"{what}: group {g} ranks {r}..{hi}: {got_set} not within {ref_set}"
                excused += sum((int(gb[g, i]), int(gt[g, i])) != (int(rb[i]), int(rt[i])) for i in range(r, hi + 1))
            r = hi + 1
    print(f"MEASURED {what} beam_select score err/bound {worst:.4g}, ranks excused {excused}")
    return excused
