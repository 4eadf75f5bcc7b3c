"""Whisper's timestamp rules, transcribed literally over Python lists and f64 from the row's TOKEN
HISTORY (not from the packed state the kernel carries): the yardstick of csrc/tsrules and
ops/reference.py ts_rules_step.

``rules(x, hist, ...)`` returns the banned ids and the two quantities of rule 5; ``apply`` the row
after the bans; ``margin`` |T - M|, the distance from the one decision that depends on f32
arithmetic -- everything else of the rule is integer logic.
"""
import math

NEG_INF = float("-inf")


def allowed(mask_row, v: int) -> bool:
    """Bit v of the sampler's packed allow-bits (int32 words, little bit order)."""
    return bool((int(mask_row[v >> 5]) >> (v & 31)) & 1)


def lse(vals) -> float:
    vals = [v for v in vals if v > NEG_INF]
    if not vals:
        return NEG_INF
    m = max(vals)
    return m + math.log(math.fsum(math.exp(v - m) for v in vals))


def rules(x, hist, vocab: int, eot: int, ts_begin: int, max_initial: int, mask_row):
    """x: the row's logits as Python floats (>= vocab of them); hist: every token sampled so far.
    Returns (banned ids, T, M)."""
    banned = set()

    def ban(lo, hi):
        banned.update(range(max(lo, 0), min(hi, vocab)))

    n = min(len(hist), 2)
    last = hist[-1] if len(hist) >= 1 else -1
    prev = hist[-2] if len(hist) >= 2 else -1
    last_ts = -1
    for t in hist:
        if t >= ts_begin:
            last_ts = t - ts_begin
    # 1
    ban(ts_begin - 1, ts_begin)
    # 2
    last_was = n >= 1 and last >= ts_begin
    pen_was = n < 2 or prev >= ts_begin
    if last_was and pen_was:
        ban(ts_begin, vocab)
    if last_was and not pen_was:
        ban(0, eot)
    # 3
    if last_ts >= 0:
        lim = last_ts if (last_was and not pen_was) else last_ts + 1
        ban(ts_begin, ts_begin + lim)
    # 4
    if n == 0:
        ban(0, ts_begin)
        if max_initial >= 0:
            ban(ts_begin + max_initial + 1, vocab)
    # 5
    live = [v for v in range(vocab) if v not in banned and allowed(mask_row, v)]
    T = lse(float(x[v]) for v in live if v >= ts_begin)
    M = max((float(x[v]) for v in live if v < ts_begin), default=NEG_INF)
    if T > M:
        ban(0, ts_begin)
    return banned, T, M


def apply(x, hist, vocab, eot, ts_begin, max_initial, mask_row):
    """The row after the rules: a new list, -inf at the banned ids, everything else the same object."""
    banned, _, _ = rules(x, hist, vocab, eot, ts_begin, max_initial, mask_row)
    return [NEG_INF if v in banned else x[v] for v in range(vocab)] + list(x[vocab:])


def margin(x, hist, vocab, eot, ts_begin, max_initial, mask_row) -> float:
    """|T - M| in f64; inf when either side is empty (the decision then rests on no arithmetic)."""
    _, T, M = rules(x, hist, vocab, eot, ts_begin, max_initial, mask_row)
    if T == NEG_INF or M == NEG_INF:
        return float("inf")
    return abs(T - M)


def other_outcome(x, hist, vocab, eot, ts_begin, max_initial, mask_row):
    """The row had rule 5 decided the other way (for rows built at T - M ~ 0)."""
    banned, T, M = rules(x, hist, vocab, eot, ts_begin, max_initial, mask_row)
    if T > M:  # undo rule 5's ban: what rules 1-4 alone ban
        b14, _, _ = rules([NEG_INF if v >= ts_begin else x[v] for v in range(vocab)], hist, vocab, eot, ts_begin,
                          max_initial, mask_row)
        banned = b14
    else:
        banned = banned | set(range(0, ts_begin))
    return [NEG_INF if v in banned else x[v] for v in range(vocab)] + list(x[vocab:])


def state_of(hist, ts_begin: int):
    """(n, last, prev, last_ts) after ``hist``."""
    last_ts = -1
    for t in hist:
        if t >= ts_begin:
            last_ts = t - ts_begin
    return [min(len(hist), 2), hist[-1] if hist else -1, hist[-2] if len(hist) >= 2 else -1, last_ts]
