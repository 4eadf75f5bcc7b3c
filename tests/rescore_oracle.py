"""An f64 numpy oracle of the per-sequence log-probabilities (csrc/rescore/rescore.h), the error
bounds the f32 kernel is held to, and the cases the kernel tests share.

Per row the kernel computes A, the log-sum-exp of every column below V, and -- for target -1 -- Ls,
the same over the end set's columns, each with its own running maximum, in the sweep of
csrc/turn/set_logprob.hip: float4 loads over 512 lanes, issued four at a time but used in the sweep's
order, a scalar head and tail; six wave shuffles; eight LDS values added left to right.  That is the
reduction shape tests/turn_oracle.py derives its bound from, so with u = 2^-24 and
k = 4 ceil(V / 2048) + 6 terms per lane:

* a depth of k + 14 additions, u each;
* a term's exponential good to 4 u, as is each of the at most k rescales it rides through and the
  one scaling to the workgroup's maximum: 5 u (k + 2) with the multiplications' own roundings;
* the exponentials' arguments rounded to f32, weighed by the terms' shares: at most u ln V, twice;
so a sum is good to u (6 k + 2 ln V + 24) relative, which the logarithm makes an absolute error of L;
logf adds 4 u (ln V + 1) and the addition max + ln sum adds u |L|:

    lse_bound(V, L) = u (6 k + 2 ln V + 24) + u (4 (ln V + 1) + |L|)

A set target is the difference of two such values, Ls = A + lp and A, and the subtraction rounds
once more (the clamp at 0 only moves a value towards the true one, which is <= 0):

    set_bound(V, A, lp) = lse_bound(V, A + lp) + lse_bound(V, A) + u |lp|

An id target is x[t] - A: x[t] is an f32 read exactly, so only A's error and the subtraction's
rounding remain:

    id_bound(V, A, lp) = lse_bound(V, A) + u |lp|

Nothing here is tuned.  The running sums are not bounded but reproduced: acc_out must equal, bit
for bit, the np.float32 additions of the kernel's own lp values onto acc_in in row order."""
import numpy as np

U = 2.0 ** -24
NINF = -np.inf


def allowed(set_row: np.ndarray, vocab: int) -> np.ndarray:
    ids = np.arange(vocab)
    return ((set_row.reshape(-1).view(np.uint32)[ids >> 5] >> (ids & 31).astype(np.uint32)) & 1).astype(bool)


def pack(bits: np.ndarray, words: int, fill=None) -> np.ndarray:
    """bits -> int32 words; the bits past len(bits) are zero, or random under a generator ``fill``
    (the kernel must not count them)."""
    b = np.zeros(words * 32, dtype=np.uint8)
    if fill is not None:
        b[:] = fill.random(words * 32) < 0.5
    b[: len(bits)] = bits
    return np.packbits(b, bitorder="little").view(np.uint32).view(np.int32).copy()


def _lse(v: np.ndarray) -> float:
    if not v.size:
        return NINF
    mx = v.max()
    return float(mx + np.log(np.exp(v - mx).sum()))


def row_reference(logits: np.ndarray, vocab: int, target: np.ndarray, end_set: np.ndarray):
    """(lp f64 [rows], A f64 [rows]) of f32 logits [>= rows, >= vocab], int32 target [rows] and the
    packed end set: the per-row rule of the contract."""
    rows = len(target)
    on = allowed(end_set, vocab)
    lp, A = np.full(rows, NINF), np.full(rows, NINF)
    for r in range(rows):
        t = int(target[r])
        if not -1 <= t < vocab:
            continue
        x = logits[r, :vocab].astype(np.float64)
        live = x > NINF  # (False for a NaN)
        A[r] = _lse(x[live])
        if not np.isfinite(A[r]):
            continue
        if t == -1:
            ls = _lse(x[live & on])
            if np.isfinite(ls):
                lp[r] = min(ls - A[r], 0.0)
        elif live[t]:
            lp[r] = min(x[t] - A[r], 0.0)
    return lp, A


def seq_sum(lp: np.ndarray, seq: np.ndarray, n_seq: int, acc_in) -> np.ndarray:
    """The running sums exactly as the contract orders them: np.float32 additions in row order."""
    acc = np.zeros(n_seq, dtype=np.float32) if acc_in is None else np.asarray(acc_in, dtype=np.float32).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(len(lp)):
            s = int(seq[r])
            if 0 <= s < n_seq:
                acc[s] = np.float32(acc[s] + np.float32(lp[r]))
    return acc


def lse_bound(vocab: int, L: float) -> float:
    k = 4 * -(-vocab // 2048) + 6
    lnv = np.log(vocab) if vocab > 1 else 0.0
    return U * (6 * k + 2 * lnv + 24) + U * (4 * (lnv + 1) + abs(L))


def set_bound(vocab: int, A: float, lp: float) -> float:
    return lse_bound(vocab, A + lp) + lse_bound(vocab, A) + U * abs(lp)


def id_bound(vocab: int, A: float, lp: float) -> float:
    return lse_bound(vocab, A) + U * abs(lp)


# ----------------------------------------------------------------------------- cases
ROLES = ("col0", "last", "set", "t_ninf", "t_nan", "t_vocab", "t_minus2", "row_ninf_id", "row_ninf_set", "far_below",
         "random", "some_ninf_set")
SEQ_MODES = ("own", "one", "mixed")
SET_MODES = ("random", "empty", "full")


def make_case(rows: int, vocab: int, seed: int, *, shift: int = 0, seq_mode: str = "mixed", set_mode: str = "random",
              acc: bool = True, spread: float = 20.0, density: float = 0.3):
    """A call's inputs as numpy arrays: logits [rows + 1, vocab + 3] uniform in +-spread, NaN in the
    padding columns and in the guard row past ``rows``; the shared end set, whose bits past ``vocab``
    are random; row r plays ROLES[(r + shift) % 12]:

    col0, last, random: an id target (column 0, vocab - 1, any); set: target -1; t_ninf, t_nan: an id
    target whose column is -inf / NaN; t_vocab, t_minus2: targets outside [-1, vocab);
    row_ninf_id, row_ninf_set: the whole row at -inf; far_below: target -1 with the set's columns
    moved so that their maximum is 160 below the other columns' maximum; some_ninf_set: target -1,
    10 % of the columns at -inf and one at NaN.

    seq_mode own: every row its own sequence (row r -> r mod 64); one: one sequence for all rows;
    mixed: interleaved sequences, of which sequence 1 has no rows, and every seventh row carries a
    value outside [0, n_seq).  ``acc``: acc_in non-zero (else null).  ``density``: the share of the ids
    in a random end set."""
    g = np.random.default_rng(seed)
    ld = vocab + 3
    words = (vocab + 31) // 32
    x = g.uniform(-spread, spread, (rows + 1, ld)).astype(np.float32)
    x[:, vocab:] = np.nan
    x[rows] = np.nan
    bits = g.random(vocab) < density
    if set_mode == "empty":
        bits[:] = False
    elif set_mode == "full":
        bits[:] = True
    roles = [ROLES[(r + shift) % len(ROLES)] for r in range(rows)]
    target = np.zeros(rows, dtype=np.int32)
    for r, role in enumerate(roles):
        row = x[r, :vocab]
        t = int(g.integers(vocab))
        if role == "col0":
            t = 0
        elif role == "last":
            t = vocab - 1
        elif role in ("set", "row_ninf_set", "far_below", "some_ninf_set"):
            t = -1
        elif role == "t_vocab":
            t = vocab
        elif role == "t_minus2":
            t = -2
        if role == "t_ninf":
            row[t] = NINF
        elif role == "t_nan":
            row[t] = np.nan
        elif role in ("row_ninf_id", "row_ninf_set"):
            row[:] = NINF
        elif role == "far_below" and bits.any() and not bits.all():
            row[bits] += np.float32(row[~bits].max() - 160.0 - row[bits].max())
        elif role == "some_ninf_set":
            row[g.random(vocab) < 0.1] = NINF
            if vocab > 2:
                row[int(g.integers(vocab))] = np.nan
        target[r] = t
    if seq_mode == "own":
        n_seq = min(rows, 64)
        seq = (np.arange(rows) % 64).astype(np.int32)
    elif seq_mode == "one":
        n_seq, seq = 1, np.zeros(rows, dtype=np.int32)
    else:
        n_seq = min(64, max(3, rows // 2))
        seq = g.integers(0, n_seq, rows).astype(np.int32)
        seq[seq == 1] = 2  # sequence 1 has no rows
        outside = np.array([-1, n_seq, 1 << 20, -(1 << 31)], dtype=np.int64)
        for j, r in enumerate(range(6, rows, 7)):
            seq[r] = np.int32(outside[j % 4])
    acc_in = g.normal(-5.0, 3.0, n_seq).astype(np.float32) if acc else None
    return dict(logits=x, vocab=vocab, target=target, end_set=pack(bits, words, fill=g), seq=seq, n_seq=n_seq,
                acc_in=acc_in, rows=rows, roles=roles)


def launch(case, dev):
    """ops.seq_logprob on the case's tensors on ``dev``.  Returns numpy (lp [rows + 1] and acc_out
    [n_seq + 1], whose last elements start and must stay a canary (77.0), the logits after the call)."""
    import torch

    import voice_enabled_browser_automation_amd.ops as ops

    rows, n_seq = case["rows"], case["n_seq"]
    x = torch.from_numpy(case["logits"].copy()).to(dev)
    t = lambda a: None if a is None else torch.from_numpy(a.copy()).to(dev)  # noqa: E731
    lp = torch.full((rows + 1,), 77.0, dtype=torch.float32, device=dev)
    acc = torch.full((n_seq + 1,), 77.0, dtype=torch.float32, device=dev)
    got = ops.seq_logprob(x, case["vocab"], t(case["target"]), t(case["end_set"]), t(case["seq"]), n_seq,
                          acc_in=t(case["acc_in"]), lp=lp[:rows], acc_out=acc[:n_seq])
    assert got[0].data_ptr() == lp.data_ptr() and got[1].data_ptr() == acc.data_ptr()
    return lp.cpu().numpy(), acc.cpu().numpy(), x.cpu().numpy()


def check_rows(lp, want_lp, want_A, target, vocab, what="", roles=None) -> float:
    """Kernel lp values against the oracle's: -inf and the sign exactly, finite values within the
    bounds.  Returns the largest error / bound."""
    assert not np.isnan(lp).any(), f"{what}: NaN in lp"
    worst = 0.0
    for r in range(len(want_lp)):
        tag = f"{what} row {r}" + (f" ({roles[r]})" if roles else "")
        v = float(lp[r])
        assert v <= 0.0, f"{tag}: log-probability {v} above 0"
        if np.isfinite(want_lp[r]):
            b = (set_bound if target[r] == -1 else id_bound)(vocab, want_A[r], want_lp[r])
            e = abs(v - want_lp[r])
            assert e <= b, f"{tag}: lp {v} vs {want_lp[r]}: off by {e:.3g} > {b:.3g}"
            worst = max(worst, e / b)
        else:
            assert v == NINF, f"{tag}: lp {v}, not -inf"
    return worst


def check(case, got, what: str = "") -> float:
    """The call's outputs against the oracle: canaries, untouched logits, the rows within their
    bounds, the sums bit-equal to the f32 sum of the kernel's own lp."""
    rows, V, n_seq = case["rows"], case["vocab"], case["n_seq"]
    lp, acc, x = got
    assert np.array_equal(x.view(np.int32), case["logits"].view(np.int32)), f"{what}: the logits were written"
    assert lp[rows] == 77.0, f"{what}: lp past rows was written"
    assert acc[n_seq] == 77.0, f"{what}: acc_out past n_seq was written"
    want_lp, want_A = row_reference(case["logits"], V, case["target"], case["end_set"])
    worst = check_rows(lp[:rows], want_lp, want_A, case["target"], V, what, case["roles"])
    want_acc = seq_sum(lp[:rows], case["seq"], n_seq, case["acc_in"])
    assert np.array_equal(acc[:n_seq].view(np.int32), want_acc.view(np.int32)), \
        f"{what}: acc_out {acc[:n_seq].tolist()} is not the f32 sum in row order {want_acc.tolist()}"
    return worst


# ----------------------------------------------------------------------------- the engine's calls
KEYS = {"scores", "scored_tokens", "common_prefix_tokens", "prompt_tokens", "cached_prefix_tokens", "ms"}


def expected_ids(ie, texts):
    from voice_enabled_browser_automation_amd.brain.prompt import llama3_chat, turn_tail

    return [ie.tok.encode("".join(turn_tail(t, llama3_chat))) for t in texts]


def common_prefix(ids):
    c = 0
    while c < min(map(len, ids)) and all(x[c] == ids[0][c] for x in ids):
        c += 1
    return c


def check_call(ie, texts, got, trace):
    """One LLMIntentEngine.rescore() call against the definition, from its traced pieces: the ids
    and the common prefix, every piece's rows against the oracle and its targets against the ids, the
    sums as a chain from zero, scores[i] the last acc_out of its sequence."""
    import torch

    from voice_enabled_browser_automation_amd import ops
    from voice_enabled_browser_automation_amd.brain.prompt import turn_text

    assert set(got) == KEYS
    norm = [turn_text(t) for t in texts]
    distinct = list(dict.fromkeys(norm))
    ids = dict(zip(distinct, expected_ids(ie, distinct)))
    c = common_prefix(list(ids.values()))
    assert got["common_prefix_tokens"] == c
    assert got["prompt_tokens"] == [len(ids[t]) for t in norm]
    assert got["scored_tokens"] == [len(ids[t]) - (c - 1) for t in norm]
    es = None
    acc, pos, last = {}, {}, {}  # per text: the verified sum so far, the next position, its slot
    for tr in trace:
        V = tr["logits"].shape[1]
        target, seq = tr["target"].numpy(), tr["seq"].numpy()
        lp = tr["lp"].numpy()
        want_lp, want_A = row_reference(tr["logits"].numpy(), V, target, tr["set"].numpy())
        check_rows(lp, want_lp, want_A, target, V, f"piece of {tr['texts']}")
        assert np.isfinite(lp).all()
        want_acc = seq_sum(lp, seq, ops.RESCORE_MAX_SEQ, tr["acc_in"].numpy())
        assert np.array_equal(tr["acc_out"].numpy().view(np.int32), want_acc.view(np.int32))
        es = tr["set"] if es is None else es
        assert torch.equal(tr["set"], es)
        j = 0
        for text, rid, slot, first, k in zip(tr["texts"], tr["ids"], tr["slots"], tr["first_pos"], tr["counts"]):
            if text not in ids:  # (a row of another call in the same iteration)
                j += k
                continue
            assert rid == ids[text] and first == pos.get(text, c - 1), "the piece continues where the last one ended"
            nxt = rid[first + 1 : first + 1 + k]
            assert target[j : j + k].tolist() == nxt + [-1] * (k - len(nxt)) and (seq[j : j + k] == slot).all()
            assert float(tr["acc_in"][slot]) == acc.get(text, 0.0), "a sum did not start from the verified one"
            acc[text], pos[text], last[text] = float(tr["acc_out"][slot]), first + k, slot
            j += k
        assert j == len(target) == len(tr["rows"]) and tr["rows"] == list(range(tr["rows"][0], tr["rows"][0] + j))
    on = np.flatnonzero(allowed(es.numpy(), es.numel() * 32))
    assert on.tolist() == ie.end_set_ids()
    assert set(pos) == set(distinct), "an alternative was not scored, or one was scored that was not asked"
    assert all(pos[t] == len(ids[t]) for t in distinct), "rows are missing"
    assert got["scores"] == [acc[t] for t in norm]
    assert all(np.isfinite(s) and s < 0.0 for s in got["scores"])
