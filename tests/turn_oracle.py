"""An f64 numpy oracle of the set log-probability (csrc/turn/turn.h), the error bounds its f32
kernel is held to, and the cases the kernel tests share.

The kernel computes two log-sum-exps per row in one sweep -- A over every column below V, Ls over
the columns of the set -- each with its own running maximum, and returns (min(Ls - A, 0), A).  Each
has the reduction shape of the score step (tests/score_oracle.py derives the same terms), so, with
u = 2^-24 (f32's unit roundoff):

* every lane accumulates k = 4 ceil(V / 2048) + 6 terms in sequence (float4 loads over 512 lanes,
  issued four at a time but used in the sweep's order, a scalar head and tail), then six wave
  shuffles and eight LDS values are added: a depth of k + 14 additions, u each;
* a term's exponential is good to 2 ulp = 4 u, and so is each of the at most k rescales
  (s * exp(m - v)) it rides through when its lane meets a new maximum, and the one scaling to the
  workgroup's maximum: 5 u (k + 2) with the multiplications' own roundings;
* the exponentials' arguments are differences rounded to f32: d u for a term d below the maximum,
  weighed by the terms' shares -- E[d] = (max - L) + H(p) <= ln V, counted twice (lane maximum,
  workgroup maximum);
so a sum is good to u (6 k + 2 ln V + 24) relative, which the logarithm turns into an absolute
error of its L; logf adds 4 u |ln sum| <= 4 u (ln V + 1) and the addition max + ln sum adds u |L|:

    lse_bound(V, L) = u (6 k + 2 ln V + 24) + u (4 (ln V + 1) + |L|)

out[:, 1] = A is held to lse_bound(V, A).  out[:, 0] is the difference of two such values, Ls =
A + lp and A, whose subtraction adds u |lp| (the clamp at 0 only moves a value towards the true one,
which is <= 0):

    lp_bound(V, A, lp) = lse_bound(V, A + lp) + lse_bound(V, A) + u |lp|

The set's sum has at most V terms, so V bounds its k and ln too.  Nothing here is tuned: a set 160
below the row's maximum stays within it because the set keeps its own maximum."""
import numpy as np

U = 2.0 ** -24
NINF = -np.inf


def allowed(set_row: np.ndarray, vocab: int) -> np.ndarray:
    ids = np.arange(vocab)
    return ((set_row.view(np.uint32)[ids >> 5] >> (ids & 31).astype(np.uint32)) & 1).astype(bool)


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


def reference(logits: np.ndarray, vocab: int, sets: np.ndarray):
    """(lp f64 [rows], A f64 [rows]) of f32 logits [rows, >= vocab] and int32 sets [1 or >= rows, words]."""
    rows = logits.shape[0]
    lp, A = np.full(rows, NINF), np.full(rows, NINF)
    for r in range(rows):
        on = allowed(sets[r if sets.shape[0] > 1 else 0], vocab)
        x = logits[r, :vocab].astype(np.float64)
        live = x > NINF  # (False for a NaN)
        A[r] = _lse(x[live])
        ls = _lse(x[live & on])
        if np.isfinite(ls) and np.isfinite(A[r]):
            lp[r] = min(ls - A[r], 0.0)
    return lp, A


def lse_bound(vocab: int, L: float) -> float:
    k = 4 * -(-vocab // 2048) + 6
    lnv = np.log(vocab) if vocab > 1 else 0.0
    return U * (6 * k + 2 * lnv + 24) + U * (4 * (lnv + 1) + abs(L))


def lp_bound(vocab: int, A: float, lp: float) -> float:
    return lse_bound(vocab, A + lp) + lse_bound(vocab, A) + U * abs(lp)


# ----------------------------------------------------------------------------- cases
ROLES = ("empty", "full", "single", "set_ninf", "row_ninf", "far_below", "some_ninf")


def make_case(rows: int, vocab: int, ld: int, per_row: bool, seed: int, shift: int = 0, spread: float = 20.0):
    """A launch's inputs as numpy arrays: logits [rows + 1, ld] uniform in +-spread, NaN in the
    padding columns and in the guard row past ``rows``; a shared or per-row set whose bits past
    ``vocab`` are random; row r plays ROLES[(r + shift) % 7].  The roles that shape the set (empty,
    full, single) shape the shared set only from row 0; the others shape the row's logits:
    set_ninf puts the set's columns at -inf, row_ninf the whole row, far_below moves the set's
    columns so that their maximum is 160 below the other columns' maximum, some_ninf puts 10 % of
    the columns at -inf and one at NaN."""
    g = np.random.default_rng(seed)
    words = (vocab + 31) // 32
    x = g.uniform(-spread, spread, (rows + 1, ld)).astype(np.float32)
    x[:, vocab:] = np.nan
    x[rows] = np.nan
    nsets = rows if per_row else 1
    bits = g.random((nsets, vocab)) < 0.5
    roles = [ROLES[(r + shift) % len(ROLES)] for r in range(rows)]
    for r in range(nsets):
        if roles[r] == "empty":
            bits[r] = False
        elif roles[r] == "full":
            bits[r] = True
        elif roles[r] == "single":
            bits[r] = False
            bits[r, int(g.integers(vocab))] = True
    for r in range(rows):
        on = bits[r if per_row else 0]
        if roles[r] == "set_ninf":
            x[r, :vocab][on] = NINF
        elif roles[r] == "row_ninf":
            x[r, :vocab] = NINF
        elif roles[r] == "far_below" and on.any() and not on.all():
            row = x[r, :vocab]
            row[on] += np.float32(row[~on].max() - 160.0 - row[on].max())
        elif roles[r] == "some_ninf":
            x[r, :vocab][g.random(vocab) < 0.1] = NINF
            if vocab > 2:
                x[r, int(g.integers(vocab))] = np.nan
    sets = np.stack([pack(b, words, fill=g) for b in bits])
    return dict(logits=x, vocab=vocab, sets=sets, rows=rows, roles=roles)


def launch(case, dev):
    """ops.set_logprob on the case's tensors on ``dev``.  Returns numpy (out [rows + 1, 2] whose last
    row starts and must stay a canary (77.0), the logits after the launch)."""
    import torch

    import voice_enabled_browser_automation_amd.ops as ops

    rows = case["rows"]
    x = torch.from_numpy(case["logits"].copy()).to(dev)
    sets = torch.from_numpy(case["sets"]).to(dev)
    out = torch.full((rows + 1, 2), 77.0, dtype=torch.float32, device=dev)
    got = ops.set_logprob(x[:rows], case["vocab"], sets, out=out[:rows])
    assert got.data_ptr() == out.data_ptr()
    return out.cpu().numpy(), x.cpu().numpy()


def check(case, got, what: str = "") -> float:
    """The launch's outputs against the oracle: canaries, untouched logits, -inf and the sign
    exactly, finite values within the bounds.  Returns the largest error / bound."""
    rows, V = case["rows"], case["vocab"]
    out, x = got
    want_lp, want_A = reference(case["logits"][:rows], V, case["sets"])
    assert np.array_equal(x.view(np.int32), case["logits"].view(np.int32)), f"{what}: the logits were written"
    assert (out[rows] == 77.0).all(), f"{what}: a row past rows was written"
    assert not np.isnan(out[:rows]).any(), f"{what}: NaN in {out[:rows].tolist()}"
    worst = 0.0
    for r in range(rows):
        tag = f"{what} row {r} ({case['roles'][r]})"
        lp, A = float(out[r, 0]), float(out[r, 1])
        assert lp <= 0.0, f"{tag}: log-probability {lp} above 0"
        if np.isfinite(want_A[r]):
            b = lse_bound(V, want_A[r])
            e = abs(A - want_A[r])
            assert e <= b, f"{tag}: A {A} vs {want_A[r]}: off by {e:.3g} > {b:.3g}"
            worst = max(worst, e / b)
        else:
            assert A == NINF, f"{tag}: A {A}, not -inf"
        if np.isfinite(want_lp[r]):
            b = lp_bound(V, want_A[r], want_lp[r])
            e = abs(lp - want_lp[r])
            assert e <= b, f"{tag}: lp {lp} vs {want_lp[r]}: off by {e:.3g} > {b:.3g}"
            worst = max(worst, e / b)
        else:
            assert lp == NINF, f"{tag}: lp {lp}, not -inf"
    return worst
