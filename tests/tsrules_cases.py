"""Inputs for the timestamp rules tests: the two vocabulary layouts, token histories of every state
class, masks in the sampler's packing, and rows whose f64 T - M sits on a chosen target."""
import math

import numpy as np

import tsrules_oracle as to

REAL = dict(V=51865, eot=50257, tsb=50364, ld=51872, max_initial=50)
# fewer columns than lanes, an unaligned tail, a mask row of 2 words, n_ts = 7
TINY = dict(V=61, eot=40, tsb=54, ld=64, max_initial=3)
TARGETS = (0.01, -0.01, 1.0, -1.0, 5.0, -5.0)


def tau(lay) -> float:
    """How close T and M may come before the kernel's f32 T may decide rule 5 differently from the
    f64 oracle.  M is a maximum of inputs: exact.  T = m + log(sum exp(x_i - m)) over at most n_ts
    values, with |x| < 32 here (asserted where the rows are built), in units of u = 2^-24:
      * the sum: each of at most n_ts additions rounds once, relative error <= u each, so at most
        n_ts * u on the sum whatever the order, and the same absolute error on its logarithm;
      * the terms: d = m - x_i rounds with relative error u, which weighs d * e^-d <= 1 / e per term
        against a sum >= 1: at most 0.37 * n_ts * u; expf is within 1 ulp: 2u relative;
      * rescalings: a running sum moved to a larger maximum takes one more expf and a product, 3u;
        a value passes at most R of them, R = the values one lane holds after its first (online; the
        first starts the sum exactly) plus the one move to the workgroup's maximum -- at most 6 for
        the real layout (1501 values over 512 lanes: one load of four, and a head or tail value),
        1 for the tiny one (fewer values than lanes);
      * logf within 1 ulp of a value <= log(n_ts) < 8 (n_ts < 2980): at most 8u;
      * the last addition rounds a |T| < 32: at most half an ulp, 16u;
    in all (1.37 * n_ts + 26 + 3 R) u: 2100u for the real layout, 38.6u for the tiny one, both below
    (n_ts + 16) * 2u = (n_ts + 16) * 2^-23 (3034u: 1.8e-4, and 46u: 2.7e-6).  First order and worst
    case; not fitted to a run."""
    return (lay["V"] - lay["tsb"] + 16) * 2.0 ** -23


def pack(bits: np.ndarray) -> np.ndarray:
    n = (len(bits) + 31) // 32 * 32
    b = np.zeros(n, dtype=np.uint8)
    b[: len(bits)] = bits
    return np.packbits(b, bitorder="little").view(np.uint32).view(np.int32).copy()


def histories(lay):
    """Token histories covering n = 0, 1, >= 2, each combination of last / prev being text or a
    timestamp, and last_ts in {-1, 0, mid, n_ts - 2, n_ts - 1}."""
    tsb, n_ts = lay["tsb"], lay["V"] - lay["tsb"]
    a, b = 5, 17
    out = [[], [a], [a, b], [b, a, b]]
    for k in (0, n_ts // 2, n_ts - 2, n_ts - 1):
        t = tsb + k
        out += [[t], [t, a], [a, t], [t, t], [t, a, b], [tsb, a, t], [tsb, a, t, t], [tsb, b, t, t, a]]
    return out


def masks(lay, rows: int, rng) -> np.ndarray:
    """Per-row masks [rows, words]: text, EOT on every other row, timestamps; about 3 % of the ids
    cleared at random, and everything from V up cleared."""
    V, eot, tsb, ld = lay["V"], lay["eot"], lay["tsb"], lay["ld"]
    ids = np.arange(ld)
    out = []
    for r in range(rows):
        bits = ((ids < eot) | ((ids >= tsb) & (ids < V))) & (rng.random(ld) > 0.03)
        bits[eot] = r % 2 == 0
        out.append(pack(bits))
    return np.stack(out)


def t_and_m(x, hist, lay, mask_row):
    _, T, M = to.rules(x.tolist(), hist, lay["V"], lay["eot"], lay["tsb"], lay["max_initial"], mask_row)
    return T, M


def rows_on_targets(lay, hists, mask, rng, targets=TARGETS) -> np.ndarray:
    """f32 logits [len(hists), ld]: N(0, 3) clipped to +-15, each row's timestamp columns shifted by
    one constant so that the f64 T - M is the row's target (the log-sum-exp moves by exactly the
    shift); rows where either side is empty stay as drawn.  Columns >= V hold the sentinel 777."""
    V, tsb, ld = lay["V"], lay["tsb"], lay["ld"]
    x = np.clip(rng.normal(0.0, 3.0, (len(hists), ld)), -15, 15).astype(np.float32)
    for r, h in enumerate(hists):
        T, M = t_and_m(x[r], h, lay, mask[r if mask.shape[0] > 1 else 0])
        if math.isfinite(T) and math.isfinite(M):
            x[r, tsb:V] = (x[r, tsb:V].astype(np.float64) + (targets[r % len(targets)] - (T - M))).astype(np.float32)
    x[:, V:] = 777.0
    assert np.abs(x[:, :V]).max() < 32
    return x


def expect_row(x_row, hist, lay, mask_row):
    """(the oracle's row as f32, |T - M|) for one row of f32 logits."""
    banned, T, M = to.rules(x_row.tolist(), hist, lay["V"], lay["eot"], lay["tsb"], lay["max_initial"], mask_row)
    want = x_row.copy()
    want[sorted(banned)] = -np.inf  # (to.apply and to.margin, from one pass over the row)
    return want, abs(T - M) if math.isfinite(T) and math.isfinite(M) else math.inf


def bits_equal(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())
