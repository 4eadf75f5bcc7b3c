"""An f64 numpy oracle of the wire audio ingest (csrc/ingest/ingest.h), the error bound its f32
kernel and host reference are held to, and the cases their tests share.

The oracle decodes G.711 by the standard's formula (sign, 3-bit exponent e, 4-bit mantissa m of the
inverted code: mu-law magnitude ((2 m + 33) << e) - 33 in 14 bits, A-law 2 m + 1 for e = 0 and
(2 m + 33) << (e - 1) otherwise in 13 bits; shifted to 16 bits), takes the channel mean in f64 and
runs the polyphase sum in f64 over the SAME f32 table, at positions computed with Fractions.

The bound (u = 2^-24, f32's unit roundoff; C channels, 2H taps).  Decoding and the scaling by 2^-15
are exact.  With a_j = (sum_c |v_jc|) / C >= |x_j| for the mean (a_j = |x_j| for one channel):

* the mean is C - 1 additions, each rounding a partial sum of magnitude <= C a_j, and one division:
  ((C - 1) C u a_j) / C + u a_j = C u a_j (nothing for one channel);
* a tap is a product and a sum, each rounded (the kernel fuses them into one rounding): every
  rounding is relative to a partial sum of magnitude <= A = sum_k |h_k| a_k, so 2 . 2H u A;
* the mean's errors pass through the filter: sum_k |h_k| C u a_k = C u A;

so |out - oracle| <= u (4H + C + 2) A, the 2 covering the second-order terms ((1 + u)^(4H + C) - 1 <
1.0001 (4H + C) u for 4H + C <= 200).  It is proportional to the signal under the filter: silence
must come out as exact zeros.  At 16 kHz there is no filter: <= u C a_i, and exact for one channel.
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
ENCODINGS = ("linear16", "mulaw", "alaw")


def g711_value(code: np.ndarray, law: str) -> np.ndarray:
    """The 16-bit value of G.711 codes, by the standard's formula."""
    c = np.asarray(code, dtype=np.int64)
    if law == "mulaw":
        c = 255 - c  # mu-law sends every bit inverted
        e, m = (c >> 4) & 7, c & 15
        mag = (((2 * m + 33) << e) - 33) * 4
        return np.where(c & 128, -mag, mag)
    c = c ^ 0x55  # A-law inverts the even bits
    e, m = (c >> 4) & 7, c & 15
    mag = np.where(e == 0, 2 * m + 1, (2 * m + 33) << np.maximum(e - 1, 0)) * 8
    return np.where(c & 128, mag, -mag)  # (A-law's sign bit set is positive)


def geometry(rate: int):
    f = Fraction(16000, rate)
    L, M = f.numerator, f.denominator
    g0 = min(Fraction(1), f)
    return L, M, int(-(-16 // g0))  # H = ceil(16 / g0)


def values(raw: np.ndarray, encoding: str, channels: int) -> np.ndarray:
    """f64 [n_frames, channels]: the decoded samples / 32768."""
    raw = np.asarray(raw, dtype=np.uint8)
    v = raw.view("<i2").astype(np.int64) if encoding == "linear16" else g711_value(raw, encoding)
    return v.reshape(-1, channels).astype(np.float64) / 32768.0


def ingest(raw, encoding, rate, channels, channel, table, outputs=None):
    """(out f64 [n_out], bound f64 [n_out]).  table: the f32 filter table [L, 2H] the kernel reads.
    outputs: only these output indices (of a long window), in their order."""
    v = values(raw, encoding, channels)
    n_in = v.shape[0]
    if channel is None:
        x, a, C = v.mean(axis=1), np.abs(v).mean(axis=1), channels
    else:
        x, a, C = v[:, channel], np.abs(v[:, channel]), 1
    L, M, H = geometry(rate)
    n_out = n_in * L // M
    i = np.arange(n_out, dtype=np.int64) if outputs is None else np.asarray(outputs, dtype=np.int64)
    assert i.size == 0 or (0 <= i.min() and i.max() < n_out)
    if L == M:
        return x[i], (U * C * a[i] if C > 1 else np.zeros(i.size))
    tab = np.asarray(table, dtype=np.float64)
    assert tab.shape == (L, 2 * H), (tab.shape, L, H)
    pos, ph = (i * M) // L, (i * M) % L
    idx = pos[:, None] - H + 1 + np.arange(2 * H)[None, :]
    ok = (idx >= 0) & (idx < n_in)
    idx = np.clip(idx, 0, max(n_in - 1, 0))
    h = tab[ph]
    out = (h * np.where(ok, x[idx], 0.0)).sum(axis=1)
    A = (np.abs(h) * np.where(ok, a[idx], 0.0)).sum(axis=1)
    return out, U * (4 * H + C + 2) * A


def exact_positions(outputs, rate: int):
    """(pos, phase) of the given outputs by exact rational arithmetic: output i lies at input time
    i * rate / 16000 = pos + phase / L."""
    r = Fraction(rate, 16000)
    L = Fraction(16000, rate).numerator
    pos, ph = [], []
    for i in outputs:
        t = i * r
        p = t.numerator // t.denominator
        pos.append(p)
        frac = (t - p) * L
        assert frac.denominator == 1
        ph.append(int(frac))
    return np.array(pos, dtype=np.int64), np.array(ph, dtype=np.int64)


# ----------------------------------------------------------------------------- cases
def encode_noise(g: np.random.Generator, n_frames: int, encoding: str, channels: int, kind: str = "noise"):
    """Wire bytes of n_frames frames: full-scale random noise (every code / every s16 value equally
    likely), or the all-max-code input (the largest positive value in every sample)."""
    n = n_frames * channels
    if encoding == "linear16":
        v = (np.full(n, 32767) if kind == "max" else g.integers(-32768, 32768, n)).astype("<i2")
        return v.view(np.uint8).copy()
    if kind == "max":
        return np.full(n, 0x80 if encoding == "mulaw" else 0xAA, dtype=np.uint8)  # +32124 / +32256
    return g.integers(0, 256, n).astype(np.uint8)


def check(got: np.ndarray, raw, encoding, rate, channels, channel, table, what=""):
    """got (f32) against the oracle within the bound; returns the largest error / bound."""
    want, bound = ingest(raw, encoding, rate, channels, channel, table)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: {got.shape} outputs, not {want.shape}"
    if got.size == 0:
        return 0.0
    err = np.abs(got - want)
    bad = err > bound
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {got.size} outputs off by more than the bound; first at "
                           f"{int(np.argmax(bad))}: {got[np.argmax(bad)]!r} vs {want[np.argmax(bad)]!r}, "
                           f"bound {bound[np.argmax(bad)]:.3g}")
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
