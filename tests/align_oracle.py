"""Float64 oracles and derived bounds for the word-alignment ops (csrc/align, ops.attn_probs /
align_cost / dtw_path / token_logprob).  Independent of ops/reference.py: plain numpy written from
the contracts.  Used by test_align_cpu.py (against the CPU reference) and test_align_kernels_gpu.py
(against the kernels); every oracle is computed from the very bf16 / f32 values the op read."""
import numpy as np
import torch

from kernel_oracle import SENTINEL  # noqa: F401  (re-export: outputs are pre-filled with it)


def gen(*key) -> torch.Generator:
    g = torch.Generator()
    g.manual_seed(sum((i + 1) * 7919 * (int(k) + 1) for i, k in enumerate(key)))
    return g


# ----------------------------------------------------------------------------- attn_probs
def probs64(q: torch.Tensor, k: torch.Tensor, heads, n_keys: int, scale: float):
    """(softmax in f64 [n_sel, T, n_keys], per-row bound factor A [n_sel, T] = scale * max_j sum_i |q_i||k_ij|)."""
    S, H, hd = k.shape
    q64 = q.double().view(q.shape[0], H, hd).numpy()
    k64 = k.double().numpy()[:n_keys]
    ref, A = [], []
    for h in heads:
        s = scale * (q64[:, h] @ k64[:, h].T)
        e = np.exp(s - s.max(axis=1, keepdims=True))
        ref.append(e / e.sum(axis=1, keepdims=True))
        A.append(scale * (np.abs(q64[:, h]) @ np.abs(k64[:, h]).T).max(axis=1))
    return np.stack(ref), np.stack(A)


def probs_bound(ref: np.ndarray, A: np.ndarray) -> np.ndarray:
    """|got - ref| <= ref (2^-17 A + 2^-16) + 2^-40: bf16 products are exact in f32 and a 64-term f32
    sum errs by at most 2^-18 sum|q_i k_i|; that error enters through the numerator and through the
    sum; 2^-16 covers the exp and the sum over the keys."""
    return ref * (2.0 ** -17 * A[..., None] + 2.0 ** -16) + 2.0 ** -40


# ----------------------------------------------------------------------------- align_cost
def reflect(i: int, n: int) -> int:
    if i < 0:
        i = -i
    if i >= n:
        i = 2 * (n - 1) - i
    return i


def cost64(probs: torch.Tensor, n_tokens: int, n_keys: int):
    """(cost f64 [n_tokens, n_keys], per-element bound): z-score over the token rows per head and
    column, numpy.median over explicit reflect-padded 7-wide windows (none for n_keys <= 3), mean
    over heads, negated.

    Bound (the median is 1-Lipschitz in the sup norm, so it is the z-score's): per head
    8 * 2^-24 * T * (1 + max over the window's columns of max_t|p| / sigma) * (1 + max over the
    window of |z| in this row), averaged over the heads like the cost itself.

    The ratio is max|p| / sigma, not max|p - mean| / sigma: the f32 mean of T values of size |p|
    errs by up to T 2^-24 mean|p|, and p - mean inherits that error in absolute terms however small
    the difference is (cancellation), so z = (p - mean) / sigma errs by T 2^-24 |p| / sigma (1 + |z|)
    -- the sigma computed from the same differences contributes the |z| factor.  With |p - mean|
    in the ratio the bound misses columns whose rows are nearly equal: T = 2, n_keys = 250, one head
    measured 1.31 x that bound at element (1, 228), where the column's two probabilities agree to
    4 digits, from a kernel that rounds once per operation."""
    p = probs.double().numpy()[:, :n_tokens, :n_keys]
    Hs, T, N = p.shape
    mu = p.mean(axis=1, keepdims=True)
    sig = np.sqrt(((p - mu) ** 2).mean(axis=1, keepdims=True) + 1e-12)
    z = (p - mu) / sig
    ratio = (np.abs(p).max(axis=1, keepdims=True) / sig)[:, 0]  # [Hs, N]
    if N > 3:
        idx = np.array([[reflect(j + e, N) for e in range(-3, 4)] for j in range(N)])  # [N, 7]
    else:
        idx = np.arange(N)[:, None]
    win = z[:, :, idx]                      # [Hs, T, N, w]
    med = np.median(win, axis=-1)
    zmax = np.abs(win).max(axis=-1)         # [Hs, T, N]
    rmax = ratio[:, idx].max(axis=-1)       # [Hs, N]
    bound = 8 * 2.0 ** -24 * T * (1 + rmax[:, None, :]) * (1 + zmax)
    return -med.mean(axis=0), bound.mean(axis=0)


# ----------------------------------------------------------------------------- dtw
def dtw_plain(cost: np.ndarray):
    """The plain double loop in f64: (D, first_frame, last_frame) with the tie rule -- the diagonal
    only if strictly smaller than both others, else the vertical step only if strictly smaller
    than both others, else the horizontal step."""
    T, N = cost.shape
    D = np.full((T, N), np.inf)
    step = np.zeros((T, N), dtype=np.int8)
    for i in range(T):
        for j in range(N):
            if i == 0 and j == 0:
                D[0, 0] = cost[0, 0]
                continue
            c0 = D[i - 1, j - 1] if i > 0 and j > 0 else np.inf
            c1 = D[i - 1, j] if i > 0 else np.inf
            c2 = D[i, j - 1] if j > 0 else np.inf
            if c0 < c1 and c0 < c2:
                D[i, j], step[i, j] = cost[i, j] + c0, 0
            elif c1 < c0 and c1 < c2:
                D[i, j], step[i, j] = cost[i, j] + c1, 1
            else:
                D[i, j], step[i, j] = cost[i, j] + c2, 2
    return (D,) + backtrack(step)


def backtrack(step: np.ndarray):
    T, N = step.shape
    first, last = np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
    i, j = T - 1, N - 1
    last[i] = j
    while i > 0 or j > 0:
        s = step[i, j]
        if s == 2:
            j -= 1
            continue
        first[i] = j
        i -= 1
        if s == 0:
            j -= 1
        last[i] = j
    return first, last


def dtw64(cost: np.ndarray):
    """dtw_plain, one anti-diagonal at a time (numpy-vectorised: the 448 x 1500 case in well under a
    second); test_align_cpu.py holds it to the plain loop."""
    c = np.asarray(cost, dtype=np.float64)
    T, N = c.shape
    D = np.full((T + 1, N + 1), np.inf)
    step = np.full((T, N), 2, dtype=np.int8)
    for d in range(T + N - 1):
        i = np.arange(max(0, d - N + 1), min(T, d + 1))
        j = d - i
        c0, c1, c2 = D[i, j], D[i, j + 1], D[i + 1, j]
        diag = (c0 < c1) & (c0 < c2)
        vert = ~diag & (c1 < c0) & (c1 < c2)
        best = np.where(diag, c0, np.where(vert, c1, c2)) if d else np.zeros(1)
        D[i + 1, j + 1] = c[i, j] + best
        step[i, j] = np.where(diag, 0, np.where(vert, 1, 2))
    return (D[1:, 1:],) + backtrack(step)


def check_path(cost: np.ndarray, first, last, what: str = "") -> None:
    """The two vectors describe a legal monotone path from (0, 0) to (T-1, N-1) -- row i covers
    frames first[i]..last[i], consecutive rows touch (a diagonal step) or overlap by one frame (a
    vertical step) -- whose f64 cost is at most the f64 optimum + (T + N) 2^-23 sum|cost| along it
    (each f32 partial sum of the kernel's table errs by 2^-24 relative per addition, on its own
    path and on the optimum's)."""
    c = np.asarray(cost, dtype=np.float64)
    T, N = c.shape
    first, last = np.asarray(first, dtype=np.int64), np.asarray(last, dtype=np.int64)
    assert first.shape == (T,) and last.shape == (T,), what
    assert first[0] == 0 and last[-1] == N - 1, f"{what}: path ends {first[0]}, {last[-1]}"
    assert (first <= last).all() and (first >= 0).all() and (last < N).all(), what
    gap = first[1:] - last[:-1]
    assert ((gap == 0) | (gap == 1)).all(), f"{what}: rows neither touch nor overlap: {gap[(gap < 0) | (gap > 1)][:5]}"
    total, mag = 0.0, 0.0
    for i in range(T):
        seg = c[i, first[i] : last[i] + 1]
        total += seg.sum()
        mag += np.abs(seg).sum()
    opt = dtw64(c)[0][-1, -1]
    slack = (T + N) * 2.0 ** -23 * mag
    print(f"{what}: path cost {total:.9g}, optimum {opt:.9g}, slack {slack:.3g}")
    assert total <= opt + slack, f"{what}: path cost {total} > optimum {opt} + {slack}"


# ----------------------------------------------------------------------------- token_logprob
def unpack_mask(mask_row: np.ndarray, n: int) -> np.ndarray:
    bits = np.unpackbits(np.ascontiguousarray(mask_row).view(np.uint8), bitorder="little")
    return bits[:n].astype(bool)


def pack_mask(bits: np.ndarray) -> np.ndarray:
    n = (len(bits) + 31) // 32 * 32
    b = np.zeros(n, dtype=np.uint8)
    b[: len(bits)] = bits
    return np.packbits(b, bitorder="little").view(np.int32).copy()


def logprob64(logits: torch.Tensor, targets, masks, vocab: int) -> np.ndarray:
    """masks: None or bool [N, vocab]."""
    x = logits.double().numpy()[:, :vocab]
    out = np.zeros(x.shape[0])
    for n in range(x.shape[0]):
        row = x[n] if masks is None else x[n][masks[n]]
        m = row.max()
        out[n] = x[n, targets[n]] - (m + np.log(np.exp(row - m).sum()))
    return out


def logprob_bound(ref: np.ndarray) -> np.ndarray:
    """2^-14 + 2^-22 |ref|: the f32 sum of <= 51866 terms split over 256 lanes errs by about 2^-16
    relative, which the log turns into an absolute error."""
    return 2.0 ** -14 + 2.0 ** -22 * np.abs(ref)
