"""An f64 numpy oracle of the nucleus step (csrc/nucleus/nucleus.h), the margin inside which its f32
cut may differ from exact arithmetic, and the cases the kernel and reference-op tests share.

Exact parts.  The penalty is one correctly rounded f32 operation per distinct valid id (numpy's
float32 `/` and `*` are that), the candidates' order is compares only, pass-through rows are copies:
all of these are compared bit for bit, with no margin.

The cut.  With K ordered, a_i = (l_i - l_0) / T, w_i = exp(a_i), c_j = sum_{i <= j} w_i, C = c_{k-1},
the row keeps ids 0 .. j*, j* = the smallest j with c_j >= top_p C.  In exact arithmetic that is the
smallest j with c_j / C >= top_p; f32 can only decide otherwise where some c_j / C is within DELTA of
top_p.  With u = 2^-24 (f32's unit roundoff):

* a_i is a subtraction and a division, u each: |da_i| <= 2 u |a_i|, which exp turns into a relative
  error 2 u |a_i| of w_i.  A weight with a_i < -A_MAX = -104 is below f32's smallest denormal
  (e^-104 < 2^-149), i.e. 0 in f32 and < 2^-149 exactly; a denormal result adds at most 2^-149
  absolute.  So |a_i| <= 104 wherever the relative term matters: 208 u.
* expf is good to 2 ulp = 4 u (the bound tests/turn_oracle.py uses for the same function).
* a sum of n <= N_MAX = 1024 non-negative terms, in any order, is good to (n - 1) u relative.
* c_j >= w_0 = 1, so the at most 1024 absolute terms of 2^-149 are below 2^-139 relative: nothing.
  So every c_j, and C, is good to e_c = (208 + 4 + 1023) u = 1235 u relative.
* the comparison is against fl(top_p C): one more u.  (top_p itself is an f32 the oracle reads
  exactly.)
So the f32 decision "c_j >= top_p C" equals the exact one unless |c_j / C - top_p| <= (2 e_c + 1) u-units
of c_j / C <= 1:

    DELTA = (2 (2 A_MAX + 4 + N_MAX - 1) + 1) u (1 + 10^-3) = 2471 u 1.001 ~ 1.474e-4

(the last factor covers the products of the first-order terms).  The generator gives every narrowed
row a top_p that is the midpoint of a gap wider than 2 DELTA between adjacent ratios (0 counts as the
ratio before the first), and asserts that it found one: every case is then unambiguous, none is
skipped, and the kernel's mask must equal the oracle's bit for bit."""
import numpy as np

U = 2.0 ** -24
A_MAX = 104.0
N_MAX = 1024
DELTA = (2 * (2 * A_MAX + 4 + N_MAX - 1) + 1) * U * 1.001
NINF = -np.inf
MAX_TOP_K = 1024
LLAMA_VOCAB = 128256
CANARY = 0x5A5A5A5A


def allowed(row: np.ndarray, vocab: int) -> np.ndarray:
    ids = np.arange(vocab)
    return ((row.view(np.uint32)[ids >> 5] >> (ids & 31).astype(np.uint32)) & 1).astype(bool)


def pack(bits: np.ndarray, words: int, fill=None) -> np.ndarray:
    """bits -> int32 words; the bits past len(bits) are zero, or random under a generator ``fill``
    (the kernel must clear them)."""
    b = np.zeros(words * 32, dtype=np.uint8)
    if fill is not None:
        b[:] = fill.random(words * 32) < 0.5
    b[: len(bits)] = bits
    return np.packbits(b, bitorder="little").view(np.uint32).view(np.int32).copy()


def penalise(x: np.ndarray, vocab: int, history: np.ndarray, theta: np.float32) -> np.ndarray:
    """Row x (f32) after the penalty: once per distinct valid id, one f32 operation each."""
    x = x.copy()
    if theta == np.float32(1.0):
        return x
    for t in dict.fromkeys(int(t) for t in history):
        if 0 <= t < vocab:
            x[t] = x[t] / theta if x[t] > 0 else x[t] * theta
    return x


def ordered_candidates(x: np.ndarray, vocab: int, on: np.ndarray) -> np.ndarray:
    """The ids of A in the contract's order: logit descending (-0 == +0), id ascending."""
    v = x[:vocab].astype(np.float64)
    ids = np.nonzero(on & (v > NINF))[0]  # (a NaN is not > -inf)
    return ids[np.lexsort((ids, -v[ids]))]


def ratios(x: np.ndarray, K: np.ndarray, T: float) -> np.ndarray:
    """c_j / C over K in f64."""
    l = x[K].astype(np.float64)
    c = np.cumsum(np.exp((l - l[0]) / T))
    return c / c[-1]


def effective_k(top_k: int, top_p: float) -> int:
    k = min(max(int(top_k), 0), MAX_TOP_K)
    return MAX_TOP_K if k == 0 and top_p < 1.0 else k


def passes_through(T: float, top_k: int, top_p: float) -> bool:
    return not T > 0.0 or (min(max(int(top_k), 0), MAX_TOP_K) == 0 and not top_p < 1.0)


def reference(case):
    """(penalised logits f32 [rows, ld], mask_out int32 [rows, words], n_kept [rows], the smallest
    distance of a ratio from its row's top_p)."""
    rows, V = case["rows"], case["vocab"]
    words = (V + 31) // 32
    x = case["logits"][:rows].copy()
    out = np.zeros((rows, words), dtype=np.int32)
    n_kept = np.zeros(rows, dtype=np.int32)
    closest = np.inf
    for r in range(rows):
        x[r] = penalise(x[r], V, case["history"][r], case["penalty"][r])
        m = case["mask"]
        on = np.ones(V, dtype=bool) if m is None else allowed(m[r if m.shape[0] > 1 else 0], V)
        T, p, k = float(case["temperature"][r]), float(case["top_p"][r]), int(case["top_k"][r])
        if passes_through(T, k, p):
            out[r] = pack(on, words)
            n_kept[r] = on.sum()
            continue
        A = ordered_candidates(x[r], V, on)
        K = A[: effective_k(k, p)]
        if not K.size:
            continue
        n = K.size
        if p < 1.0:
            q = ratios(x[r], K, T)
            n = int(np.nonzero(q >= p)[0][0]) + 1
            closest = min(closest, float(np.abs(q - p).min()))
        keep = np.zeros(V, dtype=bool)
        keep[K[:n]] = True
        out[r] = pack(keep, words)
        n_kept[r] = n
    return x, out, n_kept, closest


# ----------------------------------------------------------------------------- cases
ROLES = ("plain", "all_equal", "quantised", "few_allowed", "empty_mask", "allowed_ninf", "topk1", "topk1024", "topp1",
         "topp_first", "pass_k0", "pass_T", "history", "theta1", "k0_topp")


def _choose_top_p(g, q: np.ndarray, first: bool) -> np.float32:
    """The midpoint of a gap wider than 2 DELTA between adjacent ratios (0 before the first)."""
    edges = np.concatenate(([0.0], q))
    gaps = np.nonzero(np.diff(edges) > 2 * DELTA)[0]
    assert gaps.size, "no gap wider than 2 DELTA between the ratios: the case would be ambiguous"
    j = 0 if first else int(g.choice(gaps))
    assert j in gaps
    p = np.float32(0.5 * (edges[j] + edges[j + 1]))
    assert edges[j] + DELTA < float(p) < edges[j + 1] - DELTA
    return p


def make_case(rows: int, vocab: int, ld: int, seed: int, shift: int = 0, spread: float = 12.0, H: int = 12,
              null_mask: bool = False, shared_mask: bool = False):
    """A launch's inputs as numpy arrays: logits [rows + 1, ld] uniform in +-spread with NaN in the
    padding columns and in the guard row; per-row masks (70 % on) whose bits past ``vocab`` are
    random; a history of H ids per row with -1s and repeats; row r plays ROLES[(r + shift) % 15]."""
    g = np.random.default_rng(seed)
    words = (vocab + 31) // 32
    x = g.uniform(-spread, spread, (rows + 1, ld)).astype(np.float32)
    x[:, vocab:] = np.nan
    x[rows] = np.nan
    roles = [ROLES[(r + shift) % len(ROLES)] for r in range(rows)]
    nm = 1 if shared_mask else rows
    bits = g.random((nm, vocab)) < 0.7
    T = np.full(rows, 0.7, dtype=np.float32)
    top_p = np.ones(rows, dtype=np.float32)
    top_k = g.integers(1, 61, rows).astype(np.int32)
    theta = np.full(rows, 1.1, dtype=np.float32)
    hist = g.integers(-1, vocab, (rows, H)).astype(np.int32)
    if H > 3:
        hist[:, 3] = hist[:, 0]  # a repeat in every row
    want_p = np.ones(rows, dtype=bool)  # rows whose top_p the generator chooses below
    first = np.zeros(rows, dtype=bool)
    for r in range(rows):
        role, row = roles[r], x[r, :vocab]
        if role == "all_equal":
            row[:] = np.float32(1.5)
            theta[r] = 1.0
        elif role == "quantised":
            row[:] = g.choice(np.array([-2.0, -0.0, 0.0, 0.75, 3.0], dtype=np.float32), vocab)
        elif role == "few_allowed" and not shared_mask:
            bits[r] = False
            bits[r, g.integers(0, vocab, 3)] = True
            top_k[r] = 50
        elif role == "empty_mask" and not shared_mask:
            bits[r] = False
        elif role == "allowed_ninf":
            row[g.random(vocab) < 0.4] = NINF
            if vocab > 2:
                row[int(g.integers(vocab))] = np.nan
        elif role == "topk1":
            top_k[r] = 1
        elif role == "topk1024":
            top_k[r] = 1024
        elif role == "topp1":
            want_p[r] = False
        elif role == "topp_first":
            first[r] = True
        elif role == "pass_k0":
            top_k[r], want_p[r] = 0, False
            top_p[r] = 1.0 if r % 2 else 1.5
        elif role == "pass_T":
            T[r] = 0.0 if r % 2 else -1.0
        elif role == "history" and H > 0:
            # repeats, -1, ids out of range on both sides, ids outside the mask, both signs of logit
            theta[r] = 1.3
            a, b = int(g.integers(vocab)), int(g.integers(vocab))
            row[a], row[b] = np.float32(2.5), np.float32(-2.5)
            if not shared_mask:
                bits[r, b] = False
            h = [a, b, a, -1, vocab, b, vocab + 5, -7, 1 << 30, a, 0, vocab - 1]
            hist[r, :] = (h * (H // len(h) + 1))[:H]
        elif role == "theta1":
            theta[r] = 1.0
        elif role == "k0_topp":
            top_k[r] = 0
    mask = None if null_mask else np.stack([pack(b, words, fill=g) for b in bits])
    for r in range(rows):  # the generator's top_p, from the oracle's own ratios
        if not want_p[r] or not T[r] > 0:
            continue
        on = np.ones(vocab, dtype=bool) if mask is None else allowed(mask[r if mask.shape[0] > 1 else 0], vocab)
        xr = penalise(x[r], vocab, hist[r], theta[r])
        A = ordered_candidates(xr, vocab, on)
        if roles[r] == "quantised" and A.size > 1:
            # the k-th boundary inside a tie run: some k with equal logits at ranks k - 1 and k
            v = xr[A].astype(np.float64)
            ties = np.nonzero(v[:-1] == v[1:])[0][:MAX_TOP_K - 1]
            if ties.size:
                top_k[r] = int(g.choice(ties)) + 1
        K = A[: effective_k(int(top_k[r]), 0.5)]
        if K.size:
            top_p[r] = _choose_top_p(g, ratios(xr, K, float(T[r])), bool(first[r]))
        else:
            top_p[r] = 0.5
    return dict(logits=x, vocab=vocab, mask=mask, rows=rows, roles=roles, temperature=T, top_p=top_p, top_k=top_k,
                penalty=theta, history=hist)


def odd_ld(vocab: int) -> int:
    return vocab + 3 + (vocab % 2)  # odd, so the rows' addresses take every alignment mod 16 bytes


def kernel_cases():
    """(what, case) of every launch of tests/test_nucleus_kernel_gpu.py's oracle test: vocabularies
    1, 31, 33, 257, rows 1, 3, 64, ld = vocab and an odd ld, every role at row 0; a null mask, a shared
    mask row, H = 0 and H = 256."""
    n = len(ROLES)
    for vocab in (1, 31, 33, 257):
        for rows in (1, 3, 64):
            shifts = range(n) if rows == 1 else range(0, n, 3) if rows == 3 else (0,)
            for ld in (vocab, odd_ld(vocab)):
                for shift in shifts:
                    seed = 100000 * vocab + 1000 * rows + 10 * shift + (ld != vocab)
                    yield (f"V={vocab} ld={ld} rows={rows} shift={shift}",
                           make_case(rows, vocab, ld, seed, shift=shift))
        yield f"V={vocab} null mask", make_case(15, vocab, odd_ld(vocab), 77 + vocab, null_mask=True)
        yield f"V={vocab} shared mask", make_case(15, vocab, vocab, 78 + vocab, shared_mask=True, H=0)
        yield f"V={vocab} H=256", make_case(15, vocab, odd_ld(vocab), 79 + vocab, H=256)


def llama_case(ld: int, seed: int = 7, shift: int = 0):
    return make_case(2, LLAMA_VOCAB, ld, seed, shift=shift, spread=6.0)


def launch(case, dev):
    """ops.nucleus_step on the case's tensors on ``dev`` ("cpu": the reference op).  mask_out is a
    window of a canary-filled buffer (a guard row before and after, one more word per row than the
    vocabulary needs -- the kernel must zero it -- and two canary words after each row), n_kept a
    window between two canaries.  Returns numpy (mask buffer, n_kept buffer, logits after)."""
    import torch

    import voice_enabled_browser_automation_amd.ops as ops

    rows, V = case["rows"], case["vocab"]
    words = (V + 31) // 32
    t = lambda a: torch.from_numpy(a.copy()).to(dev)  # noqa: E731
    x = t(case["logits"])
    mask = None if case["mask"] is None else t(case["mask"])
    buf = torch.full((rows + 2, words + 3), CANARY, dtype=torch.int32, device=dev)
    nk = torch.full((rows + 2,), CANARY, dtype=torch.int32, device=dev)
    got = ops.nucleus_step(x[:rows], mask, buf[1:rows + 1, :words + 1], nk[1:rows + 1], t(case["temperature"]),
                           t(case["top_p"]), t(case["top_k"]), t(case["penalty"]), t(case["history"]), vocab=V)
    assert got.data_ptr() == buf[1:rows + 1].data_ptr()
    return buf.cpu().numpy(), nk.cpu().numpy(), x.cpu().numpy()


def check_trace_step(tr, vocab: int) -> bool:
    """One traced step of a summary request (LLMIntentEngine.keep_summary_trace) against the oracle:
    the record's pre-penalty logits row, mask_in, parameters and history go through ``reference``;
    the engine's mask_out and n_kept must equal the oracle's bit for bit and the sampled token must be
    kept.  These rows are a model's, not the generator's, so a ratio may fall within DELTA of top_p:
    f32 may then decide the cut either way (the derivation at the top), and the row is held to one
    of the two cuts around that ratio instead -- never skipped.  Returns whether it was such a row."""
    x = tr["logits"].numpy()[None, :vocab].copy()
    words = (vocab + 31) // 32
    case = dict(rows=1, vocab=vocab, logits=x, mask=tr["mask_in"].numpy()[None, :words].copy(),
                temperature=np.array([tr["temperature"]], np.float32), top_p=np.array([tr["top_p"]], np.float32),
                top_k=np.array([tr["top_k"]], np.int32), penalty=np.array([tr["penalty"]], np.float32),
                history=tr["history"].numpy()[None].copy())
    _, want, n, closest = reference(case)
    got = tr["mask_out"].numpy()
    assert not got[words:].any(), "words past the vocabulary are set"
    kept = np.nonzero(allowed(got[:words].copy(), vocab))[0]
    assert tr["n_kept"] == kept.size >= 1 and tr["token"] in kept, (tr["step"], tr["n_kept"], tr["token"])
    if closest > DELTA:
        assert tr["n_kept"] == n[0] and np.array_equal(got[:words], want[0]), \
            f"step {tr['step']}: kept {kept.size}, the oracle {n[0]} (closest ratio {closest:.3g} from top_p)"
        return False
    xr = penalise(x[0], vocab, case["history"][0], case["penalty"][0])
    K = ordered_candidates(xr, vocab, allowed(case["mask"][0], vocab))[: effective_k(tr["top_k"], tr["top_p"])]
    assert abs(kept.size - int(n[0])) <= 1 and set(kept) == set(K[: kept.size]), f"step {tr['step']}: ambiguous row"
    return True


def check(case, got, what: str = ""):
    """The launch's outputs against the oracle, all bit for bit: the penalised logits (padding columns
    and the guard row untouched), the mask rows with their zeroed tail word, n_kept, the canaries.
    Returns (rows narrowed, the smallest |ratio - top_p| met)."""
    rows, V = case["rows"], case["vocab"]
    words = (V + 31) // 32
    buf, nk, x = got
    want_x, want_mask, want_n, closest = reference(case)
    assert closest > DELTA, f"{what}: a ratio within DELTA of top_p ({closest:.3g}): the generator let it through"
    full = case["logits"].copy()
    full[:rows] = want_x
    bad = np.nonzero(x.view(np.int32) != full.view(np.int32))
    assert not bad[0].size, f"{what}: logits differ at (row, col) {list(zip(*bad))[:4]}"
    assert (buf[0] == CANARY).all() and (buf[rows + 1] == CANARY).all(), f"{what}: a guard row of mask_out was written"
    assert (buf[:, words + 1:] == CANARY).all(), f"{what}: the words after a mask_out row were written"
    assert nk[0] == CANARY and nk[rows + 1] == CANARY, f"{what}: n_kept was written outside its rows"
    narrowed = 0
    for r in range(rows):
        tag = f"{what} row {r} ({case['roles'][r]}, k={case['top_k'][r]}, p={case['top_p'][r]}, T={case['temperature'][r]})"
        assert buf[r + 1, words] == 0, f"{tag}: the trailing word is {buf[r + 1, words]:#x}, not 0"
        assert nk[r + 1] == want_n[r], f"{tag}: n_kept {nk[r + 1]}, not {want_n[r]}"
        assert np.array_equal(buf[r + 1, :words], want_mask[r]), \
            f"{tag}: kept {np.nonzero(allowed(buf[r + 1, :words].copy(), V))[0][:8]}.., want " \
            f"{np.nonzero(allowed(want_mask[r], V))[0][:8]}.."
        narrowed += not passes_through(float(case["temperature"][r]), int(case["top_k"][r]), float(case["top_p"][r]))
    return narrowed, closest
