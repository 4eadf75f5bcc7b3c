"""Inputs and per-case checks of the beam ops, shared by the CPU tests (the torch references) and the
GPU tests (the gfx950 kernels): the same properties are asked of both."""
import numpy as np
import torch

import beam_oracle as bo
import voice_enabled_browser_automation_amd.ops as ops

PAD = 1e30        # the logits' padding columns: a column >= vocab read into a result shows at once
SENTINEL = -7.0   # outputs are pre-filled: what a call must not write stays
MASKS = ("text", "text_eot", "half_one", "half_rows")
CUMS = ("first", "random", "dead")
GW = ((1, 2), (1, 5), (3, 5), (8, 8), (1, 8))


def pack(bits: np.ndarray) -> torch.Tensor:
    """bool [rows, n] -> packed int32 [rows, ceil(n / 32)] (bit v % 32 of word v / 32)."""
    rows, n = bits.shape
    b = np.zeros((rows, (n + 31) // 32 * 32), dtype=np.uint8)
    b[:, :n] = bits
    return torch.from_numpy(np.packbits(b, axis=1, bitorder="little").view(np.uint32).view(np.int32).copy())


def eot_of(vocab: int) -> int:
    return 50257 if vocab > 50257 else vocab * 3 // 4


def make(vocab: int, G: int, W: int, mask_kind: str, cum_kind: str, seed: int, scale: float = 3.0):
    """(logits [G W, ld] with PAD beyond vocab, cum, mask) on the host."""
    g = torch.Generator().manual_seed(seed)
    N = G * W
    ld = (vocab + 63) // 64 * 64 + 64
    x = torch.full((N, ld), PAD, dtype=torch.float32)
    x[:, :vocab] = torch.randn(N, vocab, generator=g) * scale
    eot = eot_of(vocab)
    ids = np.arange(vocab)
    if mask_kind == "text":
        bits = (ids < eot)[None]
    elif mask_kind == "text_eot":
        bits = (ids <= eot)[None]
    else:
        rows = 1 if mask_kind == "half_one" else N
        bits = torch.rand(rows, vocab, generator=g).numpy() < 0.5
    if cum_kind == "first":
        cum = torch.full((N,), float("-inf"))
        cum[::W] = 0.0
    else:
        cum = -torch.rand(N, generator=g) * 5
        if cum_kind == "dead":
            cum[W // 2 :: W] = float("-inf")
    return x, cum, pack(np.ascontiguousarray(bits))


def run_select(x, cum, mask, vocab, W, dev):
    """ops.beam_select on ``dev`` into sentinel-filled outputs one row and three columns larger than
    the call's; checks that the surplus is untouched and returns the written region on the host."""
    G, K = x.shape[0] // W, 2 * W
    outs = [torch.full((G + 1, K + 3), SENTINEL, dtype=dt, device=dev) for dt in (torch.float32, torch.int32, torch.int32)]
    ops.beam_select(x.to(dev), cum.to(dev), None if mask is None else mask.to(dev), vocab, W,
                    cand_score=outs[0], cand_beam=outs[1], cand_tok=outs[2])
    h = [o.cpu() for o in outs]
    for o in h:
        assert (o[G:] == SENTINEL).all() and (o[:, K:] == SENTINEL).all(), "beam_select wrote outside [G, K]"
    return tuple(o[:G, :K] for o in h)


def check_case(vocab, G, W, mask_kind, cum_kind, seed, dev, scale=3.0):
    x, cum, mask = make(vocab, G, W, mask_kind, cum_kind, seed, scale)
    ref = bo.select64(x, cum, mask, vocab, W)
    what = f"V{vocab} G{G} W{W} {mask_kind} {cum_kind}"
    assert bo.near_ties(ref) == 0, f"{what} seed {seed}: the oracle itself has a near-tie; choose another seed"
    got = run_select(x, cum, mask, vocab, W, dev)
    assert bo.check_select(got, ref, what) == 0
    return got, ref


# ---------------------------------------------------------------- edge cases
def edge_equal_logits_pick_the_lower_id(dev):
    V, W = 40, 2
    x = torch.full((2, 64), PAD)
    x[:, :V] = 0.0
    x[1, :V] = -1.0
    s, b, t = run_select(x, torch.zeros(2), None, V, W, dev)
    assert b[0].tolist() == [0, 0, 0, 0] and t[0].tolist() == [0, 1, 2, 3]
    assert (s[0] == s[0, 0]).all() and abs(float(s[0, 0]) + np.log(V)) < 1e-5


def edge_identical_rows_pick_the_lower_beam(dev):
    V, W = 200, 3
    x = torch.full((3, 256), PAD)
    row = torch.randn(V, generator=torch.Generator().manual_seed(5)) * 3
    order = torch.argsort(row, descending=True)
    row[order[1]] = row[order[0]]  # the two best ids of a row tie as well
    x[:, :V] = row
    s, b, t = run_select(x, torch.full((3,), -1.5), None, V, W, dev)
    lo, hi = sorted(int(i) for i in order[:2])
    assert b[0].tolist() == [0, 0, 1, 1, 2, 2] and t[0].tolist() == [lo, hi] * 3
    assert (s[0] == s[0, 0]).all()


def edge_row_maximum_on_a_masked_id(dev):
    V, G, W = 200, 2, 3
    x, cum, _ = make(V, G, W, "text", "random", 11)
    bits = np.ones((1, V), dtype=bool)
    bits[0, 17] = False
    x[:, 17] = 100.0  # far above everything allowed: it must neither win nor enter the lse
    ref = bo.select64(x, cum, pack(bits), V, W)
    assert bo.near_ties(ref) == 0
    got = run_select(x, cum, pack(bits), V, W, dev)
    assert bo.check_select(got, ref, "masked maximum") == 0
    assert not (got[2] == 17).any() and float(got[0].max()) > -20.0


def edge_row_maximum_on_the_padding(dev):
    V, W = 40, 2
    x, cum, mask = make(V, 1, W, "half_one", "random", 12)
    assert float(x[0, V]) > 1e29  # (PAD in f32) the row's largest value sits at id vocab
    got = run_select(x, cum, mask, V, W, dev)
    assert bo.check_select(got, bo.select64(x, cum, mask, V, W), "padding maximum") == 0
    assert np.isfinite(got[0].numpy()).all() and int(got[2].max()) < V


def edge_logits_times_fifty_stay_finite(dev):
    for V, G, W, seed in ((51865, 1, 5, 21), (200, 3, 5, 22)):
        got, _ = check_case(V, G, W, "text_eot", "random", seed, dev, scale=150.0)
        assert np.isfinite(got[0].numpy()).all()
    # +-600 outright
    V, W = 200, 2
    x = torch.full((2, 256), PAD)
    x[:, :V] = -600.0
    x[0, 3] = x[1, 9] = 600.0
    x[0, 5] = 599.0
    s, b, t = run_select(x, torch.tensor([0.0, -0.5]), None, V, W, dev)
    assert (b[0, :3].tolist(), t[0, :3].tolist()) == ([0, 1, 0], [3, 9, 5])
    assert np.isfinite(s.numpy()).all() and abs(float(s[0, 3]) + 1200.0) < 2.0


def edge_minus_infinity_entries_never_appear(dev):
    V, G, W = 200, 2, 3
    x, cum, mask = make(V, G, W, "text_eot", "random", 31)
    hole = torch.rand(G * W, V, generator=torch.Generator().manual_seed(32)) < 0.97
    x[:, :V][hole] = float("-inf")  # few finite entries: the groups' lists reach into them
    x[0, :V] = float("-inf")        # a row with nothing at all
    ref = bo.select64(x, cum, mask, V, W)
    got = run_select(x, cum, mask, V, W, dev)
    bo.check_select(got, ref, "-inf entries")
    s, b, t = got
    for g in range(G):
        for k in range(2 * W):
            if int(b[g, k]) >= 0:
                assert np.isfinite(float(x[g * W + int(b[g, k]), int(t[g, k])])) and np.isfinite(float(s[g, k]))
                assert (g, int(b[g, k])) != (0, 0)


def edge_fewer_than_k_candidates_leave_the_tail(dev):
    V, W = 51866, 4
    x, cum, _ = make(V, 2, W, "text", "first", 41)
    bits = np.zeros((1, V), dtype=bool)
    bits[0, [7, 20000, 51865]] = True
    s, b, t = run_select(x, cum, pack(bits), V, W, dev)
    for g in range(2):
        assert b[g].tolist() == [0, 0, 0] + [-1] * 5 and t[g, 3:].tolist() == [-1] * 5
        assert sorted(t[g, :3].tolist()) == [7, 20000, 51865]
        assert (s[g, 3:] == float("-inf")).all() and np.isfinite(s[g, :3].numpy()).all()
    # every row dead: nothing but the tail
    s, b, t = run_select(x, torch.full_like(cum, float("-inf")), None, V, W, dev)
    assert (b == -1).all() and (t == -1).all() and (s == float("-inf")).all()


EDGES = [edge_equal_logits_pick_the_lower_id, edge_identical_rows_pick_the_lower_beam,
         edge_row_maximum_on_a_masked_id, edge_row_maximum_on_the_padding, edge_logits_times_fifty_stay_finite,
         edge_minus_infinity_entries_never_appear, edge_fewer_than_k_candidates_leave_the_tail]


# ---------------------------------------------------------------- kv_beam_gather
KV = dict(L=2, H=3, bs=16, hd=64, sessions=8, bps=4)
PARENTS = {
    2: {"zero": [0, 0], "swap": [1, 0], "mixed": [1, 1], "identity": [0, 1]},
    5: {"zero": [0] * 5, "swap": [1, 0, 2, 3, 4], "mixed": [1, 0, 0, 3, 1], "identity": list(range(5))},
    8: {"zero": [0] * 8, "swap": [0, 1, 6, 3, 4, 5, 2, 7], "mixed": [1, 0, 0, 3, 1, 7, 5, 5], "identity": list(range(8))},
}
SLOTS = {2: [[5, 2], [7, 0]], 5: [[6, 1, 7, 3, 0]], 8: [[3, 7, 0, 5, 1, 6, 2, 4]]}  # out of order, not contiguous


def kv_caches(seed: int):
    """(k_cache, v_cache) of random bit patterns and a shuffled block table, on the host."""
    g = torch.Generator().manual_seed(seed)
    n_blocks = KV["sessions"] * KV["bps"] + 1
    shape = (KV["L"], n_blocks, KV["H"], KV["bs"], KV["hd"])
    k, v = (torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
            for _ in range(2))
    table = (1 + torch.randperm(n_blocks - 1, generator=g)).to(torch.int32).view(KV["sessions"], KV["bps"])
    return k, v, table


def kv_expected(cache16, table, slots, parents, n_ctx):
    """The permutation on the int16 view, from the contract alone."""
    want = cache16.clone()
    for g, (srow, prow) in enumerate(zip(slots, parents)):
        for w, p in enumerate(prow):
            for j in range(-(-n_ctx[g] // KV["bs"])):
                want[:, int(table[srow[w], j])] = cache16[:, int(table[srow[p], j])]
    return want


def check_gather(W: int, kind: str, n_ctx: int, dev, seed: int = 3):
    k, v, table = kv_caches(seed)
    slots = SLOTS[W]
    G = len(slots)
    parents = [PARENTS[W][kind]] + [PARENTS[W]["swap"]] * (G - 1)   # the second group differs
    ctx = [n_ctx] + [17] * (G - 1)
    kd, vd = k.clone().to(dev), v.clone().to(dev)  # (to("cpu") is no copy)
    ops.kv_beam_gather(kd, vd, table.to(dev), slots, parents, ctx)
    for name, got, before in (("k", kd, k), ("v", vd, v)):
        want = kv_expected(before.view(torch.int16), table, slots, parents, ctx)
        diff = (got.cpu().view(torch.int16) != want)
        assert not diff.any(), f"{name}_cache W{W} {kind} n_ctx {n_ctx}: {int(diff.sum())} elements differ " \
                               f"(blocks {sorted(set(diff.nonzero()[:, 1].tolist()))[:8]})"
        if kind == "identity" and G == 1:
            assert torch.equal(got.cpu().view(torch.int16), before.view(torch.int16))


# ---------------------------------------------------------------- engine scenarios (CPU and GPU)
def tone(seconds: float, f0: float) -> np.ndarray:
    t = np.arange(int(seconds * 16000)) / 16000
    return (np.sin(2 * np.pi * f0 * t) * 9000).astype(np.int16)


TONES = ((0.3, 220), (1.2, 330), (2.5, 500))


def check_trace(eng, audios, W: int, **kw):
    """decode_many with beams and ``keep_beam_trace``: every step's candidates against the oracle of
    that step's own kept logits and cum (so a legitimate divergence never propagates), the parents
    and tokens against the bookkeeping applied to the kept candidates, cum non-increasing across a
    group's live beams, and last_beams against the replayed states.  Returns (tokens, steps, steps
    in which the comparison rule excused a rank)."""
    from voice_enabled_browser_automation_amd.asr import beam as rule

    cfg = eng.model.cfg
    eng.keep_beam_trace = True
    try:
        outs = eng.decode_many(audios, beam_size=W, **kw)
        trace = eng.last_beam_trace
    finally:
        eng.keep_beam_trace = False
    n_max = kw["exact_tokens"] if kw.get("exact_tokens") is not None else kw.get("max_tokens", 96)
    cap = eng.runner.bps * eng.runner.bs
    states = [rule.BeamState(W, cfg.eot, min(n_max, cap - len(eng.prompt))) for _ in audios]
    masks = {False: eng.mask_text.cpu(), True: eng.mask_text_eot.cpu()}
    excused_steps = 0
    assert trace and [s["step"] for s in trace] == list(range(len(trace)))
    for s in trace:
        G = len(s["utts"])
        assert s["logits"].shape == (G * W, eng.model.vocab_padded)
        assert s["allow_eot"] == (kw.get("exact_tokens") is None and s["step"] >= kw.get("min_tokens", 0))
        cum = torch.tensor(s["cum"], dtype=torch.float32).reshape(-1)
        assert cum.tolist() == [c for j in s["utts"] for c in states[j].cum], "cum is not the replayed states'"
        for row in s["cum"]:
            assert all(a >= b for a, b in zip(row, row[1:])), f"cum increases across the live beams: {row}"
        ref = bo.select64(s["logits"], cum, masks[s["allow_eot"]], cfg.vocab_size, W)
        got = (s["cand_score"], s["cand_beam"], s["cand_tok"])
        excused_steps += bo.check_select(got, ref, f"step {s['step']}") > 0
        for g, j in enumerate(s["utts"]):
            cands = list(zip(got[0][g].tolist(), got[1][g].tolist(), got[2][g].tolist()))
            par, tok = rule.advance(states[j], cands)
            assert (par, tok) == (s["parents"][g], s["tokens"][g]), f"step {s['step']} utterance {j}"
    assert all(st.done for st in states)
    assert [rule.ranked(st) for st in states] == eng.last_beams
    assert outs == [h[0]["tokens"] for h in eng.last_beams]
    print(f"MEASURED beam trace W{W}: {len(trace)} steps, {excused_steps} with an excused rank")
    return outs, len(trace), excused_steps


def check_invariants(eng, n_utts: int, W: int, *, max_tokens: int, exact=None):
    cfg = eng.model.cfg
    assert len(eng.last_beams) == n_utts
    for hyps in eng.last_beams:
        assert 1 <= len(hyps) <= W
        assert len({tuple(h["tokens"]) for h in hyps}) == len(hyps), "hypotheses repeat"
        avg = [h["avg_logprob"] for h in hyps]
        assert avg == sorted(avg, reverse=True)
        for h in hyps:
            assert all(0 <= t < cfg.eot for t in h["tokens"]) and len(h["tokens"]) <= max_tokens
            assert h["sum_logprob"] <= 0.0
            n = len(h["tokens"]) + (0 if exact is not None or len(h["tokens"]) == max_tokens else 1)
            assert abs(h["avg_logprob"] - h["sum_logprob"] / n) < 1e-6
            if exact is not None:
                assert len(h["tokens"]) == exact
