"""Cases shared by the keyterm boosting tests (CPU references and GPU kernels run the same ones).

Keyterm sets over a 40-id vocabulary, chosen to collide: overlapping sequences, one a suffix of
another, the same sequence twice with different boosts, a 16-token term.  ``run_step`` runs
ops.boost_step on a device into sentinel-framed buffers and checks what must stay untouched;
``check_trace`` holds an engine's kept boosting trace to the brute-force oracle step by step."""
from typing import List, Optional, Sequence

import numpy as np
import torch

import boost_oracle as bo
import voice_enabled_browser_automation_amd.ops as ops
from voice_enabled_browser_automation_amd.asr import keyterms as kt

V, LD = 40, 48

COLLIDE = [([5, 6, 7], 1.5), ([6, 7, 8], 2.5), ([6], 0.75), ([5, 6, 9], 3.0)]
TWICE = [([3, 4], 1.0), ([3, 4], 4.0), ([4, 3], 2.0)]
SUFFIX = [([10, 11, 12, 13], 1.25), ([12, 13], 5.0), ([13], 0.5), ([11, 12, 14], 2.0)]
LONG = [(list(range(20, 36)), 6.0), ([21, 22], 1.0), ([34, 35, 20], 2.5)]
SETS = {"collide": COLLIDE, "twice": TWICE, "suffix": SUFFIX, "long": LONG}


def joint(names: Sequence[str] = ("collide", "twice", "suffix", "long")):
    """(compiled sets, bases, tables as numpy arrays) of several sets concatenated."""
    sets = [kt.compile_sequences(SETS[n], limit=V) for n in names]
    bases, *tables = kt.concat(sets)
    return sets, bases, tuple(tables)


def tables_on(tables, dev):
    return tuple(torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in tables)


def rand_logits(rows: int, ld: int, vocab: int, seed: int, pad_rows: int = 2) -> torch.Tensor:
    """f32 [rows + pad_rows, ld]: random below ``vocab`` in the first ``rows`` rows, SENTINEL elsewhere."""
    g = torch.Generator().manual_seed(seed)
    x = torch.full((rows + pad_rows, ld), bo.SENTINEL, dtype=torch.float32)
    x[:rows, :vocab] = torch.randn(rows, vocab, generator=g) * 3
    return x


def run_step(dev, tables, x: torch.Tensor, vocab: int, roots, state_in, tokens=None, parents=None, W: int = 1,
             in_place: bool = False, what: str = ""):
    """One ops.boost_step on ``dev`` against bo.table_step: logits bit for bit (the sentinel cells
    included: columns >= vocab and the rows past ``rows``), states exactly, and the state buffers'
    cells past ``rows`` untouched.  Returns (logits after, state_out) on the host."""
    rows = len(roots)
    i32 = dict(dtype=torch.int32)
    want_x, want_s = bo.table_step(tables, x, vocab, roots, state_in, tokens, parents, W)
    assert bo.bits_equal(want_x[rows:], x[rows:]) and bo.bits_equal(want_x[:, vocab:], x[:, vocab:])
    d_x = x.clone().to(dev)
    d_in = torch.full((rows + 3,), -99, **i32)
    d_in[:rows] = torch.tensor(list(state_in[:rows]), **i32)
    d_in = d_in.to(dev)
    d_out = d_in if in_place else torch.full((rows + 3,), -77, **i32).to(dev)
    kw = {}
    if tokens is not None:
        kw["tokens"] = torch.tensor(list(tokens), **i32).to(dev)
    if parents is not None:
        kw.update(parents=torch.tensor(list(parents), **i32).to(dev), W=W)
    ops.boost_step(d_x, vocab, tables_on(tables, dev), torch.tensor(list(roots), **i32).to(dev), d_in, d_out, **kw)
    got_x, got_s = d_x.cpu(), d_out.cpu()
    assert got_s[:rows].tolist() == want_s, f"{what}: states {got_s[:rows].tolist()} != {want_s}"
    assert got_s[rows:].tolist() == [-99 if in_place else -77] * 3, f"{what}: state cells past the rows were written"
    if not in_place:
        assert d_in.cpu()[:rows].tolist() == [int(s) for s in state_in[:rows]], f"{what}: state_in was written"
    bad = (got_x.view(torch.int32) != want_x.view(torch.int32)).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} logits differ from the table oracle, first at {bad[0].tolist()}"
    return got_x, got_s[:rows].tolist()


def seqs_of(ks) -> list:
    return [(list(q), b) for q, b in ks.key]


def check_trace(eng, trace: List[dict], beams: Optional[int] = None) -> int:
    """Every kept boosting launch of an engine call against the brute-force oracle: the state is the
    longest sequence prefix that is a suffix of the row's history, the logits after are the logits
    before plus bias(h, .) bit for bit (an unboosted row: unchanged), and -- greedy rows -- the chosen
    token is the masked argmax of the kept biased logits.  Returns the boosted rows checked."""
    cfg = eng.model.cfg
    checked = 0
    assert trace
    for n, s in enumerate(trace):
        rows = len(s["utts"])
        assert s["before"].shape == s["after"].shape == (rows, eng.model.vocab_padded)
        for r in range(rows):
            ks = s["sets"][r]
            if beams and not s["alive"][r]:
                continue  # (a dead beam's row has no history of its own)
            if ks is None:
                assert s["state"][r] == -1 and bo.bits_equal(s["before"][r], s["after"][r]), f"launch {n} row {r}"
            else:
                seqs, h = seqs_of(ks), s["history"][r]
                assert s["state"][r] == bo.path_states(ks, seqs)[bo.state_brute(seqs, h)], f"launch {n} row {r}: state"
                want = bo.boosted(s["before"][r], bo.bias_brute(seqs, h), cfg.vocab_size)
                assert bo.bits_equal(want, s["after"][r]), f"launch {n} row {r}: biased logits differ"
                checked += 1
            if not beams:
                assert s["tokens"][r] == bo.greedy_ref(s["after"][r], cfg.eot, s["allow_eot"]), f"launch {n} row {r}"
    return checked


def model_logits(eng, audio, histories: Sequence[Sequence[int]]) -> torch.Tensor:
    """The model's own (unbiased) next-token logits after each forced text history, [n, vocab_padded]
    on the host: one traced call of one token per history, boosted only by an unrelated one-id
    keyterm on the first row -- the trace keeps every row's logits before boosting."""
    cfg = eng.model.cfg
    keep, eng.keep_boost_trace = eng.keep_boost_trace, True
    try:
        dummy = kt.compile_sequences([([0], 1.0)], limit=cfg.eot)
        eng.decode_many([audio] * len(histories), [list(h) for h in histories], exact_tokens=1,
                        keyterms=[dummy] + [None] * (len(histories) - 1))
        return eng.last_boost_trace[0]["before"].clone()
    finally:
        eng.keep_boost_trace = keep


def pick_cycle(eng, audio, n: int = 4, total: int = 10) -> List[int]:
    """A keyterm q of ``n`` distinct ids that this model, under a huge boost, decodes as q q q ...

    bias is a maximum over matches, not a sum: with history ending inside q, the continuation q[k]
    and the restart q[0] (k = 0 always qualifies) carry the SAME boost, and the model's own logits
    decide between them.  So q is built from the model: q[0] is an id it ranks low after the bare
    prompt, and q[k] is the id it ranks highest after q[:k] (q's ids excluded).  That the
    continuation then beats the restart at every step of (q * 3)[:total] is asserted here from the
    model's unbiased logits -- a precondition of the test's inputs, not a property of the boosting."""
    cfg = eng.model.cfg
    first = model_logits(eng, audio, [[]])[0][: cfg.eot]
    q = [int(torch.argsort(first.double())[cfg.eot // 50])]
    while len(q) < n:
        row = model_logits(eng, audio, [q])[0][: cfg.eot].clone()
        row[q] = float("-inf")
        q.append(int(torch.argmax(row.double())))
    want = (q * ((total + n - 1) // n + 1))[:total]
    rows = model_logits(eng, audio, [want[:t] for t in range(total)])
    for t in range(total):
        if want[t] != q[0]:
            # (beyond one ulp at the boost the tests use: the f32 add must not merge the two)
            assert float(rows[t][want[t]]) > float(rows[t][q[0]]) + 0.01, f"step {t}: the model prefers restarting {q}"
    return q
