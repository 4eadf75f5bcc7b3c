"""The timestamp rules kernel (csrc/tsrules) against the f64 oracle (tsrules_oracle.py) on the GPU,
strict native mode.  Rows of every state class on the real vocabulary layout and on a tiny one, with
disabled rows, tokens outside the vocabulary and corrupt states among them; shared and per-row
masks; the state stepped in place and out of place; applied from the state and advanced by a token.
Every row is built with |T - M| above tau (tsrules_cases.tau: derived, not fitted), where the output
must equal the oracle's bit for bit; sentinels around the logits and the states must come back
unchanged.  A separate case holds rows built at T - M ~ 0, where either outcome of rule 5 is right."""
import numpy as np
import pytest
import torch

import tsrules_cases as tc
import tsrules_oracle as to
import voice_enabled_browser_automation_amd.ops as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 2  # sentinel rows after the logits' and the states' rows
SENT = 777.0
STATE_SENT = -12345


def build(lay, rows: int, seed: int, shared_rows: int):
    """One input set of ``rows`` rows: histories cycling through the state classes (offset by the
    seed), per-row masks, logits on the targets under those masks, and which rows are disabled, get a
    token outside the vocabulary, or carry a corrupt state.  The oracle's rows are computed once, for
    the per-row masks and -- its first ``shared_rows`` rows -- for the shared one (row 0's), and
    shared by every launch form."""
    rng = np.random.default_rng(seed)
    hs = tc.histories(lay)
    hists = [list(hs[(seed + r) % len(hs)]) for r in range(rows)]
    corrupt = [rows > 1 and r % 11 == 4 for r in range(rows)]
    hists = [[] if c else h for h, c in zip(hists, corrupt)]  # a corrupt state reads as the initial one
    mask = tc.masks(lay, rows, rng)
    case = dict(lay=lay, rows=rows, hists=hists, corrupt=corrupt, mask=mask,
                disabled=[rows > 1 and r % 7 == 3 for r in range(rows)],
                bad_tok=[rows > 1 and r % 9 == 5 for r in range(rows)])
    for shared in (False, True):
        m = mask[:1] if shared else mask
        n = shared_rows if shared else rows
        x = tc.rows_on_targets(lay, hists[:n], m, rng)
        want, margins = zip(*(tc.expect_row(x[r], hists[r], lay, m[0 if shared else r]) for r in range(n)))
        t = tc.tau(lay)
        assert all(mg > t for mg in margins), "an input row does not clear tau"
        case[shared] = dict(x=x, want=np.stack(want), mask=m)
    return case


_CASES = {}


def case_for(name: str, rows: int):
    """The largest set is built once per layout; fewer rows are its first rows (rows are independent)."""
    if name not in _CASES:
        # (the real layout's oracle rows cost 40 ms each: the shared mask is run with 1 and 5 rows there)
        _CASES[name] = build(tc.REAL, 64, 7, 5) if name == "real" else build(tc.TINY, 64, 11, 64)
    c = _CASES[name]
    out = dict(lay=c["lay"], rows=rows)
    for k in ("hists", "corrupt", "disabled", "bad_tok"):
        out[k] = c[k][:rows]
    for shared in (False, True):
        d = c[shared]
        out[shared] = dict(x=d["x"][:rows], want=d["want"][:rows], mask=d["mask"][: 1 if shared else rows])
    return out


def run(c, shared: bool, in_place: bool, advance: bool):
    """One launch; returns (logits out [rows + PAD, ld], state out, expected logits, expected state)."""
    lay, rows = c["lay"], c["rows"]
    V, tsb, ld = lay["V"], lay["tsb"], lay["ld"]
    n_ts = V - tsb
    d = c[shared]
    x = np.full((rows + PAD, ld), SENT, dtype=np.float32)
    x[:rows] = d["x"]
    want = x.copy()
    state_in = np.full((rows + PAD, 4), STATE_SENT, dtype=np.int32)
    state_want = np.full((rows + PAD, 4), STATE_SENT, dtype=np.int32)
    tokens = np.full(rows + PAD, -1, dtype=np.int32)
    enable = np.ones(rows, dtype=np.int32)
    for r in range(rows):
        h = c["hists"][r]
        moved = advance and len(h) > 0 and not c["bad_tok"][r]
        before = h[:-1] if moved else h
        st = to.state_of(before, tsb)
        if c["corrupt"][r]:  # (its history is empty: the oracle starts from nothing)
            st = [7, 3, 9, 2] if r % 2 else [1, 3, 9, n_ts]
        state_in[r] = st
        if moved:
            tokens[r] = h[-1]
        elif advance:  # no token to move on by, or a bad one: the row must be left alone
            tokens[r] = V + r if r % 2 else -1 - r
        if c["disabled"][r]:
            enable[r] = 0 if r % 2 else -3
        if c["disabled"][r] or (advance and not moved):
            state_want[r] = state_in[r]
        else:
            want[r] = d["want"][r]
            state_want[r] = to.state_of(h, tsb)
    if in_place:
        state_want[rows:] = STATE_SENT
    dx = torch.from_numpy(x).to(DEV)
    s_in = torch.from_numpy(state_in).to(DEV)
    s_out = s_in if in_place else torch.full_like(s_in, STATE_SENT)
    ops.ts_rules_step(dx[:rows], V, lay["eot"], tsb, lay["max_initial"], torch.from_numpy(d["mask"]).to(DEV),
                      torch.from_numpy(enable).to(DEV), s_in[:rows], s_out[:rows],
                      tokens=torch.from_numpy(tokens).to(DEV)[:rows] if advance else None)
    if not in_place:
        assert (s_in.cpu().numpy() == state_in).all(), "state_in was written"
    return dx.cpu().numpy(), s_out.cpu().numpy(), want, state_want


@pytest.mark.parametrize("rows", [1, 5, 64])
@pytest.mark.parametrize("name", ["real", "tiny"])
def test_every_state_class_matches_the_oracle_bit_for_bit(name, rows):
    assert ops.knob("VWA_STRICT_NATIVE")
    ops.ts_rules_ext()  # fail loudly if the library is missing
    c = case_for(name, rows)
    forms = [(s, p, a) for s in (False, True) for p in (False, True) for a in (False, True)]
    if name == "real" and rows == 64:
        forms = [f for f in forms if not f[0]]
    for shared, in_place, advance in forms:
        got, state, want, state_want = run(c, shared, in_place, advance)
        bad = [r for r in range(rows + PAD) if not tc.bits_equal(got[r], want[r])]
        assert not bad, f"rows {bad} differ (shared={shared} in_place={in_place} advance={advance})"
        assert (state == state_want).all(), f"states differ (shared={shared} in_place={in_place} advance={advance})"


@pytest.mark.parametrize("name", ["real", "tiny"])
def test_rows_built_at_a_tie_take_one_of_the_two_outcomes_and_touch_nothing_else(name):
    lay = tc.REAL if name == "real" else tc.TINY
    V, tsb, ld = lay["V"], lay["tsb"], lay["ld"]
    rng = np.random.default_rng(5)
    k = (V - tsb) // 2
    # (the closing row sits on an even row: those masks allow EOT, its only text)
    hists = [[tsb, 5, 17], [tsb, 5, tsb + k, tsb + k, 9], [tsb, 5, tsb + 1], [tsb + k, 3]]
    rows = len(hists)
    mask = tc.masks(lay, rows, rng)
    x = np.full((rows + PAD, ld), SENT, dtype=np.float32)
    x[:rows] = tc.rows_on_targets(lay, hists, mask, rng, targets=(0.0,))
    args = [(hists[r], V, lay["eot"], tsb, lay["max_initial"], mask[r]) for r in range(rows)]
    # (every row has both sides: the tie is a real one, within f32 rounding of the shift)
    assert all(to.margin(x[r].tolist(), *args[r]) < 1e-5 for r in range(rows))
    dx = torch.from_numpy(x).to(DEV)
    state = torch.tensor([to.state_of(h, tsb) for h in hists], dtype=torch.int32, device=DEV)
    ops.ts_rules_step(dx[:rows], V, lay["eot"], tsb, lay["max_initial"], torch.from_numpy(mask).to(DEV),
                      torch.ones(rows, dtype=torch.int32, device=DEV), state, state)
    got = dx.cpu().numpy()
    for r in range(rows):
        one = np.array(to.apply(x[r].tolist(), *args[r]), dtype=np.float32)
        other = np.array(to.other_outcome(x[r].tolist(), *args[r]), dtype=np.float32)
        assert not tc.bits_equal(one, other)
        assert tc.bits_equal(got[r], one) or tc.bits_equal(got[r], other), f"row {r} is neither outcome"
    assert tc.bits_equal(got[rows:], x[rows:])
    assert state.cpu().tolist() == [to.state_of(h, tsb) for h in hists]
