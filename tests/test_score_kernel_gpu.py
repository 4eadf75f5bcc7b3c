"""The score step's gfx950 kernel (csrc/score, ops.score_step) against the f64 oracle of
tests/score_oracle.py: log-probabilities and sums within the bound derived there, counts, rows left
alone, canaries and -inf exactly, and the same bits from run to run."""
import numpy as np
import pytest
import torch

import score_oracle as so
import voice_enabled_browser_automation_amd.ops as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def lib():
    return ops.score_ext()  # fail loudly if the library is missing


def measured(name: str, value: float) -> None:
    print(f"MEASURED {name} {value:.6g}")


def odd_ld(vocab: int) -> int:
    return vocab + 3 + (vocab % 2)  # odd, so the rows' addresses take every alignment mod 16 bytes


@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "per_row"])
@pytest.mark.parametrize("rows", [1, 3, 64])
@pytest.mark.parametrize("vocab", [1, 31, 33, 257])
def test_one_step_matches_the_oracle(vocab, rows, per_row):
    worst = 0.0
    for ld in (vocab, odd_ld(vocab)):
        for shift in range(len(so.ROLES)):  # (every role reaches a row, also with one row)
            case = so.make_case(rows, vocab, ld, per_row, seed=1000 * vocab + 10 * rows + shift, shift=shift)
            what = f"V={vocab} ld={ld} rows={rows} shift={shift}"
            worst = max(worst, so.check(case, so.launch(case, DEV), what))
            if shift == 0:
                so.check(case, so.launch(case, DEV, in_place=True, with_lp=False), what + " in place")
    measured(f"score_step V={vocab} rows={rows} {'per-row' if per_row else 'shared'} err/bound", worst)


def test_whisper_vocabulary_once():
    V = 51866
    worst = 0.0
    for ld, per_row in ((V, False), (odd_ld(V), True)):
        case = so.make_case(5, V, ld, per_row, seed=7, shift=0)
        worst = max(worst, so.check(case, so.launch(case, DEV), f"V={V} ld={ld}"))
    # logits of a trained model's scale, where every column counts
    case = so.make_case(3, V, V + 6, False, seed=8, spread=6.0)
    worst = max(worst, so.check(case, so.launch(case, DEV), "spread 6"))
    measured("score_step V=51866 err/bound", worst)


def test_two_launches_give_the_same_bits():
    for vocab, rows in ((257, 64), (51866, 3)):
        case = so.make_case(rows, vocab, odd_ld(vocab), True, seed=11)
        a, b = so.launch(case, DEV), so.launch(case, DEV)
        for p, q in zip(a[:3], b[:3]):
            assert np.array_equal(p.view(np.int32), q.view(np.int32))


def test_ten_chained_steps_freeze_at_eot_and_stay_within_the_bound():
    """Ten steps in place (sum_out is sum_in): fresh logits and tokens each step; row 1 draws EOT at
    step 3 and row 2 at step 0 -- their states must not move afterwards; row 3 is disabled."""
    V, rows, ld, T = 257, 5, 260, 10
    g = np.random.default_rng(5)
    eot = 5
    bits = np.ones(V, dtype=bool)
    bits[V - 1] = False
    mask_np = so.pack(bits, (V + 31) // 32)[None]
    mask = torch.from_numpy(mask_np).to(DEV)
    enable_np = np.array([1, 1, 1, 0, 1], dtype=np.int32)
    enable = torch.from_numpy(enable_np).to(DEV)
    s = torch.zeros(rows, dtype=torch.float32, device=DEV)
    c = torch.zeros(rows, 2, dtype=torch.int32, device=DEV)
    lp = torch.zeros(rows, dtype=torch.float32, device=DEV)
    want_s, want_c = np.zeros(rows), np.zeros((rows, 2), dtype=np.int64)
    bound = np.zeros(rows)
    worst = 0.0
    for t in range(T):
        x_np = g.uniform(-80, 80, (rows, ld)).astype(np.float32)
        tok_np = g.integers(6, V - 1, rows).astype(np.int32)
        if t == 3:
            tok_np[1] = eot
        if t == 0:
            tok_np[2] = eot
        x = torch.from_numpy(x_np).to(DEV)
        ops.score_step(x, V, eot, mask, enable, torch.from_numpy(tok_np).to(DEV), s, s, c, c, step_lp=lp)
        want_s, want_c, w_lp, L, active = so.step(x_np, V, eot, mask_np, enable_np, tok_np, want_s, want_c)
        bound += np.where(active, so.lp_bound(V, L, w_lp) + so.U * np.abs(want_s), 0.0)
        got_lp = lp.cpu().numpy()
        assert (got_lp[~active] == 0.0).all()
        assert (np.abs(got_lp[active] - w_lp[active]) <= so.lp_bound(V, L, w_lp)[active]).all()
        assert np.array_equal(c.cpu().numpy(), want_c)
        err = np.abs(s.cpu().numpy().astype(np.float64) - want_s)
        assert (err[bound == 0] == 0).all() and (err <= bound).all(), (t, err, bound)
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    assert want_c.tolist() == [[T, 0], [4, 1], [1, 1], [0, 0], [T, 0]]
    measured("score_step ten chained steps err/bound", worst)
