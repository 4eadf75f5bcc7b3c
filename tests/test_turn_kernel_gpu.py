"""The set log-probability's gfx950 kernel (csrc/turn, ops.set_logprob) against the f64 oracle of
tests/turn_oracle.py: both outputs within the bounds derived there, -inf exactly and never NaN,
canaries and the logits untouched, and the same bits from run to run."""
import numpy as np
import pytest

import turn_oracle as to
import voice_enabled_browser_automation_amd.ops as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def lib():
    return ops.turn_ext()  # fail loudly if the library is missing


def measured(name: str, value: float) -> None:
    print(f"MEASURED {name} {value:.6g}")


def odd_ld(vocab: int) -> int:
    return vocab + 3 + (vocab % 2)  # odd, so the rows' addresses take every alignment mod 16 bytes


@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "per_row"])
@pytest.mark.parametrize("rows", [1, 3, 64])
@pytest.mark.parametrize("vocab", [1, 31, 33, 257])
def test_one_launch_matches_the_oracle(vocab, rows, per_row):
    worst = 0.0
    for ld in (vocab, odd_ld(vocab)):
        for shift in range(len(to.ROLES)):  # (every role reaches row 0, also with one row)
            case = to.make_case(rows, vocab, ld, per_row, seed=1000 * vocab + 10 * rows + shift, shift=shift)
            what = f"V={vocab} ld={ld} rows={rows} shift={shift}"
            got = to.launch(case, DEV)
            worst = max(worst, to.check(case, got, what))
            lp0 = float(got[0][0, 0])
            role = case["roles"][0]
            if role in ("empty", "set_ninf", "row_ninf"):
                assert lp0 == -np.inf, f"{what}: {role} gave {lp0}"
            elif role == "full":
                assert -to.lp_bound(vocab, float(got[0][0, 1]), 0.0) <= lp0 <= 0.0, f"{what}: full set gave {lp0}"
            elif role == "far_below" and 0 < to.allowed(case["sets"][0], vocab).sum() < vocab:
                assert np.isfinite(lp0) and lp0 < -150.0, f"{what}: far_below gave {lp0}"
    measured(f"set_logprob V={vocab} rows={rows} {'per-row' if per_row else 'shared'} err/bound", worst)


def test_llama_vocabulary_once():
    V = 128256
    worst = 0.0
    for ld, per_row in ((V, False), (odd_ld(V), True)):
        case = to.make_case(2, V, ld, per_row, seed=7, shift=5, spread=6.0)  # (far_below, some_ninf)
        worst = max(worst, to.check(case, to.launch(case, DEV), f"V={V} ld={ld}"))
        # a sparse set, as the end set is (a few hundred ids of 128k), on plain rows
        g = np.random.default_rng(9)
        case = to.make_case(2, V, ld, per_row, seed=8, shift=0, spread=6.0)
        case["logits"][:2, :V] = g.uniform(-6.0, 6.0, (2, V)).astype(np.float32)
        bits = g.random((2 if per_row else 1, V)) < 0.004
        case["sets"] = np.stack([to.pack(b, (V + 31) // 32, fill=g) for b in bits])
        case["roles"] = ["sparse", "sparse"]
        worst = max(worst, to.check(case, to.launch(case, DEV), f"V={V} ld={ld} sparse"))
    measured("set_logprob V=128256 err/bound", worst)


def test_two_launches_give_the_same_bits():
    for vocab, rows in ((257, 64), (128256, 2)):
        case = to.make_case(rows, vocab, odd_ld(vocab), True, seed=11, spread=6.0)
        a, b = to.launch(case, DEV), to.launch(case, DEV)
        assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32))
