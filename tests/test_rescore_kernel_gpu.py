"""The per-sequence log-probability's gfx950 kernels (csrc/rescore, ops.seq_logprob) against the f64
oracle of tests/rescore_oracle.py: every row within the bounds derived there, -inf exactly and never
NaN, the sums bit-equal to the f32 sum of the kernel's own rows in row order, canaries and the
logits untouched, and the same bits from run to run."""
import numpy as np
import pytest

import rescore_oracle as ro
import voice_enabled_browser_automation_amd.ops as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
NINF_ROLES = ("t_ninf", "t_nan", "t_vocab", "t_minus2", "row_ninf_id", "row_ninf_set")


@pytest.fixture(scope="module", autouse=True)
def lib():
    return ops.rescore_ext()  # fail loudly if the library is missing


def measured(name: str, value: float) -> None:
    print(f"MEASURED {name} {value:.6g}")


def run(case, what):
    got = ro.launch(case, DEV)
    worst = ro.check(case, got, what)
    lp = got[0]
    on = ro.allowed(case["end_set"], case["vocab"])
    for r, role in enumerate(case["roles"]):
        if role in NINF_ROLES or (case["target"][r] == -1 and not on.any()):
            assert lp[r] == -np.inf, f"{what} row {r}: {role} gave {lp[r]}"
        elif role == "far_below" and 0 < on.sum() < case["vocab"]:
            assert np.isfinite(lp[r]) and lp[r] < -150.0, f"{what} row {r}: far_below gave {lp[r]}"
    return worst


@pytest.mark.parametrize("rows", [1, 3, 64, 65, 256])
@pytest.mark.parametrize("vocab", [1, 5, 33, 2049])
def test_one_call_matches_the_oracle(vocab, rows):
    worst, launches = 0.0, ops.seq_logprob_launches
    combos = [(s, m, a) for s in ro.SEQ_MODES for m in ro.SET_MODES for a in (False, True)]
    # with few rows every role reaches row 0 by the shift; with many, one shift holds them all
    shifts = range(len(ro.ROLES)) if rows < len(ro.ROLES) else (0, 5)
    n = 0
    for shift in shifts:
        for k, (seq_mode, set_mode, acc) in enumerate(combos):
            if rows >= 64 and (k + shift) % 3:  # a third of the combinations at the large row counts
                continue
            case = ro.make_case(rows, vocab, seed=1000 * vocab + 10 * rows + shift, shift=shift, seq_mode=seq_mode,
                                set_mode=set_mode, acc=acc)
            worst = max(worst, run(case, f"V={vocab} rows={rows} shift={shift} {seq_mode} {set_mode} acc={acc}"))
            n += 1
    assert ops.seq_logprob_launches == launches + n
    measured(f"seq_logprob V={vocab} rows={rows} err/bound", worst)


@pytest.mark.parametrize("rows", [1, 3, 64, 65, 256])
def test_llama_vocabulary(rows):
    V = 128256
    # a sparse set, as the end set is (a few hundred ids of 128k)
    case = ro.make_case(rows, V, seed=7 + rows, shift=rows % 12, seq_mode="mixed", acc=True, spread=6.0,
                        density=0.004)
    measured(f"seq_logprob V={V} rows={rows} err/bound", run(case, f"V={V} rows={rows}"))


def test_every_role_at_the_llama_vocabulary_with_one_row():
    V = 128256
    worst = 0.0
    for shift in range(len(ro.ROLES)):
        case = ro.make_case(1, V, seed=100 + shift, shift=shift, seq_mode="own", acc=bool(shift % 2), spread=6.0)
        worst = max(worst, run(case, f"V={V} rows=1 shift={shift}"))
    case = ro.make_case(3, V, seed=99, shift=1, set_mode="empty", spread=6.0)
    worst = max(worst, run(case, f"V={V} rows=3 empty set"))
    measured(f"seq_logprob V={V} roles err/bound", worst)


def test_two_calls_give_the_same_bits():
    for vocab, rows in ((2049, 256), (128256, 3)):
        case = ro.make_case(rows, vocab, seed=11, spread=6.0)
        a, b = ro.launch(case, DEV), ro.launch(case, DEV)
        assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32))
        assert np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
