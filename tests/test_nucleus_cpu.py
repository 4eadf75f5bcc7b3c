"""The nucleus step's case generator and its CPU reference op (ops.nucleus_step on host tensors)
against the f64 oracle of tests/nucleus_oracle.py.  The generator must leave no case ambiguous: for
every launch the GPU test will draw, no ratio c_j / C lies within DELTA of the row's top_p.  On those
cases the reference op equals the oracle bit for bit."""
import numpy as np
import pytest
import torch

import nucleus_oracle as no
import voice_enabled_browser_automation_amd.ops as ops


@pytest.fixture(scope="module")
def cases():
    return list(no.kernel_cases())


def test_delta_is_what_the_derivation_gives():
    assert no.DELTA == (2 * (2 * 104 + 4 + 1023) + 1) * 2.0 ** -24 * 1.001
    assert 1.4e-4 < no.DELTA < 1.5e-4 and 2 * no.DELTA < 1.0 / no.MAX_TOP_K  # an all-equal row always has a gap


def test_no_generated_case_is_ambiguous(cases):
    closest, narrowed, roles0 = np.inf, 0, set()
    for what, case in cases:
        _, _, n_kept, c = no.reference(case)
        assert c > no.DELTA, f"{what}: a ratio {c:.3g} from top_p"
        closest = min(closest, c)
        roles0.add(case["roles"][0])
        narrowed += sum(not no.passes_through(float(t), int(k), float(p))
                        for t, k, p in zip(case["temperature"], case["top_k"], case["top_p"]))
    assert roles0 == set(no.ROLES), "every role reaches row 0"
    assert narrowed > 500
    print(f"MEASURED nucleus cases {len(cases)} narrowed rows {narrowed} closest ratio {closest:.3g} "
          f"(DELTA {no.DELTA:.3g})")


def test_the_llama_cases_are_unambiguous():
    for ld in (no.LLAMA_VOCAB, no.odd_ld(no.LLAMA_VOCAB)):
        for shift in (0, 1):
            assert no.reference(no.llama_case(ld, shift=shift))[3] > no.DELTA


def test_the_roles_do_what_they_say():
    case = no.make_case(15, 257, 257, seed=5)
    _, mask, n, _ = no.reference(case)
    role = {name: r for r, name in enumerate(case["roles"])}
    on = lambda r: no.allowed(case["mask"][r], 257)  # noqa: E731
    assert n[role["all_equal"]] >= 1
    kept = np.nonzero(no.allowed(mask[role["all_equal"]], 257))[0]
    assert np.array_equal(kept, np.nonzero(on(role["all_equal"]))[0][:len(kept)]), "ties are filled by id"
    assert n[role["empty_mask"]] == 0 and not mask[role["empty_mask"]].any()
    assert n[role["few_allowed"]] <= 3
    assert n[role["topk1"]] == 1 and n[role["topp_first"]] == 1
    assert n[role["topp1"]] == min(case["top_k"][role["topp1"]], on(role["topp1"]).sum())
    for r in (role["pass_k0"], role["pass_T"]):
        assert n[r] == on(r).sum() and np.array_equal(no.allowed(mask[r], 257), on(r))
    r = role["quantised"]
    x = no.penalise(case["logits"][r], 257, case["history"][r], case["penalty"][r])
    A = no.ordered_candidates(x, 257, on(r))
    k = int(case["top_k"][r])
    assert x[A[k - 1]] == x[A[k]] and A[k - 1] < A[k], "the k-th boundary is inside a tie run"


def test_the_penalty_is_applied_once_per_distinct_id():
    x = np.array([2.0, -2.0, 0.0, 5.0], dtype=np.float32)
    h = np.array([0, 0, 1, -1, 9, 1, 0], dtype=np.int32)
    th = np.float32(1.3)
    got = no.penalise(x, 4, h, th)
    assert got.tolist() == [np.float32(2.0) / th, np.float32(-2.0) * th, 0.0, 5.0]
    assert np.array_equal(no.penalise(x, 4, h, np.float32(1.0)).view(np.int32), x.view(np.int32))


def test_the_reference_op_equals_the_oracle_bitwise(cases):
    rows = 0
    for what, case in cases:
        no.check(case, no.launch(case, "cpu"), what)
        rows += case["rows"]
    print(f"MEASURED nucleus reference op rows checked {rows}")


def test_the_reference_op_at_the_llama_vocabulary():
    case = no.llama_case(no.odd_ld(no.LLAMA_VOCAB))
    no.check(case, no.launch(case, "cpu"), "llama")


def test_the_wrapper_takes_the_reference_on_host_tensors_and_never_the_library(monkeypatch):
    monkeypatch.setattr(ops, "nucleus_ext", lambda: (_ for _ in ()).throw(AssertionError("library reached")))
    before = ops.nucleus_launches
    x = torch.tensor([[1.0, 3.0, 3.0, 2.0, -1.0]])
    out, n = torch.full((1, 1), -1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    f = lambda v: torch.tensor([v], dtype=torch.float32)  # noqa: E731
    ops.nucleus_step(x, None, out, n, f(1.0), f(1.0), torch.tensor([3], dtype=torch.int32), f(2.0),
                     torch.tensor([[3, 3, 4]], dtype=torch.int32))
    assert x.tolist() == [[1.0, 3.0, 3.0, 1.0, -2.0]]
    assert int(n) == 3 and int(out[0, 0]) == 0b00111  # ids 1, 2 (tie, by id), then 0 and 3 tie at 1.0: 0 wins
    assert ops.nucleus_launches == before
