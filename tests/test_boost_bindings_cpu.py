"""The keyterm boosting bindings (csrc/boost/bindings.cpp, _vwa_boost.so) reject host tensors in
their own validation, before anything reaches the HIP runtime -- the convention of
test_bindings_cpu.py and the align / sot / beam binding tests: the exported entry point is called
with well-shaped, right-dtype CPU tensors and must raise a RuntimeError that names the offending
argument.

Runs only where there is NO GPU: on a GPU machine a missed device check would hand a host pointer
to a kernel, and this file must never be the thing that does that."""
import os
import re

import pytest
import torch

import boost_cases as bc
import boost_oracle as bo
import voice_enabled_browser_automation_amd.ops as ops
from voice_enabled_browser_automation_amd.ops.build import BOOST_SO

F32, I32 = torch.float32, torch.int32


def z(*shape, dtype=F32):
    return torch.zeros(*shape, dtype=dtype)


# entry point -> (the argument its message must name, a builder of CPU arguments)
CASES = {
    "boost_step": ("logits", lambda: (z(4, 48), 40, z(6, dtype=I32), z(3, dtype=I32), z(3, dtype=I32), z(3),
                                      z(5, dtype=I32), z(4, dtype=I32), z(4, dtype=I32), z(4, dtype=I32),
                                      z(4, dtype=I32), None, 1)),
}


@pytest.fixture(scope="module")
def E():
    if not os.path.exists(BOOST_SO):
        pytest.skip("keyterm boosting library not built here (python -c 'import __graft_entry__ as g; g.build()')")
    if torch.cuda.is_available():
        pytest.skip("host tensors are only ever offered to the bindings where there is no GPU to launch on")
    return ops.boost_ext()


@pytest.mark.parametrize("name", sorted(CASES))
def test_cpu_tensors_are_rejected_by_the_binding(E, name):
    arg, build = CASES[name]
    with pytest.raises(RuntimeError) as ei:
        getattr(E, name)(*build())
    msg = str(ei.value).splitlines()[0]
    assert "HIP error" not in str(ei.value) and "no ROCm-capable device" not in str(ei.value), msg
    assert re.search(rf"\b({arg})\b", msg), f"{name}: message does not name {arg!r}: {msg}"


def test_the_entry_points_are_exactly_these(E):
    names = {n for n in dir(E) if not n.startswith("_") and callable(getattr(E, n))}
    assert names == {"boost_step"}, sorted(names)
    takes = {n for n in names if "Tensor" in (getattr(E, n).__doc__ or "").splitlines()[0].split("->")[0]}
    assert takes == set(CASES)
    assert (E.MAX_ROWS, E.MAX_STATES, E.MAX_EDGES) == (ops.BOOST_MAX_ROWS, ops.BOOST_MAX_STATES, ops.BOOST_MAX_EDGES)
    assert ops.BOOST_CAP_STATES <= ops.BOOST_MAX_STATES and ops.BOOST_CAP_EDGES <= ops.BOOST_MAX_EDGES


def test_the_wrapper_takes_the_reference_on_host_tensors_and_never_the_library(monkeypatch):
    """ops.boost_step on CPU tensors is the Python reference (no library needed), and it agrees
    with the table-level oracle on a call that uses tokens, parents and an unboosted row."""
    monkeypatch.setattr(ops, "boost_ext", lambda: (_ for _ in ()).throw(AssertionError("library reached")))
    sets, bases, tables = bc.joint()
    roots = [bases[0], bases[0], -1, bases[2]]
    state_in = [bases[0] + sets[0].run([5]), bases[0] + sets[0].run([5, 6]), 7, bases[2] + sets[2].run([10, 11])]
    x = bc.rand_logits(4, bc.LD, bc.V, 1)
    got, states = bc.run_step("cpu", tables, x, bc.V, roots, state_in, tokens=[6, 7, 3, 12], parents=[1, 0, 0, 1], W=2,
                              what="host")
    assert states[2] == 7 and bo.bits_equal(got[2], x[2])  # the unboosted row keeps its state and its logits
    assert not bo.bits_equal(got[0], x[0])


def test_the_wrapper_validates_before_it_launches():
    sets, bases, tables = bc.joint(("collide",))
    t = bc.tables_on(tables, "cpu")
    x, i32 = z(2, 48), dict(dtype=I32)
    r, s = torch.zeros(2, **i32), torch.zeros(4, **i32)
    for kw, match in ((dict(parents=torch.zeros(2, **i32), W=2, state_out=s), "only without parents"),
                      (dict(state_out=s[1:]), "must not overlap"),
                      (dict(parents=torch.zeros(2, **i32), W=3, state_out=torch.zeros(2, **i32)), "groups of W"),
                      (dict(tokens=torch.zeros(1, **i32), state_out=s), "tokens"),
                      (dict(tokens=torch.zeros(2), state_out=s), "tokens")):
        with pytest.raises(ValueError, match=match):
            ops.boost_step(x, 40, t, r, s, kw.pop("state_out"), **kw)
    with pytest.raises(ValueError, match="vocab"):
        ops.boost_step(x, 49, t, r, s, s)
    with pytest.raises(ValueError, match="roots"):
        ops.boost_step(x, 40, t, torch.zeros(3, **i32), s, s)
    with pytest.raises(ValueError, match="edge_off"):
        ops.boost_step(x, 40, (t[0][:-1],) + t[1:], r, s, s)


def test_the_boost_kernel_uses_no_scratch():
    """The gfx950 code object's metadata (the reader of tests/test_beam_cpu.py): no private segment,
    no spilled registers."""
    from test_beam_cpu import _kernels

    ks = {k: v for k, v in _kernels(os.path.join("boost", "boost_step.hip.o")).items() if "boost_step_kernel" in k}
    assert ks, "boost_step_kernel not in the object"
    assert all(v[0] == 0 and v[2] == 0 for v in ks.values()), \
        f"boost_step_kernel uses scratch (private segment bytes, VGPRs, spilled VGPRs): {ks}"
    print(f"MEASURED boost_step_kernel (scratch bytes, VGPRs, spills) {list(ks.values())}")
