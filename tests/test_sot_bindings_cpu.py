"""The start-of-transcript probe bindings (csrc/sot/bindings.cpp, _vwa_sot.so) reject host tensors in
their own validation, before anything reaches the HIP runtime -- the convention of
test_bindings_cpu.py and test_align_bindings_cpu.py: every exported entry point that takes tensors
is called with well-shaped, right-dtype CPU tensors and must raise a RuntimeError that names the
offending argument.

Runs only where there is NO GPU: on a GPU machine a missed device check would hand a host pointer
to a kernel, and this file must never be the thing that does that."""
import os
import re

import pytest
import torch

import voice_enabled_browser_automation_amd.ops as ops
from voice_enabled_browser_automation_amd.ops.build import SOT_SO

F32, I32 = torch.float32, torch.int32


def z(*shape, dtype=F32):
    return torch.zeros(*shape, dtype=dtype)


# entry point -> (the argument its message must name, a builder of CPU arguments)
CASES = {
    "sot_probe": ("logits", lambda: (z(2, 48), 40, 7, 5, [0b11111, 0, 0, 0], 0, z(2, 5), z(2, dtype=I32), z(2), z(2),
                                     z(4, dtype=I32), z(2, dtype=I32))),
}


@pytest.fixture(scope="module")
def E():
    if not os.path.exists(SOT_SO):
        pytest.skip("SOT probe library not built here (python -c 'import __graft_entry__ as g; g.build()')")
    if torch.cuda.is_available():
        pytest.skip("host tensors are only ever offered to the bindings where there is no GPU to launch on")
    return ops.sot_ext()


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
    assert names == {"sot_probe"}, sorted(names)
    takes = {n for n in names if "Tensor" in (getattr(E, n).__doc__ or "").splitlines()[0].split("->")[0]}
    assert takes == set(CASES), (sorted(takes - set(CASES)), sorted(set(CASES) - takes))


def test_the_wrapper_takes_the_reference_on_host_tensors_and_never_the_library():
    """ops.sot_probe on CPU tensors is the reference (no library needed); the library itself is only
    reached with GPU tensors."""
    x = z(1, 48)
    x[0, 9] = 1.0
    probs, tok, conf, nsp = ops.sot_probe(x, 40, 7, 5, 0)
    assert tok.tolist() == [9] and probs.shape == (1, 5) and abs(float(probs.sum()) - 1) < 1e-6
