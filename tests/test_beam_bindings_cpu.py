"""The beam search bindings (csrc/beam/bindings.cpp, _vwa_beam.so) reject host tensors in their own
validation, before anything reaches the HIP runtime -- the convention of test_bindings_cpu.py,
test_align_bindings_cpu.py and test_sot_bindings_cpu.py: every exported entry point that takes
tensors is called with well-shaped, right-dtype CPU tensors and must raise a RuntimeError that names
the offending argument.

Runs only where there is NO GPU: on a GPU machine a missed device check would hand a host pointer
to a kernel, and this file must never be the thing that does that."""
import os
import re

import pytest
import torch

import voice_enabled_browser_automation_amd.ops as ops
from voice_enabled_browser_automation_amd.ops.build import BEAM_SO

F32, I32, BF16 = torch.float32, torch.int32, torch.bfloat16


def z(*shape, dtype=F32):
    return torch.zeros(*shape, dtype=dtype)


# entry point -> (the argument its message must name, a builder of CPU arguments)
CASES = {
    "beam_select": ("logits", lambda: (z(4, 48), z(4), z(1, 2, dtype=I32), 40, 2, z(2, 4), z(2, 4, dtype=I32),
                                       z(2, 4, dtype=I32), z(4096, dtype=I32))),
    "kv_beam_gather": ("k_cache", lambda: (z(2, 9, 3, 16, 64, dtype=BF16), z(2, 9, 3, 16, 64, dtype=BF16),
                                           z(2, 4, dtype=I32), z(1, 2, dtype=I32), z(1, 2, dtype=I32),
                                           z(1, dtype=I32), 64)),
}


@pytest.fixture(scope="module")
def E():
    if not os.path.exists(BEAM_SO):
        pytest.skip("beam search library not built here (python -c 'import __graft_entry__ as g; g.build()')")
    if torch.cuda.is_available():
        pytest.skip("host tensors are only ever offered to the bindings where there is no GPU to launch on")
    return ops.beam_ext()


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
    assert names == {"beam_select", "kv_beam_gather", "beam_select_workspace"}, sorted(names)
    takes = {n for n in names if "Tensor" in (getattr(E, n).__doc__ or "").splitlines()[0].split("->")[0]}
    assert takes == set(CASES), (sorted(takes - set(CASES)), sorted(set(CASES) - takes))
    assert (E.MAX_WIDTH, E.MAX_ROWS, E.MAX_VOCAB) == (ops.BEAM_MAX_WIDTH, ops.BEAM_MAX_ROWS, ops.BEAM_MAX_VOCAB)
    # the wrapper's workspace covers the library's need at the largest launch
    for vocab in (40, 8192, 8193, 51866, 1 << 20):
        assert E.beam_select_workspace(64, vocab) <= ops.BEAM_MAX_ROWS * ((vocab + 8191) // 8192) * 34 * 4


def test_the_wrappers_take_the_reference_on_host_tensors_and_never_the_library(monkeypatch):
    """ops.beam_select / ops.kv_beam_gather on CPU tensors are the references (no library needed)."""
    monkeypatch.setattr(ops, "beam_ext", lambda: (_ for _ in ()).throw(AssertionError("library reached")))
    x = z(2, 48)
    x[0, 9] = 1.0
    s, b, t = ops.beam_select(x, torch.tensor([0.0, float("-inf")]), None, 40, 2)
    assert (int(b[0, 0]), int(t[0, 0])) == (0, 9) and s.shape == (1, 4)
    k = torch.arange(2 * 9 * 3 * 16 * 8, dtype=torch.float32).view(2, 9, 3, 16, 8).to(BF16)
    v = k.clone()
    table = torch.arange(1, 9, dtype=I32).view(2, 4)
    ops.kv_beam_gather(k, v, table, [[1, 0]], [[0, 0]], [16])
    assert torch.equal(k[:, 1], k[:, 5]) and torch.equal(v[:, 1], v[:, 5]) and not torch.equal(k[:, 2], k[:, 6])
