"""The set log-probability bindings (csrc/turn/bindings.cpp, _vwa_turn.so) reject host tensors in
their own validation, before anything reaches the HIP runtime -- the convention of
test_bindings_cpu.py and the other small libraries' binding tests: the exported entry point is
called with well-shaped, right-dtype CPU tensors and must raise a RuntimeError that names the
offending argument.  The wrapper (ops.set_logprob) rejects every malformed argument before it
launches, and takes the Python reference on host tensors.

The binding cases run only where there is NO GPU: on a GPU machine a missed device check would hand
a host pointer to a kernel, and this file must never be the thing that does that."""
import math
import os
import re

import pytest
import torch

import voice_enabled_browser_automation_amd.ops as ops
from voice_enabled_browser_automation_amd.ops.build import KERNEL_LIBS, TURN_SO

F32, I32 = torch.float32, torch.int32


def z(*shape, dtype=F32):
    return torch.zeros(*shape, dtype=dtype)


# entry point -> (the argument its message must name, a builder of CPU arguments)
CASES = {
    "set_logprob": ("logits", lambda: (z(4, 64), 61, z(1, 2, dtype=I32), z(4, 2))),
}


@pytest.fixture(scope="module")
def E():
    if not os.path.exists(TURN_SO):
        pytest.skip("set log-probability library not built here (python -c 'import __graft_entry__ as g; g.build()')")
    if torch.cuda.is_available():
        pytest.skip("host tensors are only ever offered to the bindings where there is no GPU to launch on")
    return ops.turn_ext()


def test_the_library_is_a_row_of_the_build():
    assert ("turn", "_vwa_turn") in KERNEL_LIBS and TURN_SO.endswith("_vwa_turn.so")


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
    assert names == {"set_logprob"}, sorted(names)
    takes = {n for n in names if "Tensor" in (getattr(E, n).__doc__ or "").splitlines()[0].split("->")[0]}
    assert takes == set(CASES)
    assert (E.MAX_ROWS, E.MAX_VOCAB) == (ops.TURN_MAX_ROWS, ops.TURN_MAX_VOCAB) == (64, 1 << 20)


def test_the_wrapper_takes_the_reference_on_host_tensors_and_never_the_library(monkeypatch):
    monkeypatch.setattr(ops, "turn_ext", lambda: (_ for _ in ()).throw(AssertionError("library reached")))
    x = torch.randn(3, 64)
    x[:, 61:] = float("nan")
    x[2, :61] = float("-inf")
    before = x.clone()
    sets = torch.tensor([[0b1010, 0], [-1, -1], [-1, -1]], dtype=I32)
    out = ops.set_logprob(x, 61, sets)
    assert torch.equal(x.view(I32), before.view(I32)) and out.shape == (3, 2) and out.dtype == F32
    A = torch.logsumexp(x[0, :61].double(), 0)
    want = float(torch.logsumexp(x[0, [1, 3]].double(), 0) - A)
    assert abs(float(out[0, 0]) - want) < 1e-5 and abs(float(out[0, 1]) - float(A)) < 1e-5
    assert abs(float(out[1, 0])) < 1e-6                                   # the full set
    assert out[2].tolist() == [-math.inf, -math.inf]                      # a row at -inf
    shared = ops.set_logprob(x[:2], 61, sets[:1])                         # one shared row of bits
    assert torch.equal(shared[0], out[0]) and float(shared[1, 0]) < 0.0
    assert float(ops.set_logprob(x[:1], 61, z(1, 2, dtype=I32))[0, 0]) == -math.inf   # the empty set


def test_the_wrapper_validates_before_it_launches():
    i32 = dict(dtype=I32)
    x, sets = z(2, 64), z(1, 2, **i32)
    buf = torch.zeros(256)

    def call(**kw):
        a = dict(logits=x, vocab=61, sets=sets, out=None)
        a.update(kw)
        return ops.set_logprob(a["logits"], a["vocab"], a["sets"], out=a["out"])

    call()
    call(out=z(2, 2), sets=z(2, 2, **i32))
    call(logits=z(4, 70)[:2, :64])                                          # a row stride above the row length
    for kw, match in (
            # wrong dtype or shape
            (dict(logits=z(2, 64, dtype=torch.float16)), "logits"), (dict(logits=z(64)), "logits"),
            (dict(logits=z(2, 128)[:, ::2]), "logits"), (dict(logits=z(1, 64).expand(2, 64)), "logits"),
            (dict(sets=z(1, 1, **i32)), "sets"), (dict(sets=z(2, **i32)), "sets"), (dict(sets=z(1, 2)), "sets"),
            (dict(sets=z(3, 2, **i32)[:, :1]), "sets"), (dict(sets=z(1, 2, **i32).expand(2, 2)), "sets"),
            (dict(out=z(2)), "out"), (dict(out=z(3, 2)), "out"), (dict(out=z(2, 2, **i32)), "out"),
            (dict(out=z(2, 4)[:, :2]), "out"),
            # rows = 0 and 65
            (dict(logits=z(0, 64)), "logits"), (dict(logits=z(65, 64)), "logits"),
            # vocab past the row length or the library's limit
            (dict(vocab=65), "vocab"), (dict(vocab=0), "vocab"),
            # out inside the logits or the set
            (dict(logits=buf[:128].view(2, 64), out=buf[60:64].view(2, 2)), "overlap logits"),
            (dict(logits=buf[:128].view(2, 64), out=buf[124:128].view(2, 2)), "overlap logits"),
            (dict(sets=buf[128:132].view(I32).view(2, 2), out=buf[130:134].view(2, 2)), "overlap sets")):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    # the columns past vocab of the last row are not the logits': out may sit there
    call(logits=buf[:128].view(2, 64), out=buf[125:129].view(2, 2))
    if torch.cuda.is_available():  # wrong device
        with pytest.raises(ValueError, match="sets"):
            call(logits=x.cuda())


def test_the_set_logprob_kernel_uses_no_scratch():
    """The gfx950 code object's metadata (the reader of tests/test_beam_cpu.py): no private segment,
    no spilled registers."""
    from test_beam_cpu import _kernels

    ks = {k: v for k, v in _kernels(os.path.join("turn", "set_logprob.hip.o")).items() if "set_logprob_kernel" in k}
    assert ks, "set_logprob_kernel not in the object"
    assert all(v[0] == 0 and v[2] == 0 for v in ks.values()), \
        f"set_logprob_kernel uses scratch (private segment bytes, VGPRs, spilled VGPRs): {ks}"
    print(f"MEASURED set_logprob_kernel (scratch bytes, VGPRs, spills) {list(ks.values())}")
