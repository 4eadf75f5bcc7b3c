"""The per-sequence log-probability bindings (csrc/rescore/bindings.cpp, _vwa_rescore.so) reject host
tensors in their own validation, before anything reaches the HIP runtime -- the convention of
test_bindings_cpu.py and the other small libraries' binding tests.  The wrapper (ops.seq_logprob)
rejects every malformed argument before it launches, and takes the Python reference on host tensors.

The binding cases run only where there is NO GPU: on a GPU machine a missed device check would hand
a host pointer to a kernel, and this file must never be the thing that does that."""
import math
import os
import re

import numpy as np
import pytest
import torch

import rescore_oracle as ro
import voice_enabled_browser_automation_amd.ops as ops
from voice_enabled_browser_automation_amd.ops.build import KERNEL_LIBS, RESCORE_SO

F32, I32 = torch.float32, torch.int32


def z(*shape, dtype=F32):
    return torch.zeros(*shape, dtype=dtype)


# entry point -> (the argument its message must name, a builder of CPU arguments)
CASES = {
    "seq_logprob": ("logits", lambda: (z(4, 64), 61, z(4, dtype=I32), z(2, dtype=I32), z(4, dtype=I32), 2, None, z(4),
                                       z(2))),
}


@pytest.fixture(scope="module")
def E():
    if not os.path.exists(RESCORE_SO):
        pytest.skip("per-sequence log-probability library not built here (python -c 'import __graft_entry__ as g; "
                    "g.build()')")
    if torch.cuda.is_available():
        pytest.skip("host tensors are only ever offered to the bindings where there is no GPU to launch on")
    return ops.rescore_ext()


def test_the_library_is_a_row_of_the_build():
    assert ("rescore", "_vwa_rescore") in KERNEL_LIBS and RESCORE_SO.endswith("_vwa_rescore.so")


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
    assert names == {"seq_logprob"}, sorted(names)
    assert (E.MAX_ROWS, E.MAX_SEQ, E.MAX_VOCAB) == (ops.RESCORE_MAX_ROWS, ops.RESCORE_MAX_SEQ, ops.RESCORE_MAX_VOCAB) \
        == (256, 64, 1 << 20)


def test_the_wrapper_takes_the_reference_on_host_tensors_and_never_the_library(monkeypatch):
    monkeypatch.setattr(ops, "rescore_ext", lambda: (_ for _ in ()).throw(AssertionError("library reached")))
    launches = ops.seq_logprob_launches
    x = torch.randn(5, 64)
    x[:, 61:] = float("nan")
    x[2, :61] = float("-inf")
    before = x.clone()
    es = torch.tensor([0b1010, 0], dtype=I32)
    target = torch.tensor([3, -1, 0, 61, 60], dtype=I32)
    seq = torch.tensor([0, 0, 1, 2, 0], dtype=I32)
    acc_in = torch.tensor([1.5, 0.0, -2.0, 7.0])
    lp, acc = ops.seq_logprob(x, 61, target, es, seq, 4, acc_in=acc_in)
    assert torch.equal(x.view(I32), before.view(I32)) and lp.shape == (5,) and acc.shape == (4,)
    assert lp.dtype == acc.dtype == F32 and ops.seq_logprob_launches == launches
    A = torch.logsumexp(x[:, :61].double(), 1)
    assert abs(float(lp[0]) - float(x[0, 3] - A[0])) < 1e-5
    assert abs(float(lp[1]) - float(torch.logsumexp(x[1, [1, 3]].double(), 0) - A[1])) < 1e-5
    assert float(lp[2]) == -math.inf and float(lp[3]) == -math.inf       # a row at -inf, a target past the vocabulary
    assert abs(float(lp[4]) - float(x[4, 60] - A[4])) < 1e-5
    want = np.float32(np.float32(np.float32(1.5) + lp[0].numpy()) + lp[1].numpy()) + lp[4].numpy()
    assert float(acc[0]) == float(want) and acc[1:].tolist() == [-math.inf, -math.inf, 7.0]
    lp0, acc0 = ops.seq_logprob(x, 61, target, es, seq, 4)                # acc_in None: zeros
    assert torch.equal(lp0, lp) and float(acc0[3]) == 0.0


@pytest.mark.parametrize("vocab,rows", [(1, 1), (5, 3), (33, 13), (257, 30)])
def test_the_reference_op_matches_the_oracle(vocab, rows):
    for shift in (0, 3, 7):
        for seq_mode in ro.SEQ_MODES:
            for set_mode in ro.SET_MODES:
                case = ro.make_case(rows, vocab, seed=100 * vocab + shift, shift=shift, seq_mode=seq_mode,
                                    set_mode=set_mode, acc=bool(shift))
                ro.check(case, ro.launch(case, "cpu"), f"V={vocab} rows={rows} shift={shift} {seq_mode} {set_mode}")


def test_the_wrapper_validates_before_it_launches():
    i32 = dict(dtype=I32)
    buf = torch.zeros(512)
    ibuf = torch.zeros(64, **i32)

    def call(**kw):
        a = dict(logits=z(3, 64), vocab=61, target=z(3, **i32), end_set=z(2, **i32), seq=z(3, **i32), n_seq=2,
                 acc_in=None, lp=None, acc_out=None)
        a.update(kw)
        return ops.seq_logprob(a["logits"], a["vocab"], a["target"], a["end_set"], a["seq"], a["n_seq"],
                               acc_in=a["acc_in"], lp=a["lp"], acc_out=a["acc_out"])

    call()
    call(acc_in=z(2), lp=z(3), acc_out=z(2), end_set=z(1, 2, **i32))
    call(logits=z(4, 70)[:, :64])                                           # more rows, a row stride above the length
    for kw, match in (
            # wrong dtype or shape
            (dict(logits=z(3, 64, dtype=torch.float16)), "logits"), (dict(logits=z(64)), "logits"),
            (dict(logits=z(3, 128)[:, ::2]), "logits"), (dict(logits=z(1, 64).expand(3, 64)), "logits"),
            (dict(target=z(3)), "target"), (dict(target=z(3, 1, **i32)), "target"), (dict(target=z(6, **i32)[::2]), "target"),
            (dict(end_set=z(1, **i32)), "end_set"), (dict(end_set=z(2)), "end_set"), (dict(end_set=z(4, **i32)[::2]), "end_set"),
            (dict(seq=z(2, **i32)), "seq"), (dict(seq=z(3)), "seq"), (dict(seq=z(4, **i32)), "seq"),
            (dict(lp=z(4)), "lp"), (dict(lp=z(3, **i32)), "lp"), (dict(lp=z(3, 1)), "lp"),
            (dict(acc_out=z(3)), "acc_out"), (dict(acc_out=z(2, **i32)), "acc_out"),
            (dict(acc_in=z(3)), "acc_in"), (dict(acc_in=z(2, dtype=torch.float64)), "acc_in"),
            # rows = 0, more targets than logits rows, 257 rows
            (dict(target=z(0, **i32), seq=z(0, **i32)), "target"), (dict(target=z(4, **i32), seq=z(4, **i32)), "target"),
            (dict(logits=z(257, 64), target=z(257, **i32), seq=z(257, **i32)), "target"),
            # vocab past the row length, n_seq outside [1, 64]
            (dict(vocab=65), "vocab"), (dict(vocab=0), "vocab"), (dict(n_seq=0), "n_seq"), (dict(n_seq=65), "n_seq"),
            # an output inside an input, the outputs inside each other
            (dict(logits=buf[:192].view(3, 64), lp=buf[60:63]), "lp must not overlap logits"),
            (dict(logits=buf[:192].view(3, 64), acc_out=buf[187:189]), "acc_out must not overlap logits"),
            (dict(acc_in=buf[200:202], acc_out=buf[201:203]), "acc_out must not overlap acc_in"),
            (dict(acc_in=buf[200:202], acc_out=buf[200:202]), "acc_out must not overlap acc_in"),
            (dict(acc_in=buf[200:202], lp=buf[199:202]), "lp must not overlap acc_in"),
            (dict(lp=buf[300:303], acc_out=buf[302:304]), "acc_out must not overlap lp"),
            (dict(target=ibuf[:3], lp=ibuf[2:5].view(F32)), "lp must not overlap target"),
            (dict(seq=ibuf[8:11], acc_out=ibuf[10:12].view(F32)), "acc_out must not overlap seq"),
            (dict(end_set=ibuf[16:18], lp=ibuf[17:20].view(F32)), "lp must not overlap end_set")):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    # the columns past vocab of the last row are not the logits': an output may sit there
    call(logits=buf[:192].view(3, 64), lp=buf[189:192])
    if torch.cuda.is_available():  # wrong device
        with pytest.raises(ValueError, match="target"):
            call(logits=z(3, 64).cuda())


def test_the_kernels_use_no_scratch():
    """The gfx950 code object's metadata (the reader of tests/test_beam_cpu.py): no private segment,
    no spilled registers."""
    from test_beam_cpu import _kernels

    ks = {k: v for k, v in _kernels(os.path.join("rescore", "seq_logprob.hip.o")).items()
          if "row_logprob_kernel" in k or "seq_sum_kernel" in k}
    assert len(ks) == 2, f"the two kernels are not in the object: {sorted(ks)}"
    assert all(v[0] == 0 and v[2] == 0 for v in ks.values()), \
        f"a kernel uses scratch (private segment bytes, VGPRs, spilled VGPRs): {ks}"
    print(f"MEASURED seq_logprob kernels (scratch bytes, VGPRs, spills) {list(ks.values())}")
