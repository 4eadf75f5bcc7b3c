"""The wire audio ingest bindings (csrc/ingest/bindings.cpp, _vwa_ingest.so) reject what they cannot
run in their own validation, before anything reaches the HIP runtime -- the convention of
test_nucleus_bindings_cpu.py and the other small libraries' binding tests: a wrong dtype, device or
contiguity, a byte count that is not whole frames, an unsupported rate, more than 8 channels, a table
of the wrong shape, an ``out`` that is too short.

The binding checks the format and every shape (host metadata) before any device, so host tensors
reach each of those rejects; a call that is well-formed in everything but the device ends at "raw
must be a GPU tensor".  ops.ingest states the same rules in front of it.  The binding cases run only
where there is NO GPU: on a GPU machine a missed device check would hand a host pointer to a kernel,
and this file must never be the thing that does that."""
import os
import re

import pytest
import torch

import voice_enabled_browser_automation_amd.ops as ops
from voice_enabled_browser_automation_amd.asr.wire import MAX_CHANNELS, SAMPLE_RATES, AudioFormat
from voice_enabled_browser_automation_amd.ops.build import INGEST_SO, KERNEL_LIBS

U8, F32 = torch.uint8, torch.float32


@pytest.fixture(scope="module")
def E():
    if not os.path.exists(INGEST_SO):
        pytest.skip("ingest library not built here (python -c 'import __graft_entry__ as g; g.build()')")
    if torch.cuda.is_available():
        pytest.skip("host tensors are only ever offered to the bindings where there is no GPU to launch on")
    return ops.ingest_ext()


def test_the_library_is_a_row_of_the_build():
    assert ("ingest", "_vwa_ingest") in KERNEL_LIBS and INGEST_SO.endswith("_vwa_ingest.so")
    assert len({so for _, so in KERNEL_LIBS}) == len(KERNEL_LIBS)


def _args(**kw):
    a = dict(raw=torch.zeros(8, dtype=U8), encoding=1, sample_rate=8000, channels=1, channel=-1,
             table=ops.ingest_tables(8000), out=torch.zeros(16))
    a.update(kw)
    return a


def test_cpu_tensors_are_rejected_by_the_binding(E):
    """Well-formed in everything but the device: the message names raw and no HIP call was made."""
    with pytest.raises(RuntimeError) as ei:
        E.ingest(**_args())
    msg = str(ei.value).splitlines()[0]
    assert "HIP error" not in str(ei.value) and "no ROCm-capable device" not in str(ei.value), msg
    assert re.search(r"\braw\b", msg) and "GPU tensor" in msg, msg


@pytest.mark.parametrize("kw, names", [
    # wrong dtype, rank, contiguity
    (dict(raw=torch.zeros(8, dtype=torch.int8)), "raw"), (dict(raw=torch.zeros(2, 4, dtype=U8)), "raw"),
    (dict(raw=torch.zeros(16, dtype=U8)[::2]), "raw"),
    # a byte count that is not whole frames
    (dict(raw=torch.zeros(7, dtype=U8), channels=2), "whole frames of 2"),
    (dict(raw=torch.zeros(9, dtype=U8), encoding=0), "whole frames of 2"),
    (dict(raw=torch.zeros(20, dtype=U8), encoding=0, channels=3), "whole frames of 6"),
    # an unsupported rate, encoding, channel count, channel
    (dict(sample_rate=16001), "sample_rate"), (dict(sample_rate=96000), "sample_rate"), (dict(sample_rate=0), "sample_rate"),
    (dict(encoding=3), "encoding"), (dict(encoding=-1), "encoding"),
    (dict(channels=9, raw=torch.zeros(9, dtype=U8)), "channels"), (dict(channels=0), "channels"),
    (dict(channel=1), "channel"), (dict(channel=-2), "channel"),
    # a table of the wrong shape or dtype
    (dict(table=torch.zeros(2, 31)), "table"), (dict(table=torch.zeros(1, 32)), "table"), (dict(table=torch.zeros(64)), "table"),
    (dict(table=torch.zeros(2, 32, dtype=torch.float64)), "table"), (dict(table=torch.zeros(2, 64)[:, ::2]), "table"),
    (dict(sample_rate=48000), "table"),  # (the 8 kHz table at 48 kHz)
    # an out that is too short, or not f32, 1-D, contiguous
    (dict(out=torch.zeros(15)), "out"), (dict(out=torch.zeros(16, dtype=torch.float64)), "out"),
    (dict(out=torch.zeros(4, 4)), "out"), (dict(out=torch.zeros(32)[::2]), "out"),
])
def test_the_binding_rejects_malformed_arguments_before_any_device_check(E, kw, names):
    with pytest.raises(RuntimeError) as ei:
        E.ingest(**_args(**kw))
    msg = str(ei.value).splitlines()[0]
    assert "GPU tensor" not in msg and "HIP error" not in str(ei.value), msg
    assert re.search(names, msg), f"message does not name {names!r}: {msg}"


def test_the_entry_points_are_exactly_these(E):
    names = {n for n in dir(E) if not n.startswith("_") and callable(getattr(E, n))}
    assert names == {"ingest", "geometry"}, sorted(names)
    assert (E.MAX_CHANNELS, E.MAX_FRAMES) == (ops.INGEST_MAX_CHANNELS, ops.INGEST_MAX_FRAMES) == (MAX_CHANNELS, 1 << 30)


def test_the_binding_knows_the_same_rates_and_geometry(E):
    for rate in SAMPLE_RATES:
        assert tuple(E.geometry(rate)) == ops.ingest_geometry(rate)
    for rate in (0, -8000, 7999, 16001, 44000, 96000, 1 << 40):
        with pytest.raises(RuntimeError, match="sample_rate"):
            E.geometry(rate)


def test_the_wrapper_validates_before_it_launches():
    z = torch.zeros(24, dtype=U8)
    mu8 = AudioFormat("mulaw", 8000, 1)
    assert len(ops.ingest(z, mu8)) == 48
    assert len(ops.ingest(z, AudioFormat("linear16", 48000, 2))) == 2
    for raw, fmt, kw, match in (
            # wrong dtype, rank, contiguity
            (z.to(torch.int16), mu8, {}, "raw"), (z.view(4, 6), mu8, {}, "raw"), (z[::2], mu8, {}, "raw"),
            (z.numpy(), mu8, {}, "raw"),
            # not whole frames
            (z[:23], AudioFormat("linear16", 16000, 1), {}, "whole frames of 2"),
            (z[:23], AudioFormat("alaw", 8000, 3), {}, "whole frames of 3"),
            (z[:22], AudioFormat("linear16", 44100, 4), {}, "whole frames of 8"),
            # linear16 at an odd address
            (torch.zeros(25, dtype=U8)[1:], AudioFormat("linear16", 16000, 1), {}, "aligned"),
            # out: dtype, contiguity, too short
            (z, mu8, dict(out=torch.zeros(48, dtype=torch.float64)), "out"),
            (z, mu8, dict(out=torch.zeros(96)[::2]), "out"), (z, mu8, dict(out=torch.zeros(47)), "out"),
            (z, mu8, dict(out=torch.zeros(2, 24)), "out"),
            # not a format
            (z, ("mulaw", 8000, 1), {}, "AudioFormat")):
        with pytest.raises(ValueError, match=match):
            ops.ingest(raw, fmt, **kw)
    buf = torch.zeros(64, dtype=U8)
    with pytest.raises(ValueError, match="overlap"):
        ops.ingest(buf[:8], AudioFormat("mulaw", 16000, 1), out=buf[4:36].view(F32))
    if torch.cuda.is_available():  # wrong device
        with pytest.raises(ValueError, match="out is on"):
            ops.ingest(z.cuda(), mu8, out=torch.zeros(48))


def test_the_launcher_states_the_same_limits():
    """ingest.h is the contract: the limits the wrapper enforces are the header's, and the span a
    workgroup stages fits its LDS array at every supported rate."""
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "csrc", "ingest", "ingest.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"constexpr int (kIngest\w+) = (\d+);", text)}
    assert consts["kIngestMaxChannels"] == ops.INGEST_MAX_CHANNELS == MAX_CHANNELS
    assert re.search(r"kIngestMaxFrames = \(int64_t\)1 << 30;", text)
    assert re.search(r"kIngestLinear16 = 0, kIngestMulaw = 1, kIngestAlaw = 2;", text)
    assert [AudioFormat(e).code for e in ("linear16", "mulaw", "alaw")] == [0, 1, 2]
    geo = [ops.ingest_geometry(r) for r in SAMPLE_RATES]
    assert max(L for L, _, _ in geo) == consts["kIngestMaxL"] and max(H for _, _, H in geo) == consts["kIngestMaxH"]
    assert max((consts["kIngestBlock"] - 1) * M // L + 1 + 2 * H for L, M, H in geo) <= consts["kIngestMaxSpan"]


def test_the_ingest_kernels_use_no_scratch():
    """The gfx950 code object's metadata (the reader of tests/test_beam_cpu.py): no private segment,
    no spilled registers."""
    from test_beam_cpu import _kernels

    ks = {k: v for k, v in _kernels(os.path.join("ingest", "ingest_resample.hip.o")).items() if "ingest_" in k}
    assert len(ks) == 2, f"ingest_copy_kernel and ingest_resample_kernel, not {sorted(ks)}"
    assert all(v[0] == 0 and v[2] == 0 for v in ks.values()), \
        f"an ingest kernel uses scratch (private segment bytes, VGPRs, spilled VGPRs): {ks}"
    print(f"MEASURED ingest kernels (scratch bytes, VGPRs, spills) {ks}")
