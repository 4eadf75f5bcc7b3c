"""The wire audio ingest kernels (csrc/ingest/ingest_resample.hip) on the GPU against the f64 oracle
(tests/ingest_oracle.py, which derives the bound): every G.711 code, the three encodings at rates
that upsample, pass through and downsample by a rational and by an integer ratio, 1..3 channels mixed
and selected, and window lengths that are shorter than the filter, that end one output before and
one after a workgroup's 256, and that leave a ragged tail after sixteen workgroups."""
import numpy as np
import pytest
import torch

import ingest_oracle as O
import voice_enabled_browser_automation_amd.ops as ops
from voice_enabled_browser_automation_amd.asr.wire import AudioFormat

pytestmark = pytest.mark.gpu

DEV = "cuda"
RATES = (8000, 16000, 44100, 48000)
MIXES = ((1, None), (2, None), (3, None), (1, 0), (2, 1), (3, 2))  # (channels, channel): downmix, and channel = C - 1


@pytest.fixture(scope="module", autouse=True)
def lib():
    return ops.ingest_ext()  # fail loudly if the library is missing


def gpu(raw: np.ndarray, fmt: AudioFormat, guard: int = 8):
    """ops.ingest on the GPU into a buffer with canaries behind n_out; returns the outputs."""
    n_out = fmt.n_out(len(raw) // fmt.frame_bytes)
    out = torch.full((n_out + guard,), 77.0, dtype=torch.float32, device=DEV)
    got = ops.ingest(torch.from_numpy(raw).to(DEV), fmt, out=out)
    assert len(got) == n_out and (n_out == 0 or got.data_ptr() == out.data_ptr())
    host = out.cpu().numpy()
    assert (host[n_out:] == 77.0).all(), "written past n_out"
    return host[:n_out]


def lengths(rate: int):
    """1, H - 1 (a window shorter than the filter), the input length of 256 outputs -+ 1 (a workgroup
    seam) and 4099 frames (a ragged tail)."""
    L, M, H = O.geometry(rate)
    n256 = -(-256 * M // L)
    assert n256 * L // M == 256
    return (1, H - 1, n256 - 1, n256 + 1, 4099)


@pytest.mark.parametrize("law", ("mulaw", "alaw"))
def test_every_code_is_the_formulas_value(law):
    codes = np.arange(256, dtype=np.uint8)
    want = (O.g711_value(codes, law).astype(np.float64) / 32768.0).astype(np.float32)
    got = gpu(codes, AudioFormat(law, 16000, 1))
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    # ... and as the second channel of two, selected
    two = np.stack([codes[::-1], codes], 1).reshape(-1)
    assert np.array_equal(gpu(two, AudioFormat(law, 16000, 2, 1)).view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("encoding", O.ENCODINGS)
def test_against_the_oracle(encoding, rate):
    g = np.random.default_rng(1000 * O.ENCODINGS.index(encoding) + rate)
    tab = ops.ingest_tables(rate).numpy()
    worst, launches = 0.0, ops.ingest_launches
    for channels, channel in MIXES:
        fmt = AudioFormat(encoding, rate, channels, channel)
        for n_in in lengths(rate):
            raw = O.encode_noise(g, n_in, encoding, channels)
            worst = max(worst, O.check(gpu(raw, fmt), raw, encoding, rate, channels, channel, tab,
                                       f"{encoding} {rate} C={channels} ch={channel} n_in={n_in}"))
        # the all-max-code input: every sample the largest positive value
        raw = O.encode_noise(g, 4099, encoding, channels, "max")
        got = gpu(raw, fmt)
        worst = max(worst, O.check(got, raw, encoding, rate, channels, channel, tab,
                                   f"{encoding} {rate} C={channels} ch={channel} max"))
        if rate != 16000:  # rows sum to 1: away from the edges a constant comes out as itself
            _, _, H = O.geometry(rate)
            mid = got[2 * H: len(got) - 2 * H]
            top = O.values(raw[: fmt.frame_bytes], encoding, channels)[0, 0]
            assert np.abs(mid - top).max() <= 4 * H * O.U * top
    n_launched = ops.ingest_launches - launches
    assert n_launched == len(MIXES) * (len(lengths(rate)) + 1)
    print(f"MEASURED ingest {encoding} {rate}: largest error / bound {worst:.3f} over {n_launched} launches")


@pytest.mark.parametrize("rate", (8000, 44100, 48000))
def test_silence_is_exact_zeros_and_a_stereo_pair_cancels(rate):
    fmt = AudioFormat("linear16", rate, 2)
    assert not gpu(np.zeros(4099 * 4, dtype=np.uint8), fmt).any()
    g = np.random.default_rng(rate)
    x = g.integers(-32767, 32768, 4099).astype("<i2")
    assert not gpu(np.stack([x, -x], 1).reshape(-1).view(np.uint8), fmt).any()


@pytest.mark.parametrize("rate", RATES)
def test_two_launches_give_the_same_bits(rate):
    g = np.random.default_rng(rate)
    fmt = AudioFormat("mulaw", rate, 3)
    raw = O.encode_noise(g, 20011, "mulaw", 3)
    a, b = gpu(raw, fmt), gpu(raw, fmt)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    # ... and the same as a window's worth launched as part of a longer buffer's prefix
    t = torch.from_numpy(np.concatenate([raw, raw])).to(DEV)
    c = ops.ingest(t[: len(raw)], fmt).cpu().numpy()
    assert np.array_equal(a.view(np.int32), c.view(np.int32))


@pytest.mark.parametrize("rate", (44100, 48000))
def test_a_full_window(rate):
    """30 s of stereo, 1875 workgroups, every one reading its own span: checked against the oracle
    at the start, at the end and at 20 000 outputs drawn across the window."""
    g = np.random.default_rng(rate)
    fmt = AudioFormat("linear16", rate, 2)
    raw = O.encode_noise(g, 30 * rate, "linear16", 2)
    got = gpu(raw, fmt)
    assert len(got) == 480000
    pick = np.unique(np.concatenate([np.arange(1024), np.arange(480000 - 1024, 480000),
                                     g.integers(0, 480000, 20000)]))
    want, bound = O.ingest(raw, "linear16", rate, 2, None, ops.ingest_tables(rate).numpy(), outputs=pick)
    err = np.abs(got[pick].astype(np.float64) - want)
    assert (err <= bound).all(), f"{int((err > bound).sum())} outputs off; first at {int(pick[np.argmax(err > bound)])}"
    print(f"MEASURED ingest 30 s {rate} Hz stereo: largest error / bound {float((err / bound).max()):.3f}")
