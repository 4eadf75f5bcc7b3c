"""The wire audio ingest on the host: ops.ingest's torch reference against the f64 oracle
(tests/ingest_oracle.py, which derives the bound), and the filter design itself -- what a tone in
the band comes out as, what a tone that would alias comes out as, and what the two-point linear
interpolation of ops.pcm16_to_f32 makes of the same tones.

Tone levels are measured on one second of a full-scale (32767) PCM16 sine: the RMS of the output's
middle (the first and last 100 ms dropped: the window's edges read zeros) against the RMS of the
sine, in dB.  A tone at or above 9 kHz cannot exist at 16 kHz: whatever comes out of it is an
alias.  0.45 x rate is such a tone for the rates above 20 kHz only -- for a lower rate it lies in the
band the output keeps, so it is not a stop-band case there."""
import math

import numpy as np
import pytest
import torch

import ingest_oracle as O
import voice_enabled_browser_automation_amd.ops as ops
from voice_enabled_browser_automation_amd.asr.wire import SAMPLE_RATES, AudioFormat, FormatError, mono_int16
from voice_enabled_browser_automation_amd.ops import reference as ref

RESAMPLED = [r for r in SAMPLE_RATES if r != 16000]


def run(raw: np.ndarray, fmt: AudioFormat) -> np.ndarray:
    return ops.ingest(torch.from_numpy(raw), fmt).numpy()


def tone(rate: int, hz: float, seconds: float = 1.0) -> np.ndarray:
    n = np.arange(int(rate * seconds))
    return np.round(32767.0 * np.sin(2 * np.pi * hz * n / rate)).astype("<i2")


def level_db(out: np.ndarray, out_rate: int = 16000) -> float:
    mid = out[out_rate // 10: len(out) - out_rate // 10].astype(np.float64)
    rms = math.sqrt(float(np.mean(mid ** 2)))
    return 20 * math.log10(max(rms, 1e-12) / ((32767.0 / 32768.0) / math.sqrt(2)))


def stop_tones(rate: int):
    return sorted({hz for hz in (9000.0, 12000.0, 0.45 * rate) if 9000.0 <= hz < rate / 2})


def test_the_table_is_the_design():
    hs = []
    for rate in SAMPLE_RATES:
        L, M, H = ops.ingest_geometry(rate)
        assert (L, M, H) == O.geometry(rate) and math.gcd(L, M) == 1 and L * rate == M * 16000
        tab = ops.ingest_tables(rate)
        assert tab.dtype == torch.float32 and tuple(tab.shape) == (L, 2 * H) and tab.is_contiguous()
        assert ops.ingest_tables(rate) is tab  # cached
        assert L <= 640 and tab.numel() * 4 <= 80 * 1024
        assert torch.allclose(tab.double().sum(1), torch.ones(L, dtype=torch.float64), atol=2e-6)
        # phase 0 peaks on the sample it sits on; the last phase leans on the next one
        assert int(tab[0].argmax()) == H - 1 and int(tab[L - 1].argmax()) in (H - 1, H)
        hs.append(H)
    assert hs == [16, 16, 16, 16, 23, 24, 32, 45, 48]


@pytest.mark.parametrize("rate", SAMPLE_RATES)
@pytest.mark.parametrize("encoding", O.ENCODINGS)
def test_host_reference_against_the_oracle(encoding, rate):
    g = np.random.default_rng(rate + len(encoding))
    L, M, H = O.geometry(rate)
    tab = ops.ingest_tables(rate).numpy()
    worst = 0.0
    for channels, channel in ((1, None), (2, None), (3, None), (2, 1), (3, 2), (8, None), (8, 5)):
        for n_in, kind in ((1, "noise"), (H - 1, "noise"), (777, "noise"), (333, "max")):
            raw = O.encode_noise(g, n_in, encoding, channels, kind)
            fmt = AudioFormat(encoding, rate, channels, channel)
            got = run(raw, fmt)
            assert len(got) == n_in * L // M == fmt.n_out(n_in)
            worst = max(worst, O.check(got, raw, encoding, rate, channels, channel, tab,
                                       f"{encoding} {rate} C={channels} ch={channel} n={n_in} {kind}"))
    print(f"MEASURED host reference {encoding} {rate}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("law", ("mulaw", "alaw"))
def test_g711_codes_decode_to_the_standards_values(law):
    codes = np.arange(256, dtype=np.uint8)
    want = O.g711_value(codes, law)
    assert want.min() < -32000 and want.max() > 32000 and len(set(want.tolist())) >= 254
    got = run(codes, AudioFormat(law, 16000, 1))
    assert np.array_equal(got, (want / 32768.0).astype(np.float32))
    assert np.array_equal(ref._g711_table(law).numpy(), want)
    assert np.array_equal(mono_int16(codes.tobytes(), AudioFormat(law, 8000, 1)), want.astype(np.int16))


def test_16k_is_a_pass_through_not_a_filter():
    g = np.random.default_rng(5)
    pcm = g.integers(-32767, 32768, 1000).astype("<i2")  # (-32768 has no negative in s16)
    got = run(pcm.view(np.uint8), AudioFormat())
    assert np.array_equal(got, pcm.astype(np.float32) / np.float32(32768.0))
    assert np.array_equal(got, ops.pcm16_to_f32(torch.from_numpy(pcm.astype(np.int16))).numpy())
    st = np.stack([pcm, -pcm], 1).reshape(-1)  # a stereo pair that cancels
    assert not run(st.view(np.uint8), AudioFormat("linear16", 16000, 2)).any()
    assert np.array_equal(run(st.view(np.uint8), AudioFormat("linear16", 16000, 2, 0)), got)


@pytest.mark.parametrize("rate", RESAMPLED)
def test_pass_band_tones_keep_their_level(rate):
    for hz in (1000.0, 3000.0, 6000.0):
        if hz >= rate / 2:
            continue  # (no such tone at this rate)
        db = level_db(run(tone(rate, hz).view(np.uint8), AudioFormat("linear16", rate, 1)))
        print(f"MEASURED {rate} Hz input, {hz:.0f} Hz tone: {db:+.3f} dB")
        assert abs(db) <= 0.1, f"{rate}: a {hz:.0f} Hz tone comes out at {db:+.3f} dB"


@pytest.mark.parametrize("rate", [r for r in RESAMPLED if stop_tones(r)])
def test_stop_band_tones_are_gone_and_linear_interpolation_keeps_them(rate):
    for hz in stop_tones(rate):
        pcm = tone(rate, hz)
        db = level_db(run(pcm.view(np.uint8), AudioFormat("linear16", rate, 1)))
        lin = level_db(ops.pcm16_to_f32(torch.from_numpy(pcm.astype(np.int16)), in_rate=rate).numpy())
        print(f"MEASURED {rate} Hz input, {hz:.0f} Hz tone: ingest {db:+.1f} dB, pcm16_to_f32 {lin:+.1f} dB")
        assert db <= -75.0, f"{rate}: a {hz:.0f} Hz tone aliases at {db:+.1f} dB"
        assert lin > -10.0, f"{rate}: pcm16_to_f32 already removes the {hz:.0f} Hz tone ({lin:+.1f} dB)"


def test_every_rate_above_16k_has_stop_band_cases():
    assert [r for r in RESAMPLED if stop_tones(r)] == [22050, 24000, 32000, 44100, 48000]
    assert stop_tones(48000) == [9000.0, 12000.0, 21600.0] and stop_tones(22050) == [9000.0, 0.45 * 22050]


@pytest.mark.parametrize("rate", RESAMPLED)
def test_positions_are_the_exact_rational_ones(rate):
    """An impulse of 1/2 at input sample j comes out as table[phase_i][j - pos_i + H - 1] / 2 -- one
    exact product -- at every output i whose taps reach j, with (pos, phase) from Fractions: at the
    start of a window and at the end of a full 30 s one."""
    L, M, H = O.geometry(rate)
    tab = ops.ingest_tables(rate).numpy()
    n_in = 30 * rate
    pcm = np.zeros(n_in, dtype="<i2")
    marks = [0, 3 * H, n_in // 2 + 3, n_in - 1 - 3 * H, n_in - 1]  # more than 2H apart: no output sees two
    pcm[marks] = 16384
    got = run(pcm.view(np.uint8), AudioFormat("linear16", rate, 1))
    n_out = n_in * L // M
    assert len(got) == n_out == 480000
    want = np.zeros(n_out, dtype=np.float32)
    near = sorted({i for j in marks for i in range(max(0, (j - H) * L // M - 2), min(n_out, (j + H) * L // M + 3))})
    pos, ph = O.exact_positions(near, rate)
    hit = 0
    for i, p, f in zip(near, pos, ph):
        for j in marks:
            if 0 <= j - p + H - 1 < 2 * H:
                want[i] = np.float32(0.5) * tab[f, j - p + H - 1]  # one product, exact; the other taps add zeros
                hit += 1
    assert hit >= len(marks) * (2 * H * L // M - 1) - 2 * (H * L // M + 1)  # (the window's ends cut two in half)
    assert np.array_equal(got, want)


def test_n_out_is_the_formula():
    for rate in SAMPLE_RATES:
        L, M, _ = O.geometry(rate)
        for n_in in (0, 1, 2, 3, 159, 160, 441, 442, 4099):
            raw = np.zeros(n_in, dtype=np.uint8)
            assert len(run(raw, AudioFormat("mulaw", rate, 1))) == n_in * L // M


def test_formats_and_arguments_are_validated():
    for kw, param in ((dict(encoding="opus"), "encoding"), (dict(sample_rate=16001), "sample_rate"),
                      (dict(sample_rate="8000"), "sample_rate"), (dict(channels=0), "channels"),
                      (dict(channels=9), "channels"), (dict(channels=2, channel=2), "channel"),
                      (dict(channel=-1), "channel")):
        with pytest.raises(FormatError) as ei:
            AudioFormat(**kw)
        assert ei.value.param == param and param in str(ei.value)
    z = torch.zeros(12, dtype=torch.uint8)
    with pytest.raises(ValueError, match="whole frames"):
        ops.ingest(z[:11], AudioFormat("linear16", 16000, 2))
    with pytest.raises(ValueError, match="uint8"):
        ops.ingest(z.to(torch.int8), AudioFormat())
    with pytest.raises(ValueError, match="contiguous"):
        ops.ingest(z[::2], AudioFormat("mulaw", 8000, 1))
    with pytest.raises(ValueError, match="out must be"):
        ops.ingest(z, AudioFormat("mulaw", 8000, 1), out=torch.zeros(23))
    with pytest.raises(ValueError, match="AudioFormat"):
        ops.ingest(z, "mulaw")
    out = torch.full((30,), 7.0)
    got = ops.ingest(z, AudioFormat("mulaw", 8000, 1), out=out)
    assert got.data_ptr() == out.data_ptr() and len(got) == 24 and bool((out[24:] == 7.0).all())
