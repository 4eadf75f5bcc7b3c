"""The wire format from the query string to the session, with fake recognisers: what /stream refuses
(HTTP 400 before the upgrade, the JSON body naming the parameter), what a session with a format does
with packets that end inside a frame, what clock its events run on, that the router passes the
options on, and that a connection without them is served exactly as before."""
import asyncio
import json

import aiohttp
import numpy as np
import pytest
from aiohttp.test_utils import TestClient, TestServer

import ingest_oracle as O
from voice_enabled_browser_automation_amd.asr.streaming import Hypothesis, StreamingAsrSession, results_event
from voice_enabled_browser_automation_amd.asr.wire import (AudioFormat, FormatError, WireAudio, decode_int16,
                                                           format_from_query, mono_int16)
from voice_enabled_browser_automation_amd.voice.router import build_router
from voice_enabled_browser_automation_amd.voice.server import build_app

REFUSED = [("encoding=opus", "encoding"), ("encoding=flac&sample_rate=16000", "encoding"), ("encoding=", "encoding"),
           ("sample_rate=16001", "sample_rate"), ("sample_rate=96000", "sample_rate"), ("sample_rate=8k", "sample_rate"),
           ("encoding=mulaw&sample_rate=0", "sample_rate"), ("channels=0", "channels"), ("channels=9", "channels"),
           ("channels=two", "channels"), ("channels=2&channel=2", "channel"), ("channel=1", "channel"),
           ("channels=2&channel=-1", "channel"), ("multichannel=true", "multichannel"),
           ("encoding=mulaw&sample_rate=8000&channels=2&multichannel=true", "multichannel")]


class Recorder:
    """A session double that remembers the format it was made with."""

    made = []

    def __init__(self, keyterms=None, fmt=None):
        self.fmt, self.bytes = fmt, 0
        Recorder.made.append(self)

    def push(self, data):
        self.bytes += len(data)
        return [results_event(f"{self.bytes}", is_final=True, start=0, duration=1.0, model="fake")]

    def flush(self):
        return []


class OldAsr:
    """A recogniser from before the wire options: its factory takes no ``fmt``."""

    def push(self, data):
        return [results_event("partial", is_final=False, start=0, duration=0.06, model="fake")]

    def flush(self):
        return []


def _app(factory):
    return build_app(factory, brain_url="http://127.0.0.1:9/parse", executor_url="http://127.0.0.1:9",
                     debounce_ms=60000)


def test_the_query_is_read_in_one_place():
    assert format_from_query({}) is None and format_from_query({"keyterm": "x", "multichannel": "false"}) is None
    assert format_from_query({"encoding": "mulaw", "sample_rate": "8000"}) == AudioFormat("mulaw", 8000, 1)
    assert format_from_query({"sample_rate": "48000", "channels": "2", "channel": "1"}) == \
        AudioFormat("linear16", 48000, 2, 1)
    assert format_from_query({"encoding": "ALAW"}) == AudioFormat("alaw", 16000, 1)
    assert format_from_query({"encoding": "linear16"}) == AudioFormat() and AudioFormat().is_default
    for qs, param in REFUSED:
        with pytest.raises(FormatError) as ei:
            format_from_query(dict(kv.split("=") for kv in qs.split("&")))
        assert ei.value.param == param, qs


def test_every_refused_parameter_is_a_400_before_the_upgrade():
    async def go():
        Recorder.made = []
        async with TestClient(TestServer(_app(lambda keyterms=None, fmt=None: Recorder(keyterms, fmt)))) as c:
            for qs, param in REFUSED:
                r = await c.get("/stream?" + qs)
                body = await r.json()
                assert r.status == 400 and body["error"] == "unsupported_audio_format" and body["param"] == param, qs
                assert param in body["message"], body
                with pytest.raises(aiohttp.WSServerHandshakeError) as ei:
                    await c.ws_connect("/stream?" + qs)
                assert ei.value.status == 400
            assert Recorder.made == []
            m = await (await c.get("/metrics")).json()
            assert m["counters"]["asr_wire_rejected"] == 2 * len(REFUSED) and "connections" not in m["counters"]
        # a recogniser that cannot take a format refuses every format, and still serves the plain stream
        async with TestClient(TestServer(_app(lambda: OldAsr()))) as c:
            r = await c.get("/stream?encoding=mulaw&sample_rate=8000")
            assert r.status == 400 and (await r.json())["param"] == "encoding"
            ws = await c.ws_connect("/stream")
            assert json.loads((await ws.receive()).data) == {"type": "info", "payload": "deepgram_connected"}
            await ws.close()

    asyncio.run(go())


def test_the_session_gets_the_format_and_the_counters_count():
    async def go():
        Recorder.made = []
        async with TestClient(TestServer(_app(lambda keyterms=None, fmt=None: Recorder(keyterms, fmt)))) as c:
            ws = await c.ws_connect("/stream?encoding=mulaw&sample_rate=8000&keyterm=Grafana")
            assert json.loads((await ws.receive()).data) == {"type": "info", "payload": "deepgram_connected"}
            assert json.loads((await ws.receive()).data) == {"type": "info", "payload": {"state": "open"}}
            await ws.send_bytes(b"\xff" * 481)
            fin = json.loads((await ws.receive()).data)
            assert fin["type"] == "transcript_final"
            await ws.close()
            ws = await c.ws_connect("/stream?sample_rate=48000&channels=2&channel=1")
            await ws.receive()
            await ws.close()
            ws = await c.ws_connect("/stream")
            await ws.receive()
            await ws.send_bytes(b"\0" * 100)
            await ws.receive()
            await ws.close()
            assert [r.fmt for r in Recorder.made] == [AudioFormat("mulaw", 8000, 1), AudioFormat("linear16", 48000, 2, 1),
                                                      None]
            m = (await (await c.get("/metrics")).json())["counters"]
            assert m['asr_wire_sessions{encoding="mulaw",sample_rate="8000"}'] == 1
            assert m['asr_wire_sessions{encoding="linear16",sample_rate="48000"}'] == 1
            assert m["asr_wire_bytes"] == 481 and m["connections"] == 3 and m["audio_frames"] == 2

    asyncio.run(go())


def test_a_connection_without_parameters_sends_exactly_todays_frames():
    """The same packets through a factory that knows nothing of formats (called with no arguments,
    as ever) and through one that does (and gets fmt=None -- no format): the same frames, and they are
    the frames tests/test_voice_server.py pins."""
    async def frames(factory):
        async with TestClient(TestServer(_app(factory))) as c:
            ws = await c.ws_connect("/stream")
            got = [json.loads((await ws.receive()).data) for _ in range(2)]
            for _ in range(3):
                await ws.send_bytes(b"\x01\x00" * 960)
                got.append(json.loads((await ws.receive()).data))
            await ws.close()
            m = (await (await c.get("/metrics")).json())["counters"]
            return got, {k: v for k, v in m.items() if k.startswith("asr_wire")}

    seen = []

    def aware(keyterms=None, fmt=None):
        seen.append(fmt)
        return OldAsr()

    old, m_old = asyncio.run(frames(lambda: OldAsr()))
    new, m_new = asyncio.run(frames(aware))
    assert old == new and seen == [None] and m_old == m_new == {}
    assert old[:2] == [{"type": "info", "payload": "deepgram_connected"}, {"type": "info", "payload": {"state": "open"}}]
    assert [f["type"] for f in old[2:]] == ["transcript_partial"] * 3


def test_the_router_forwards_the_options_and_refuses_what_a_worker_would():
    async def go():
        Recorder.made = []
        worker = TestServer(_app(lambda keyterms=None, fmt=None: Recorder(keyterms, fmt)))
        await worker.start_server()
        router = TestServer(build_router([str(worker.make_url(""))], probe_s=60, max_fails=1))
        await router.start_server()
        async with aiohttp.ClientSession() as http:
            r = await http.get(router.make_url("/stream?encoding=opus"))
            assert r.status == 400 and (await r.json())["param"] == "encoding"
            r = await http.get(router.make_url("/stream?multichannel=true"))
            assert r.status == 400 and (await r.json())["param"] == "multichannel"
            ws = await http.ws_connect(router.make_url("/stream?encoding=alaw&sample_rate=8000&channels=2&channel=0"))
            await ws.send_bytes(b"\x55" * 64)
            while True:
                msg = json.loads((await ws.receive(timeout=10)).data)
                if msg["type"] == "transcript_final":
                    break
            assert msg["payload"]["channel"]["alternatives"][0]["transcript"] == "64"
            await ws.close()
            assert [r.fmt for r in Recorder.made] == [AudioFormat("alaw", 8000, 2, 0)]
            h = await (await http.get(router.make_url("/health"))).json()
            assert h["healthy_workers"] == 1  # a refused format is not a dead worker
        await router.close()
        await worker.close()

    asyncio.run(go())


# ----------------------------------------------------------------------------- the session
class WireRec:
    """A recogniser double for sessions with a format: the transcript names the window it was given."""

    def __init__(self):
        self.seen = []

    def recognize(self, pcm, prefix=(), **kw):
        assert isinstance(pcm, WireAudio)
        self.seen.append((pcm.fmt, pcm.raw.tobytes()))
        return Hypothesis([], f"{pcm.n_frames} frames {len(pcm)} samples")


class PcmRec:
    def recognize(self, pcm, prefix=(), **kw):
        assert isinstance(pcm, np.ndarray) and pcm.dtype == np.int16
        return Hypothesis([], f"{len(pcm)} frames {len(pcm) * 2} samples")


def _encode(values: np.ndarray, law: str) -> np.ndarray:
    """The law's nearest code for every int16 value (by search over the standard's 256 values)."""
    table = O.g711_value(np.arange(256), law)
    order = np.argsort(table)
    sv = table[order]
    k = np.clip(np.searchsorted(sv, values), 1, 255)
    k = np.where(np.abs(sv[k - 1] - values) <= np.abs(sv[k] - values), k - 1, k)
    return order[k].astype(np.uint8)


def _speech(rate: int, channels: int = 1, seed: int = 3) -> np.ndarray:
    """0.5 s of silence, 1.5 s of loud noise, 0.7 s of silence; int16 [n, channels]."""
    g = np.random.default_rng(seed)
    n0, n1, n2 = rate // 2, 3 * rate // 2, 7 * rate // 10
    x = np.concatenate([np.zeros((n0, channels)), g.integers(-12000, 12000, (n1, channels)),
                        np.zeros((n2, channels))])
    return x.astype(np.int16)


def _session(rec, **kw):
    return StreamingAsrSession(rec, partial_every_s=0.5, endpoint_silence_s=0.3, spec_silence_s=0.0,
                               energy_threshold=300.0, noise_mult=0.0, **kw)


def _drive(s, packets):
    out = []
    for p in packets:
        out += s.push(p)
    return out + s.flush()


def test_packets_that_end_inside_a_frame_change_nothing():
    """mu-law at 8 kHz, two channels (a frame is two bytes): the stream as 60 ms packets, and the same
    bytes cut at odd offsets -- every packet's first byte sent alone; every packet boundary one byte
    late, then one byte early.  The odd byte waits for the rest of its frame, so every
    push hands the session the same whole frames as the uncut stream did (the VAD's 20 ms frames
    start with a push, so a cut at a whole frame would move them: that is today's session too), and
    the events, the session's counters and every window the recogniser was given are the same."""
    fmt = AudioFormat("mulaw", 8000, 2)
    wire = _encode(_speech(8000, 2).reshape(-1), "mulaw").tobytes()
    step = 960  # 60 ms of two-byte frames
    whole = [wire[i: i + step] for i in range(0, len(wire), step)]
    ends = [min(len(wire), (k + 1) * step + (1 if k % 2 == 0 else 0)) for k in range(len(whole))]
    shifted = [wire[a:b] for a, b in zip([0] + ends[:-1], ends[:-1] + [len(wire)])]
    assert b"".join(shifted) == wire
    results = []
    for cut in ("none", "first byte", "late and early"):
        packets = {"none": whole, "first byte": [q for p in whole for q in (p[:1], p[1:])],
                   "late and early": shifted}[cut]
        assert cut == "none" or sum(len(p) % 2 for p in packets) > len(whole) // 2
        rec = WireRec()
        s = _session(rec, fmt=fmt)
        ev = _drive(s, packets)
        results.append((ev, rec.seen, {k: v for k, v in s.stats.items() if k != "asr_ms"}))
        assert s._carry == b""
    base = results[0]
    flags = [e["is_final"] for e in base[0]]
    assert len(flags) >= 3 and flags[-1] and not any(flags[:-1]), base[0]  # partials, then the final
    assert all(fmt_ == fmt and len(raw) % 2 == 0 for fmt_, raw in base[1])
    for r in results[1:]:
        assert r == base


@pytest.mark.parametrize("fmt", [AudioFormat("mulaw", 8000, 1), AudioFormat("alaw", 8000, 2, 1),
                                 AudioFormat("linear16", 44100, 2)], ids=str)
def test_start_and_duration_are_seconds_of_audio(fmt):
    """A session with a format against a plain PCM16 session at the same rate fed the decoded mono
    samples: the same events at the same times, so every time the session tells -- start, duration,
    the endpoint, the minimum speech -- runs on the format's own sample rate."""
    rate = fmt.sample_rate
    x = _speech(rate, fmt.channels)
    if fmt.encoding == "linear16":
        wire = x.astype("<i2").tobytes()
    else:
        wire = _encode(x.reshape(-1), fmt.encoding).tobytes()
    mono = mono_int16(wire, fmt)
    assert np.array_equal(decode_int16(wire, fmt).shape, x.shape)
    ms60 = 60 * rate // 1000
    a = _drive(_session(WireRec(), fmt=fmt),
               [wire[i: i + ms60 * fmt.frame_bytes] for i in range(0, len(wire), ms60 * fmt.frame_bytes)])
    pcm = mono.astype("<i2").tobytes()
    b = _drive(_session(PcmRec(), rate=rate), [pcm[i: i + ms60 * 2] for i in range(0, len(pcm), ms60 * 2)])
    assert len(a) == len(b) >= 2 and a[-1]["is_final"]

    def strip(ev):
        ev = json.loads(json.dumps(ev))
        ev["channel"]["alternatives"][0]["transcript"] = ""
        return ev

    assert [strip(e) for e in a] == [strip(e) for e in b]
    fin = a[-1]
    # the leading 0.5 s: 0.3 s of it is dropped at the endpoint, so the utterance starts at 0.3 s; the
    # final fires 0.3 s into the trailing silence: 0.2 + 1.5 + 0.3 s of audio, to within a VAD frame
    assert abs(fin["start"] - 0.3) <= 0.021 and abs(fin["duration"] - 2.0) <= 0.021, fin
    n = round(fin["duration"] * rate)
    assert fin["channel"]["alternatives"][0]["transcript"] == f"{n} frames {fmt.n_out(n)} samples"


def test_without_a_format_the_session_is_todays():
    s = _session(PcmRec())
    assert s.fmt is None and s.rate == 16000 and s._pcm.dtype == np.int16 and s._pcm.ndim == 1
    x = _speech(16000)[:, 0].astype("<i2").tobytes()
    ev = _drive(s, [x[i: i + 1921] for i in range(0, len(x), 1921)])  # (odd packets: the carry is a byte)
    assert ev and ev[-1]["is_final"] and isinstance(s.buf, np.ndarray)
    assert abs(ev[-1]["duration"] - 2.0) <= 0.021
