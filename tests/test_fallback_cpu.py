"""Whisper's quality gate and temperature fallback on the host (asr/fallback.py), the streaming
session's use of it with a fake recogniser, the voice server's counters, the engine's retry loop on
the CPU build, and the CPU reference of ops.score_step against the f64 oracle."""
import math
import zlib
from concurrent.futures import Future

import numpy as np
import pytest

import score_oracle as so
from voice_enabled_browser_automation_amd.asr import fallback as fb
from voice_enabled_browser_automation_amd.asr.fallback import FallbackPolicy
from voice_enabled_browser_automation_amd.asr.streaming import Hypothesis, StreamingAsrSession


# ----------------------------------------------------------------------------- the rule
def test_compression_ratio_is_whispers():
    for text in ("click " * 40, "open the third result and scroll down to the reviews", "é" * 30):
        raw = text.encode("utf-8")
        assert fb.compression_ratio(text) == len(raw) / len(zlib.compress(raw))
    assert fb.compression_ratio("click " * 40) > 2.4 > fb.compression_ratio("open the third result and scroll down")


def test_avg_logprob_divides_by_the_text_tokens_plus_one():
    assert fb.avg_logprob(-6.0, 5) == -1.0 and fb.avg_logprob(-3.0, 0) == -3.0
    e = fb.score_entry(-6.0, 5, 0.4, 3)
    assert e == dict(sum_logprob=-6.0, tokens=5, avg_logprob=-1.0, temperature=0.4, attempts=3, passed=True,
                     failed_on=None)


def test_the_verdict_per_threshold():
    p = FallbackPolicy()
    loop, fine = "click " * 40, "open the third result"
    assert fb.needs_fallback(-0.5, fine, p) == (False, None)
    assert fb.needs_fallback(-1.0, fine, p) == (False, None)  # (below the threshold, not at it)
    assert fb.needs_fallback(-1.01, fine, p) == (True, "logprob")
    assert fb.needs_fallback(-0.1, loop, p) == (True, "compression_ratio")
    assert fb.needs_fallback(-5.0, loop, p) == (True, "compression_ratio")  # (Whisper tests it first)
    assert fb.needs_fallback(float("-inf"), fine, p) == (True, "logprob")
    assert fb.needs_fallback(float("nan"), fine, p) == (True, "logprob")
    assert fb.needs_fallback(-0.1, "", p) == (False, None)
    no_lp = FallbackPolicy(logprob_threshold=None)
    assert fb.needs_fallback(-50.0, fine, no_lp) == (False, None)
    assert fb.needs_fallback(-50.0, loop, no_lp) == (True, "compression_ratio")
    no_cr = FallbackPolicy(compression_ratio_threshold=None)
    assert fb.needs_fallback(-0.1, loop, no_cr) == (False, None)
    assert fb.needs_fallback(-2.0, loop, no_cr) == (True, "logprob")
    assert fb.needs_fallback(-99.0, loop, FallbackPolicy(logprob_threshold=None,
                                                        compression_ratio_threshold=None)) == (False, None)


def test_policy_validation():
    p = FallbackPolicy()
    assert p.temperatures == (0.0, 0.2, 0.4, 0.6, 0.8, 1.0) and (p.logprob_threshold, p.compression_ratio_threshold) \
        == (-1.0, 2.4)
    assert FallbackPolicy(temperatures=[0, 0, 2]).temperatures == (0.0, 0.0, 2.0)
    assert hash(FallbackPolicy()) == hash(FallbackPolicy())
    for bad in ((), (0.2, 0.1), (-0.1,), (0, 2.5), tuple(range(9)), (float("nan"),), "abc", (0, None)):
        with pytest.raises(ValueError, match="temperatures"):
            FallbackPolicy(temperatures=bad)
    with pytest.raises(ValueError, match="logprob_threshold"):
        FallbackPolicy(logprob_threshold=0.5)
    with pytest.raises(ValueError, match="compression_ratio_threshold"):
        FallbackPolicy(compression_ratio_threshold=0.0)
    assert fb.parse_temperatures("0, 0.2,0.4") == (0.0, 0.2, 0.4)
    with pytest.raises(ValueError, match="temperatures"):
        fb.parse_temperatures("0,x")


def test_the_retry_loop_with_a_fake_decoder():
    """Utterance 0 passes at once; 1 passes at the third temperature; 2 never passes; 3 fails but
    the no-speech gate rejects it, so it is not retried."""
    policy = FallbackPolicy(temperatures=(0.0, 0.4, 0.8), compression_ratio_threshold=None)
    calls = []
    table = {0: [-0.2], 1: [-3.0, -2.0, -0.5], 2: [-4.0, -5.0, -6.0], 3: [-9.0]}

    def attempt(utts, T):
        k = len(calls)
        calls.append((list(utts), T))
        return [(table[j][k] * 5, 4, f"text {j} {k}") for j in utts]

    out = fb.run(attempt, 4, policy, gated=lambda i: i == 3)
    assert calls == [([0, 1, 2, 3], 0.0), ([1, 2], 0.4), ([1, 2], 0.8)]
    assert [(e["attempts"], e["temperature"], e["passed"], e["failed_on"]) for e in out] == \
        [(1, 0.0, True, None), (3, 0.8, True, None), (3, 0.8, False, "logprob"), (1, 0.0, False, "logprob")]
    assert out[1]["avg_logprob"] == -0.5 and out[2]["sum_logprob"] == -30.0 and out[2]["tokens"] == 4
    # it stops at the first pass: nothing is decoded once everyone passed
    calls.clear()
    table = {0: [-0.2], 1: [-0.3]}
    out = fb.run(attempt, 2, policy)
    assert calls == [([0, 1], 0.0)] and all(e["passed"] and e["attempts"] == 1 for e in out)


# ----------------------------------------------------------------------------- the engine's loop (CPU build)
def test_the_engine_retries_the_rejected_utterances_on_the_kept_encoder_output():
    import beam_cases
    from voice_enabled_browser_automation_amd.asr.engine import AsrEngine
    from voice_enabled_browser_automation_amd.models.config import get_config
    from voice_enabled_browser_automation_amd.models.whisper import WhisperModel
    from voice_enabled_browser_automation_amd.tokenizer import load_tokenizer

    model = WhisperModel(get_config("whisper-test"), device="cpu", seed=3)
    eng = AsrEngine(model, load_tokenizer("whisper"), max_sessions=4)
    aud = [eng.pcm_to_audio(beam_cases.tone(s, f)) for s, f in beam_cases.TONES]
    plain = eng.decode_many(aud, max_tokens=6)
    assert eng._score_bufs is None and eng.last_scores == []  # nothing of the feature before its first call
    free = list(eng.free_slots)
    with pytest.raises(ValueError, match="beam_size"):
        eng.decode_many(aud[:1], max_tokens=6, beam_size=2, score=True)
    assert eng.free_slots == free and eng._score_bufs is None
    assert eng.decode_many(aud, max_tokens=6, score=True) == plain
    base = [s["avg_logprob"] for s in eng.last_scores]
    assert all(s["attempts"] == 1 and s["passed"] and s["temperature"] == 0.0 and s["tokens"] == 6
               for s in eng.last_scores)
    order = sorted(range(3), key=lambda i: base[i])
    thr = (base[order[0]] + base[order[1]]) / 2
    calls = []
    real = model.encode
    model.encode = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        policy = FallbackPolicy(temperatures=(0.0, 0.5, 1.0), logprob_threshold=thr, compression_ratio_threshold=None)
        outs = eng.decode_many(aud, max_tokens=6, fallback=policy)
    finally:
        model.encode = real
    assert len(calls) == 1
    sc = eng.last_scores
    for i in range(3):
        if i == order[0]:
            assert sc[i]["attempts"] >= 2 and sc[i]["temperature"] in (0.5, 1.0)
            assert sc[i]["passed"] == (sc[i]["avg_logprob"] >= thr)
        else:
            assert sc[i]["attempts"] == 1 and sc[i]["passed"] and outs[i] == plain[i] and sc[i]["avg_logprob"] == base[i]
    assert eng.last_stats["retried"] == sc[order[0]]["attempts"] - 1
    assert sorted(eng.free_slots) == sorted(free)
    with pytest.raises(ValueError, match="temperatures"):
        eng.decode_many(aud, max_tokens=6, temperatures=[0.1])
    with pytest.raises(ValueError, match="temperatures"):
        eng.decode_many(aud, max_tokens=6, temperatures=[0, 0, 0], fallback=policy)
    with pytest.raises(TypeError, match="FallbackPolicy"):
        eng.decode_many(aud, max_tokens=6, fallback=True)
    assert eng.decode_many(aud, max_tokens=6) == plain


# ----------------------------------------------------------------------------- streaming
def _tone(seconds, amp=8000):
    t = np.arange(int(seconds * 16000)) / 16000
    return (np.sin(2 * np.pi * 180 * t) * amp).astype(np.int16)


def _feed(sess, pcm, pkt=960):
    ev = []
    for i in range(0, len(pcm), pkt):
        ev += sess.push(pcm[i:i + pkt].tobytes())
    return ev


class ScriptedRec:
    """Every pass pops the next (text, avg_logprob, attempts, passed) of the script; it records
    the keywords each pass came with."""

    def __init__(self, script):
        self.script = list(script)
        self.kw = []

    def recognize(self, pcm, prefix=(), **kw):
        self.kw.append(kw)
        text, avg, attempts, passed = self.script.pop(0)
        hyp = Hypothesis([1, 2], text)
        if kw.get("fallback") is not None:
            hyp.score = dict(sum_logprob=avg * 3, tokens=2, avg_logprob=avg, temperature=0.2 * (attempts - 1),
                             attempts=attempts, passed=passed, failed_on=None if passed else "logprob")
            hyp.confidence = math.exp(avg)
        return hyp

    def recognize_async(self, pcm, prefix=(), **kw):
        f = Future()
        f.set_result(self.recognize(pcm, prefix, **kw))
        return f


def _session(rec, **kw):
    a = dict(partial_every_s=0.5, endpoint_silence_s=0.3, spec_silence_s=0.0, energy_threshold=300)
    a.update(kw)
    return StreamingAsrSession(rec, **a)


def _finals(ev):
    return [e for e in ev if e.get("is_final")]


def test_finals_carry_the_returned_attempts_confidence_and_partials_stay_unscored():
    rec = ScriptedRec([("open", -0.1, 1, True), ("open the", -0.3, 2, True)])
    s = _session(rec, fallback=True)
    assert isinstance(s.fallback, FallbackPolicy) and s.fallback == FallbackPolicy()
    ev = _feed(s, _tone(0.7)) + _feed(s, np.zeros(8000, np.int16))
    assert "fallback" not in rec.kw[0] and rec.kw[-1]["fallback"] is s.fallback
    (f,) = _finals(ev)
    alt = f["channel"]["alternatives"][0]
    assert alt["transcript"] == "open the" and alt["confidence"] == math.exp(-0.3)
    assert set(f) == {"type", "channel_index", "duration", "start", "is_final", "speech_final", "channel", "metadata"}
    assert (s.stats["fallback_passes"], s.stats["fallback_retries"], s.stats["fallback_rejected"]) == (1, 1, 0)
    # off (the default): no pass carries the keyword, the confidence is what it was
    rec = ScriptedRec([("open", 0, 1, True), ("open the", 0, 1, True)])
    s = _session(rec)
    assert s.fallback is None
    (f,) = _finals(_feed(s, _tone(0.7)) + _feed(s, np.zeros(8000, np.int16)))
    assert all("fallback" not in kw for kw in rec.kw) and f["channel"]["alternatives"][0]["confidence"] == 0.0
    assert s.stats["fallback_passes"] == 0


def test_a_speculative_final_is_adopted_only_when_it_passed():
    policy = FallbackPolicy(temperatures=(0.0, 0.3, 0.6))
    # it passed: it is the final, no pass after the endpoint
    rec = ScriptedRec([("go back", -0.2, 1, True)])
    s = _session(rec, fallback=policy, partial_every_s=10.0, spec_silence_s=0.12)
    spoken = []
    s.on_speculative = spoken.append
    (f,) = _finals(_feed(s, _tone(1.0)) + _feed(s, np.zeros(8000, np.int16)))
    assert len(rec.kw) == 1 and rec.kw[0]["fallback"].temperatures == (0.0,)
    assert rec.kw[0]["fallback"].logprob_threshold == policy.logprob_threshold
    assert f["channel"]["alternatives"][0]["transcript"] == "go back" and spoken == ["go back"]
    assert s.stats["spec_used"] == 1 and s.stats["spec_rejected"] == 0
    # it failed: the real final pass runs with the whole schedule, and the brain was not started on it
    rec = ScriptedRec([("click click", -3.0, 1, False), ("click", -0.4, 3, True)])
    s = _session(rec, fallback=policy, partial_every_s=10.0, spec_silence_s=0.12)
    spoken = []
    s.on_speculative = spoken.append
    (f,) = _finals(_feed(s, _tone(1.0)) + _feed(s, np.zeros(8000, np.int16)))
    assert [kw["fallback"].temperatures for kw in rec.kw] == [(0.0,), (0.0, 0.3, 0.6)]
    assert f["channel"]["alternatives"][0]["transcript"] == "click" and spoken == []
    assert f["channel"]["alternatives"][0]["confidence"] == math.exp(-0.4)
    assert s.stats["spec_rejected"] == 1 and s.stats["fallback_retries"] == 2


def test_fallback_reject_empties_a_final_whose_last_attempt_fails():
    script = [("delete everything", -4.0, 6, False)]
    s = _session(ScriptedRec(script), fallback=True, fallback_reject=True, partial_every_s=10.0)
    (f,) = _finals(_feed(s, _tone(0.7)) + _feed(s, np.zeros(8000, np.int16)))
    assert f["channel"]["alternatives"][0]["transcript"] == "" and f["channel"]["alternatives"][0]["confidence"] == 0.0
    assert (s.stats["fallback_rejected"], s.stats["fallback_retries"], s.stats["fallback_passes"]) == (1, 5, 1)
    # without the setting the last attempt is emitted, as Whisper does
    s = _session(ScriptedRec(script), fallback=True, partial_every_s=10.0)
    assert not s.fallback_reject
    (f,) = _finals(_feed(s, _tone(0.7)) + _feed(s, np.zeros(8000, np.int16)))
    assert f["channel"]["alternatives"][0]["transcript"] == "delete everything" and s.stats["fallback_rejected"] == 0


def test_the_settings_build_the_policy(monkeypatch):
    from voice_enabled_browser_automation_amd.utils import env

    assert env.knob("VWA_ASR_FALLBACK") is False and env.knob("VWA_ASR_FALLBACK_REJECT") is False
    assert (env.knob("VWA_ASR_TEMPERATURES"), env.knob("VWA_ASR_LOGPROB_THRESHOLD"),
            env.knob("VWA_ASR_COMPRESSION_RATIO")) == ("0,0.2,0.4,0.6,0.8,1.0", -1.0, 2.4)
    for name in ("VWA_ASR_LOGPROB_THRESHOLD", "VWA_ASR_COMPRESSION_RATIO"):
        assert "NOT tuned" in env.Settings.model_fields[name].description
    monkeypatch.setenv("VWA_ASR_FALLBACK", "1")
    monkeypatch.setenv("VWA_ASR_TEMPERATURES", "0,0.5")
    monkeypatch.setenv("VWA_ASR_LOGPROB_THRESHOLD", "-0.7")
    monkeypatch.setenv("VWA_ASR_FALLBACK_REJECT", "1")
    s = StreamingAsrSession(lambda pcm: "x")
    assert s.fallback == FallbackPolicy(temperatures=(0.0, 0.5), logprob_threshold=-0.7) and s.fallback_reject
    monkeypatch.setenv("VWA_ASR_TEMPERATURES", "0.5,0.2")
    with pytest.raises(ValueError, match="temperatures"):
        StreamingAsrSession(lambda pcm: "x")
    assert StreamingAsrSession(lambda pcm: "x", fallback=False).fallback is None


def test_the_batcher_batches_fallback_passes_among_themselves():
    from voice_enabled_browser_automation_amd.asr.streaming import AsrBatcher

    calls = []

    class Eng:
        free_slots = list(range(8))
        last_scores = []
        last_sot = []
        model = type("M", (), {"device": None, "cfg": type("C", (), {"eot": 50256, "no_timestamps": 50362,
                                                                      "n_text_ctx": 448})()})()
        tok = type("T", (), {"decode": staticmethod(lambda ids: " ".join(map(str, ids)))})()

        def max_prefix(self):
            return 400

        def pcm_to_audio(self, pcm):
            return pcm

        def decode_many(self, audios, prefixes=None, **kw):
            calls.append((len(audios), kw.get("fallback")))
            if kw.get("fallback") is not None:
                self.last_scores = [fb.score_entry(-1.0 * (i + 1), 1, 0.2, 2) for i in range(len(audios))]
            return [[7] for _ in audios]

    b = AsrBatcher(Eng(), words=False)
    try:
        policy = FallbackPolicy()
        with b._cv:  # (queue all four before the scheduler takes a round)
            futs = []
            for fbk in (None, policy, None, FallbackPolicy()):
                fut = Future()
                b._q.append((np.zeros(160, np.int16), [], fut, False, None, 1, None, False, fbk))
                futs.append(fut)
            b._cv.notify()
        hyps = [f.result(timeout=10) for f in futs]
    finally:
        b.close()
    assert sorted(calls, key=lambda c: c[1] is not None) == [(2, None), (2, policy)]
    assert hyps[0].score is None and hyps[0].confidence == 0.0
    assert hyps[1].score["avg_logprob"] == -0.5 and hyps[1].confidence == math.exp(-0.5)
    assert hyps[3].score["avg_logprob"] == -1.0 and hyps[3].score["attempts"] == 2
    assert b.stats["fallback_passes"] == 2
    # a beam or timestamp pass drops the policy
    b2 = AsrBatcher(Eng(), words=False)
    try:
        f = b2.recognize_async(np.zeros(160, np.int16), (), timestamps=True, fallback=policy)
        f.result(timeout=10)
    finally:
        b2.close()
    assert calls[-1][1] is None


def test_the_voice_server_counts_the_fallback():
    """/metrics: asr_fallback_passes / asr_fallback_retries / asr_fallback_rejected follow the
    session's counters (voice/server.py count_boosted)."""
    import asyncio
    import json

    from aiohttp.test_utils import TestClient, TestServer

    from voice_enabled_browser_automation_amd.voice.server import build_app

    class Session:
        def __init__(self):
            self.stats = {"fallback_passes": 0, "fallback_retries": 0, "fallback_rejected": 0}

        def push(self, data):
            self.stats["fallback_passes"] += 1
            self.stats["fallback_retries"] += 2
            self.stats["fallback_rejected"] += 1
            return [{"type": "Results", "is_final": False, "channel": {"alternatives": [{"transcript": "x"}]}}]

        def flush(self):
            return []

    async def go():
        app = build_app(lambda: Session(), brain_url="http://127.0.0.1:9/parse", executor_url="http://127.0.0.1:9",
                        debounce_ms=60000)
        async with TestClient(TestServer(app)) as c:
            ws = await c.ws_connect("/stream")
            for _ in range(2):
                json.loads((await ws.receive(timeout=5.0)).data)
            for _ in range(2):
                await ws.send_bytes(b"\0" * 320)
                assert json.loads((await ws.receive(timeout=5.0)).data)["type"] == "transcript_partial"
            snap = await (await c.get("/metrics")).json()
            assert snap["counters"]["asr_fallback_passes"] == 2 and snap["counters"]["asr_fallback_retries"] == 4
            assert snap["counters"]["asr_fallback_rejected"] == 2 and "asr_boosted_passes" not in snap["counters"]
            await ws.close()

    asyncio.run(go())


# ----------------------------------------------------------------------------- the CPU reference
@pytest.mark.parametrize("vocab,rows,per_row", [(1, 3, True), (31, 1, False), (33, 3, True), (257, 64, False),
                                                (257, 9, True)])
def test_the_cpu_reference_matches_the_oracle(vocab, rows, per_row):
    for shift in range(len(so.ROLES)):
        case = so.make_case(rows, vocab, vocab + 3, per_row, seed=31 * vocab + shift, shift=shift)
        so.check(case, so.launch(case, "cpu"), f"V={vocab} shift={shift}")
        so.check(case, so.launch(case, "cpu", in_place=True, with_lp=False), f"V={vocab} shift={shift} in place")
