"""Timestamp decoding without a GPU: the Python reference step (ops/reference.py ts_rules_step)
against the f64 oracle over every state class, a greedy walk under the rules, the segment helpers,
the engine on whisper-test, the long-form cut of the streaming session with a scripted recognizer,
and the voice server's handling of a final whose speaker has not stopped."""
import asyncio
import json

import numpy as np
import pytest
import torch
from aiohttp import web
from aiohttp.test_utils import TestClient, TestServer

import beam_cases
import tsrules_cases as tc
import tsrules_oracle as to
import voice_enabled_browser_automation_amd.ops as ops
from voice_enabled_browser_automation_amd.asr import segments as sg
from voice_enabled_browser_automation_amd.asr.engine import TS_MAX_INITIAL, AsrEngine, ts_state
from voice_enabled_browser_automation_amd.asr.streaming import Hypothesis, StreamingAsrSession
from voice_enabled_browser_automation_amd.models.config import get_config
from voice_enabled_browser_automation_amd.models.whisper import WhisperModel
from voice_enabled_browser_automation_amd.tokenizer import load_tokenizer
from voice_enabled_browser_automation_amd.voice.server import build_app

I32 = torch.int32
MID = dict(V=300, eot=200, tsb=220, ld=304, max_initial=10)  # n_ts = 80: room for a walk


# ---------------------------------------------------------------- the reference step
def step(lay, x, mask, enable, state, tokens=None, out=None):
    xs = torch.from_numpy(x.copy())
    s_in = torch.tensor(state, dtype=I32)
    s_out = s_in if out is None else out
    ops.ts_rules_step(xs, lay["V"], lay["eot"], lay["tsb"], lay["max_initial"], torch.from_numpy(mask),
                      torch.tensor(enable, dtype=I32), s_in, s_out,
                      tokens=None if tokens is None else torch.tensor(tokens, dtype=I32))
    return xs.numpy(), s_out.tolist()


@pytest.mark.parametrize("lay", [tc.TINY, MID], ids=["tiny", "mid"])
def test_the_reference_matches_the_oracle_over_every_state_class(lay):
    rng = np.random.default_rng(3)
    hists = tc.histories(lay)
    rows = len(hists)
    assert {tuple(to.state_of(h, lay["tsb"])[:1]) for h in hists} == {(0,), (1,), (2,)}
    mask = tc.masks(lay, rows, rng)
    x = tc.rows_on_targets(lay, hists, mask, rng)
    want = np.stack([tc.expect_row(x[r], hists[r], lay, mask[r])[0] for r in range(rows)])
    # applied from the state
    got, state = step(lay, x, mask, [1] * rows, [to.state_of(h, lay["tsb"]) for h in hists])
    assert tc.bits_equal(got, want)
    assert state == [to.state_of(h, lay["tsb"]) for h in hists]
    # advanced by the last token, out of place; rows with no token to give get one outside the vocabulary
    before = [to.state_of(h[:-1], lay["tsb"]) for h in hists]
    toks = [h[-1] if h else -1 - r for r, h in enumerate(hists)]
    out = torch.full((rows, 4), -7, dtype=I32)
    got, state = step(lay, x, mask, [1] * rows, before, toks, out)
    for r, h in enumerate(hists):
        assert tc.bits_equal(got[r], want[r] if h else x[r]), r
        assert state[r] == (to.state_of(h, lay["tsb"]) if h else before[r])
    # a shared mask row
    xs = tc.rows_on_targets(lay, hists, mask[:1], rng)
    got, _ = step(lay, xs, mask[:1], [1] * rows, [to.state_of(h, lay["tsb"]) for h in hists])
    assert tc.bits_equal(got, np.stack([tc.expect_row(xs[r], hists[r], lay, mask[0])[0] for r in range(rows)]))


def test_disabled_rows_bad_tokens_and_corrupt_states():
    lay = tc.TINY
    V, tsb, n_ts = lay["V"], lay["tsb"], lay["V"] - lay["tsb"]
    rng = np.random.default_rng(4)
    hists = [[tsb + 1, 5], [tsb + 1, 5], [tsb + 1, 5], [], [], [7]]
    mask = tc.masks(lay, len(hists), rng)
    x = tc.rows_on_targets(lay, hists, mask, rng)
    states = [to.state_of([tsb + 1], tsb)] * 3 + [[3, 1, 2, 0], [1, 5, -1, n_ts], [-1, 9, 9, 9]]
    got, state = step(lay, x, mask, [0, -2, 1, 1, 1, 1], states, [5, 5, V, 8, -1, 7])
    for r in (0, 1, 2, 4):  # disabled, disabled, token past the vocabulary, negative token
        assert tc.bits_equal(got[r], x[r]) and state[r] == states[r]
    # corrupt states read as the initial one: row 3 then moves on by 8, row 5 by 7
    for r, h in ((3, [8]), (5, [7])):
        assert tc.bits_equal(got[r], tc.expect_row(x[r], h, lay, mask[r])[0]) and state[r] == to.state_of(h, tsb)
    # ... and applied with no token they are the empty history
    got, state = step(lay, x, mask, [1] * 6, states)
    for r in (3, 4, 5):
        assert tc.bits_equal(got[r], tc.expect_row(x[r], [], lay, mask[r])[0]) and state[r] == [0, -1, -1, -1]


def test_a_greedy_walk_under_the_rules_keeps_whisper_s_invariants():
    """200 steps of argmax over random logits (a walk ends at EOT or after 40 steps, and the next
    starts from nothing): the rules never
    ban every id the mask allows, the timestamps never decrease, and a walk starts with a timestamp
    of at most max_initial."""
    lay = MID
    V, eot, tsb = lay["V"], lay["eot"], lay["tsb"]
    rng = np.random.default_rng(9)
    ids = np.arange(lay["ld"])
    bits = (ids <= eot) | ((ids >= tsb) & (ids < V))
    mask = tc.pack(bits)[None]
    state = torch.zeros(1, 4, dtype=I32)
    hist, walks, tok = [], 0, None
    for _ in range(200):
        x = torch.from_numpy(rng.normal(0.0, 3.0, (1, lay["ld"])).astype(np.float32))
        x[0, tsb:V] += 2.0  # (timestamps often enough to matter)
        x[0, eot] += 4.0
        if tok is None:
            state[0] = torch.tensor([0, -1, -1, -1], dtype=I32)
            hist, walks = [], walks + 1
        ops.ts_rules_step(x, V, eot, tsb, lay["max_initial"], torch.from_numpy(mask), torch.ones(1, dtype=I32), state,
                          state, tokens=None if tok is None else torch.tensor([tok], dtype=I32))
        live = torch.from_numpy(bits[:V]) & torch.isfinite(x[0, :V])
        assert live.any(), f"every allowed id is banned after {hist}"
        tok = int(torch.where(live, x[0, :V], torch.tensor(float("-inf"))).argmax())
        if not hist:
            assert tsb <= tok <= tsb + lay["max_initial"]
        if tok >= tsb:
            assert all(tok >= t for t in hist if t >= tsb), f"{tok} after {hist}"
        assert state[0].tolist() == to.state_of(hist, tsb)
        hist.append(tok)
        if tok == eot or len(hist) == 40:
            tok = None
    assert walks >= 2 and sum(t >= tsb for t in hist) >= 1


# ---------------------------------------------------------------- segments
def test_segments_and_cut_index_on_hand_written_sequences():
    B, E = 1000, 900
    tok = type("T", (), {"decode": staticmethod(lambda ids: " ".join(map(str, ids)))})
    closed = [B, 1, 2, B + 50, B + 50, 3, B + 120]
    assert sg.segments(closed, B, E, tok) == [dict(start=0.0, end=1.0, tokens=[1, 2], text="1 2"),
                                              dict(start=1.0, end=2.4, tokens=[3], text="3")]
    assert sg.cut_index(closed, B) == 6
    # a single trailing timestamp opens a segment nobody closed: the cut is the last closing one
    trailing = closed + [B + 120]
    assert sg.segments(trailing, B, E, tok) == sg.segments(closed, B, E, tok) and sg.cut_index(trailing, B) == 6
    # text after the last pair
    tail = trailing + [4, 5]
    assert sg.segments(tail, B, E, tok)[-1] == dict(start=2.4, end=None, tokens=[4, 5], text="4 5")
    assert sg.cut_index(tail, B) == 6
    # no timestamps at all; only an opening one; EOT and the other specials are not text
    assert sg.segments([1, 2], B, E) == [dict(start=None, end=None, tokens=[1, 2], text=None)]
    assert sg.cut_index([1, 2], B) is None and sg.cut_index([B, 1, 2], B) is None and sg.cut_index([], B) is None
    assert sg.cut_index([B], B) is None and sg.segments([B], B, E) == []
    assert sg.segments([B, 1, E, B + 10], B, E)[0]["tokens"] == [1]
    assert ts_state([], B) == [0, -1, -1, -1] and ts_state([B + 3, 1, 2], B) == [2, 2, 1, 3]
    assert ts_state(closed, B) == to.state_of(closed, B) == [2, B + 120, 3, 120]


# ---------------------------------------------------------------- the engine on the CPU
@pytest.fixture(scope="module")
def eng():
    model = WhisperModel(get_config("whisper-test"), device="cpu", seed=0)
    return AsrEngine(model, load_tokenizer("whisper"), max_sessions=6)


@pytest.fixture(scope="module")
def audios(eng):
    return [eng.pcm_to_audio(beam_cases.tone(s, f)) for s, f in beam_cases.TONES]


def check_invariants(eng, toks):
    cfg = eng.model.cfg
    tsb = cfg.no_timestamps + 1
    assert toks and tsb <= toks[0] <= tsb + TS_MAX_INITIAL
    ts = [t for t in toks if t >= tsb]
    assert ts == sorted(ts)
    assert all(t < cfg.eot or tsb <= t < cfg.vocab_size for t in toks)


def test_decode_many_with_timestamps_on_the_cpu(eng, audios):
    cfg = eng.model.cfg
    tsb = cfg.no_timestamps + 1
    fresh = AsrEngine(eng.model, eng.tok, max_sessions=2)
    plain = fresh.decode_many(audios[:2], max_tokens=10, timestamps=[False, False])
    assert fresh._ts_bufs is None and fresh.mask_ts is None and fresh.last_segments == [None, None]
    assert plain == fresh.decode_many(audios[:2], max_tokens=10)
    free = list(eng.free_slots)
    eng.keep_ts_trace = True
    try:
        outs = eng.decode_many(audios[:2], max_tokens=10, timestamps=[True, False])
        trace = eng.last_ts_trace
    finally:
        eng.keep_ts_trace = False
    assert outs[1] == plain[1], "the plain row of a mixed call changed"
    check_invariants(eng, outs[0])
    assert eng.last_stats["timestamps"] == 1 and sorted(eng.free_slots) == sorted(free)
    assert eng.last_segments[1] is None and eng.last_segments[0] == sg.segments(outs[0], tsb, cfg.eot, eng.tok)
    # every traced step: the rules never ban everything, and the logits are the oracle's
    assert len(trace) == 10
    checked = 0
    for s in trace:
        for i, j in enumerate(s["utts"]):
            before, after = s["before"][i].numpy(), s["after"][i].numpy()
            if not s["enable"][i]:
                assert tc.bits_equal(before, after)
                continue
            assert s["history"][i] == outs[0][: len(s["history"][i])]
            args = (s["history"][i], cfg.vocab_size, cfg.eot, tsb, TS_MAX_INITIAL, s["mask"][i].numpy())
            assert to.margin(before.tolist(), *args) > 1e-9
            assert tc.bits_equal(after[: cfg.vocab_size], np.array(to.apply(before.tolist(), *args)[: cfg.vocab_size],
                                                                   dtype=np.float32))
            assert np.isfinite(after[: cfg.vocab_size]).any()
            checked += 1
    assert checked == 10
    # the same call without the trace, and the utterance alone
    assert eng.decode_many(audios[:2], max_tokens=10, timestamps=[True, False]) == outs
    assert eng.decode_many(audios[:1], max_tokens=10, timestamps=[True]) == outs[:1]
    # a boosted timestamp row: the rules read the biased logits
    ks = eng.compile_keyterms([("Grafana", 5.0)])
    eng.keep_ts_trace = eng.keep_boost_trace = True
    try:
        b = eng.decode_many(audios[:1], max_tokens=6, timestamps=[True], keyterms=[ks])
        for sb, st in zip(eng.last_boost_trace, eng.last_ts_trace):
            assert tc.bits_equal(sb["after"].numpy(), st["before"].numpy())
        assert len(eng.last_boost_trace) == len(eng.last_ts_trace) == 6
    finally:
        eng.keep_ts_trace = eng.keep_boost_trace = False
    check_invariants(eng, b[0])


def test_the_argument_errors_come_before_anything_is_launched(eng, audios, monkeypatch):
    free = list(eng.free_slots)
    monkeypatch.setattr(eng.model, "mel_batch", lambda *a, **k: (_ for _ in ()).throw(AssertionError("launched")))
    with pytest.raises(ValueError, match="beam_size"):
        eng.decode_many(audios[:1], timestamps=[True], beam_size=2)
    with pytest.raises(ValueError, match="words"):
        eng.decode_many(audios[:1], timestamps=[True], words=True)
    with pytest.raises(ValueError, match="prefix"):
        eng.decode_many(audios[:2], [[], [5]], timestamps=[False, True])
    with pytest.raises(ValueError, match="entries"):
        eng.decode_many(audios[:2], timestamps=[True])
    assert eng.free_slots == free


# ---------------------------------------------------------------- streaming long-form
TSB = 50364


class ScriptedRecognizer:
    """Answers a timestamp pass with the scripted tokens and any other pass with the length of the
    audio it was given; records every call."""

    ts_begin = TSB

    def __init__(self, ts_tokens):
        self.ts_tokens = list(ts_tokens)
        self.calls = []

    def recognize(self, pcm, prefix=(), **kw):
        self.calls.append((np.array(pcm, copy=True), list(prefix), dict(kw)))
        if kw.get("timestamps"):
            return Hypothesis(list(self.ts_tokens), "boundary")
        return Hypothesis([], f"text of {len(pcm)}")


def speech(n, base=0):
    """Loud samples that tell where they came from."""
    return ((np.arange(base, base + n) % 3000) + 2000).astype("<i2")


def session(rec, **kw):
    return StreamingAsrSession(rec, max_window_s=2.0, partial_every_s=100.0, energy_threshold=100.0,
                               endpoint_silence_s=0.5, spec_silence_s=0.0, **kw)


def test_a_full_window_is_cut_at_the_last_closed_segment(monkeypatch):
    monkeypatch.setenv("VWA_ASR_LONGFORM_MIN_S", "1.0")
    # <|0.00|> a b <|1.20|> <|1.20|> c : the last closing timestamp is 1.2 s
    rec = ScriptedRecognizer([TSB, 5, 6, TSB + 60, TSB + 60, 7])
    s = session(rec, longform=True, language="de", keyterms=["Grafana"])
    pcm = speech(32000 + 8000)
    events = s.push(pcm[:32000].tobytes())
    assert len(events) == 1 and s.stats["longform_cuts"] == 1 and s.stats["longform_fallbacks"] == 0
    ev = events[0]
    assert ev["is_final"] is True and ev["speech_final"] is False
    assert ev["duration"] == 1.2 and ev["start"] == 0.0
    assert ev["channel"]["alternatives"][0]["transcript"] == "text of 19200"
    # the boundary pass: the whole window, timestamps, the session's language and keyterms, no prefix
    (b_pcm, b_prefix, b_kw), (f_pcm, f_prefix, f_kw) = rec.calls
    assert len(b_pcm) == 32000 and b_prefix == [] and b_kw == dict(timestamps=True, language="de", keyterms=["Grafana"])
    assert np.array_equal(f_pcm, pcm[:19200]) and f_prefix == [] and "timestamps" not in f_kw
    # the carried audio is exactly buf[cut:], the utterance stays open on the stream's clock
    assert np.array_equal(s.buf, pcm[19200:32000]) and s.speech > 0 and s.t_offset == pytest.approx(1.2)
    assert s.committed == [] and s.prev_tokens == [] and s.last_partial == ""
    assert s.push(pcm[32000:].tobytes()) == []
    nxt = s.flush()
    assert len(nxt) == 1 and nxt[0]["start"] == 1.2 and nxt[0]["speech_final"] is True
    assert nxt[0]["duration"] == pytest.approx((12800 + 8000) / 16000) and np.array_equal(rec.calls[-1][0], pcm[19200:])


@pytest.mark.parametrize("script", [[TSB, 5, 6, TSB + 25, TSB + 25, 7], [TSB, 5, 6, 7], [5, 6], [TSB, 5, TSB + 150]],
                         ids=["cut below the minimum", "no closing timestamp", "no timestamps", "cut past the window"])
def test_without_a_usable_cut_the_whole_window_is_finalised_as_before(monkeypatch, script):
    monkeypatch.setenv("VWA_ASR_LONGFORM_MIN_S", "1.0")
    pcm = speech(32000)
    old = session(ScriptedRecognizer(script), longform=False)
    want = old.push(pcm.tobytes())
    s = session(ScriptedRecognizer(script), longform=True)
    assert s.push(pcm.tobytes()) == want and len(want) == 1 and want[0]["speech_final"] is True
    assert s.stats["longform_fallbacks"] == 1 and s.stats["longform_cuts"] == 0
    assert len(s.buf) == 0 and s.speech == 0 and s.t_offset == old.t_offset == 2.0


def test_with_the_knob_off_no_pass_asks_for_timestamps(monkeypatch):
    monkeypatch.delenv("VWA_ASR_LONGFORM", raising=False)
    rec = ScriptedRecognizer([TSB, 5, 6, TSB + 60])
    s = session(rec)
    assert s.longform is False
    ev = s.push(speech(32000).tobytes())
    assert len(ev) == 1 and ev[0]["speech_final"] is True and ev[0]["duration"] == 2.0
    assert rec.calls and not any("timestamps" in kw for _, _, kw in rec.calls)
    assert s.stats["longform_cuts"] == s.stats["longform_fallbacks"] == 0
    monkeypatch.setenv("VWA_ASR_LONGFORM", "1")
    assert session(rec).longform is True and session(rec, longform=False).longform is False


def test_the_recognizers_serve_a_timestamp_pass(eng):
    from voice_enabled_browser_automation_amd.asr.streaming import AsrBatcher, EngineRecognizer

    cfg = eng.model.cfg
    pcm = beam_cases.tone(*beam_cases.TONES[0])
    seen = {}
    real = eng.decode_many

    def spy(audios, prefixes=None, **kw):
        seen.update(kw, prefixes=prefixes, n=len(audios))
        return real(audios, prefixes, **dict(kw, max_tokens=min(kw.get("max_tokens", 96), 6)))

    rec = EngineRecognizer(eng, max_tokens=3)
    assert rec.ts_begin == cfg.no_timestamps + 1
    try:
        eng.decode_many = spy
        hyp = rec.recognize(pcm, [5, 6], words=True, beam=3, timestamps=True)
        assert seen["max_tokens"] == cfg.n_text_ctx // 2 and seen["timestamps"] == [True] and not seen["prefixes"]
        assert "beam_size" not in seen and "words" not in seen
        check_invariants(eng, hyp.tokens)
        assert hyp.segments == eng.last_segments[0] and hyp.text == eng.tok.decode([t for t in hyp.tokens if t < cfg.eot]).strip()
        b = AsrBatcher(eng, max_tokens=3)
        try:
            seen.clear()
            futs = [b.recognize_async(pcm, timestamps=True), b.recognize_async(pcm), b.recognize_async(pcm, timestamps=True)]
            res = [f.result(timeout=120) for f in futs]
        finally:
            b.close()
        assert res[0].tokens == res[2].tokens == hyp.tokens and res[0].segments == hyp.segments
        assert res[1].segments == [] and all(t < cfg.eot for t in res[1].tokens)
    finally:
        del eng.decode_many


# ---------------------------------------------------------------- the voice server
class CutSession:
    """An ASR session double: the first audio frame gives a final whose speaker has not stopped, the
    second the final that ends the utterance."""

    def __init__(self):
        self.n = 0
        self.stats = {}

    def push(self, data):
        self.n += 1
        ev = {"type": "Results", "is_final": True, "speech_final": self.n > 1,
              "channel": {"alternatives": [{"transcript": "open the dashboard and" if self.n == 1 else "click deploy"}]}}
        return [ev]

    def flush(self):
        return []


def test_a_final_whose_speaker_has_not_stopped_starts_no_brain_call():
    async def go():
        calls, called = [], asyncio.Event()

        async def parse(req):
            calls.append((await req.json())["text"])
            called.set()
            return web.json_response({"ok": True, "intents": []})

        brain = web.Application()
        brain.router.add_post("/parse", parse)
        async with TestServer(brain) as bs:
            app = build_app(CutSession, brain_url=str(bs.make_url("/parse")), executor_url="http://127.0.0.1:9",
                            debounce_ms=0, commit_ms=0, spec_brain=False)
            async with TestClient(TestServer(app)) as c:
                ws = await c.ws_connect("/stream")
                for _ in range(2):
                    await ws.receive(timeout=5)
                await ws.send_bytes(b"\0" * 320)
                fr = json.loads((await ws.receive(timeout=5)).data)
                assert fr["type"] == "transcript_final" and fr["payload"]["speech_final"] is False
                for _ in range(5):  # (a debounce of 0 ms would have fired by now)
                    await asyncio.sleep(0)
                snap = await (await c.get("/metrics")).json()
                assert snap["counters"]["finals"] == 1 and snap["counters"]["longform_finals"] == 1 and calls == []
                await ws.send_bytes(b"\0" * 320)
                assert json.loads((await ws.receive(timeout=5)).data)["payload"]["speech_final"] is True
                await asyncio.wait_for(called.wait(), 5)
                assert calls == ["open the dashboard and click deploy"]
                await ws.close()

    asyncio.run(go())
