"""Keyterm boosting through AsrEngine on the GPU (whisper-test, strict native mode), with graphs and
eager.  The traced runs (stepped from the host) are held to the brute-force oracle at every step;
the captured device loop must give the traced run's tokens; the boost-1e4 repetition and
prefix-straddling cases of the CPU test are repeated; a boosted beam call has every step's biased
logits checked; and the persistent one-launch decoder is not entered for a boosted call."""
import pytest
import torch

import beam_cases
import boost_cases as bc
import boost_oracle as bo
import voice_enabled_browser_automation_amd.ops as ops
from voice_enabled_browser_automation_amd.asr import keyterms as kt
from voice_enabled_browser_automation_amd.asr.engine import AsrEngine
from voice_enabled_browser_automation_amd.models.config import get_config
from voice_enabled_browser_automation_amd.models.whisper import WhisperModel
from voice_enabled_browser_automation_amd.tokenizer import load_tokenizer

pytestmark = pytest.mark.gpu

DEV = "cuda"
SESSIONS = 10
MODES = pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])


@pytest.fixture(scope="module")
def model():
    ops.boost_ext()  # fail loudly if the library is missing
    return WhisperModel(get_config("whisper-test"), device=DEV, seed=3)


_ENG = {}


def engine(model, graphs: bool) -> AsrEngine:
    if graphs not in _ENG:
        _ENG[graphs] = AsrEngine(model, load_tokenizer("whisper"), max_sessions=SESSIONS, use_graphs=graphs)
    return _ENG[graphs]


@pytest.fixture(scope="module")
def audios(model):
    eng = engine(model, True)
    return [eng.pcm_to_audio(beam_cases.tone(s, f)) for s, f in beam_cases.TONES]


@pytest.fixture(scope="module")
def cycle(model, audios):
    return bc.pick_cycle(engine(model, True), audios[0])


def sets_for(eng, cycle):
    text = eng.compile_keyterms(["Grafana", ("pull request", 3.0), "open Browserbase"], 2.0)
    plain = eng.decode_many([torch.zeros(4000, device=DEV)], exact_tokens=3)[0]
    ids = kt.compile_sequences([(plain[:2], 0.5), (plain[:1] + cycle[:2], 4.0), (cycle, 6.0), (cycle[1:3], 2.5)],
                               limit=eng.model.cfg.eot)
    return text, ids


def traced(eng, *a, **kw):
    eng.keep_boost_trace = True
    try:
        return eng.decode_many(*a, **kw), eng.last_boost_trace
    finally:
        eng.keep_boost_trace = False


@MODES
def test_traced_runs_match_the_oracle_and_the_device_loop_gives_the_same_tokens(model, audios, cycle, graphs):
    assert ops.knob("VWA_STRICT_NATIVE")
    eng = engine(model, graphs)
    text, ids = sets_for(eng, cycle)
    for ks, prefix, kw in ((ids, [], dict(max_tokens=8)), (ids, cycle[:2], dict(exact_tokens=7)),
                           (text, [], dict(exact_tokens=6))):
        outs, trace = traced(eng, audios[:1], [prefix], keyterms=[ks], **kw)
        assert bc.check_trace(eng, trace) == len(trace) >= 1
        # the same call without the trace: with graphs, the captured single-session device loop
        assert eng.decode_many(audios[:1], [prefix], keyterms=[ks], **kw) == outs
        assert eng.last_stats["boosted"] == 1
    if graphs:
        assert eng.device_loop and any(k[3] for k in eng.loop_graphs), "no boosted loop graph was captured"
    # batched rows: mixed sets, a plain row, a forced prefix, rows dropping out
    outs, trace = traced(eng, audios + audios[:1], [[], cycle[:2], [], cycle[:1]], max_tokens=7,
                         keyterms=[ids, ids, None, text])
    assert bc.check_trace(eng, trace) >= 6
    assert eng.decode_many(audios + audios[:1], [[], cycle[:2], [], cycle[:1]], max_tokens=7,
                           keyterms=[ids, ids, None, text]) == outs


@MODES
def test_a_keyterm_straddles_the_forced_prefix(model, audios, cycle, graphs):
    eng = engine(model, graphs)
    q = cycle
    ks = kt.compile_sequences([(q, 1e4)], limit=eng.model.cfg.eot)
    assert eng.decode_many(audios[:1], exact_tokens=10, keyterms=[ks]) == [(q * 3)[:10]]
    assert eng.decode_many(audios[:1], [q[:2]], exact_tokens=10, keyterms=[ks]) == [(q[2:] + q * 3)[:10]]
    outs = eng.decode_many(audios[:2], [q[:2], q[:3]], exact_tokens=4, keyterms=[ks, ks])
    assert outs == [(q[2:] + q)[:4], (q[3:] + q)[:4]]
    assert eng.decode_many(audios[:1], [q[:2]], exact_tokens=4, keyterms=[ks], beam_size=3) == [(q[2:] + q)[:4]]
    # a plain call in between is what it was (the boosted loop graph is a separate one)
    plain = eng.decode_many(audios[:1], exact_tokens=6)
    assert eng.decode_many(audios[:1], exact_tokens=6, keyterms=[None]) == plain != [(q * 2)[:6]]


@MODES
def test_boosted_beams_read_the_biased_logits_and_keep_the_beam_invariants(model, audios, cycle, graphs):
    eng = engine(model, graphs)
    text, ids = sets_for(eng, cycle)
    eng.keep_boost_trace = True
    try:
        _, steps, _ = beam_cases.check_trace(eng, audios[:2], 3, max_tokens=6, keyterms=[ids, text],
                                             prefixes=[cycle[:1], []])
        trace, beam_trace = eng.last_boost_trace, eng.last_beam_trace
        assert len(trace) == steps and bc.check_trace(eng, trace, beams=3) >= steps
        for s, b in zip(trace, beam_trace):
            assert bo.bits_equal(s["after"], b["logits"]), "the select did not read the biased logits"
            assert s["parents"] == b["parents"] and s["tokens"] == b["tokens"]
        beam_cases.check_invariants(eng, 2, 3, max_tokens=6)
        eng.decode_many(audios, max_tokens=5, beam_size=2, keyterms=[None, ids, text])
        assert bc.check_trace(eng, eng.last_boost_trace, beams=2) >= 4
    finally:
        eng.keep_boost_trace = False


def test_the_persistent_decoder_is_not_entered_for_a_boosted_call(model, audios, cycle, monkeypatch):
    """Counted at the model's entry point: a plain single-session call still asks the persistent
    decoder for its loop steps (whether this model takes them is its own decision); a boosted call
    never reaches it."""
    eng = AsrEngine(model, load_tokenizer("whisper"), max_sessions=2, use_graphs=True)
    assert eng.device_loop
    calls = []
    real = model.wdec_loop_step
    monkeypatch.setattr(model, "wdec_loop_step", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    plain = eng.decode_many(audios[:1], exact_tokens=6)
    assert calls, "a plain device-loop call no longer reaches the persistent decoder's entry"
    n = len(calls)
    ks = kt.compile_sequences([(cycle, 1e4)], limit=eng.model.cfg.eot)
    assert eng.decode_many(audios[:1], exact_tokens=6, keyterms=[ks]) == [(cycle * 2)[:6]]
    assert len(calls) == n, "a boosted call entered the persistent decoder"
    assert not eng._persistent_loop_ok(object()) and eng._persistent_loop_ok(None)
    assert eng.decode_many(audios[:1], exact_tokens=6) == plain


def test_a_larger_batch_between_two_boosted_single_sessions_does_not_strand_the_loop_graph(model, audios, cycle):
    """A fresh engine, as a worker lives: one boosted session alone (the loop graph is captured), then
    a batch with more rows than any before, then the session alone again.  The captured graph and
    the eager first step hand the token over in one buffer for the engine's life, so the second
    single-session call gives the traced run's tokens, and the prefix-straddling ones."""
    eng = AsrEngine(model, load_tokenizer("whisper"), max_sessions=SESSIONS, use_graphs=True)
    assert eng.device_loop
    text, ids = sets_for(eng, cycle)
    big = kt.compile_sequences([(cycle, 1e4)], limit=eng.model.cfg.eot)
    tok_buf = eng.d_tok.data_ptr()
    want, trace = traced(eng, audios[:1], [cycle[:2]], keyterms=[ids], exact_tokens=7)  # (host-stepped: no graph)
    assert bc.check_trace(eng, trace) == 7 and not any(k[3] for k in eng.loop_graphs)
    first = eng.decode_many(audios[:1], [cycle[:2]], keyterms=[ids], exact_tokens=7)
    assert first == want and any(k[3] for k in eng.loop_graphs)
    assert eng.decode_many(audios[:1], [cycle[:2]], exact_tokens=10, keyterms=[big]) == [(cycle[2:] + cycle * 3)[:10]]
    rows = eng.decode_many(audios * 2 + audios[:1], max_tokens=4, keyterms=[ids, None, text, ids, None, text, None])
    assert len(rows) == 7
    assert eng.decode_many(audios[:1], [cycle[:2]], keyterms=[ids], exact_tokens=7) == want
    assert eng.decode_many(audios[:1], [cycle[:2]], exact_tokens=10, keyterms=[big]) == [(cycle[2:] + cycle * 3)[:10]]
    assert eng.decode_many(audios[:1], exact_tokens=10, keyterms=[big]) == [(cycle * 3)[:10]]
    assert eng.d_tok.data_ptr() == tok_buf
