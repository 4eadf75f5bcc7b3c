"""Language detection, the translate task and the no-speech gate on the CPU: the reference probe
against the float64 oracle (tests/sot_oracle.py), the config / language tables, whisper-test end to
end through AsrEngine, the streaming session with a scripted recognizer, and the settings."""
import numpy as np
import pytest
import torch

import sot_oracle as so
import voice_enabled_browser_automation_amd.ops as ops
from voice_enabled_browser_automation_amd.asr.engine import AsrEngine
from voice_enabled_browser_automation_amd.asr.streaming import (EngineRecognizer, Hypothesis, StreamingAsrSession,
                                                                results_event)
from voice_enabled_browser_automation_amd.models.config import get_config
from voice_enabled_browser_automation_amd.models.whisper import WhisperModel
from voice_enabled_browser_automation_amd.tokenizer import load_tokenizer
from voice_enabled_browser_automation_amd.tokenizer.languages import (WHISPER_LANGUAGES, language_code,
                                                                       language_token)
from voice_enabled_browser_automation_amd.tokenizer.train import whisper_special_tokens

F32, I32 = torch.float32, torch.int32
KNOBS = ("VWA_ASR_LANGUAGE", "VWA_ASR_LANGUAGES", "VWA_ASR_TASK", "VWA_ASR_NO_SPEECH")


@pytest.fixture(autouse=True)
def _defaults(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


# ----------------------------------------------------------------------------- reference op
@pytest.mark.parametrize("layout", [(51865, 50259, 99, 50362), (200, 60, 65, 190), (300, 100, 128, 5), (40, 7, 1, 0)])
@pytest.mark.parametrize("kind", ["all", "some"])
def test_reference_probe_matches_the_f64_oracle(layout, kind):
    vocab, lang0, n_lang, ns = layout
    R = 5
    x = torch.full((R, vocab + 3), 1e30)
    x[:, :vocab] = torch.randn(R, vocab, generator=so.gen(31, vocab)) * 3.0
    x[1, lang0 + n_lang - 1] = x[1, lang0] = 40.0           # a tie: the lower id
    if n_lang > 1:
        x[2, lang0 : lang0 + n_lang : 2] = float("-inf")    # -inf entries (not all of them)
    allow = (1 << n_lang) - 1
    if kind == "some" and n_lang > 1:
        allow &= ~0b1 & ~(1 << (n_lang // 2))
    probs = torch.full((R + 1, n_lang + 2), so.SENTINEL)
    tok = torch.full((R + 1,), so.SENT_I, dtype=I32)
    dst = torch.full((8,), so.SENT_I, dtype=I32)
    got = ops.sot_probe(x, vocab, lang0, n_lang, ns, allow, lang_probs=probs[:R], lang_tok=tok[:R], tok_dst=dst,
                        dst_rows=torch.tensor([3, -1, 0, -1, 9], dtype=I32))
    assert (probs[R:] == so.SENTINEL).all() and (probs[:, n_lang:] == so.SENTINEL).all() and tok[R] == so.SENT_I
    ref = so.probe64(x, vocab, lang0, n_lang, allow, ns)
    so.check_probe((probs[:R, :n_lang], tok[:R], got[2], got[3]), ref, f"reference {layout} {kind}")
    assert dst.tolist() == [int(tok[2]), so.SENT_I, so.SENT_I, int(tok[0])] + [so.SENT_I] * 4  # (9: out of range)
    if kind == "all":
        assert tok[1] == lang0


def test_reference_probe_all_minus_infinity_and_rejections():
    x = torch.randn(2, 48, generator=so.gen(32))
    x[0, 8:12] = float("-inf")
    probs, tok, conf, nsp = ops.sot_probe(x, 40, 7, 5, 0, 0b11110)
    assert tok.tolist()[0] == 8 and torch.isnan(probs[0, 1:]).all() and probs[0, 0] == 0 and torch.isnan(conf[0])
    assert 7 <= tok[1] < 12 and torch.isfinite(probs[1]).all()
    for bad in (dict(n_lang=0), dict(n_lang=129), dict(lang0=-1), dict(lang0=36), dict(vocab=49), dict(ns=-1),
                dict(ns=40), dict(allow=0), dict(allow=1 << 5)):
        k = dict(vocab=40, lang0=7, n_lang=5, ns=0, allow=None)
        k.update(bad)
        with pytest.raises(ValueError):
            ops.sot_probe(x, k["vocab"], k["lang0"], k["n_lang"], k["ns"], k["allow"])
    with pytest.raises(ValueError):
        ops.sot_probe(x[:0], 40, 7, 5, 0)
    with pytest.raises(ValueError):
        ops.sot_probe(x, 40, 7, 5, 0, lang_probs=torch.zeros(2, 4))


# ----------------------------------------------------------------------------- tables
def test_config_ids_of_both_layouts():
    a, b = get_config("whisper-tiny"), get_config("whisper-large-v3")
    assert (a.translate, a.transcribe, a.no_speech, a.no_timestamps, a.n_langs) == (50358, 50359, 50362, 50363, 99)
    assert (b.translate, b.transcribe, b.no_speech, b.no_timestamps, b.n_langs) == (50359, 50360, 50363, 50364, 100)


@pytest.mark.parametrize("name,n_vocab", [("whisper-tiny", 51865), ("whisper-large-v3", 51866)])
def test_language_codes_round_trip_and_match_the_special_token_layout(name, n_vocab):
    cfg = get_config(name)
    specials = whisper_special_tokens(n_vocab)
    codes = WHISPER_LANGUAGES[: cfg.n_langs]
    assert len(set(codes)) == cfg.n_langs == n_vocab - 51766
    for c in codes:
        t = language_token(cfg, c)
        assert language_code(cfg, t) == c
        assert specials[t - 50257] == f"<|{c}|>"
    assert language_token(cfg, "en") == cfg.lang_en and language_token(cfg, " ES ") == cfg.lang_en + 3
    assert specials[cfg.translate - 50257] == "<|translate|>" and specials[cfg.no_speech - 50257] == "<|nospeech|>"
    assert specials[cfg.transcribe - 50257] == "<|transcribe|>" and specials[cfg.sot - 50257] == "<|startoftranscript|>"
    with pytest.raises(ValueError):
        language_token(cfg, "xx")
    for t in (cfg.lang_en - 1, cfg.translate):
        with pytest.raises(ValueError):
            language_code(cfg, t)
    if cfg.n_langs == 99:
        with pytest.raises(ValueError):
            language_token(cfg, "yue")
        tok = load_tokenizer("whisper")  # the bundled tokenizer has the 51865 layout
        for c in codes:
            tid = tok.token_to_id(f"<|{c}|>")
            assert tid is None or tid == language_token(cfg, c)
        for s, t in (("<|translate|>", cfg.translate), ("<|nospeech|>", cfg.no_speech)):
            assert tok.token_to_id(s) in (None, t)
    else:
        assert language_token(cfg, "yue") == cfg.translate - 1


# ----------------------------------------------------------------------------- engine, whisper-test
def _engine(**kw):
    w = WhisperModel(get_config("whisper-test"), device="cpu", seed=3)
    return AsrEngine(w, load_tokenizer("whisper"), max_sessions=3, **kw)


@pytest.fixture(scope="module")
def engine():
    return _engine()


def _tone(seconds, f0):
    t = np.arange(int(seconds * 16000)) / 16000
    return (np.sin(2 * np.pi * f0 * t) * 9000).astype(np.int16)


@pytest.fixture(scope="module")
def audios(engine):
    return [engine.pcm_to_audio(_tone(s, f)) for s, f in ((0.3, 220), (1.2, 330), (2.5, 500))]


def _steps(eng, fn):
    """fn()'s result and the number of runner.step calls it made."""
    n = [0]
    step = eng.runner.step

    def counting(*a, **k):
        n[0] += 1
        return step(*a, **k)

    eng.runner.step = counting
    try:
        return fn(), n[0]
    finally:
        del eng.runner.step


def test_auto_decodes_what_the_reported_language_forced_decodes(engine, audios):
    free = sorted(engine.free_slots)
    a = engine.decode_many(audios[:1], max_tokens=6, languages=["auto"])
    lang = engine.last_sot[0]["language"]
    assert lang in WHISPER_LANGUAGES[:99] and 0 < engine.last_sot[0]["language_confidence"] <= 1
    b = engine.decode_many(audios[:1], max_tokens=6, languages=[lang])
    assert a == b and len(a[0]) > 0
    assert engine.last_sot[0] == dict(language=lang, language_confidence=None, no_speech_prob=None, gated=False)
    assert sorted(engine.free_slots) == free


def test_a_mixed_batch_with_forced_prefixes_is_self_consistent_and_costs_one_more_step(engine, audios):
    free = sorted(engine.free_slots)
    prefixes = [[], [11, 12, 13], [14]]
    base, n0 = _steps(engine, lambda: engine.decode_many(audios, prefixes, max_tokens=5))
    a, n1 = _steps(engine, lambda: engine.decode_many(audios, prefixes, max_tokens=5, languages=["auto", "fr", None]))
    sot = engine.last_sot
    assert [s["language"] for s in sot[1:]] == ["fr", "en"]
    b, n2 = _steps(engine, lambda: engine.decode_many(audios, prefixes, max_tokens=5,
                                                      languages=[sot[0]["language"], "fr", "en"]))
    assert a == b
    assert b[2] == base[2], "the default session of a mixed batch decodes what it decodes alone"
    assert n2 == n0 and n1 == n0 + 1, (n0, n1, n2)
    assert sorted(engine.free_slots) == free


def test_last_sot_equals_the_reference_probe_of_the_kept_logits(engine, audios):
    cfg = engine.model.cfg
    engine.keep_sot = True
    try:
        engine.decode_many(audios, max_tokens=2, languages=["auto", "de", None])
        sot = engine.last_sot
    finally:
        engine.keep_sot = False
    x = torch.stack([s["logits"] for s in sot])
    assert x.shape == (3, engine.model.vocab_padded)
    probs, tok, conf, nsp = ops.sot_probe(x, cfg.vocab_size, cfg.lang_en, cfg.n_langs, cfg.no_speech)
    ref = so.probe64(x, cfg.vocab_size, cfg.lang_en, cfg.n_langs, (1 << 99) - 1, cfg.no_speech)
    so.check_probe((torch.stack([s["lang_probs"] for s in sot]), tok, conf, nsp), ref, "engine")
    assert sot[0]["language"] == language_code(cfg, int(ref[1][0]))
    assert sot[0]["language_confidence"] == float(conf[0])
    assert sot[1]["language_confidence"] == float(probs[1, WHISPER_LANGUAGES.index("de")])
    assert [s["no_speech_prob"] for s in sot] == nsp.tolist()
    assert float(probs.max()) < 0.1, "random weights: near-uniform language probabilities"


def test_translate_stages_the_translate_id_at_position_2(engine, audios):
    cfg = engine.model.cfg
    seen = []
    step = engine.runner.step
    engine.runner.step = lambda rows, *a, **k: (seen.append(list(rows)), step(rows, *a, **k))[1]
    try:
        engine.decode_many(audios[:1], max_tokens=1, task="translate", languages=["es"])
        engine.decode_many(audios[:1], max_tokens=1)
    finally:
        del engine.runner.step
    slot = seen[0][0][0]
    assert seen[0] == [(slot, cfg.sot, 0), (slot, cfg.lang_en + 3, 1), (slot, cfg.translate, 2),
                       (slot, cfg.no_timestamps, 3)]
    assert [r[1] for r in seen[1]] == [cfg.sot, cfg.lang_en, cfg.transcribe, cfg.no_timestamps]  # today's rows
    with pytest.raises(ValueError):
        engine.decode_many(audios[:1], task="summarise")
    with pytest.raises(ValueError):
        engine.decode_many(audios[:1], languages=["xx"])
    assert sorted(engine.free_slots) == [0, 1, 2]


def test_a_restricted_language_set_never_reports_a_language_outside_it(audios):
    eng = _engine(languages_allowed=["de", "ja", "sw"], language="auto")
    assert eng.prompt[1] == language_token(eng.model.cfg, "de")  # the placeholder: the lowest allowed id
    eng.keep_sot = True
    eng.decode_many(audios, max_tokens=1)
    for s in eng.last_sot:
        assert s["language"] in ("de", "ja", "sw")
        on = [WHISPER_LANGUAGES.index(c) for c in ("de", "ja", "sw")]
        off = [i for i in range(99) if i not in on]
        assert abs(float(s["lang_probs"][on].sum()) - 1) < 1e-6 and (s["lang_probs"][off] == 0).all()
    with pytest.raises(ValueError):
        _engine(languages_allowed=["de", "xx"])


def test_the_threshold_gates_every_session_or_none_without_another_step(engine, audios):
    base, n0 = _steps(engine, lambda: engine.decode_many(audios, max_tokens=3))
    for thr, want in ((1e-9, True), (1.0, False)):
        engine.no_speech_threshold = thr
        try:
            got, n1 = _steps(engine, lambda: engine.decode_many(audios, max_tokens=3))
            sot = engine.last_sot
        finally:
            engine.no_speech_threshold = 0.0
        assert got == base, "a gated session is still decoded, and the probe changes no token"
        assert n1 == n0
        assert [s["gated"] for s in sot] == [want] * 3 and all(0 < s["no_speech_prob"] < 1 for s in sot)
        assert [s["language"] for s in sot] == ["en"] * 3 and all(0 < s["language_confidence"] < 1 for s in sot)


def test_words_align_under_the_detected_language(engine, audios):
    a = engine.decode_many(audios[:2], max_tokens=4, min_tokens=4, words=True, languages=["auto", None])
    als = engine.last_alignments
    assert [al.tokens for al in als] == a and all(np.isfinite(al.logprobs).all() for al in als)
    lang = engine.last_sot[0]["language"]
    b = engine.decode_many(audios[:2], max_tokens=4, min_tokens=4, words=True, languages=[lang, None])
    assert a == b
    for x, y in zip(als, engine.last_alignments):
        assert x.first_frame == y.first_frame and x.last_frame == y.last_frame
        assert np.allclose(x.logprobs, y.logprobs, atol=1e-5)


def test_the_engine_recognizer_fills_the_hypothesis(engine):
    rec = EngineRecognizer(engine, max_tokens=3)
    h = rec.recognize(_tone(0.5, 300))
    assert (h.language, h.language_confidence, h.no_speech_prob) == ("en", None, None)
    h = rec.recognize(_tone(0.5, 300), language="auto")
    assert h.language in WHISPER_LANGUAGES and 0 < h.language_confidence < 1 and 0 < h.no_speech_prob < 1
    h2 = rec.recognize(_tone(0.5, 300), language=h.language)
    assert h2.tokens == h.tokens


# ----------------------------------------------------------------------------- streaming
class Scripted:
    """A recognizer that records how it was asked and answers from a script of (language, no-speech
    probability) per pass (the last entry repeats)."""

    def __init__(self, script=(("es", 0.01),)):
        self.calls = []
        self.script = list(script)

    def recognize(self, pcm, prefix=(), words=False, language=None):
        lang, nsp = self.script[min(len(self.calls), len(self.script) - 1)]
        self.calls.append(language)
        return Hypothesis([1, 2], "hola amigo", language=lang if language == "auto" else language,
                          language_confidence=0.7, no_speech_prob=nsp)


class OldSignature:
    def __init__(self):
        self.calls = 0

    def recognize(self, pcm, prefix=()):
        self.calls += 1
        return Hypothesis([1, 2], "hello there")


def _speech(seconds=1.6):
    rate = 16000
    t = np.arange(int(seconds * rate)) / rate
    return np.concatenate([(np.sin(2 * np.pi * 220 * t) * 9000).astype(np.int16), np.zeros(int(0.6 * rate), np.int16)])


def _stream(sess, pcm=None, flush=True):
    pcm = _speech() if pcm is None else pcm
    events = []
    for i in range(0, len(pcm), 960):
        events += sess.push(pcm[i : i + 960].tobytes())
    return events + (sess.flush() if flush else [])


def _session(rec, **kw):
    return StreamingAsrSession(rec, partial_every_s=0.5, endpoint_silence_s=0.3, energy_threshold=300,
                               spec_silence_s=0.0, **kw)


def test_results_event_language_fields_are_optional():
    plain = results_event("hi", is_final=True, start=0, duration=1, model="m")
    assert "detected_language" not in plain["channel"] and "languages" not in plain["channel"]["alternatives"][0]
    assert plain["metadata"] == {"model_info": {"name": "m"}}
    ev = results_event("hi", is_final=True, start=0, duration=1, model="m", language="es", language_confidence=0.9)
    assert ev["channel"]["detected_language"] == "es" and ev["channel"]["language_confidence"] == 0.9
    assert ev["channel"]["alternatives"][0]["languages"] == ["es"]
    ev = results_event("", is_final=True, start=0, duration=1, model="m", no_speech_prob=0.8)
    assert ev["metadata"]["no_speech_prob"] == 0.8
    assert (Hypothesis().language, Hypothesis().language_confidence, Hypothesis().no_speech_prob) == (None,) * 3


def test_the_language_is_locked_at_the_first_commit_and_cleared_at_the_next_utterance():
    rec = Scripted([("es", 0.01), ("pt", 0.01), ("it", 0.01)])
    sess = _session(rec, language="auto")
    events = _stream(sess, flush=False)  # partials at 0.5 / 1.0 / 1.5 s, then the endpoint's final
    # pass 1 commits nothing (no previous hypothesis); pass 2 commits -> its language, "pt", is locked
    assert rec.calls == ["auto", "auto", "pt", "pt"], rec.calls
    assert sess._lang_lock is None and sess.committed == []  # the final reset the utterance
    finals = [e for e in events if e["is_final"]]
    assert len(finals) == 1 and finals[0]["channel"]["detected_language"] == "pt"
    assert finals[0]["channel"]["alternatives"][0]["languages"] == ["pt"]
    assert finals[0]["channel"]["language_confidence"] == 0.7
    n = len(rec.calls)
    _stream(sess, flush=False)
    assert rec.calls[n : n + 2] == ["auto", "auto"], "the next utterance detects again"


def test_event_fields_are_absent_when_off_and_an_old_signature_recognizer_still_works():
    rec = OldSignature()
    events = _stream(_session(rec))
    assert rec.calls >= 2 and any(e["is_final"] for e in events)
    for e in events:
        assert e == results_event("hello there", is_final=e["is_final"], start=e["start"], duration=e["duration"],
                                  model="whisper")
    rec = Scripted()
    events = _stream(_session(rec))  # defaults: no language= keyword, no language in the events
    assert set(rec.calls) == {None}
    assert all("detected_language" not in e["channel"] for e in events)
    events = _stream(_session(Scripted(), language="es"))
    assert events and all(e["channel"]["detected_language"] == "es" for e in events)


def test_a_gated_final_is_empty_and_a_gated_partial_commits_nothing():
    rec = Scripted([("es", 0.9)])
    sess = _session(rec, language="auto", no_speech_threshold=0.6)
    events = _stream(sess, flush=False)
    assert len(rec.calls) == 4 and rec.calls == ["auto"] * 4, "gated partials commit nothing: no language lock"
    assert sess.stats["committed_tokens"] == 0 and sess.stats["partials"] == 0
    assert len(events) == 1 and events[0]["is_final"]
    alt = events[0]["channel"]["alternatives"][0]
    assert (alt["transcript"], alt["words"], alt["confidence"]) == ("", [], 0.0)
    assert events[0]["metadata"]["no_speech_prob"] == 0.9
    assert sess.stats["no_speech"] == 1 and sess.stats["finals"] == 1
    # threshold off: the same hypotheses pass
    sess = _session(Scripted([("es", 0.9)]), language="auto", no_speech_threshold=0.0)
    events = _stream(sess, flush=False)
    assert events[-1]["channel"]["alternatives"][0]["transcript"] == "hola amigo" and sess.stats["no_speech"] == 0
    assert "no_speech_prob" not in events[-1]["metadata"]


@pytest.mark.parametrize("nsp,called", [(0.9, 0), (0.1, 1)])
def test_on_speculative_is_not_called_when_gated(nsp, called):
    sess = StreamingAsrSession(Scripted([("es", nsp)]), partial_every_s=10.0, endpoint_silence_s=0.4,
                               energy_threshold=300, spec_silence_s=0.1, no_speech_threshold=0.6)
    heard = []
    sess.on_speculative = heard.append
    events = _stream(sess, flush=False)
    assert sess.stats["spec_used"] == 1 and len(heard) == called
    assert [e["channel"]["alternatives"][0]["transcript"] for e in events if e["is_final"]] == ["hola amigo" if called else ""]


# ----------------------------------------------------------------------------- settings
def test_each_knob_drives_the_engine_and_the_session(monkeypatch):
    eng = _engine()
    cfg = eng.model.cfg
    assert (eng.language, eng.task, eng.allow, eng.no_speech_threshold) == ("en", "transcribe", (1 << 99) - 1, 0.0)
    assert eng.prompt == [cfg.sot, cfg.lang_en, cfg.transcribe, cfg.no_timestamps] and eng.max_prefix() == 448 - 5
    sess = _session(Scripted())
    assert sess.language is None and sess.no_speech_threshold == 0.0
    monkeypatch.setenv("VWA_ASR_LANGUAGE", "auto")
    monkeypatch.setenv("VWA_ASR_LANGUAGES", "es, pt")
    monkeypatch.setenv("VWA_ASR_TASK", "translate")
    monkeypatch.setenv("VWA_ASR_NO_SPEECH", "0.6")
    eng = _engine()
    assert (eng.language, eng.task, eng.no_speech_threshold) == ("auto", "translate", 0.6)
    assert eng.allow == (1 << 3) | (1 << 8)
    assert eng.prompt == [cfg.sot, cfg.lang_en + 3, cfg.translate, cfg.no_timestamps]
    sess = _session(Scripted())
    assert sess.language == "auto" and sess.no_speech_threshold == 0.6
    eng.decode_many([eng.pcm_to_audio(_tone(0.4, 250))], max_tokens=1)
    assert eng.last_sot[0]["language"] in ("es", "pt") and eng.last_sot[0]["gated"] in (True, False)
    monkeypatch.setenv("VWA_ASR_LANGUAGE", "fr")
    assert _engine().prompt[1] == cfg.lang_en + 6 and _session(Scripted()).language == "fr"
    monkeypatch.setenv("VWA_ASR_TASK", "dictate")
    with pytest.raises(ValueError):
        _engine()


def test_the_batcher_mixes_fixed_and_auto_passes(engine):
    from voice_enabled_browser_automation_amd.asr.streaming import AsrBatcher

    bat = AsrBatcher(engine, max_tokens=3)
    try:
        futs = [bat.recognize_async(_tone(0.5, 300), language="auto"),
                bat.recognize_async(_tone(0.7, 400), [11], language="fr"), bat.recognize_async(_tone(0.4, 500))]
        hyps = [f.result(timeout=120) for f in futs]
    finally:
        bat.close()
    assert hyps[0].language in WHISPER_LANGUAGES and 0 < hyps[0].language_confidence < 1
    assert hyps[1].language == "fr" and hyps[1].tokens[:1] == [11] and hyps[2].language == "en"
    assert sorted(engine.free_slots) == [0, 1, 2]
