"""Beam finals of a session that rescores (StreamingAsrSession(rescore=True), VWA_RESCORE) carry every
alternative's ``logprob``, the first included: the ``sum_logprob`` of the engine's ``last_beams`` entry.
Without it the events are what they were; partials, greedy finals and finals cut to one alternative
never carry it."""
import json

import numpy as np
import pytest

from voice_enabled_browser_automation_amd.asr import streaming as st

BEAMS = [dict(tokens=[7, 8], sum_logprob=-1.25, avg_logprob=-0.5), dict(tokens=[7, 9], sum_logprob=-2.5, avg_logprob=-1.0),
         dict(tokens=[6], sum_logprob=-2.75, avg_logprob=-1.5), dict(tokens=[5, 5, 5], sum_logprob=-9.0, avg_logprob=-2.0)]
SPEECH = (np.sin(np.arange(16000 * 2) * 0.2) * 9000).astype(np.int16).tobytes()


class Tok:
    def decode(self, ids):
        return " ".join(str(i) for i in ids)


class Eng:
    tok = Tok()


class Rec:
    """A recogniser whose beam passes return the hypothesis the engine recogniser builds from BEAMS."""

    def recognize(self, pcm, prefix=(), **kw):
        w = kw.get("beam", 1)
        if w > 1:
            return st._hypothesis(Eng, list(prefix) + BEAMS[0]["tokens"], len(pcm), beams=BEAMS[:w], prefix=prefix)
        return st._hypothesis(Eng, list(prefix) + BEAMS[0]["tokens"], len(pcm))


def finals_of(**kw):
    s = st.StreamingAsrSession(Rec(), partial_every_s=0.5, spec_silence_s=0, words=False, language="en", **kw)
    events = s.push(SPEECH) + s.flush()
    finals = [e for e in events if e.get("is_final")]
    partials = [e for e in events if e.get("type") == "Results" and not e.get("is_final")]
    assert len(finals) == 1 and partials
    return finals[0], partials


def test_the_hypothesis_keeps_the_beams_sum_logprobs():
    hyp = st._hypothesis(Eng, [7, 8], 16000, beams=BEAMS, prefix=())
    assert hyp.beam_logprobs == [-1.25, -2.5, -2.75, -9.0] and len(hyp.alternatives) == 3
    assert all(set(a) == {"transcript", "confidence"} for a in hyp.alternatives)
    assert st._hypothesis(Eng, [7, 8], 16000).beam_logprobs == []


def test_logprob_is_present_only_with_rescore_and_is_the_beams_sum_logprob():
    on, partials = finals_of(beam=4, alternatives=3, rescore=True)
    alts = on["channel"]["alternatives"]
    assert [a["transcript"] for a in alts] == ["7 8", "7 9", "6"]
    assert [a["logprob"] for a in alts] == [h["sum_logprob"] for h in BEAMS[:3]]
    assert all("logprob" not in a for p in partials for a in p["channel"]["alternatives"])
    off, _ = finals_of(beam=4, alternatives=3, rescore=False)
    assert all("logprob" not in a for a in off["channel"]["alternatives"])
    # but for the logprobs the two events are the same bytes
    for a in alts:
        del a["logprob"]
    assert json.dumps(on) == json.dumps(off)


def test_greedy_finals_and_single_alternatives_carry_none():
    for kw in (dict(beam=1, alternatives=1), dict(beam=4, alternatives=1)):
        ev, _ = finals_of(rescore=True, **kw)
        assert len(ev["channel"]["alternatives"]) == 1 and "logprob" not in ev["channel"]["alternatives"][0]


def test_the_default_comes_from_the_setting(monkeypatch):
    monkeypatch.delenv("VWA_RESCORE", raising=False)
    assert st.StreamingAsrSession(Rec(), beam=2, alternatives=2).rescore is False
    monkeypatch.setenv("VWA_RESCORE", "1")
    assert st.StreamingAsrSession(Rec(), beam=2, alternatives=2).rescore is True
    assert st.StreamingAsrSession(Rec(), beam=2, alternatives=2, rescore=False).rescore is False


def test_the_settings_are_declared_and_rescore_needs_alternatives(monkeypatch):
    from voice_enabled_browser_automation_amd.utils import env

    for name in ("VWA_RESCORE", "VWA_RESCORE_URL", "VWA_RESCORE_WEIGHT", "VWA_ASR_BEAM", "VWA_ASR_ALTERNATIVES"):
        monkeypatch.delenv(name, raising=False)
    f = env.Settings.model_fields
    assert f["VWA_RESCORE"].default is False and f["VWA_RESCORE_URL"].default is None
    assert f["VWA_RESCORE_WEIGHT"].default == 0.5 and "NOT tuned" in f["VWA_RESCORE_WEIGHT"].description
    assert env.settings().VWA_RESCORE is False
    monkeypatch.setenv("VWA_RESCORE", "1")
    with pytest.raises(ValueError, match="VWA_ASR_ALTERNATIVES"):
        env.settings()                                    # VWA_ASR_ALTERNATIVES = 1: nothing to rescore
    monkeypatch.setenv("VWA_ASR_BEAM", "4")
    monkeypatch.setenv("VWA_ASR_ALTERNATIVES", "3")
    s = env.settings()
    assert s.VWA_RESCORE is True and s.VWA_RESCORE_WEIGHT == 0.5
    monkeypatch.setenv("VWA_RESCORE_WEIGHT", "-0.1")
    with pytest.raises(ValueError):
        env.settings()
