"""Language detection and the no-speech probability through AsrEngine on the GPU (whisper-test,
strict native mode).  Random weights give near-uniform language probabilities, so nothing here
compares a language detected on the GPU with one detected elsewhere: a call with "auto" is held to a
second call on the same device with the reported language forced, and the probe's outputs to the
float64 oracle of the SOT logits the engine itself kept (tests/sot_oracle.py)."""
import numpy as np
import pytest
import torch

import sot_oracle as so
import voice_enabled_browser_automation_amd.ops as ops
from voice_enabled_browser_automation_amd.asr.engine import AsrEngine
from voice_enabled_browser_automation_amd.models.config import get_config
from voice_enabled_browser_automation_amd.models.whisper import WhisperModel
from voice_enabled_browser_automation_amd.tokenizer import load_tokenizer
from voice_enabled_browser_automation_amd.tokenizer.languages import language_code, language_token

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _tone(seconds, f0):
    t = np.arange(int(seconds * 16000)) / 16000
    return (np.sin(2 * np.pi * f0 * t) * 9000).astype(np.int16)


@pytest.fixture(scope="module")
def model():
    ops.sot_ext()  # fail loudly if the library is missing
    return WhisperModel(get_config("whisper-test"), device=DEV, seed=3)


_ENG = {}


def engine(model, graphs: bool) -> AsrEngine:
    if graphs not in _ENG:
        _ENG[graphs] = AsrEngine(model, load_tokenizer("whisper"), max_sessions=3, use_graphs=graphs)
    return _ENG[graphs]


@pytest.fixture(scope="module")
def audios(model):
    eng = engine(model, True)
    return [eng.pcm_to_audio(_tone(s, f)) for s, f in ((0.3, 220), (1.2, 330), (2.5, 500))]


def _check_kept(eng, langs):
    """last_sot (keep_sot) against the oracle of the engine's own SOT logits."""
    cfg = eng.model.cfg
    sot = eng.last_sot
    x = torch.stack([s["logits"] for s in sot])
    assert x.shape == (len(langs), eng.model.vocab_padded)
    ref = so.probe64(x, cfg.vocab_size, cfg.lang_en, cfg.n_langs, eng.allow, cfg.no_speech)
    probs = torch.stack([s["lang_probs"] for s in sot])
    tok = [language_token(cfg, s["language"]) if l == "auto" else int(ref[1][i])
           for i, (s, l) in enumerate(zip(sot, langs))]
    conf = [s["language_confidence"] if l == "auto" else ref[2][i] for i, (s, l) in enumerate(zip(sot, langs))]
    so.check_probe((probs, np.array(tok), np.array(conf), np.array([s["no_speech_prob"] for s in sot])), ref,
                   f"engine {langs}")
    for i, (s, l) in enumerate(zip(sot, langs)):
        if l == "auto":  # the detected id is the oracle's argmax of those same logits
            assert s["language"] == language_code(cfg, int(ref[1][i]))
        else:
            j = language_token(cfg, s["language"]) - cfg.lang_en
            assert abs(s["language_confidence"] - ref[0][i, j]) <= so.prob_bound(ref[0][i, j])


@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
def test_one_session_auto_equals_the_reported_language_forced(model, audios, graphs):
    """B = 1: with graphs the device-resident decode loop."""
    assert ops.knob("VWA_STRICT_NATIVE")
    eng = engine(model, graphs)
    default = eng.decode_many(audios[1:2], max_tokens=8)
    assert eng.decode_many(audios[1:2], max_tokens=8, languages=[None], task="transcribe") == default
    eng.keep_sot = True
    try:
        a = eng.decode_many(audios[1:2], max_tokens=8, languages=["auto"])
        _check_kept(eng, ["auto"])
    finally:
        eng.keep_sot = False
    lang = eng.last_sot[0]["language"]
    assert eng.decode_many(audios[1:2], max_tokens=8, languages=[lang]) == a
    assert len(eng.free_slots) == 3


@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
def test_a_mixed_batch_auto_equals_the_reported_language_forced(model, audios, graphs):
    eng = engine(model, graphs)
    prefixes = [[], [11, 12, 13], [14]]
    default = eng.decode_many(audios, prefixes, exact_tokens=6)
    assert eng.decode_many(audios, prefixes, exact_tokens=6, languages=[None] * 3) == default
    langs = ["auto", "fr", None]
    eng.keep_sot = True
    try:
        a = eng.decode_many(audios, prefixes, exact_tokens=6, languages=langs)
        _check_kept(eng, ["auto", "fr", "en"])
    finally:
        eng.keep_sot = False
    sot = eng.last_sot
    assert [s["language"] for s in sot[1:]] == ["fr", "en"]
    assert eng.decode_many(audios, prefixes, exact_tokens=6, languages=[sot[0]["language"], "fr", "en"]) == a
    assert eng.decode_many(audios, prefixes, exact_tokens=6) == default  # nothing the probe left behind changes a decode
    assert len(eng.free_slots) == 3


def test_graphs_on_and_off_give_equal_tokens(model, audios):
    prefixes = [[], [11, 12, 13], [14]]
    out = []
    for graphs in (True, False):
        eng = engine(model, graphs)
        out.append((eng.decode_many(audios, prefixes, exact_tokens=6, languages=["auto", "auto", "de"]),
                    [s["language"] for s in eng.last_sot],
                    eng.decode_many(audios[:1], max_tokens=8, languages=["auto"]), eng.last_sot[0]["language"]))
    assert out[0] == out[1]


def test_the_gate_reads_the_prompt_steps_own_sot_row(model, audios):
    """Gate on, no auto session: same tokens as the default call, probabilities within the bounds."""
    eng = engine(model, True)
    default = eng.decode_many(audios, exact_tokens=4)
    eng.no_speech_threshold, eng.keep_sot = 0.6, True
    try:
        assert eng.decode_many(audios, exact_tokens=4) == default
        _check_kept(eng, ["en"] * 3)
        assert all(s["gated"] == (s["no_speech_prob"] > 0.6) for s in eng.last_sot)
    finally:
        eng.no_speech_threshold, eng.keep_sot = 0.0, False
