"""Beam search through AsrEngine on the GPU (whisper-test, strict native mode), with graphs and eager.
Random weights make every hypothesis improbable, so nothing here compares transcripts with another
implementation: every step's candidates are held to the float64 oracle of that step's own kept logits
(tests/beam_oracle.py), the choices to the bookkeeping function, and every returned hypothesis to a
teacher-forced rescoring through the existing decoder step -- which a K/V gather that left a stale
parent's context behind cannot pass.

The engines have 11 session slots: two utterances of five beams take 10 and the rescoring pass one
more."""
import numpy as np
import pytest
import torch

import beam_cases as bc
import beam_oracle as bo
import voice_enabled_browser_automation_amd.ops as ops
from voice_enabled_browser_automation_amd.asr.engine import AsrEngine
from voice_enabled_browser_automation_amd.models.config import get_config
from voice_enabled_browser_automation_amd.models.whisper import WhisperModel
from voice_enabled_browser_automation_amd.tokenizer import load_tokenizer

pytestmark = pytest.mark.gpu

DEV = "cuda"
SESSIONS = 11
MODES = pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])


@pytest.fixture(scope="module")
def model():
    ops.beam_ext()  # fail loudly if the library is missing
    return WhisperModel(get_config("whisper-test"), device=DEV, seed=3)


_ENG = {}


def engine(model, graphs: bool) -> AsrEngine:
    if graphs not in _ENG:
        _ENG[graphs] = AsrEngine(model, load_tokenizer("whisper"), max_sessions=SESSIONS, use_graphs=graphs)
    return _ENG[graphs]


@pytest.fixture(scope="module")
def audios(model):
    eng = engine(model, True)
    return [eng.pcm_to_audio(bc.tone(s, f)) for s, f in bc.TONES]


@MODES
def test_every_step_matches_the_oracle_and_the_bookkeeping(model, audios, graphs):
    assert ops.knob("VWA_STRICT_NATIVE")
    eng = engine(model, graphs)
    steps = excused = 0
    for n, W, kw in ((2, 3, dict(max_tokens=8)), (1, 5, dict(max_tokens=8)), (3, 2, dict(max_tokens=8)),
                     (2, 4, dict(exact_tokens=6))):
        _, s, e = bc.check_trace(eng, audios[:n], W, **kw)
        steps, excused = steps + s, excused + e
        bc.check_invariants(eng, n, W, max_tokens=kw.get("max_tokens", 6), exact=kw.get("exact_tokens"))
        assert eng.last_stats["beam_size"] == W and eng.last_stats["beam_ms"] > 0.0
    print(f"MEASURED beam trace: {excused} of {steps} steps needed an excused rank")
    assert steps >= 20 and excused * 20 <= steps


def _teacher_forced(eng, slot, prompt, tokens, ended: bool, exact: bool, min_tokens: int = 0):
    """Log-probabilities of ``tokens`` (and the EOT after them when ``ended``) from ONE decoder step
    over prompt + tokens on ``slot``, under the masks the sampler used."""
    cfg = eng.model.cfg
    seq = list(prompt) + list(tokens)
    logits = eng.runner.step([(slot, t, p) for p, t in enumerate(seq)])
    targets = list(tokens) + ([cfg.eot] if ended else [])
    rows = logits[len(prompt) - 1 : len(prompt) - 1 + len(targets)]
    mask = torch.cat([eng.mask_text if (exact or k < min_tokens) else eng.mask_text_eot for k in range(len(targets))])
    return ops.token_logprob(rows.contiguous(), targets, mask, cfg.vocab_size).cpu().double().numpy()


def _greedy_d0(eng, slot, audio) -> float:
    """The largest per-token difference between step-by-step greedy log-probabilities and their
    teacher-forced rescoring: code this feature does not touch (runner.step, token_logprob), one row
    a step against all rows in one step."""
    cfg = eng.model.cfg
    toks = eng.decode_many([audio], max_tokens=8)[0]
    m = eng.model
    eng.set_cross_batch([slot], m.encode(m.mel_batch([audio])))
    prompt = list(eng.prompt)
    logits = eng._prompt_logits([slot], [prompt])
    step_lp = []
    for k, t in enumerate(toks):
        step_lp.append(float(ops.token_logprob(logits[:1].contiguous(), [t], eng.mask_text_eot, cfg.vocab_size)[0]))
        logits = eng.runner.step([(slot, t, len(prompt) + k)])
    tf = _teacher_forced(eng, slot, prompt, toks, False, False)
    return float(np.abs(np.array(step_lp) - tf).max()) if toks else 0.0


@MODES
def test_every_hypothesis_rescores_to_its_reported_sum(model, audios, graphs):
    eng = engine(model, graphs)
    m = eng.model
    spare = eng.free_slots[0]  # the slot the engine takes last: free during every call below
    d0 = max(_greedy_d0(eng, spare, a) for a in audios[:2])
    worst = 0.0
    for B, W in ((1, 3), (2, 3), (1, 5), (2, 5)):
        eng.decode_many(audios[:B], max_tokens=8, beam_size=W)
        beams = [list(h) for h in eng.last_beams]
        assert len(eng.free_slots) == SESSIONS
        for i in range(B):
            eng.set_cross_batch([spare], m.encode(m.mel_batch([audios[i]])))
            assert len(beams[i]) == W
            for h in beams[i]:
                ended = len(h["tokens"]) < 8
                lp = _teacher_forced(eng, spare, eng.prompt, h["tokens"], ended, False)
                n = len(lp)
                diff = abs(float(lp.sum()) - h["sum_logprob"])
                tol = n * 4 * d0 + n * float(bo.score_bound(32.0, h["avg_logprob"], h["sum_logprob"], m.cfg.vocab_size))
                worst = max(worst, diff)
                assert diff <= tol, f"B{B} W{W} utterance {i} {h}: rescored {lp.sum()} (tolerance {tol}, d0 {d0})"
    print(f"MEASURED beam rescoring ({'graphs' if graphs else 'eager'}): d0 {d0:.4g}, largest |rescored sum - reported| {worst:.4g}")


@MODES
def test_slots_cross_table_and_greedy_are_as_before(model, audios, graphs):
    eng = engine(model, graphs)
    free, table = list(eng.free_slots), eng.runner.b.cross_table.clone()
    greedy = eng.decode_many(audios, max_tokens=8)
    free_g = list(eng.free_slots)
    outs = eng.decode_many(audios, max_tokens=8, beam_size=3)
    bc.check_invariants(eng, 3, 3, max_tokens=8)
    assert outs == [h[0]["tokens"] for h in eng.last_beams]
    assert eng.free_slots == free_g and sorted(free_g) == sorted(free)
    assert torch.equal(eng.runner.b.cross_table, table)
    eng.decode_many(audios[:2], exact_tokens=6, beam_size=5)
    bc.check_invariants(eng, 2, 5, max_tokens=6, exact=6)
    assert all(len(h) == 5 for h in eng.last_beams)
    assert eng.decode_many(audios, max_tokens=8) == greedy
    with pytest.raises(RuntimeError, match="exceed the .* free ASR session slots"):
        eng.decode_many(audios, max_tokens=8, beam_size=4)  # 12 > 11
    assert sorted(eng.free_slots) == sorted(free) and torch.equal(eng.runner.b.cross_table, table)


@MODES
def test_width_one_is_the_greedy_call(model, audios, graphs, monkeypatch):
    eng = engine(model, graphs)
    want = [eng.decode_many(audios[:n], max_tokens=8) for n in (1, 3)]

    def boom(*a, **k):
        raise AssertionError("beam op reached with beam_size = 1")

    monkeypatch.setattr(ops, "beam_select", boom)
    monkeypatch.setattr(ops, "kv_beam_gather", boom)
    assert [eng.decode_many(audios[:n], max_tokens=8, beam_size=1) for n in (1, 3)] == want
    assert "beam_size" not in eng.last_stats


@MODES
def test_words_and_language_detection_with_beams(model, audios, graphs):
    eng = engine(model, graphs)
    outs = eng.decode_many(audios[:2], max_tokens=8, beam_size=3, words=True)
    assert [a.tokens for a in eng.last_alignments] == outs == [h[0]["tokens"] for h in eng.last_beams]
    for a in eng.last_alignments:
        assert len(a.logprobs) == len(a.tokens) == len(a.first_frame) and all(lp <= 0.0 for lp in a.logprobs)
    outs = eng.decode_many(audios[:2], max_tokens=8, beam_size=3, languages=["auto", None])
    assert eng.last_sot[0]["language"] and eng.last_sot[0]["language_confidence"] is not None
    assert len(outs) == 2 and len(eng.free_slots) == SESSIONS
