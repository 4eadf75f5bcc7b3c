"""Word timestamps and confidences on the CPU: the reference alignment ops against independent
float64 code (tests/align_oracle.py), word grouping on hand-made token lists, the streaming
events with the feature off and on, and whisper-test end to end."""
import numpy as np
import pytest
import torch

import align_oracle as ao
import voice_enabled_browser_automation_amd.ops as ops
from voice_enabled_browser_automation_amd.asr.engine import AsrEngine
from voice_enabled_browser_automation_amd.asr.streaming import (EngineRecognizer, Hypothesis, StreamingAsrSession,
                                                                results_event)
from voice_enabled_browser_automation_amd.asr.words import Alignment, confidence, group_words
from voice_enabled_browser_automation_amd.models.config import get_config
from voice_enabled_browser_automation_amd.models.whisper import WhisperModel
from voice_enabled_browser_automation_amd.tokenizer import load_tokenizer

BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32


# ----------------------------------------------------------------------------- reference ops
@pytest.mark.parametrize("T,n_keys,H,heads", [(1, 1, 2, [1]), (5, 7, 2, [1]), (33, 250, 6, [5, 0, 3])])
def test_reference_attn_probs_matches_f64_softmax(T, n_keys, H, heads):
    g = ao.gen(1, T, n_keys)
    S = 260
    q = torch.randn(T, H * 64, generator=g).to(BF)
    k = torch.randn(S, H, 64, generator=g).to(BF)
    out = torch.full((len(heads), T, S), ao.SENTINEL, dtype=F32)
    ops.attn_probs(q, k, heads, n_keys, 0.125, out)
    ref, A = ao.probs64(q, k, heads, n_keys, 0.125)
    got = out[:, :, :n_keys].double().numpy()
    assert (np.abs(got - ref) <= 4 * ao.probs_bound(ref, A)).all()  # (torch's f32 matmul: not the MFMA's order)
    assert (out[:, :, n_keys:] == ao.SENTINEL).all()
    with pytest.raises(ValueError):
        ops.attn_probs(q, k, [H], n_keys, 0.125, out)


@pytest.mark.parametrize("Hs,T,n_keys", [(1, 1, 7), (6, 2, 3), (1, 33, 4), (6, 33, 6), (6, 5, 1), (1, 2, 250)])
def test_reference_align_cost_matches_f64_median_of_reflect_padded_windows(Hs, T, n_keys):
    S = 256
    p = torch.softmax(torch.randn(Hs, T + 1, S, generator=ao.gen(2, Hs, T, n_keys)), dim=-1)
    out = torch.full((T + 1, S), ao.SENTINEL, dtype=F32)
    ops.align_cost(p, T, n_keys, out)
    ref, bound = ao.cost64(p, T, n_keys)
    got = out[:T, :n_keys].double().numpy()
    assert (np.abs(got - ref) <= bound).all(), np.abs(got - ref).max()
    if T == 1:
        assert (got == 0).all()
    assert (out[T:] == ao.SENTINEL).all() and (out[:, n_keys:] == ao.SENTINEL).all()


def test_reflect_padding_does_not_repeat_the_edge():
    assert [ao.reflect(i, 10) for i in (-3, -1, 0, 9, 10, 12)] == [3, 1, 0, 9, 8, 6]


DTW_SHAPES = [(1, 1), (1, 9), (9, 1), (5, 5), (12, 5), (40, 61)]


@pytest.mark.parametrize("T,N", DTW_SHAPES)
def test_diagonal_oracle_equals_the_plain_double_loop(T, N):
    for zero in (False, True):
        c = np.zeros((T, N)) if zero else torch.randint(-8, 9, (T, N), generator=ao.gen(3, T, N)).double().numpy()
        D0, f0, l0 = ao.dtw_plain(c)
        D1, f1, l1 = ao.dtw64(c)
        assert (D0 == D1).all() and (f0 == f1).all() and (l0 == l1).all()


@pytest.mark.parametrize("T,N", DTW_SHAPES)
def test_reference_dtw_equals_the_plain_double_loop_ties_included(T, N):
    for zero in (False, True):
        c = torch.zeros(T, N) if zero else torch.randint(-8, 9, (T, N), generator=ao.gen(3, T, N)).float()
        cost = torch.full((T + 1, N + 3), ao.SENTINEL, dtype=F32)
        cost[:T, :N] = c
        first = torch.full((T + 1,), int(ao.SENTINEL), dtype=I32)
        last = first.clone()
        ops.dtw_path(cost, T, N, first, last)
        _, f0, l0 = ao.dtw_plain(c.double().numpy())
        assert first[:T].tolist() == f0.tolist() and last[:T].tolist() == l0.tolist()
        assert first[T] == int(ao.SENTINEL) and last[T] == int(ao.SENTINEL)


def test_all_zero_costs_take_the_horizontal_step_on_every_tie():
    first, last = ops.dtw_path(torch.zeros(4, 6), 4, 6)
    # backtrack from (3, 5): horizontal to (3, 0), then up the first column
    assert first.tolist() == [0, 0, 0, 0] and last.tolist() == [0, 0, 0, 5]


def test_reference_dtw_path_is_optimal_on_random_costs():
    c = torch.randn(30, 47, generator=ao.gen(4))
    first, last = ops.dtw_path(c, 30, 47)
    ao.check_path(c.numpy(), first.tolist(), last.tolist(), "cpu 30x47")


@pytest.mark.parametrize("N,V", [(1, 100), (5, 100), (3, 1000)])
def test_reference_token_logprob_matches_f64_logsumexp(N, V):
    g = ao.gen(5, N, V)
    Vp = (V + 15) // 16 * 16
    logits = torch.full((N, Vp), 1e30, dtype=F32)
    logits[:, :V] = torch.randn(N, V, generator=g) * 3
    targets = torch.randint(0, V, (N,), generator=g).tolist()
    ref = ao.logprob64(logits, targets, None, V)
    got = ops.token_logprob(logits, targets, None, V).double().numpy()
    assert (np.abs(got - ref) <= ao.logprob_bound(ref)).all()
    bits = torch.rand(N, V, generator=g).numpy() < 0.5
    bits[np.arange(N), targets] = True
    mask = torch.from_numpy(np.stack([ao.pack_mask(b) for b in bits]))
    ref = ao.logprob64(logits, targets, bits, V)
    got = ops.token_logprob(logits, targets, mask, V).double().numpy()
    assert (np.abs(got - ref) <= ao.logprob_bound(ref)).all()
    only = np.zeros((N, V), dtype=bool)
    only[np.arange(N), targets] = True
    mask = torch.from_numpy(np.stack([ao.pack_mask(b) for b in only]))
    assert (ops.token_logprob(logits, targets, mask, V) == 0).all()
    # host-known targets: out of range and masked-out ones are rejected by the wrapper
    with pytest.raises(ValueError):
        ops.token_logprob(logits, [V] * N, None, V)
    with pytest.raises(ValueError):
        ops.token_logprob(logits, [(t + 1) % V for t in targets], mask, V)


# ----------------------------------------------------------------------------- word grouping
TOKS = {0: b" Hello", 1: b",", 2: b" wor", 3: b"ld", 4: b" caf", 5: b"\xc3", 6: b"\xa9", 7: b' "', 8: b"Hi", 9: b'!"',
        10: b"Yes", 11: b" \xe2\x82", 12: b"\xac"}


def _al(tokens, first=None, last=None, lp=None, n_keys=100):
    n = len(tokens)
    first = first if first is not None else [5 * i for i in range(n)]
    last = last if last is not None else [5 * i + 4 for i in range(n)]
    return Alignment(list(tokens), first, last, lp if lp is not None else [-0.1] * n, n_keys)


def test_multi_token_words_take_first_start_last_end_and_mean_logprob():
    al = _al([0, 1, 2, 3], first=[3, 10, 12, 20], last=[9, 11, 19, 30], lp=[-0.2, -0.4, -1.0, 0.0])
    w = group_words(al, TOKS.__getitem__, t_offset=2.0, duration=10.0)
    assert [x["punctuated_word"] for x in w] == ["Hello,", "world"]
    assert [x["word"] for x in w] == ["hello", "world"]
    assert w[0]["start"] == 2.06 and w[0]["end"] == 2.24   # 0.02 * 3, 0.02 * (11 + 1)
    assert w[1]["start"] == 2.24 and w[1]["end"] == 2.62
    assert w[0]["confidence"] == round(float(np.exp(-0.3)), 4) and w[1]["confidence"] == round(float(np.exp(-0.5)), 4)
    assert set(w[0]) == {"word", "punctuated_word", "start", "end", "confidence"}


def test_a_split_utf8_character_is_merged_into_one_unit():
    w = group_words(_al([4, 5, 6, 11, 12]), TOKS.__getitem__)
    assert [x["punctuated_word"] for x in w] == ["café", "€"]
    assert w[0]["start"] == 0.0 and w[0]["end"] == 0.3 and w[1]["start"] == 0.3 and w[1]["end"] == 0.5
    # a transcript cut inside a character still yields a word
    assert len(group_words(_al([4, 5]), TOKS.__getitem__)) == 1


def test_leading_punctuation_is_stripped_from_word_only():
    w = group_words(_al([7, 8, 9]), TOKS.__getitem__)
    assert len(w) == 1 and w[0]["punctuated_word"] == '"Hi!"' and w[0]["word"] == "hi"


def test_a_single_token_is_one_word_and_end_is_clipped_to_the_utterance():
    w = group_words(_al([10], first=[0], last=[49], lp=[-0.5]), TOKS.__getitem__, t_offset=1.0, duration=0.7)
    assert w == [{"word": "yes", "punctuated_word": "Yes", "start": 1.0, "end": 1.7,
                  "confidence": round(float(np.exp(-0.5)), 4)}]
    assert group_words(_al([]), TOKS.__getitem__) == [] and confidence([]) == 0.0


# ----------------------------------------------------------------------------- events
def test_results_event_defaults_are_unchanged():
    ev = results_event("hi", is_final=True, start=1.23456, duration=2.0, model="m")
    assert ev == {"type": "Results", "channel_index": [0, 1], "duration": 2.0, "start": 1.235, "is_final": True,
                  "speech_final": True,
                  "channel": {"alternatives": [{"transcript": "hi", "confidence": 0.0, "words": []}]},
                  "metadata": {"model_info": {"name": "m"}}}
    assert Hypothesis().words == [] and Hypothesis().confidence == 0.0
    ev = results_event("hi", is_final=True, start=0, duration=1, model="m", confidence=0.5, words=[{"word": "hi"}])
    assert ev["channel"]["alternatives"][0] == {"transcript": "hi", "confidence": 0.5, "words": [{"word": "hi"}]}


class Scripted:
    """A recognizer that records how it was asked; on a words pass it returns one word."""

    def __init__(self, takes_words):
        self.calls = []
        self.takes_words = takes_words
        if takes_words:
            self.recognize = self._recognize_words

    def recognize(self, pcm, prefix=()):
        self.calls.append(None)
        return Hypothesis([1, 2], "hello there")

    def _recognize_words(self, pcm, prefix=(), words=False):
        self.calls.append(words)
        if not words:
            return Hypothesis([1, 2], "hello there")
        return Hypothesis([1, 2], "hello there", [{"word": "hello", "punctuated_word": "hello", "start": 0.1,
                                                   "end": 0.4, "confidence": 0.9}], 0.8)


def _stream(sess):
    rate = 16000
    t = np.arange(int(1.6 * rate)) / rate
    speech = (np.sin(2 * np.pi * 220 * t) * 9000).astype(np.int16)
    lead = np.zeros(int(0.5 * rate), np.int16)   # dropped leading silence: the stream clock moves on
    pcm = np.concatenate([lead, speech, np.zeros(int(0.6 * rate), np.int16)])
    events = []
    for i in range(0, len(pcm), 960):
        events += sess.push(pcm[i : i + 960].tobytes())
    return events + sess.flush()


def _session(rec, **kw):
    return StreamingAsrSession(rec, partial_every_s=0.5, endpoint_silence_s=0.3, energy_threshold=300,
                               spec_silence_s=0.0, **kw)


def test_with_words_off_the_events_equal_todays(monkeypatch):
    monkeypatch.delenv("VWA_ASR_WORDS", raising=False)
    rec = Scripted(takes_words=False)  # (today's recognizer signature: any words= argument would raise)
    events = _stream(_session(rec))
    finals = [e for e in events if e["is_final"]]
    partials = [e for e in events if not e["is_final"]]
    assert len(finals) == 1 and partials
    for e in events:
        assert e == results_event("hello there", is_final=e["is_final"], start=e["start"], duration=e["duration"],
                                  model="whisper")
        assert e["channel"]["alternatives"][0] == {"transcript": "hello there", "confidence": 0.0, "words": []}


@pytest.mark.parametrize("how", ["argument", "knob"])
def test_with_words_on_the_final_carries_the_words_and_partials_do_not(monkeypatch, how):
    rec = Scripted(takes_words=True)
    if how == "knob":
        monkeypatch.setenv("VWA_ASR_WORDS", "1")
        sess = _session(rec)
    else:
        monkeypatch.delenv("VWA_ASR_WORDS", raising=False)
        sess = _session(rec, words=True)
    events = _stream(sess)
    finals = [e for e in events if e["is_final"]]
    partials = [e for e in events if not e["is_final"]]
    assert len(finals) == 1 and partials
    assert rec.calls.count(True) == 1 and rec.calls[-1] is True  # only the final pass asked
    for e in partials:
        assert e["channel"]["alternatives"][0]["words"] == [] and e["channel"]["alternatives"][0]["confidence"] == 0.0
    alt = finals[0]["channel"]["alternatives"][0]
    t0 = finals[0]["start"]
    assert t0 > 0  # the leading silence was dropped: words are on the stream clock
    assert alt["confidence"] == 0.8
    assert alt["words"] == [{"word": "hello", "punctuated_word": "hello", "start": round(0.1 + t0, 3),
                             "end": round(0.4 + t0, 3), "confidence": 0.9}]


def test_the_speculative_final_pass_asks_for_words():
    rec = Scripted(takes_words=True)
    sess = StreamingAsrSession(rec, partial_every_s=10.0, endpoint_silence_s=0.4, energy_threshold=300,
                               spec_silence_s=0.1, words=True)
    events = _stream(sess)
    finals = [e for e in events if e["is_final"]]
    assert rec.calls == [True] and sess.stats["spec_used"] == 1
    assert len(finals) == 1 and finals[0]["channel"]["alternatives"][0]["words"][0]["word"] == "hello"


# ----------------------------------------------------------------------------- whisper-test end to end
@pytest.fixture(scope="module")
def engine():
    w = WhisperModel(get_config("whisper-test"), device="cpu", seed=3)
    return AsrEngine(w, load_tokenizer("whisper"), max_sessions=3)


def _tone(seconds, f0):
    t = np.arange(int(seconds * 16000)) / 16000
    return (np.sin(2 * np.pi * f0 * t) * 9000).astype(np.int16)


def check_alignment(al, n_samples, eng):
    n = len(al.tokens)
    assert al.n_keys == min(1500, -(-n_samples // 320))
    assert len(al.first_frame) == len(al.last_frame) == len(al.logprobs) == n
    assert all(a <= b for a, b in zip(al.first_frame, al.first_frame[1:]))
    assert all(0 <= f <= l < al.n_keys for f, l in zip(al.first_frame, al.last_frame))
    assert all(lp <= 0 and np.isfinite(lp) for lp in al.logprobs)
    dur = n_samples / 16000
    words = eng.words_of(al, duration=dur)
    assert all(0 <= w["start"] <= w["end"] <= round(dur, 3) and 0 <= w["confidence"] <= 1 for w in words)
    return words


def test_alignment_heads_default_config_and_checkpoint(tmp_path, monkeypatch):
    from dataclasses import replace

    from safetensors.torch import save_file

    from voice_enabled_browser_automation_amd.runtime.weights import LazySafetensors

    cfg = get_config("whisper-test")
    assert cfg.alignment_heads is None and cfg.align_heads() == ((1, 0), (1, 1))  # upper half of 2 layers
    assert get_config("whisper-large-v3").align_heads()[0] == (16, 0) and len(get_config("whisper-tiny").align_heads()) == 12
    # a generation_config.json beside the checkpoint fills the field
    save_file({"x": torch.zeros(1)}, str(tmp_path / "model.safetensors"))
    assert LazySafetensors(str(tmp_path)).generation_config() is None
    (tmp_path / "generation_config.json").write_text('{"alignment_heads": [[1, 1], [0, 0]]}')
    w = LazySafetensors(str(tmp_path))
    assert w.generation_config() == {"alignment_heads": [[1, 1], [0, 0]]}
    monkeypatch.setattr(WhisperModel, "_load", lambda self, weights: None)  # (random weights stand in)
    m = WhisperModel(cfg, device="cpu", weights=w)
    assert m.cfg.alignment_heads == ((1, 1), (0, 0))
    layers, n = m.align_layers()
    assert n == 2 and [(l, h.tolist(), off) for l, h, off in layers] == [(0, [0], 0), (1, [1], 1)]
    # an explicit field wins over the file; a head outside the model is an error
    assert WhisperModel(replace(cfg, alignment_heads=((1, 0),)), device="cpu", weights=w).align_layers()[1] == 1
    with pytest.raises(ValueError):
        WhisperModel(replace(cfg, alignment_heads=((2, 0),)), device="cpu").align_layers()
    eng = AsrEngine(m, load_tokenizer("whisper"), max_sessions=1)
    audio = eng.pcm_to_audio(_tone(1.0, 220))
    assert eng.decode_many([audio], exact_tokens=6, words=True) == eng.decode_many([audio], exact_tokens=6)
    assert check_alignment(eng.last_alignments[0], 16000, eng)


def test_whisper_test_words_on_returns_the_same_tokens_and_a_valid_alignment(engine):
    pcms = [_tone(1.0, 220), _tone(2.5, 330), _tone(0.31, 440)]
    audios = [engine.pcm_to_audio(p) for p in pcms]
    # 40 tokens for three sessions: 132 teacher-forced rows, three steps, sessions split across steps
    plain = engine.decode_many(audios, exact_tokens=40)
    prefix = [plain[0][:3], [], plain[2][:1]]
    base = engine.decode_many(audios, prefix, exact_tokens=40)
    with_words = engine.decode_many(audios, prefix, exact_tokens=40, words=True)
    assert with_words == base
    assert len(engine.free_slots) == 3
    for i, al in enumerate(engine.last_alignments):
        assert al.tokens == prefix[i] + base[i]
        assert check_alignment(al, len(pcms[i]), engine)
    # EOT-terminated decoding (the sampler's other mask) and the recognizer's hypothesis
    rec = EngineRecognizer(engine, max_tokens=6, words=True)
    h0 = rec.recognize(pcms[1], words=True)
    h1 = rec.recognize(pcms[1])
    assert h0.tokens == h1.tokens and h0.text == h1.text and h1.words == [] and h1.confidence == 0.0
    if h0.tokens:
        assert h0.words and 0 < h0.confidence <= 1
    off = EngineRecognizer(engine, max_tokens=6, words=False).recognize(pcms[1], words=True)
    assert off.words == [] and off.tokens == h1.tokens
