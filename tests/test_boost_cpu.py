"""Keyterm boosting on the CPU: the compiler (asr/keyterms.py) and the reference step against the
brute-force definition, the tables' invariants, variants and rejections, the engine on whisper-test
held step by step to the oracle through all three decode paths, and the streaming layers with a fake
engine.  Every comparison of logits is bitwise and every comparison of states and tokens exact."""
import random
import threading
import types

import numpy as np
import pytest
import torch

import beam_cases
import boost_cases as bc
import boost_oracle as bo
import voice_enabled_browser_automation_amd.ops as ops
from voice_enabled_browser_automation_amd.asr import keyterms as kt
from voice_enabled_browser_automation_amd.asr import streaming as st
from voice_enabled_browser_automation_amd.asr.engine import AsrEngine
from voice_enabled_browser_automation_amd.models.config import get_config
from voice_enabled_browser_automation_amd.models.whisper import WhisperModel
from voice_enabled_browser_automation_amd.tokenizer import load_tokenizer

V = bc.V


# ---------------------------------------------------------------- compiler and reference step
def histories(seqs, n: int, seed: int):
    """Random histories over the 40-id vocabulary, salted with pieces of the sequences so that
    partial matches, overlaps and completions all occur."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        h = []
        while len(h) < rng.randint(0, 24):
            if rng.random() < 0.6:
                q = rng.choice(seqs)[0]
                a = rng.randint(0, len(q) - 1)
                h += q[a : rng.randint(a + 1, len(q))]
            else:
                h.append(rng.randrange(V))
        out.append(h)
    return out


@pytest.mark.parametrize("name", sorted(bc.SETS))
def test_compiler_and_reference_step_match_the_brute_force_definition(name):
    seqs = bc.SETS[name]
    ks = kt.compile_sequences(seqs, limit=V)
    states = bo.path_states(ks, seqs)
    tables = (ks.edge_off, ks.edge_tok, ks.edge_next, ks.edge_bias, np.zeros(ks.n_states, np.int32))
    t_tables = bc.tables_on(tables, "cpu")
    i32 = dict(dtype=torch.int32)
    for n, h in enumerate(histories(seqs, 60, 7)):
        # the host automaton, token by token
        s = 0
        for k, t in enumerate(h):
            s = ks.step(s, t)
            assert s == states[bo.state_brute(seqs, h[: k + 1])], (name, h[: k + 1])
        assert ks.run(h) == s
        want = bo.bias_brute(seqs, h)
        assert {t: b for t, b in ks.bias(s).items()} == {t: float(np.float32(b)) for t, b in want.items()}
        # the reference step: from the state before the last token, on that token (or apply only)
        x = bc.rand_logits(1, bc.LD, V, 100 + n, pad_rows=1)
        y = x.clone()
        out = torch.full((1,), -5, **i32)
        if h:
            ops.boost_step(y, V, t_tables, torch.zeros(1, **i32), torch.tensor([ks.run(h[:-1])], **i32), out,
                           tokens=torch.tensor([h[-1]], **i32))
        else:
            ops.boost_step(y, V, t_tables, torch.zeros(1, **i32), torch.zeros(1, **i32), out)
        assert int(out[0]) == s
        assert bo.bits_equal(y[0], bo.boosted(x[0], want, V)) and bo.bits_equal(y[1], x[1]), (name, h)


def test_the_same_sequence_twice_takes_the_larger_boost_and_a_suffix_term_keeps_its_own():
    assert bo.bias_brute(bc.TWICE, [3]) == {3: 4.0, 4: 4.0}
    ks = kt.compile_sequences(bc.TWICE, limit=V)
    assert ks.bias(ks.run([3]))[4] == 4.0 and ks.bias(ks.run([4]))[3] == 4.0  # ([3, 4] restarting beats [4, 3]'s 2.0)
    ks = kt.compile_sequences(bc.SUFFIX, limit=V)
    s = ks.run([10, 11, 12])
    assert ks.bias(s)[13] == 5.0 and ks.bias(s)[14] == 2.0  # [12, 13] and [11, 12, 14] inside [10, 11, 12, 13]
    assert kt.compile_sequences(list(reversed(bc.SUFFIX)), limit=V) is ks  # cached by content


@pytest.mark.parametrize("names", [("collide",), ("collide", "twice", "suffix", "long"), ("long", "long", "suffix")])
def test_table_invariants(names):
    sets, bases, (off, tok, nxt, bias, root) = bc.joint(names)
    S, E = len(root), len(tok)
    assert len(off) == S + 1 and off[0] == 0 and off[-1] == E and (np.diff(off) >= 0).all()
    assert len(nxt) == len(bias) == E and bias.dtype == np.float32 and (bias > 0).all()
    assert S == sum(k.n_states for k in sets) and E == sum(k.n_edges for k in sets)
    for base, ks in zip(bases, sets):
        assert (root[base : base + ks.n_states] == base).all() and root[base] == base
        for s in range(base, base + ks.n_states):
            lst = tok[off[s] : off[s + 1]]
            assert (np.diff(lst) > 0).all(), f"state {s}: tokens do not ascend strictly"
            assert ((nxt[off[s] : off[s + 1]] > base) & (nxt[off[s] : off[s + 1]] < base + ks.n_states)).all()
        assert off[base + 1] - off[base] == len({q[0] for q, _ in ks.key})  # a root's list: its children
    assert sorted(set(root.tolist())) == sorted(bases)


class Tok:
    """A word-piece stand-in: a letter is the id of its code point, a space joins the next letter
    (+ 1000), like a byte-level BPE's leading-space pieces."""

    def encode(self, text):
        out, space = [], False
        for ch in text:
            if ch == " ":
                space = True
                continue
            out.append(ord(ch) + (1000 if space else 0))
            space = False
        return out


def test_variants_and_rejections():
    assert kt.variants("grafana") == ["grafana", " grafana", "Grafana", " Grafana"]
    assert kt.variants(" Pull request ") == ["Pull request", " Pull request", "pull request", " pull request"]
    assert kt.variants("OK") == ["OK", " OK", "ok", " ok"]
    ks = kt.compile_keyterms(["ab", ("Ab", 3.0)], Tok(), 5000, default_boost=1.5)
    # both terms expand to the same four spellings: de-duplicated, each with the larger boost
    assert dict(ks.key) == {(97, 98): 3.0, (1097, 98): 3.0, (65, 98): 3.0, (1065, 98): 3.0}
    ks = kt.compile_keyterms(["ab", ("C d", 3.0)], Tok(), 5000, default_boost=1.5)
    assert dict(ks.key) == {(97, 98): 1.5, (1097, 98): 1.5, (65, 98): 1.5, (1065, 98): 1.5, (67, 1100): 3.0,
                            (1067, 1100): 3.0, (99, 1100): 3.0, (1099, 1100): 3.0}
    assert kt.compile_keyterms([], Tok(), 5000) is None
    for bad, match in (([""], "non-empty"), (["x" * 17], "17 tokens"), ([("ab", 0.0)], "positive"),
                       ([("ab", float("nan"))], "finite"), ([("ab", float("inf"))], "finite"),
                       ([("ab", -1.0)], "positive"), ([("ab", "much")], "not a number")):
        with pytest.raises(ValueError, match=match):
            kt.compile_keyterms(bad, Tok(), 5000, default_boost=1.0)
    with pytest.raises(ValueError, match="'ab'.*below 98"):
        kt.compile_keyterms(["ab"], Tok(), 98)  # an id at or above eot: a special id
    with pytest.raises(ValueError, match="1..16"):
        kt.compile_sequences([([], 1.0)], limit=V)
    with pytest.raises(ValueError, match="below 40"):
        kt.compile_sequences([([3, 40], 1.0)], limit=V)
    assert kt.compile_sequences([(list(range(16)), 1e-3)], limit=V).n_states == 17  # any finite positive boost


# ---------------------------------------------------------------- the engine on the CPU
@pytest.fixture(scope="module")
def eng():
    model = WhisperModel(get_config("whisper-test"), device="cpu", seed=0)
    return AsrEngine(model, load_tokenizer("whisper"), max_sessions=10)


@pytest.fixture(scope="module")
def audios(eng):
    return [eng.pcm_to_audio(beam_cases.tone(s, f)) for s, f in beam_cases.TONES]


@pytest.fixture(scope="module")
def cycle(eng, audios):
    return bc.pick_cycle(eng, audios[0])


@pytest.fixture()
def traced(eng):
    eng.keep_boost_trace = True
    yield eng
    eng.keep_boost_trace = False


def _sets(eng, cycle):
    """Two keyterm sets for the traced runs: real text terms, and sequences built on the ids this
    model decodes (so that partial matches, completions and restarts happen in the trace)."""
    text = eng.compile_keyterms(["Grafana", ("pull request", 3.0), "open Browserbase"], 2.0)
    plain = eng.decode_many([torch.zeros(4000)], exact_tokens=3)[0]
    ids = kt.compile_sequences([(plain[:2], 0.5), (plain[:1] + cycle[:2], 4.0), (cycle, 6.0), (cycle[1:3], 2.5)],
                               limit=eng.model.cfg.eot)
    return text, ids


def test_engine_greedy_and_batched_rows_match_the_oracle_at_every_step(traced, audios, cycle):
    eng = traced
    text, ids = _sets(eng, cycle)
    outs = eng.decode_many(audios[:1], max_tokens=8, keyterms=[ids])  # one session: steps from the host
    assert len(eng.last_boost_trace) == max(1, len(outs[0]) + (len(outs[0]) < 8)) and eng.last_stats["boosted"] == 1
    assert bc.check_trace(eng, eng.last_boost_trace) >= 1
    # a batch mixing sets, a plain row and a forced prefix; rows drop out at different steps
    outs = eng.decode_many(audios + audios[:1], [[], cycle[:2], [], cycle[:1]], max_tokens=7,
                           keyterms=[ids, ids, None, text])
    trace = eng.last_boost_trace
    assert bc.check_trace(eng, trace) >= 6 and eng.last_stats["boosted"] == 3
    assert trace[0]["history"] == [[], cycle[:2], [], cycle[:1]] and trace[0]["utts"] == [0, 1, 2, 3]
    for s in trace[1:]:  # the history of a row is its prefix and what it has decoded
        for j, h in zip(s["utts"], s["history"]):
            assert h == ([[], cycle[:2], [], cycle[:1]][j] + outs[j])[: len(h)]
    # exact mode (no end of text): every row runs every step
    eng.decode_many(audios[:2], exact_tokens=5, keyterms=[text, ids])
    assert len(eng.last_boost_trace) == 5 and bc.check_trace(eng, eng.last_boost_trace) == 10


def test_engine_beams_match_the_oracle_at_every_step(traced, audios, cycle):
    eng = traced
    text, ids = _sets(eng, cycle)
    # bc.check_trace of the beam tests runs the call: the select's kept logits are the biased ones
    outs, steps, _ = beam_cases.check_trace(eng, audios[:2], 3, max_tokens=6, keyterms=[ids, text],
                                            prefixes=[cycle[:1], []])
    trace, beam_trace = eng.last_boost_trace, eng.last_beam_trace
    assert len(trace) == steps
    assert bc.check_trace(eng, trace, beams=3) >= steps
    for s, b in zip(trace, beam_trace):
        assert s["utts"] == [j for j in b["utts"] for _ in range(3)]
        assert bo.bits_equal(s["after"], b["logits"]), "the select did not read the biased logits"
        assert s["parents"] == b["parents"] and s["tokens"] == b["tokens"]
    beam_cases.check_invariants(eng, 2, 3, max_tokens=6)
    # a plain row among boosted ones, and an utterance that finishes early (its rows move up)
    eng.decode_many(audios, max_tokens=5, beam_size=2, keyterms=[None, ids, text])
    assert bc.check_trace(eng, eng.last_boost_trace, beams=2) >= 4


def test_a_keyterm_straddles_the_forced_prefix(eng, audios, cycle):
    q = cycle
    ks = kt.compile_sequences([(q, 1e4)], limit=eng.model.cfg.eot)
    assert eng.decode_many(audios[:1], exact_tokens=10, keyterms=[ks]) == [(q * 3)[:10]]
    # the prefix's last two tokens are the keyterm's first two: decoding continues inside it
    assert eng.decode_many(audios[:1], [q[:2]], exact_tokens=10, keyterms=[ks]) == [(q[2:] + q * 3)[:10]]
    # batched rows and beams see the same prefix state
    outs = eng.decode_many(audios[:2], [q[:2], q[:3]], exact_tokens=4, keyterms=[ks, ks])
    assert outs == [(q[2:] + q)[:4], (q[3:] + q)[:4]]
    assert eng.decode_many(audios[:1], [q[:2]], exact_tokens=4, keyterms=[ks], beam_size=3) == [(q[2:] + q)[:4]]


def test_off_means_off(eng, audios, monkeypatch):
    before = eng.decode_many(audios[:2], max_tokens=8)
    beams = eng.decode_many(audios[:1], max_tokens=6, beam_size=3)
    bufs = eng._boost_bufs

    def boom(*a, **k):
        raise AssertionError("ops.boost_step reached without keyterms")

    monkeypatch.setattr(ops, "boost_step", boom)
    monkeypatch.setattr(ops, "boost_ext", boom)
    assert eng.decode_many(audios[:2], max_tokens=8, keyterms=None) == before
    assert eng.decode_many(audios[:2], max_tokens=8, keyterms=[None, None]) == before
    assert eng.decode_many(audios[:1], max_tokens=6, beam_size=3, keyterms=[None]) == beams
    assert eng._boost_bufs is bufs and "boosted" not in eng.last_stats  # nothing allocated either
    fresh = AsrEngine(eng.model, eng.tok, max_sessions=2)
    fresh.decode_many(audios[:1], max_tokens=2, keyterms=[None])
    assert fresh._boost_bufs is None


def test_capacity_and_argument_errors_come_before_anything_is_launched(eng, audios, monkeypatch):
    free = list(eng.free_slots)
    rng = random.Random(3)
    big = [kt.compile_sequences([([rng.randrange(5000) for _ in range(16)], 1.0) for _ in range(200)], limit=50000)
           for _ in range(3)]
    assert sum(k.n_states for k in big) > ops.BOOST_CAP_STATES >= max(k.n_states for k in big)
    monkeypatch.setattr(eng.model, "mel_batch", lambda *a: (_ for _ in ()).throw(AssertionError("launched")))
    with pytest.raises(RuntimeError, match="keyterm automata hold .* more than the engine's tables"):
        eng.decode_many(audios, max_tokens=2, keyterms=big)
    with pytest.raises(ValueError, match="2 entries for 3 utterances"):
        eng.decode_many(audios, max_tokens=2, keyterms=big[:2])
    with pytest.raises(TypeError, match="not a compiled KeytermSet"):
        eng.decode_many(audios[:1], max_tokens=2, keyterms=[["Grafana"]])
    assert eng.free_slots == free


def test_identical_sets_share_one_automaton_and_unchanged_tables_are_not_copied_again(eng, audios):
    a = eng.compile_keyterms(["Grafana"], 2.0)
    b = eng.compile_keyterms([("Grafana", 2.0)])
    assert a is b
    eng.decode_many(audios[:2], max_tokens=2, keyterms=[a, b])
    assert eng._boost_bufs.key == (a.key,)
    root = eng._boost_bufs.tables[4]
    assert int((root == 0).sum()) == a.n_states and int((root == -1).sum()) == ops.BOOST_CAP_STATES - a.n_states


# ---------------------------------------------------------------- streaming and batcher (fake engine)
class FakeEngine:
    """decode_many records (ids of the passes, their keyterm sets) and answers one token per pass."""

    def __init__(self, slots: int, gate: threading.Event = None):
        self.free_slots = list(range(slots))
        self.model = types.SimpleNamespace(device=None, cfg=types.SimpleNamespace(eot=5000))
        self.tok = Tok()
        self.tok.decode = lambda toks: " ".join(str(t) for t in toks)
        self.calls = []
        self.last_alignments, self.last_sot, self.last_beams = [], [], []
        self.gate = gate

    def max_prefix(self):
        return 100

    def pcm_to_audio(self, pcm):
        return pcm

    def decode_many(self, audios, prefixes, keyterms=None, **kw):
        if self.gate is not None:
            self.gate.wait(10)
        ids = [int(a[0]) for a in audios]
        self.calls.append((ids, None if keyterms is None else [None if k is None else k.key for k in keyterms]))
        return [[i] for i in ids]


def _pcm(i):
    return np.full(160, i, dtype=np.int16)


def test_batcher_mixes_sets_in_one_batch_and_splits_a_round_that_exceeds_the_tables():
    gate = threading.Event()
    eng = FakeEngine(8, gate)
    b = st.AsrBatcher(eng, words=False)
    ka, kb, kc = (b.compile_keyterms([t]) for t in ("ab", "cd", "efgh"))
    assert ka is b.compile_keyterms([("ab", 2.0)]) and b.compile_keyterms([]) is None
    try:
        first = b.recognize_async(_pcm(1))  # occupies the scheduler until the gate opens
        while b.queue_depth():
            pass
        b.cap_states = ka.n_states + kb.n_states + 1  # room for two of the three sets
        futs = [b.recognize_async(_pcm(i), keyterms=k) for i, k in
                ((2, ka), (3, None), (4, ["cd"]), (5, kc), (6, ka), (7, None))]
        gate.set()
        assert [f.result(timeout=20).tokens for f in futs] == [[i] for i in range(2, 8)]
        first.result(timeout=20)
    finally:
        gate.set()
        b.close()
    assert eng.calls[0] == ([1], None)  # a plain batch carries no keyword at all
    # one batch mixes two sets, plain passes and a repeated set; the pass whose set does not fit waits
    assert eng.calls[1] == ([2, 3, 4, 6, 7], [ka.key, None, kb.key, ka.key, None])
    assert eng.calls[2] == ([5], [kc.key])
    assert b.stats["boosted_passes"] == 4 and b.stats["passes"] == 7
    small = st.AsrBatcher(FakeEngine(4), words=False)
    small.cap_states = 3
    try:
        with pytest.raises(ValueError, match="exceed the engine's tables"):
            small.recognize_async(_pcm(1), keyterms=["efgh"])
    finally:
        small.close()


def test_engine_recognizer_compiles_text_terms_and_passes_the_set():
    eng = FakeEngine(4)
    rec = st.EngineRecognizer(eng, words=False)
    rec.recognize(_pcm(3), keyterms=[("ab", 1.0)])
    rec.recognize(_pcm(4))
    ks = rec.compile_keyterms([("ab", 1.0)])
    assert eng.calls == [([3], [ks.key]), ([4], None)]


class Recorder:
    """A recognizer that records every pass's keywords."""

    def __init__(self):
        self.passes = []

    def recognize(self, pcm, prefix=(), **kw):
        self.passes.append(kw)
        return st.Hypothesis([len(self.passes)], f"pass {len(self.passes)}")


def _speech(seconds: float) -> bytes:
    t = np.arange(int(seconds * 16000)) / 16000
    return (np.sin(2 * np.pi * 300 * t) * 8000).astype("<i2").tobytes()


def test_session_passes_its_set_on_every_pass_and_set_keyterms_applies_at_the_next():
    rec = Recorder()
    s = st.StreamingAsrSession(rec, partial_every_s=0.5, spec_silence_s=0.1, endpoint_silence_s=0.3,
                               keyterms=[("Grafana", 2.0)], language="en")
    s.push(_speech(0.6))                      # a partial
    assert rec.passes[-1]["keyterms"] == [("Grafana", 2.0)]
    s.set_keyterms([("Browserbase", 3.0)])
    assert len(rec.passes) == 1               # nothing runs because of it
    s.push(_speech(0.6))                      # the next partial carries the new set
    assert rec.passes[-1]["keyterms"] == [("Browserbase", 3.0)]
    s.push(b"\0" * int(0.2 * 32000))          # the speculative final
    s.push(b"\0" * int(0.2 * 32000))          # the endpoint: the speculative pass is the final
    assert len(rec.passes) == 3 and all(p["keyterms"] == [("Browserbase", 3.0)] for p in rec.passes[1:])
    assert s.stats["boosted_passes"] == 3 and s.stats["finals"] == 1
    s.set_keyterms(None)
    s.push(_speech(0.6))
    assert "keyterms" not in rec.passes[-1] and s.stats["boosted_passes"] == 3
    # a session without keyterms never passes the keyword (recognizers with the old signature)
    plain = st.StreamingAsrSession(lambda pcm: "hi", partial_every_s=0.5)
    assert plain.push(_speech(0.6)) and plain.keyterms is None
    # with a compiling recognizer the set is compiled once, when it is set -- and a bad term raises there
    eng = FakeEngine(4)
    s2 = st.StreamingAsrSession(st.EngineRecognizer(eng, words=False), partial_every_s=0.5, keyterms=["ab"])
    assert isinstance(s2.keyterms, kt.KeytermSet)
    with pytest.raises(ValueError, match="17 tokens"):
        s2.set_keyterms(["x" * 17])
    assert isinstance(s2.keyterms, kt.KeytermSet)
    s2.push(_speech(0.6))
    assert eng.calls[-1][1] == [s2.keyterms.key]


def test_tables_count_as_loaded_only_once_their_copy_is_queued(eng, audios, monkeypatch):
    """A call that fails between writing the pinned mirror and the first staging copy leaves the
    engine holding no set: the next call with the same sets copies the tables (it must not trust a
    device block that never received them)."""
    rng = random.Random(5)
    ks = kt.compile_sequences([([rng.randrange(4000) for _ in range(3)], 1.0 + k) for k in range(5)], limit=50000)
    good = eng.model.mel_batch
    monkeypatch.setattr(eng.model, "mel_batch", lambda *a: (_ for _ in ()).throw(RuntimeError("encoder failed")))
    with pytest.raises(RuntimeError, match="encoder failed"):
        eng.decode_many(audios[:1], max_tokens=2, keyterms=[ks])
    assert eng._boost_bufs.key is None
    monkeypatch.setattr(eng.model, "mel_batch", good)
    eng.keep_boost_trace = True
    try:
        eng.decode_many(audios[:1], max_tokens=3, keyterms=[ks])
        assert eng._boost_bufs.key == (ks.key,) and bc.check_trace(eng, eng.last_boost_trace) >= 1
        assert torch.equal(eng._boost_bufs.tables[1][: ks.n_edges], torch.from_numpy(ks.edge_tok))
    finally:
        eng.keep_boost_trace = False
    assert eng.d_tok.numel() >= 64  # one token buffer for the engine's life (captured loops read it)
