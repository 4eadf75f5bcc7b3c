"""Beam search on the CPU: the torch references of both ops against the oracle and the contract
(tests/beam_cases.py asks the GPU kernels the same), the kernels' resource budget, the host
bookkeeping with scripted candidates, the engine scenario with whisper-test, the batcher with a fake
engine, the final event's alternatives and the two settings."""
import math
import os
import re
import struct
import subprocess
import threading
import types

import numpy as np
import pytest
import torch

import beam_cases as bc
import voice_enabled_browser_automation_amd.ops as ops
from voice_enabled_browser_automation_amd.asr import beam as rule
from voice_enabled_browser_automation_amd.asr import streaming as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
CPU = "cpu"


# ---------------------------------------------------------------- the references
@pytest.mark.parametrize("gw", range(len(bc.GW)), ids=[f"G{g}W{w}" for g, w in bc.GW])
@pytest.mark.parametrize("vocab", [200, 40])
def test_reference_beam_select_matches_the_oracle(vocab, gw):
    G, W = bc.GW[gw]
    for mi, mask_kind in enumerate(bc.MASKS):
        for ci, cum_kind in enumerate(bc.CUMS):
            bc.check_case(vocab, G, W, mask_kind, cum_kind, 5000 + 100 * gw + 10 * mi + ci + vocab, CPU)


@pytest.mark.parametrize("edge", bc.EDGES, ids=[e.__name__[5:] for e in bc.EDGES])
def test_reference_beam_select_edge(edge):
    edge(CPU)


@pytest.mark.parametrize("kind", ["zero", "swap", "mixed", "identity"])
@pytest.mark.parametrize("W", [2, 5, 8])
def test_reference_kv_beam_gather(W, kind):
    for n_ctx in (1, 16, 17, 64):
        bc.check_gather(W, kind, n_ctx, CPU)


def test_wrappers_reject_bad_arguments_before_anything_runs():
    x, cum = torch.zeros(72, 64), torch.zeros(72)
    mask = torch.full((1, 2), -1, dtype=torch.int32)
    for rows, vocab, W, kw in ((4, 40, 1, {}), (9, 40, 9, {}), (72, 40, 8, {}), (7, 40, 2, {}), (4, 65, 2, {}),
                               (4, 40, 2, dict(mask=mask.long())), (4, 40, 2, dict(mask=mask[:, :1])),
                               (4, 40, 2, dict(cand_beam=torch.zeros(2, 4))),
                               (4, 40, 2, dict(cand_tok=torch.zeros(2, 3, dtype=torch.int32)))):
        with pytest.raises(ValueError):
            ops.beam_select(x[:rows], cum[:rows], kw.pop("mask", mask), vocab, W, **kw)
    with pytest.raises(ValueError):
        ops.beam_select(x[:4].double(), cum[:4], mask, 40, 2)
    k, v, table = bc.kv_caches(4)
    before = k.clone()
    good = dict(slots=bc.SLOTS[5], parents=[[1, 0, 0, 3, 1]], n_ctx=[16])
    for bad in (dict(slots=[[3]], parents=[[0]]), dict(parents=[[1, 0, 5, 3, 1]]), dict(parents=[[1, 0, -1, 3, 1]]),
                dict(slots=[[6, 1, 8, 3, 0]]), dict(slots=[[6, 1, 6, 3, 0]]), dict(n_ctx=[65]), dict(max_ctx=65),
                dict(parents=[[1, 0, 0]]), dict(slots=[[0, 1]] * 33, parents=[[1, 0]] * 33, n_ctx=[1] * 33)):
        a = {**good, **bad}
        with pytest.raises(ValueError):
            ops.kv_beam_gather(k, v, table, a["slots"], a["parents"], a["n_ctx"], max_ctx=a.get("max_ctx"))
    with pytest.raises(ValueError):
        ops.kv_beam_gather(k, v.float(), table, **good)
    with pytest.raises(ValueError):
        ops.kv_beam_gather(k, v, table.long(), **good)
    assert torch.equal(k.view(torch.int16), before.view(torch.int16))


# ---------------------------------------------------------------- resources
def _kernels(obj_rel):
    """name -> metadata text of every gfx950 kernel in a built object (the offload bundle's code
    object, read with llvm-readelf --notes: tests/test_kernel_resources_cpu.py's way)."""
    path = os.path.join(ROOT, "build", "native", obj_rel)
    if not os.path.exists(path) or not os.path.exists(READELF):
        pytest.skip("kernel objects not built here (python -c 'import __graft_entry__ as g; g.build()')")
    data = open(path, "rb").read()
    i = data.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert i >= 0, "no offload bundle in " + obj_rel
    p = i + 24
    (n,) = struct.unpack_from("<Q", data, p)
    p += 8
    code = None
    for _ in range(n):
        off, size, tl = struct.unpack_from("<QQQ", data, p)
        p += 24
        triple = data[p : p + tl].decode()
        p += tl
        if "gfx950" in triple:
            code = data[i + off : i + off + size]
    assert code is not None, "no gfx950 code object in " + obj_rel
    tmp = os.path.join("/tmp", f"vwa_{os.getpid()}_{os.path.basename(obj_rel)}.co")
    with open(tmp, "wb") as fh:
        fh.write(code)
    try:
        notes = subprocess.run([READELF, "--notes", tmp], capture_output=True, text=True, check=True).stdout
    finally:
        os.unlink(tmp)
    out = {}
    for m in re.finditer(r"\.name:\s+(\S+)", notes):
        blk = notes[m.start() : m.start() + 3000]
        nxt = blk.find(".name:", 10)
        blk = blk[:nxt] if nxt > 0 else blk
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        vg = re.search(r"\.vgpr_count:\s+(\d+)", blk)
        sp = re.search(r"\.vgpr_spill_count:\s+(\d+)", blk)
        if ps and vg:
            out[m.group(1)] = (int(ps.group(1)), int(vg.group(1)), int(sp.group(1)) if sp else 0)
    return out


def test_beam_kernels_use_no_scratch():
    for obj, pats in (("beam/beam_select.hip.o", ("lse_part_kernel", "row_topk_kernel", "group_merge_kernel")),
                      ("beam/kv_gather.hip.o", ("kv_beam_gather_kernel",))):
        ks = _kernels(obj)
        for pat in pats:
            hit = {k: v for k, v in ks.items() if pat in k}
            assert hit, f"{pat} not in {obj}: {sorted(ks)}"
            bad = {k: v for k, v in hit.items() if v[0] > 0 or v[2] > 0}
            assert not bad, f"{pat} uses scratch (private segment bytes, VGPRs, spilled VGPRs): {bad}"
            print(f"MEASURED {pat} (scratch bytes, VGPRs, spills) {list(hit.values())}")


# ---------------------------------------------------------------- bookkeeping
EOT = 99
NONE = (float("-inf"), -1, -1)


def test_first_step_only_beam_zero_is_alive():
    st = rule.BeamState(3, EOT, 8)
    assert st.cum == [0.0, float("-inf"), float("-inf")] and st.tokens == [[], [], []] and not st.done
    par, tok = rule.advance(st, [(-1.0, 0, 5), (-2.0, 0, 7), (-3.0, 0, 2), (-4.0, 0, 9), (-5.0, 0, 1), (-6.0, 0, 3)])
    assert (par, tok) == ([0, 0, 0], [5, 7, 2])
    assert st.tokens == [[5], [7], [2]] and st.cum == [-1.0, -2.0, -3.0] and not st.finished and not st.done


def test_eot_candidates_above_the_last_live_one_are_finished_and_the_walk_stops_there():
    st = rule.BeamState(2, EOT, 8, tokens=[[1], [2]], cum=[-1.0, -1.5])
    par, tok = rule.advance(st, [(-1.2, 0, EOT), (-1.6, 1, 4), (-1.7, 0, 6), (-1.8, 1, EOT)])
    assert (par, tok) == ([1, 0], [4, 6])
    # the first EOT is finished; the one ranked after the W-th live candidate is not
    assert [h["tokens"] for h in st.finished] == [[1]] and st.finished[0]["sum_logprob"] == -1.2
    assert st.finished[0]["avg_logprob"] == pytest.approx(-0.6)  # the EOT counts in the length
    assert st.tokens == [[2, 4], [1, 6]] and not st.done


def test_an_utterance_stops_at_w_finished():
    st = rule.BeamState(2, EOT, 8, tokens=[[1], [2]], cum=[-1.0, -1.5])
    rule.advance(st, [(-1.2, 0, EOT), (-1.6, 1, EOT), (-1.7, 0, 6), (-1.8, 1, 3)])
    assert st.done and [h["tokens"] for h in st.finished] == [[1], [2]]
    # a finished list that is full takes no more
    st = rule.BeamState(2, EOT, 8, tokens=[[1], [2]], cum=[-1.0, -1.5])
    st.finished = [rule.hypothesis([7], -0.5, 2)]
    rule.advance(st, [(-1.2, 0, EOT), (-1.6, 1, EOT), (-1.7, 0, 6), (-1.8, 1, 3)])
    assert st.done and [h["tokens"] for h in st.finished] == [[7], [1]]


def test_the_token_limit_fills_the_list_from_live_beams():
    st = rule.BeamState(3, EOT, 2, tokens=[[1], [2], [3]], cum=[-1.0, -1.5, -1.6])
    st.finished = [rule.hypothesis([], -0.9, 1), rule.hypothesis([1], -3.0, 2)]
    rule.advance(st, [(-1.1, 0, 4), (-1.7, 1, 5), (-1.9, 2, 6), NONE, NONE, NONE])
    assert st.done and len(st.finished) == 3
    assert st.finished[2] == rule.hypothesis([1, 4], -1.1, 2)  # no EOT: two tokens scored
    hyps = rule.ranked(st)
    assert [h["tokens"] for h in hyps] == [[1, 4], [], [1]]


def test_ranking_is_length_normalised_and_a_longer_hypothesis_can_win():
    st = rule.BeamState(2, EOT, 8)
    st.finished = [rule.hypothesis([1], -2.0, 2), rule.hypothesis([1, 2, 3, 4, 5], -3.0, 6)]
    hyps = rule.ranked(st)
    assert [h["tokens"] for h in hyps] == [[1, 2, 3, 4, 5], [1]]  # -0.5 beats -1.0 although -3 < -2
    assert hyps[0]["avg_logprob"] == -0.5 and hyps[1]["avg_logprob"] == -1.0


def test_fewer_candidates_than_beams_leave_dead_rows_and_none_ends_the_utterance():
    st = rule.BeamState(3, EOT, 8)
    par, tok = rule.advance(st, [(-1.0, 0, 5), NONE, NONE, NONE, NONE, NONE])
    assert (par, tok) == ([0, 1, 2], [5, 0, 0]) and st.cum == [-1.0, float("-inf"), float("-inf")] and not st.done
    rule.advance(st, [NONE] * 6)
    assert st.done and rule.ranked(st) == [rule.hypothesis([], 0.0, 0)]
    assert rule.BeamState(3, EOT, 0).done


# ---------------------------------------------------------------- the engine scenario on the CPU
@pytest.fixture(scope="module")
def eng():
    from voice_enabled_browser_automation_amd.asr.engine import AsrEngine
    from voice_enabled_browser_automation_amd.models.config import get_config
    from voice_enabled_browser_automation_amd.models.whisper import WhisperModel
    from voice_enabled_browser_automation_amd.tokenizer import load_tokenizer

    model = WhisperModel(get_config("whisper-test"), device="cpu", seed=3)
    return AsrEngine(model, load_tokenizer("whisper"), max_sessions=8, use_graphs=False)


@pytest.fixture(scope="module")
def audios(eng):
    return [eng.pcm_to_audio(bc.tone(s, f)) for s, f in bc.TONES]


def test_engine_trace_matches_the_oracle_and_the_bookkeeping(eng, audios):
    free, table = list(eng.free_slots), eng.runner.b.cross_table.clone()
    greedy = eng.decode_many(audios[:2], max_tokens=8)
    free_after_greedy = list(eng.free_slots)
    total = 0
    for n, W in ((2, 3), (1, 5), (2, 4)):
        outs, steps, excused = bc.check_trace(eng, audios[:n], W, max_tokens=8)
        assert excused == 0  # (on the CPU the reference's f32 scores stand in for the kernel's)
        total += steps
        bc.check_invariants(eng, n, W, max_tokens=8)
        assert eng.last_stats["beam_size"] == W and "beam_ms" not in eng.last_stats
        assert eng.free_slots == free_after_greedy and torch.equal(eng.runner.b.cross_table, table)
    assert total >= 20
    assert sorted(eng.free_slots) == sorted(free)
    assert eng.decode_many(audios[:2], max_tokens=8) == greedy  # nothing a beam call left behind changes a decode


def test_engine_exact_tokens_min_tokens_and_prefixes(eng, audios):
    outs, _, excused = bc.check_trace(eng, audios[:2], 3, exact_tokens=6)
    assert excused == 0 and [len(o) for o in outs] == [6, 6]
    bc.check_invariants(eng, 2, 3, max_tokens=6, exact=6)
    assert all(len(h) == 3 for h in eng.last_beams)
    outs, _, _ = bc.check_trace(eng, audios[:1], 2, max_tokens=8, min_tokens=3)
    assert all(len(h["tokens"]) >= 3 for h in eng.last_beams[0])
    out = eng.decode_many(audios[:2], [[11, 12, 13], []], max_tokens=5, beam_size=2)
    assert len(out) == 2 and all(len(o) <= 5 for o in out)


def test_engine_width_one_is_the_greedy_path_and_never_reaches_the_beam_ops(eng, audios, monkeypatch):
    want = eng.decode_many(audios, max_tokens=8)

    def boom(*a, **k):
        raise AssertionError("beam op reached with beam_size = 1")

    monkeypatch.setattr(ops, "beam_select", boom)
    monkeypatch.setattr(ops, "kv_beam_gather", boom)
    monkeypatch.setattr(ops, "beam_ext", boom)
    assert eng.decode_many(audios, max_tokens=8, beam_size=1) == want
    assert "beam_size" not in eng.last_stats


def test_engine_slot_budget_and_bad_widths(eng, audios):
    free = list(eng.free_slots)
    with pytest.raises(RuntimeError, match="exceed the .* free ASR session slots"):
        eng.decode_many(audios, max_tokens=4, beam_size=3)  # 9 > 8
    for bad in (0, 9, -1):
        with pytest.raises(ValueError):
            eng.decode_many(audios[:1], max_tokens=4, beam_size=bad)
    assert eng.free_slots == free


def test_engine_words_and_auto_language_with_beams(eng, audios):
    outs = eng.decode_many(audios[:2], max_tokens=6, beam_size=3, words=True)
    assert [a.tokens for a in eng.last_alignments] == outs == [h[0]["tokens"] for h in eng.last_beams]
    outs = eng.decode_many(audios[:2], max_tokens=6, beam_size=3, languages=["auto", None])
    assert eng.last_sot[0]["language"] and eng.last_sot[0]["language_confidence"] is not None and len(outs) == 2


# ---------------------------------------------------------------- batcher, events, settings
class FakeEngine:
    """decode_many records its calls and answers with tokens that name the pass (its first sample)."""

    def __init__(self, slots: int, gate: threading.Event = None):
        self.free_slots = list(range(slots))
        self.model = types.SimpleNamespace(device=None)
        self.tok = types.SimpleNamespace(decode=lambda toks: " ".join(str(t) for t in toks))
        self.calls = []
        self.last_alignments, self.last_sot, self.last_beams = [], [], []
        self.gate = gate

    def max_prefix(self):
        return 100

    def pcm_to_audio(self, pcm):
        return pcm

    def decode_many(self, audios, prefixes, beam_size=1, **kw):
        if self.gate is not None:
            self.gate.wait(10)
        assert len(audios) * beam_size <= len(self.free_slots), "the batcher asked for more slots than there are"
        ids = [int(a[0]) for a in audios]
        self.calls.append((beam_size, ids))
        if beam_size > 1:
            self.last_beams = [[dict(tokens=[i, r], sum_logprob=-1.0 - r, avg_logprob=-0.5 - r) for r in range(beam_size)]
                               for i in ids]
        return [[i, 0] if beam_size > 1 else [i] for i in ids]


def _pcm(i):
    return np.full(160, i, dtype=np.int16)


def test_batcher_runs_beam_and_greedy_passes_as_separate_calls_and_never_fails_a_beam_pass_for_slots():
    gate = threading.Event()
    eng = FakeEngine(8, gate)
    b = st.AsrBatcher(eng, words=False)
    try:
        first = b.recognize_async(_pcm(1))          # occupies the scheduler until the gate opens
        while b.queue_depth():
            pass
        futs = {i: b.recognize_async(_pcm(i), beam=w) for i, w in ((2, 1), (3, 3), (4, 3), (5, 1), (6, 3), (7, 5))}
        gate.set()
        res = {i: f.result(timeout=20) for i, f in futs.items()}
        assert first.result(timeout=20).tokens == [1]
    finally:
        gate.set()
        b.close()
    assert eng.calls[0] == (1, [1])
    # round 2: the greedy passes in one call, the width-3 passes that fit 8 slots (two of three) in
    # another, the width-5 pass in a third; the third width-3 pass waits for the next round
    assert eng.calls[1:] == [(1, [2, 5]), (3, [3, 4]), (5, [7]), (3, [6])]
    for i, w in ((2, 1), (5, 1)):
        assert res[i].tokens == [i] and res[i].alternatives == []
    for i, w in ((3, 3), (4, 3), (6, 3), (7, 5)):
        assert res[i].tokens == [i, 0] and len(res[i].alternatives) == w - 1
        assert res[i].confidence == pytest.approx(math.exp(-0.5))
        assert res[i].alternatives[0] == dict(transcript=f"{i} 1", confidence=pytest.approx(math.exp(-1.5)))
    assert b.stats["passes"] == 7 and b.stats["batches"] == 5
    with pytest.raises(ValueError):
        st.AsrBatcher(FakeEngine(4), words=False).recognize_async(_pcm(1), beam=5)  # can never fit


def test_engine_recognizer_passes_the_width_and_builds_alternatives_on_the_prefix():
    eng = FakeEngine(8)
    rec = st.EngineRecognizer(eng, words=False)
    hyp = rec.recognize(_pcm(9), [41, 42], beam=3)
    assert eng.calls == [(3, [9])] and hyp.tokens == [41, 42, 9, 0]
    assert [a["transcript"] for a in hyp.alternatives] == ["41 42 9 1", "41 42 9 2"]
    assert rec.recognize(_pcm(9)).alternatives == [] and eng.calls[-1] == (1, [9])


def test_final_event_carries_the_alternatives_in_deepgrams_shape():
    base = st.results_event("go home", is_final=True, start=1.0, duration=2.0, model="m", confidence=0.7,
                            words=[{"word": "go", "start": 1.0, "end": 1.2, "confidence": 0.9}])
    ev = st.results_event("go home", is_final=True, start=1.0, duration=2.0, model="m", confidence=0.7,
                          words=[{"word": "go", "start": 1.0, "end": 1.2, "confidence": 0.9}],
                          alternatives=[dict(transcript="go hum", confidence=0.2), dict(transcript="no home", confidence=0.1)])
    alts = ev["channel"]["alternatives"]
    assert len(alts) == 3 and alts[0] == base["channel"]["alternatives"][0]
    assert alts[1:] == [{"transcript": "go hum", "confidence": 0.2, "words": []},
                        {"transcript": "no home", "confidence": 0.1, "words": []}]
    ev["channel"]["alternatives"] = alts[:1]
    assert ev == base


def test_session_asks_only_final_passes_for_beams_and_cuts_the_alternatives():
    asked = []

    class Rec:
        def recognize(self, pcm, prefix=(), **kw):
            asked.append(kw)
            h = st.Hypothesis([1, 2], "click it", confidence=0.4)
            if kw.get("beam", 1) > 1:
                h.alternatives = [dict(transcript=f"alt {r}", confidence=0.3 / r) for r in range(1, kw["beam"])]
            return h

    speech = (np.sin(np.arange(16000 * 2) * 0.2) * 9000).astype(np.int16).tobytes()
    for beam, n_alt, want in ((5, 3, 3), (5, 1, 1), (1, 1, 1)):
        asked.clear()
        s = st.StreamingAsrSession(Rec(), partial_every_s=0.5, spec_silence_s=0, words=False, language="en",
                                   beam=beam, alternatives=n_alt)
        events = s.push(speech) + s.flush()
        finals = [e for e in events if e.get("is_final")]
        assert len(finals) == 1 and [e for e in events if not e.get("is_final")]
        alts = finals[0]["channel"]["alternatives"]
        assert len(alts) == want and alts[0]["transcript"] == "click it"
        assert alts[0]["confidence"] == (0.4 if beam > 1 else 0.0)  # words off: exp(avg_logprob) of the best
        assert [a["transcript"] for a in alts[1:]] == [f"alt {r}" for r in range(1, want)]
        assert [k.get("beam", 1) for k in asked] == [1] * (len(asked) - 1) + [beam]
        assert all("beam" not in k for k in asked) if beam == 1 else True
    with pytest.raises(ValueError):
        st.StreamingAsrSession(Rec(), beam=3, alternatives=4)
    with pytest.raises(ValueError):
        st.StreamingAsrSession(Rec(), beam=9)


def test_both_settings_are_declared_and_bad_values_are_rejected(monkeypatch):
    from voice_enabled_browser_automation_amd.utils import env

    for name in ("VWA_ASR_BEAM", "VWA_ASR_ALTERNATIVES"):
        f = env.Settings.model_fields[name]
        assert f.default == 1 and f.annotation is int and f.description
        monkeypatch.delenv(name, raising=False)
    assert env.asr_beam_knobs() == (1, 1)
    monkeypatch.setenv("VWA_ASR_BEAM", "5")
    monkeypatch.setenv("VWA_ASR_ALTERNATIVES", "3")
    assert env.asr_beam_knobs() == (5, 3)
    s = env.settings()
    assert (s.VWA_ASR_BEAM, s.VWA_ASR_ALTERNATIVES) == (5, 3)
    for beam, alt in (("0", "1"), ("9", "1"), ("5", "6"), ("5", "0"), ("x", "1")):
        monkeypatch.setenv("VWA_ASR_BEAM", beam)
        monkeypatch.setenv("VWA_ASR_ALTERNATIVES", alt)
        with pytest.raises(ValueError):
            env.asr_beam_knobs()
        with pytest.raises(ValueError):
            env.settings()


def test_a_stream_final_through_the_engine_carries_three_ranked_alternatives(eng):
    rec = st.EngineRecognizer(eng, max_tokens=6, words=False)
    s = st.StreamingAsrSession(rec, partial_every_s=60.0, spec_silence_s=0, words=False, beam=5, alternatives=3)
    events = s.push(bc.tone(1.2, 330).tobytes()) + s.flush()
    finals = [e for e in events if e.get("is_final")]
    assert len(finals) == 1
    alts = finals[0]["channel"]["alternatives"]
    assert len(alts) == 3 and len(eng.last_beams[0]) == 5
    conf = [a["confidence"] for a in alts]
    assert conf == sorted(conf, reverse=True) and all(0.0 < c <= 1.0 for c in conf)
    assert conf == [pytest.approx(math.exp(h["avg_logprob"])) for h in eng.last_beams[0][:3]]
    assert all(a["words"] == [] for a in alts[1:]) and alts[0]["transcript"] == eng.tok.decode(eng.last_beams[0][0]["tokens"]).strip()
    assert len(eng.free_slots) == 8
