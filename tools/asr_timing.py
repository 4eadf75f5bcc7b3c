"""Whisper transcription time split (encoder / decoder) with and without the chained decoder
launches (models/whisper.py, skinny_stream.hip chain_kernel SEQ 1/2), fixed 40-token work on the
bench's synthetic 10 s utterance.  One JSON line per mode.
python tools/asr_timing.py [--asr whisper-large-v3] [--reps 10]
python tools/asr_timing.py --words [--asr whisper-large-v3]   # the final pass without / with word timestamps
python tools/asr_timing.py --language auto [--asr whisper-large-v3]   # the pass with a fixed / a detected language
python tools/asr_timing.py --beam 5 [--asr whisper-large-v3]   # beam search against W greedy rows, per token step
python tools/asr_timing.py --keyterms 50 [--batch-rows 8]   # the boosted step against plain rows
python tools/asr_timing.py --timestamps [--batch-rows 8]   # the timestamp rules step against plain rows, and the boundary pass
python tools/asr_timing.py --fallback [--batch-rows 8]   # the scored step against plain rows, and a forced two-attempt pass

decode_us_per_token = host time from the encoder's launch to the last token / tokens (includes the
encoder and cross K/V projections still running after their launch); decode_gpu_us_per_token = the
decoder's stream time (4-token prompt step + the token loop, CUDA events) / tokens."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import synth_speech  # noqa: E402
from voice_enabled_browser_automation_amd import ops  # noqa: E402
from voice_enabled_browser_automation_amd.asr.engine import AsrEngine  # noqa: E402
from voice_enabled_browser_automation_amd.models.config import get_config  # noqa: E402
from voice_enabled_browser_automation_amd.models.whisper import WhisperModel  # noqa: E402
from voice_enabled_browser_automation_amd.tokenizer import load_tokenizer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asr", default="whisper-tiny")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tokens", type=int, default=40)
    ap.add_argument("--batch", default="", help="also time transcribe_many over B utterances (comma list)")
    ap.add_argument("--modes", default="0,p",
                    help="decoder forms to time: 0 per-kernel, 1 chained launches (VWA_CHAIN_ASR), p the persistent "
                         "one-launch decoder (VWA_ASR_PERSIST, whisper-large)")
    ap.add_argument("--words", action="store_true",
                    help="time the final pass without and with word timestamps (the alignment pass after the decode)")
    ap.add_argument("--language", default=None,
                    help="time the same pass with the default fixed language and with this one (auto: detected from "
                         "the start-of-transcript logits, one more one-row decoder step and the probe)")
    ap.add_argument("--beam", type=int, default=0,
                    help="time beam search of this width: per token step the select, the K/V gather and the whole "
                         "step, beside the same number of sessions decoded greedily as W independent rows")
    ap.add_argument("--keyterms", type=int, default=0,
                    help="time keyterm boosting with this many terms: the boosting launch alone (1 row and "
                         "--batch-rows rows), and whole decode steps plain against boosted, for one session (the "
                         "device loop; plain takes the persistent decoder where the model has one) and for "
                         "--batch-rows batched sessions")
    ap.add_argument("--timestamps", action="store_true",
                    help="time timestamp decoding: the rules launch alone (1 row and --batch-rows rows, beside the "
                         "boost launch of the same run), whole decode steps plain against timestamps for one session "
                         "(the device loop; plain takes the persistent decoder where the model has one) and for "
                         "--batch-rows batched sessions, and the boundary pass of a full 30 s window")
    ap.add_argument("--fallback", action="store_true",
                    help="time the quality gate: the score launch alone (1 row and --batch-rows rows), whole decode "
                         "steps plain against scored for one session (the device loop; plain takes the persistent "
                         "decoder where the model has one) and for --batch-rows batched sessions, and a final pass "
                         "forced into two attempts against the same pass with one")
    ap.add_argument("--batch-rows", type=int, default=8)
    ap.add_argument("--small-max-m", type=int, default=None,
                    help="A/B: rows up to which small weights take the one-tile kernel (16: the tiled GEMM above 16)")
    a = ap.parse_args()
    ops.ext()
    if a.small_max_m is not None:
        ops.SMALL_MAX_M = a.small_max_m
    m = WhisperModel(get_config(a.asr), device="cuda", seed=0)
    if a.batch:  # concurrent sessions' batched pass (bench.py --concurrent: one per round)
        sizes = [int(x) for x in a.batch.split(",")]
        eng = AsrEngine(m, load_tokenizer("whisper"), max_sessions=max(sizes))
        for B in sizes:
            audios = [eng.pcm_to_audio(synth_speech(10.0, seed=100 + j)) for j in range(B)]
            for _ in range(2):
                eng.transcribe_many(audios, exact_tokens=a.tokens)
            ts, enc, dec = [], [], []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.transcribe_many(audios, exact_tokens=a.tokens)
                ts.append((time.perf_counter() - t0) * 1e3)
                s = getattr(eng, "last_stats", {}) or {}
                enc.append(s.get("encode_ms", 0.0))
                dec.append(s.get("decode_ms", 0.0))
            print(json.dumps(dict(tool="asr_timing", asr=a.asr, batch=B, tokens=a.tokens,
                                  total_ms=round(statistics.median(ts), 2), encode_ms=round(statistics.median(enc), 2),
                                  decode_ms=round(statistics.median(dec), 2))), flush=True)
        return
    if a.words:  # the final pass with and without the word-alignment pass (decode_many(words=True))
        eng = AsrEngine(m, load_tokenizer("whisper"), max_sessions=2)
        audio = eng.pcm_to_audio(synth_speech(10.0, seed=100))
        toks = {}
        for on in (False, True, False, True):  # interleaved: off / on / off / on, reps each
            for _ in range(2):
                eng.decode_many([audio], exact_tokens=a.tokens, words=on)
            tot, al = [], []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                toks.setdefault(on, eng.decode_many([audio], exact_tokens=a.tokens, words=on)[0])
                tot.append((time.perf_counter() - t0) * 1e3)
                al.append(eng.last_stats.get("align_ms", 0.0))
            q = statistics.quantiles(tot, n=4) if len(tot) >= 4 else [min(tot), statistics.median(tot), max(tot)]
            print(json.dumps(dict(tool="asr_timing", asr=a.asr, words=on, tokens=a.tokens, reps=a.reps,
                                  total_ms=round(statistics.median(tot), 3), total_ms_min=round(min(tot), 3),
                                  total_ms_max=round(max(tot), 3), total_ms_q1=round(q[0], 3),
                                  total_ms_q3=round(q[2], 3), align_ms=round(statistics.median(al), 3),
                                  align_heads=m.align_layers()[1])), flush=True)
        print(json.dumps(dict(tool="asr_timing", asr=a.asr, same_tokens=toks[False] == toks[True])), flush=True)
        return
    if a.beam:  # one utterance with W beams against W sessions decoded greedily (decode_many(beam_size=))
        W = a.beam
        eng = AsrEngine(m, load_tokenizer("whisper"), max_sessions=W)
        audio = eng.pcm_to_audio(synth_speech(10.0, seed=100))
        P = len(eng.prompt)

        def timed(fn):
            fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
            for e0, e1 in ev:
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev) * 1e3

        # the two kernels alone, at the context of the pass's last step (event-timed, one call each)
        b = eng.runner.b
        i32 = dict(dtype=torch.int32, device="cuda")
        cum = -torch.rand(W, device="cuda")
        logits = torch.randn(W, m.vocab_padded, device="cuda") * 3
        select_us = timed(lambda: ops.beam_select(logits, cum, eng.mask_text, m.cfg.vocab_size, W))
        slots = torch.arange(W, **i32)[None].contiguous()
        parents = ((torch.arange(W, **i32) + 1) % W)[None].contiguous()  # every beam moves
        n_ctx = torch.tensor([P + a.tokens], **i32)
        gather_us = timed(lambda: ops.kv_beam_gather(b.k_cache, b.v_cache, b.block_table, slots, parents, n_ctx,
                                                     max_ctx=P + a.tokens))
        res = {}
        for kind in ("greedy_rows", "beam", "greedy_rows", "beam"):  # interleaved, reps each
            kw = dict(beam_size=W) if kind == "beam" else {}
            batch = [audio] if kind == "beam" else [audio] * W
            for _ in range(2):
                eng.decode_many(batch, exact_tokens=a.tokens, **kw)
            dgpu, bms = [], []
            for _ in range(a.reps):
                eng.decode_many(batch, exact_tokens=a.tokens, **kw)
                dgpu.append(eng.last_stats.get("decode_gpu_ms") or 0.0)
                bms.append(eng.last_stats.get("beam_ms") or 0.0)
            res[kind] = (statistics.median(dgpu) * 1e3 / a.tokens, statistics.median(bms) * 1e3 / a.tokens)
        g, bm = res["greedy_rows"][0], res["beam"]
        print(json.dumps(dict(tool="asr_timing", asr=a.asr, beam=W, tokens=a.tokens, reps=a.reps,
                              context=P + a.tokens, select_us=round(select_us, 1), gather_us=round(gather_us, 1),
                              beam_step_us=round(bm[0], 1), beam_ops_and_copies_us_per_step=round(bm[1], 1),
                              greedy_rows_step_us=round(g, 1),
                              kernels_share_of_greedy_step=round((select_us + gather_us) / g, 4),
                              step_overhead_share=round(bm[0] / g - 1.0, 4))), flush=True)
        return
    if a.keyterms:  # decode_many(keyterms=): the boosting launch, and boosted steps against plain ones
        from voice_enabled_browser_automation_amd.asr import keyterms as kt

        R = a.batch_rows
        eng = AsrEngine(m, load_tokenizer("whisper"), max_sessions=R)
        audio = eng.pcm_to_audio(synth_speech(10.0, seed=100))
        words = ["Grafana", "Browserbase", "pull request", "dashboard", "Kubernetes", "open settings", "checkout",
                 "wireless earbuds", "sign in", "GitHub"]
        ks = eng.compile_keyterms([f"{words[i % len(words)]} {i // len(words)}".strip() if i >= len(words)
                                   else words[i] for i in range(a.keyterms)])

        def timed(fn):
            fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
            for e0, e1 in ev:
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev) * 1e3

        # the launch alone, on tables of its own (the set's, as kt.concat lays them out): every row at
        # the root, moving by the first token of a term, in place
        _, *tabs = kt.concat([ks])
        tabs = tuple(torch.from_numpy(t).cuda() for t in tabs)
        i32 = dict(dtype=torch.int32, device="cuda")
        roots, state = torch.zeros(R, **i32), torch.zeros(R, **i32)
        tok = torch.full((R,), ks.key[0][0][0], **i32)
        launch = {}
        for rows in (1, R):
            x = torch.randn(rows, m.vocab_padded, device="cuda")
            launch[rows] = timed(lambda: ops.boost_step(x, m.cfg.vocab_size, tabs, roots[:rows], state,
                                                        state, tokens=tok[:rows]))
        res = {}
        for kind in ("plain_1", "boost_1", "plain_rows", "boost_rows") * 2:  # interleaved, reps each
            n = 1 if kind.endswith("_1") else R
            kw = dict(keyterms=[ks] * n) if kind.startswith("boost") else {}
            for _ in range(2):
                eng.decode_many([audio] * n, exact_tokens=a.tokens, **kw)
            dgpu = []
            for _ in range(a.reps):
                eng.decode_many([audio] * n, exact_tokens=a.tokens, **kw)
                dgpu.append(eng.last_stats.get("decode_gpu_ms") or 0.0)
            res.setdefault(kind, []).append(statistics.median(dgpu) * 1e3 / a.tokens)
        step = {k: min(v) for k, v in res.items()}
        print(json.dumps(dict(tool="asr_timing", asr=a.asr, keyterms=a.keyterms, states=ks.n_states, edges=ks.n_edges,
                              tokens=a.tokens, reps=a.reps, rows=R, boost_launch_us_1_row=round(launch[1], 1),
                              boost_launch_us_rows=round(launch[R], 1),
                              plain_step_us_1=round(step["plain_1"], 1), boost_step_us_1=round(step["boost_1"], 1),
                              plain_step_us_rows=round(step["plain_rows"], 1),
                              boost_step_us_rows=round(step["boost_rows"], 1),
                              persistent_used_by_plain=bool(getattr(m, "_wdec", None)),
                              step_overhead_share_1=round(step["boost_1"] / step["plain_1"] - 1.0, 4),
                              step_overhead_share_rows=round(step["boost_rows"] / step["plain_rows"] - 1.0, 4))),
              flush=True)
        return
    if a.timestamps:  # decode_many(timestamps=): the rules launch, and timestamp steps against plain ones
        from voice_enabled_browser_automation_amd.asr import keyterms as kt
        from voice_enabled_browser_automation_amd.asr.engine import TS_MAX_INITIAL

        R = a.batch_rows
        cfg = m.cfg
        eng = AsrEngine(m, load_tokenizer("whisper"), max_sessions=R)
        audio = eng.pcm_to_audio(synth_speech(10.0, seed=100))
        window = eng.pcm_to_audio(synth_speech(30.0, seed=101))

        def timed(fn):
            fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
            for e0, e1 in ev:
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev) * 1e3

        # the launch alone, in the two states that cost most and least: text after text (the text
        # maximum and the timestamps' log-sum-exp are both read, little is written) and text after a
        # pair of timestamps (1501 columns written, the text read); beside it the boost launch of the
        # same run (ten terms), which reads a few table entries and writes a few logits
        eng._ts_setup()
        i32 = dict(dtype=torch.int32, device="cuda")
        tsb = cfg.no_timestamps + 1
        enable = torch.ones(R, **i32)
        ks = eng.compile_keyterms(["Grafana", "Browserbase", "pull request", "dashboard", "Kubernetes", "open settings",
                                   "checkout", "wireless earbuds", "sign in", "GitHub"])
        _, *tabs = kt.concat([ks])
        tabs = tuple(torch.from_numpy(t).cuda() for t in tabs)
        roots, bstate = torch.zeros(R, **i32), torch.zeros(R, **i32)
        btok = torch.full((R,), ks.key[0][0][0], **i32)
        launch = {}
        for rows in (1, R):
            x = torch.randn(rows, m.vocab_padded, device="cuda") * 3
            for name, st in (("text", [2, 5, 6, 10]), ("pair", [2, tsb + 10, tsb + 10, 10])):
                state = torch.tensor([st] * rows, **i32)
                out = torch.empty_like(state)
                launch[name, rows] = timed(lambda: ops.ts_rules_step(x, cfg.vocab_size, cfg.eot, tsb, TS_MAX_INITIAL,
                                                                     eng.mask_ts_eot, enable[:rows], state, out))
            launch["boost", rows] = timed(lambda: ops.boost_step(x, cfg.vocab_size, tabs, roots[:rows], bstate, bstate,
                                                                 tokens=btok[:rows]))
        res = {}
        for kind in ("plain_1", "ts_1", "plain_rows", "ts_rows") * 2:  # interleaved, reps each
            n = 1 if kind.endswith("_1") else R
            kw = dict(timestamps=[True] * n) if kind.startswith("ts") else {}
            for _ in range(2):
                eng.decode_many([audio] * n, exact_tokens=a.tokens, **kw)
            dgpu = []
            for _ in range(a.reps):
                eng.decode_many([audio] * n, exact_tokens=a.tokens, **kw)
                dgpu.append(eng.last_stats.get("decode_gpu_ms") or 0.0)
            res.setdefault(kind, []).append(statistics.median(dgpu) * 1e3 / a.tokens)
        step = {k: min(v) for k, v in res.items()}
        # the boundary pass of a full window: 30 s, half the decoder's context in tokens, one session
        n_b = cfg.n_text_ctx // 2
        for _ in range(2):
            eng.decode_many([window], exact_tokens=n_b, timestamps=[True])
        tot = []
        for _ in range(max(3, a.reps // 2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.decode_many([window], exact_tokens=n_b, timestamps=[True])
            tot.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps(dict(tool="asr_timing", asr=a.asr, timestamps=True, tokens=a.tokens, reps=a.reps, rows=R,
                              rules_launch_us_text_1_row=round(launch["text", 1], 1),
                              rules_launch_us_pair_1_row=round(launch["pair", 1], 1),
                              rules_launch_us_text_rows=round(launch["text", R], 1),
                              rules_launch_us_pair_rows=round(launch["pair", R], 1),
                              boost_launch_us_1_row=round(launch["boost", 1], 1),
                              boost_launch_us_rows=round(launch["boost", R], 1),
                              plain_step_us_1=round(step["plain_1"], 1), ts_step_us_1=round(step["ts_1"], 1),
                              plain_step_us_rows=round(step["plain_rows"], 1), ts_step_us_rows=round(step["ts_rows"], 1),
                              persistent_used_by_plain=bool(getattr(m, "_wdec", None)),
                              ts_call_takes_persistent=eng._persistent_loop_ok(None, object()),
                              step_overhead_share_1=round(step["ts_1"] / step["plain_1"] - 1.0, 4),
                              step_overhead_share_rows=round(step["ts_rows"] / step["plain_rows"] - 1.0, 4),
                              boundary_pass_tokens=n_b, boundary_pass_ms=round(statistics.median(tot), 2),
                              boundary_pass_ms_min=round(min(tot), 2), boundary_pass_ms_max=round(max(tot), 2))),
              flush=True)
        return
    if a.fallback:  # decode_many(score= / fallback=): the score launch, scored steps against plain ones, a retry
        from voice_enabled_browser_automation_amd.asr.fallback import FallbackPolicy

        R = a.batch_rows
        cfg = m.cfg
        eng = AsrEngine(m, load_tokenizer("whisper"), max_sessions=R)
        audio = eng.pcm_to_audio(synth_speech(10.0, seed=100))

        def timed(fn):
            fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
            for e0, e1 in ev:
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev) * 1e3

        i32 = dict(dtype=torch.int32, device="cuda")
        enable = torch.ones(R, **i32)
        tok = torch.full((R,), 1000, **i32)
        launch = {}
        for rows in (1, R):
            x = torch.randn(rows, m.vocab_padded, device="cuda") * 3
            sm, cn = torch.zeros(rows, device="cuda"), torch.zeros(rows, 2, **i32)
            lp = torch.zeros(rows, device="cuda")
            s2, c2 = torch.zeros_like(sm), torch.zeros_like(cn)
            launch[rows] = timed(lambda: ops.score_step(x, cfg.vocab_size, cfg.eot, eng.mask_text_eot, enable[:rows],
                                                        tok[:rows], sm, s2, cn, c2, step_lp=lp))
        res = {}
        for kind in ("plain_1", "score_1", "plain_rows", "score_rows") * 2:  # interleaved, reps each
            n = 1 if kind.endswith("_1") else R
            kw = dict(score=True) if kind.startswith("score") else {}
            for _ in range(2):
                eng.decode_many([audio] * n, exact_tokens=a.tokens, **kw)
            dgpu = []
            for _ in range(a.reps):
                eng.decode_many([audio] * n, exact_tokens=a.tokens, **kw)
                dgpu.append(eng.last_stats.get("decode_gpu_ms") or 0.0)
            res.setdefault(kind, []).append(statistics.median(dgpu) * 1e3 / a.tokens)
        step = {k: min(v) for k, v in res.items()}
        # one final pass (one session) with one attempt -- a threshold every decode passes -- and forced into
        # two: a threshold none passes and a schedule of two temperatures; the encoder runs once in both
        one = FallbackPolicy(temperatures=(0.0, 0.2), logprob_threshold=None, compression_ratio_threshold=None)
        two = FallbackPolicy(temperatures=(0.0, 0.2), logprob_threshold=0.0, compression_ratio_threshold=None)
        tot = {"one": [], "two": []}
        dec = {"one": [], "two": []}
        for name, pol in (("one", one), ("two", two)) * 2:
            for _ in range(2):
                eng.decode_many([audio], exact_tokens=a.tokens, fallback=pol)
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.decode_many([audio], exact_tokens=a.tokens, fallback=pol)
                tot[name].append((time.perf_counter() - t0) * 1e3)
                dec[name].append(eng.last_stats.get("decode_gpu_ms") or 0.0)
            assert eng.last_scores[0]["attempts"] == (1 if name == "one" else 2)
        print(json.dumps(dict(tool="asr_timing", asr=a.asr, fallback=True, tokens=a.tokens, reps=a.reps, rows=R,
                              score_launch_us_1_row=round(launch[1], 1), score_launch_us_rows=round(launch[R], 1),
                              plain_step_us_1=round(step["plain_1"], 1), score_step_us_1=round(step["score_1"], 1),
                              plain_step_us_rows=round(step["plain_rows"], 1),
                              score_step_us_rows=round(step["score_rows"], 1),
                              persistent_used_by_plain=bool(getattr(m, "_wdec", None)),
                              scored_call_takes_persistent=eng._persistent_loop_ok(None, None, object()),
                              step_overhead_share_1=round(step["score_1"] / step["plain_1"] - 1.0, 4),
                              step_overhead_share_rows=round(step["score_rows"] / step["plain_rows"] - 1.0, 4),
                              one_attempt_pass_ms=round(statistics.median(tot["one"]), 2),
                              two_attempt_pass_ms=round(statistics.median(tot["two"]), 2),
                              one_attempt_decode_gpu_ms=round(statistics.median(dec["one"]), 2),
                              two_attempt_decode_gpu_ms=round(statistics.median(dec["two"]), 2))),
              flush=True)
        return
    if a.language:  # the pass with the fixed default language and with --language (decode_many(languages=))
        eng = AsrEngine(m, load_tokenizer("whisper"), max_sessions=2)
        audio = eng.pcm_to_audio(synth_speech(10.0, seed=100))
        for lang in (None, a.language, None, a.language):  # interleaved, reps each
            kw = {} if lang is None else {"languages": [lang]}
            for _ in range(2):
                eng.decode_many([audio], exact_tokens=a.tokens, **kw)
            tot, dgpu = [], []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.decode_many([audio], exact_tokens=a.tokens, **kw)
                tot.append((time.perf_counter() - t0) * 1e3)
                dgpu.append(eng.last_stats.get("decode_gpu_ms") or 0.0)
            q = statistics.quantiles(tot, n=4) if len(tot) >= 4 else [min(tot), statistics.median(tot), max(tot)]
            sot = eng.last_sot[0]
            print(json.dumps(dict(tool="asr_timing", asr=a.asr, language=lang or eng.language, tokens=a.tokens,
                                  reps=a.reps, total_ms=round(statistics.median(tot), 3),
                                  total_ms_min=round(min(tot), 3), total_ms_max=round(max(tot), 3),
                                  total_ms_q1=round(q[0], 3), total_ms_q3=round(q[2], 3),
                                  decode_gpu_ms=round(statistics.median(dgpu), 3), used_language=sot["language"],
                                  no_speech_prob=sot["no_speech_prob"])), flush=True)
        return
    audio = None
    texts = {}
    for chain in a.modes.split(","):
        os.environ["VWA_CHAIN_ASR"] = "1" if chain == "1" else "0"
        os.environ["VWA_ASR_PERSIST"] = "1" if chain == "p" else "0"
        m.reset_chains()
        eng = AsrEngine(m, load_tokenizer("whisper"), max_sessions=2)
        audio = eng.pcm_to_audio(synth_speech(10.0, seed=100))
        for _ in range(2):
            eng.transcribe(audio, exact_tokens=a.tokens)
        enc, dec, tot, dgpu = [], [], [], []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            texts[chain] = eng.transcribe(audio, exact_tokens=a.tokens)
            s = eng.last_stats
            enc.append(s["encode_ms"])
            dec.append(s["decode_ms"])
            tot.append(s["total_ms"])
            if s.get("decode_gpu_ms") is not None:
                dgpu.append(s["decode_gpu_ms"])
        print(json.dumps(dict(tool="asr_timing", asr=a.asr, chain=chain == "1", persistent=chain == "p",
                              persistent_used=bool(getattr(m, "_wdec", None)), tokens=a.tokens,
                              encode_ms=round(statistics.median(enc), 2), decode_ms=round(statistics.median(dec), 2),
                              total_ms=round(statistics.median(tot), 2),
                              decode_us_per_token=round(1e3 * statistics.median(dec) / a.tokens, 1),
                              # the decoder's own stream time (prompt step + token loop), from events:
                              # decode_ms starts when the encoder is LAUNCHED, so it also holds the
                              # encoder / cross K/V tail still running then
                              decode_gpu_us_per_token=round(1e3 * statistics.median(dgpu) / a.tokens, 1) if dgpu else None,
                              chained=bool(m.chain_descs()))), flush=True)
    if len(texts) >= 2:
        print(json.dumps(dict(tool="asr_timing", same_text=len(set(texts.values())) == 1,
                              modes=list(texts), error=bool(m.chain_error()))), flush=True)


if __name__ == "__main__":
    main()
