"""The optional launches around the sampler of a decode step (asr/engine.py), and their one order:

    keyterm boost (ops.boost_step) -> timestamp rules (ops.ts_rules_step) -> sampler -> score (ops.score_step)

The rules compare the biased logits, and the score is taken under the distribution that was sampled:
the order is part of the results, and `LogitSteps` is the only place that knows it.  Each feature is
a ``*Buffers`` (the engine's fixed device memory, built on the feature's first call -- captured loop
graphs address it) and a ``*Run`` (one decode_many call's use of it).  A run's ``step`` has two forms:
from the state the host staged (``first``: the apply form), afterwards in place by the tokens the
sampler left on the device (the advance form); ``restage`` stages again only when the rows changed."""
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from .. import ops


class _Run:
    """What the runs share: the rows staged (``utts``), their histories for the next launch
    (``hist``: built only where they are read -- to stage, or for the trace) and the trace."""

    def restage(self, utts: Sequence[int], hist_of: Callable[[], List]) -> bool:
        """Row i is now utterance utts[i]: staged again (``stage``) when those are not the rows the
        device's states are those of.  Returns whether it staged: the next ``step`` is then ``first``."""
        first = list(utts) != self.utts
        self.hist = hist_of() if first or self.trace is not None else ()
        if first:
            self.stage(utts, self.hist)
        return first

    def note(self, **kw) -> None:
        if self.trace:
            self.trace[-1].update(kw)


class BoostBuffers:
    """The engine's keyterm boosting memory (built on the first boosted call): one int32 device
    block of fixed size -- captured loop graphs address it -- and its pinned mirror,

        roots [R] | state0 [R] | edge_off [CS + 1] | state_root [CS] | edge_tok | edge_next | edge_bias [CE each]

    R = ops.BOOST_MAX_ROWS, CS / CE = ops.BOOST_CAP_STATES / BOOST_CAP_EDGES, plus two work state
    rows.  Every launch covers all CS states and CE edges: states past those in use carry root -1 and
    an empty list, so a stale state index becomes the row's root."""

    def __init__(self, dev):
        R, CS, CE = ops.BOOST_MAX_ROWS, ops.BOOST_CAP_STATES, ops.BOOST_CAP_EDGES
        n = 2 * R + (CS + 1) + CS + 3 * CE
        self.h = torch.zeros(n, dtype=torch.int32, pin_memory=dev.type == "cuda")
        self.d = torch.zeros(n, dtype=torch.int32, device=dev)
        self.head = 2 * R
        self.work = torch.zeros(2, R, dtype=torch.int32, device=dev)
        self.key = None  # the automata the device tables hold (their keys, in table order; None: none)
        self.bases: Dict[Tuple, int] = {}

        def views(t):
            o = 2 * R
            parts = []
            for m in (CS + 1, CS, CE, CE, CE):
                parts.append(t[o : o + m])
                o += m
            off, root, tok, nxt, bias = parts
            return t[:R], t[R : 2 * R], (off, tok, nxt, bias.view(torch.float32), root)

        self.h_roots, self.h_state0, self.h_tables = views(self.h)
        self.roots, self.state0, self.tables = views(self.d)


class BoostRun(_Run):
    """One decode_many call's keyterm boosting: which automaton each utterance has, where it sits in
    the engine's tables, and the launches (ops.boost_step) in the three forms the decode paths use.
    ``trace``: with AsrEngine.keep_boost_trace, one entry per launch."""

    def __init__(self, bufs: BoostBuffers, sets: Sequence, vocab: int, trace: Optional[List[Dict]]):
        from . import keyterms as kt

        self.b = bufs
        self.sets = list(sets)
        self.vocab = vocab
        self.trace = trace
        distinct: Dict[Tuple, object] = {}
        for ks in self.sets:
            if ks is not None:
                if not isinstance(ks, kt.KeytermSet):
                    raise TypeError(f"keyterms: {type(ks).__name__} is not a compiled KeytermSet (asr/keyterms.py)")
                distinct.setdefault(ks.key, ks)
        S = sum(ks.n_states for ks in distinct.values())
        E = sum(ks.n_edges for ks in distinct.values())
        if S > ops.BOOST_CAP_STATES or E > ops.BOOST_CAP_EDGES:
            raise RuntimeError(f"the call's {len(distinct)} keyterm automata hold {S} states / {E} edges: more than the "
                               f"engine's tables ({ops.BOOST_CAP_STATES} / {ops.BOOST_CAP_EDGES})")
        self.distinct = distinct
        self.base: List[int] = []
        self.cur = 0
        self.n = 0
        self.utts: List[int] = []
        self.dirty = False

    def load(self) -> None:
        """Writes the call's tables into the pinned mirror when the device holds others (the copy
        itself goes with the first ``stage``)."""
        from . import keyterms as kt

        keys = tuple(self.distinct)
        b = self.b
        if b.key != keys:
            bases, off, tok, nxt, bias, root = kt.concat(list(self.distinct.values()))
            h_off, h_tok, h_nxt, h_bias, h_root = b.h_tables
            S, E = len(root), len(tok)
            h_off.fill_(E)
            h_off[: S + 1] = torch.from_numpy(off)
            h_root.fill_(-1)
            h_root[:S] = torch.from_numpy(root)
            h_tok[:E] = torch.from_numpy(tok)
            h_nxt[:E] = torch.from_numpy(nxt)
            h_bias[:E] = torch.from_numpy(bias)
            # (the device holds these only once stage() has queued the copy: until then it holds no
            # set at all, so a call that fails in between leaves nothing a later call could trust)
            b.key = None
            b.bases = dict(zip(keys, bases))
            self.dirty = True
        self.keys = keys
        self.base = [-1 if ks is None else b.bases[ks.key] for ks in self.sets]

    def stage(self, utts: Sequence[int], hist: Sequence[Sequence[int]]) -> None:
        """Row i is utterance utts[i] with text history hist[i]: its root and the state its
        automaton is in after that history go to the device (with the tables, when they changed:
        one copy either way)."""
        b = self.b
        self.n = n = len(utts)
        assert 1 <= n <= ops.BOOST_MAX_ROWS
        roots = [self.base[j] for j in utts]
        b.h_roots.fill_(-1)
        b.h_roots[:n] = torch.tensor(roots, dtype=torch.int32)
        b.h_state0[:n] = torch.tensor([0 if r < 0 else r + self.sets[j].run(h) for r, j, h in zip(roots, utts, hist)],
                                      dtype=torch.int32)
        m = b.h.numel() if self.dirty else b.head
        b.d[:m].copy_(b.h[:m], non_blocking=True)
        if self.dirty:
            b.key = self.keys
        self.dirty = False
        self.utts = list(utts)

    def _launch(self, x: torch.Tensor, state_in, state_out, **kw) -> None:
        n = self.n
        assert x.shape[0] == n
        before = x.cpu().clone() if self.trace is not None else None
        ops.boost_step(x, self.vocab, self.b.tables, self.b.roots[:n], state_in, state_out, **kw)
        if self.trace is not None:
            roots = [self.base[j] for j in self.utts]
            self.trace.append(dict(utts=list(self.utts), history=[list(h) for h in self.hist], before=before,
                                   after=x.cpu().clone(), sets=[self.sets[j] for j in self.utts],
                                   state=[-1 if r < 0 else s - r for s, r in zip(state_out[:n].tolist(), roots)]))

    def step(self, x: torch.Tensor, tokens: Optional[torch.Tensor], first: bool) -> None:
        """``first`` (after ``stage``): the staged states' biases (no token to move on by);
        afterwards every row moves on by its own last token, in place."""
        if first:
            self.cur = 0
        w = self.b.work[self.cur]
        self._launch(x, self.b.state0 if first else w, w, tokens=None if first else tokens)

    def follow(self, x: torch.Tensor, tokens: torch.Tensor, parents: torch.Tensor, W: int) -> None:
        """Beams: row r continues the state of its group's beam parents[r], then moves on by tokens[r]."""
        self._launch(x, self.b.work[self.cur], self.b.work[1 - self.cur], tokens=tokens, parents=parents, W=W)
        self.cur = 1 - self.cur


TS_MAX_INITIAL = 50  # the first timestamp of a window may be at most 1.0 s (Whisper's max_initial_timestamp)


class TsBuffers:
    """The engine's timestamp rules memory (built on the first timestamp call): one int32 device
    block of fixed size -- captured loop graphs address it -- and its pinned mirror,

        enable [R] | state0 [R, 4]

    R = ops.TS_MAX_ROWS, plus the work states [R, 4] the launches step in place."""

    def __init__(self, dev):
        R = ops.TS_MAX_ROWS
        self.h = torch.zeros(5 * R, dtype=torch.int32, pin_memory=dev.type == "cuda")
        self.d = torch.zeros(5 * R, dtype=torch.int32, device=dev)
        self.work = torch.zeros(R, 4, dtype=torch.int32, device=dev)
        self.h_enable, self.h_state0 = self.h[:R], self.h[R:].view(R, 4)
        self.enable, self.state0 = self.d[:R], self.d[R:].view(R, 4)


def ts_state(hist: Sequence[int], ts_begin: int) -> List[int]:
    """The rules' state (n, last, prev, last_ts) after the sampled tokens ``hist`` (csrc/tsrules/tsrules.h)."""
    n = len(hist)
    return [min(n, 2), hist[-1] if n >= 1 else -1, hist[-2] if n >= 2 else -1,
            next((t - ts_begin for t in reversed(hist) if t >= ts_begin), -1)]


class TsRun(_Run):
    """One decode_many call's timestamp rules: which utterances decode with timestamps, and the
    launches (ops.ts_rules_step) in the two forms the greedy paths use.  ``trace``: with
    AsrEngine.keep_ts_trace, one entry per launch."""

    def __init__(self, bufs: TsBuffers, flags: Sequence[bool], cfg, trace: Optional[List[Dict]]):
        self.b = bufs
        self.flags = [bool(f) for f in flags]
        self.vocab, self.eot, self.ts_begin = cfg.vocab_size, cfg.eot, cfg.no_timestamps + 1
        self.trace = trace
        self.n = 0
        self.utts: List[int] = []

    def stage(self, utts: Sequence[int], hist: Sequence[Sequence[int]]) -> None:
        """Row i is utterance utts[i] with the sampled tokens hist[i]: whether the rules hold for it
        and the state they are in after that history go to the device (one copy)."""
        b = self.b
        self.n = n = len(utts)
        assert 1 <= n <= ops.TS_MAX_ROWS
        b.h_enable.zero_()
        b.h_enable[:n] = torch.tensor([int(self.flags[j]) for j in utts], dtype=torch.int32)
        b.h_state0[:n] = torch.tensor([ts_state(h, self.ts_begin) for h in hist], dtype=torch.int32)
        b.d.copy_(b.h, non_blocking=True)
        self.utts = list(utts)

    def _launch(self, x: torch.Tensor, mask: torch.Tensor, state_in, state_out, tokens=None) -> None:
        n = self.n
        assert x.shape[0] == n
        before = x.cpu().clone() if self.trace is not None else None
        ops.ts_rules_step(x, self.vocab, self.eot, self.ts_begin, TS_MAX_INITIAL, mask, self.b.enable[:n], state_in,
                          state_out, tokens=tokens)
        if self.trace is not None:
            self.trace.append(dict(utts=list(self.utts), history=[list(h) for h in self.hist], before=before,
                                   after=x.cpu().clone(), enable=[self.flags[j] for j in self.utts],
                                   mask=mask.cpu().clone(), state=state_out[:n].tolist()))

    def step(self, x: torch.Tensor, mask: torch.Tensor, tokens: Optional[torch.Tensor], first: bool) -> None:
        """``first`` (after ``stage``): the rules at the staged states (no token to move on by);
        afterwards every row moves on by its own last token, in place."""
        w = self.b.work
        self._launch(x, mask, self.b.state0 if first else w, w, tokens=None if first else tokens)


class ScoreBuffers:
    """The engine's transcript score memory (built on the first scored call): one int32 device block
    of fixed size -- captured loop graphs address it -- and its pinned mirror,

        enable [R] | temperature [R] (f32) | sum0 [R] (f32) | cnt0 [R, 2]

    R = ops.SCORE_MAX_ROWS, plus the work block the launches step in place and ONE device-to-host
    copy reads:  sum [R] (f32) | cnt [R, 2] | step_lp [R] (f32)."""

    def __init__(self, dev):
        R = ops.SCORE_MAX_ROWS
        f32 = torch.float32
        self.h = torch.zeros(5 * R, dtype=torch.int32, pin_memory=dev.type == "cuda")
        self.d = torch.zeros(5 * R, dtype=torch.int32, device=dev)
        self.work = torch.zeros(4 * R, dtype=torch.int32, device=dev)

        def views(t):
            return t[:R], t[R : 2 * R].view(f32), t[2 * R : 3 * R].view(f32), t[3 * R :].view(R, 2)

        self.h_enable, self.h_temp, self.h_sum0, self.h_cnt0 = views(self.h)
        self.enable, self.temp, self.sum0, self.cnt0 = views(self.d)
        w = self.work
        self.sum, self.cnt, self.step_lp = w[:R].view(f32), w[R : 3 * R].view(R, 2), w[3 * R :].view(f32)


class ScoreRun(_Run):
    """One decode_many call's transcript scores: every utterance's temperature, the sums the host
    holds (sum of log-probabilities, tokens counted, done), and the launches (ops.score_step) the
    greedy paths make after each sampler launch.  ``trace``: with AsrEngine.keep_score_trace, one
    entry per launch."""

    def __init__(self, bufs: ScoreBuffers, B: int, cfg, trace: Optional[List[Dict]]):
        self.b = bufs
        self.vocab, self.eot = cfg.vocab_size, cfg.eot
        self.trace = trace
        self.temps = [0.0] * B          # this attempt's temperature, per utterance
        self.sums = [0.0] * B           # the host's copy of every utterance's state
        self.cnts = [[0, 0] for _ in range(B)]
        self.attempt = 0
        self.n = 0
        self.utts: List[int] = []
        self.fresh = False

    def begin(self, utts: Sequence[int], temperatures: Sequence[float], attempt: int) -> None:
        """A new attempt for ``utts`` at those temperatures: their sums start again."""
        self.attempt = attempt
        for j, t in zip(utts, temperatures):
            self.temps[j], self.sums[j], self.cnts[j] = float(t), 0.0, [0, 0]
        self.utts = []

    def stage(self, utts: Sequence[int], hist=()) -> None:
        """Row i is utterance utts[i]: the sums the device holds come to the host (``read``), then its
        temperature and the state the host holds for it go to the device (one copy each way); the
        next launch reads the staged state."""
        self.read()
        b = self.b
        self.n = n = len(utts)
        assert 1 <= n <= ops.SCORE_MAX_ROWS
        b.h_enable.zero_()
        b.h_enable[:n] = 1
        b.h_temp[:n] = torch.tensor([self.temps[j] for j in utts], dtype=torch.float32)
        b.h_sum0[:n] = torch.tensor([self.sums[j] for j in utts], dtype=torch.float32)
        b.h_cnt0[:n] = torch.tensor([self.cnts[j] for j in utts], dtype=torch.int32)
        b.d.copy_(b.h, non_blocking=True)
        self.utts = list(utts)
        self.fresh = True

    def step(self, x: torch.Tensor, mask: torch.Tensor, tokens: torch.Tensor, first: bool) -> None:
        """After the sampler wrote ``tokens``: every row's sum moves on by its token's log-probability
        -- from the staged state (``first``), afterwards in place."""
        b = self.b
        n = self.n
        assert x.shape[0] == n
        self.fresh = False
        si, ci = (b.sum0, b.cnt0) if first else (b.sum, b.cnt)
        ops.score_step(x, self.vocab, self.eot, mask, b.enable[:n], tokens, si, b.sum, ci, b.cnt, step_lp=b.step_lp)
        if self.trace is not None:
            self.trace.append(dict(utts=list(self.utts), attempt=self.attempt, logits=x.cpu().clone(),
                                   mask=mask.cpu().clone(), tokens=tokens[:n].tolist(),
                                   temperature=[self.temps[j] for j in self.utts],
                                   step_lp=b.step_lp[:n].tolist()))

    def read(self) -> None:
        """The staged rows' states come to the host (one copy of the work block)."""
        if not self.utts or self.fresh:  # (nothing launched since the stage: the host's copy stands)
            self.utts = []
            return
        R = ops.SCORE_MAX_ROWS
        h = self.b.work.cpu()
        sums = h[:R].view(torch.float32).tolist()
        cnts = h[R : 3 * R].view(R, 2).tolist()
        for i, j in enumerate(self.utts):
            self.sums[j], self.cnts[j] = sums[i], cnts[i]
        self.utts = []


class LogitSteps:
    """One decode_many call's optional runs (None: off -- nothing of it is launched), stepped in the
    one order.  Per token step, over the live rows:

        first = restage(live, outs)            # (a single session: once, before its device loop)
        mask, temperature = before_sample(logits, tokens, allow_eot, first)
        <the sampler, with that mask and temperature>
        after_sample(logits, mask, tokens, first)

    ``first`` is an argument and never read from this object: a captured loop graph's warm-up and
    capture run the same steps and would flip such state.  ``mask_of(allow_eot, ts)``: the engine's
    fixed one-row masks (AsrEngine._mask); ``forced``: every utterance's text prefix."""

    def __init__(self, mask_of: Callable[..., torch.Tensor], forced: Sequence[Sequence[int]],
                 boost: Optional[BoostRun] = None, ts: Optional[TsRun] = None, score: Optional[ScoreRun] = None):
        self.mask_of, self.forced = mask_of, forced
        self.boost, self.ts, self.score = boost, ts, score
        # some run keeps a trace (host copies at every launch): the call is stepped from the host
        self.traced = any(r is not None and r.trace is not None for r in (boost, ts, score))
        # the tail of a loop graph's key (AsrEngine.loop_graphs): a graph holds exactly these launches
        self.graph_key = (boost is not None, ts is not None) + ((True,) if score is not None else ())
        self.masks: Optional[Tuple[torch.Tensor, ...]] = None  # the staged rows' masks, without / with EOT

    def restage(self, live: Sequence[int], outs: Sequence[List[int]]) -> bool:
        """Row i is utterance live[i], which has decoded outs[live[i]].  While the live set stands the
        runs' states move on by the sampler's tokens, on the device; when a row has dropped out and
        the rows have moved up they are staged again from what the host holds anyway (one copy per
        run; the scores are read first).  With rules every row brings its own mask (text rows the
        text mask), rebuilt only here; a single row's are the engine's own tensors, which a captured
        graph may address.  Returns whether it staged: a call's runs stage together, one answer serves."""
        hists = ((self.boost, lambda: [self.forced[j] + outs[j] for j in live]),  # (a term may straddle the prefix)
                 (self.ts, lambda: [outs[j] for j in live]), (self.score, tuple))
        first = {run.restage(live, hist_of) for run, hist_of in hists if run is not None}
        assert len(first) <= 1
        if self.ts is not None and True in first:
            rows = [[self.mask_of(e, self.ts.flags[j]) for j in live] for e in (False, True)]
            self.masks = tuple(r[0] if len(r) == 1 else torch.cat(r) for r in rows)
        return True in first

    def before_sample(self, logits: torch.Tensor, tokens: torch.Tensor, allow_eot: bool, first: bool):
        """The boost, then the rules on the biased logits: from the staged states (``first``), or
        moving on by ``tokens`` (the previous step's, on the device: no host wait).  Returns the
        sampler's (mask, temperatures or None)."""
        if self.boost is not None:
            self.boost.step(logits, tokens, first)
        mask = self.mask_of(allow_eot) if self.ts is None else self.masks[allow_eot]
        if self.ts is not None:
            self.ts.step(logits, mask, tokens, first)
        return mask, None if self.score is None else self.score.b.temp[: logits.shape[0]]

    def after_sample(self, logits: torch.Tensor, mask: torch.Tensor, tokens: torch.Tensor, first: bool) -> None:
        """The score, on the logits and the mask the sampler read and the ``tokens`` it wrote."""
        if self.score is not None:
            self.score.step(logits, mask, tokens, first)

    def note(self, **kw) -> None:
        """Adds to the step's trace entries (the tokens the host read)."""
        for run in (self.boost, self.ts):
            if run is not None:
                run.note(**kw)

    def finish(self) -> None:
        """A pass has ended: the scores come to the host (one copy), and a later pass stages anew."""
        if self.score is not None:
            self.score.read()
        for run in (self.boost, self.ts):
            if run is not None:
                run.utts = []
