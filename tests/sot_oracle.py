"""Float64 oracle and derived bounds for the start-of-transcript probe (csrc/sot, ops.sot_probe).
Independent of ops/reference.py: plain numpy written from the contract in csrc/sot/sot.h, computed
from the very f32 logits the op read.  Used by test_sot_cpu.py (against the CPU reference and the
CPU engine) and by test_sot_kernel_gpu.py / test_sot_engine_gpu.py (against the kernel)."""
import numpy as np
import torch

from align_oracle import gen, logprob_bound  # noqa: F401  (gen: re-export for the tests)
from kernel_oracle import SENTINEL  # noqa: F401  (re-export: outputs are pre-filled with it)

SENT_I = int(SENTINEL)
F32_DENORMAL = 2.0 ** -149


def allow_ids(allow: int, n_lang: int) -> np.ndarray:
    """Language indices (not token ids) whose bit is set, ascending."""
    return np.array([i for i in range(n_lang) if (allow >> i) & 1], dtype=np.int64)


def probe64(logits: torch.Tensor, vocab: int, lang0: int, n_lang: int, allow: int, no_speech_id: int):
    """(lang_probs f64 [R, n_lang], lang_tok int64 [R], lang_conf f64 [R], no_speech f64 [R]).

    no_speech: softmax over the ids < vocab at no_speech_id.  lang_probs: softmax over the allowed
    language ids with their own maximum subtracted, exactly 0 elsewhere (NaN on the allowed ids when
    every one of them is -inf).  lang_tok: the lowest allowed id whose raw logit equals the maximum
    over the allowed ids (the lowest allowed id when none does).  lang_conf: its probability."""
    x = logits.double().numpy()[:, :vocab]
    R = x.shape[0]
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    no_speech = e[:, no_speech_id] / e.sum(axis=1)
    ids = allow_ids(allow, n_lang)
    assert len(ids), "empty language set"
    sub = x[:, lang0 + ids]
    ml = sub.max(axis=1, keepdims=True)
    first = np.argmax(sub == ml, axis=1)  # (first True; 0 = the lowest allowed id when there is none)
    tok = lang0 + ids[first]
    probs = np.zeros((R, n_lang))
    with np.errstate(invalid="ignore"):
        es = np.exp(sub - ml)
        probs[:, ids] = es / es.sum(axis=1, keepdims=True)
    conf = probs[np.arange(R), tok - lang0]
    return probs, tok, conf, no_speech


def prob_bound(p: np.ndarray) -> np.ndarray:
    """|got - p| <= p (2^-14 + 2^-22 |ln p|) + one f32 denormal.

    align_oracle.logprob_bound's argument: the f32 sum of <= 51866 terms split over 256 lanes errs by
    about 2^-16 relative, expf and the logit difference add a few 2^-24 relative each plus 2^-24
    |x - max| = 2^-24 |ln p| (up to the log of the sum) absolute in the exponent; 2^-14 + 2^-22
    |ln p| bounds the error of ln(got), hence -- being far below 1 -- the relative error of got.
    A probability below the f32 range comes back as 0 or a denormal: one denormal of slack."""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(p > 0, logprob_bound(np.log(p)), 0.0)
    return p * rel + F32_DENORMAL


ROW_SUM_BOUND = 2.0 ** -15  # each row's language probabilities sum to 1 (test_attn_probs' bound for 1500 terms)


def check_probe(got, ref, what: str = "") -> float:
    """got: (lang_probs [R, n_lang], lang_tok, lang_conf, no_speech) as host tensors / arrays of the
    written region; ref: probe64's tuple.  Asserts exact ids, exact zeros, the bounds and the row
    sums; returns the largest error / bound."""
    gp, gt, gc, gn = (np.asarray(t.double().numpy() if isinstance(t, torch.Tensor) else t) for t in got)
    rp, rt, rc, rn = ref
    assert (gt.astype(np.int64) == rt).all(), f"{what}: lang_tok {gt[gt != rt][:5]} != {rt[gt != rt][:5]}"
    assert (gp[rp == 0] == 0).all(), f"{what}: a probability that must be exactly 0 is not"
    worst = 0.0
    for name, g, r in (("lang_probs", gp, rp), ("lang_conf", gc, rc), ("no_speech", gn, rn)):
        assert np.isfinite(g).all(), f"{what}: {name} not finite"
        ratio = (np.abs(g - r) / prob_bound(r)).max()
        print(f"MEASURED {what} {name} err/bound {ratio:.4g}")
        assert ratio <= 1.0, f"{what}: {name} err/bound {ratio}"
        worst = max(worst, ratio)
    dev = np.abs(gp.sum(axis=1) - 1).max()
    print(f"MEASURED {what} row sum deviation {dev:.4g}")
    assert dev <= ROW_SUM_BOUND, f"{what}: language probabilities sum to 1 +- {dev}"
    return worst
