"""The start-of-transcript probe kernel (csrc/sot, _vwa_sot.so) against the float64 oracle computed
from the very f32 logits the kernel read (tests/sot_oracle.py), with derived bounds; outputs are
pre-filled with kernel_oracle.SENTINEL so regions the kernel must not write can be checked.  Each
test prints what it measures (run with -s)."""
import numpy as np
import pytest
import torch

import sot_oracle as so
import voice_enabled_browser_automation_amd.ops as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, I32 = torch.float32, torch.int32
SENT, SENT_I = so.SENTINEL, so.SENT_I
PAD = 1e30  # in the columns at or beyond vocab: a kernel that reads them fails loudly

# (vocab, lang0, n_lang, no_speech_id)
LAYOUTS = {
    "v51865": (51865, 50259, 99, 50362),
    "v51866": (51866, 50259, 100, 50363),
    "v200": (200, 60, 65, 190),     # a vocabulary smaller than the workgroup; a half-filled second lane group
    "v300": (300, 100, 128, 5),
    "v40": (40, 7, 1, 0),
}
R_MAX = 64


@pytest.fixture(scope="module", autouse=True)
def _native():
    ops.sot_ext()  # fail loudly if the library is missing


def padded(x: torch.Tensor, vocab: int) -> torch.Tensor:
    """x [R, vocab] in a buffer whose row length is vocab padded to 16 (at least one padding column)."""
    ld = (vocab + 16) // 16 * 16
    buf = torch.full((x.shape[0], ld), PAD, dtype=F32)
    buf[:, :vocab] = x
    return buf


_LOGITS = {}


def logits_of(name: str):
    """One [64, ld] logits buffer per layout (host, device), shared by every case."""
    if name not in _LOGITS:
        vocab = LAYOUTS[name][0]
        x = padded(torch.randn(R_MAX, vocab, generator=so.gen(21, vocab)) * 3.0, vocab)
        _LOGITS[name] = (x, x.to(DEV))
    return _LOGITS[name]


def allow_of(kind: str, n_lang: int, key: int) -> int:
    if kind == "all":
        return (1 << n_lang) - 1
    rng = np.random.default_rng(1000 + key)
    if kind == "one":
        return 1 << int(rng.integers(n_lang))
    a = 0
    while a == 0:
        a = sum(1 << i for i in range(n_lang) if rng.random() < 0.5)
    return a


_REF = {}


def ref_of(name: str, kind: str):
    """The oracle of all 64 rows of a (layout, allow) pair, computed once (rows are independent)."""
    if (name, kind) not in _REF:
        vocab, lang0, n_lang, ns = LAYOUTS[name]
        allow = allow_of(kind, n_lang, vocab)
        _REF[(name, kind)] = (allow, so.probe64(logits_of(name)[0], vocab, lang0, n_lang, allow, ns))
    return _REF[(name, kind)]


def run(xd, rows, layout, allow, *, ldp_extra=3, row_extra=2, dst=None, n_dst=70):
    """The op on xd[:rows] into sentinel-filled outputs.  Returns host copies:
    (lang_probs [rows + row_extra, n_lang + ldp_extra], lang_tok, lang_conf, no_speech, tok_dst)."""
    vocab, lang0, n_lang, ns = layout
    R = rows + row_extra
    probs = torch.full((R, n_lang + ldp_extra), SENT, dtype=F32, device=DEV)
    tok = torch.full((R,), SENT_I, dtype=I32, device=DEV)
    conf = torch.full((R,), SENT, dtype=F32, device=DEV)
    nsp = torch.full((R,), SENT, dtype=F32, device=DEV)
    tok_dst = dst_rows = None
    if dst is not None:
        tok_dst = torch.full((n_dst,), SENT_I, dtype=I32, device=DEV)
        dst_rows = torch.tensor(dst, dtype=I32, device=DEV)
    ops.sot_probe(xd[:rows], vocab, lang0, n_lang, ns, allow, lang_probs=probs[:rows], lang_tok=tok[:rows],
                  lang_conf=conf[:rows], no_speech=nsp[:rows], tok_dst=tok_dst, dst_rows=dst_rows)
    return probs.cpu(), tok.cpu(), conf.cpu(), nsp.cpu(), None if tok_dst is None else tok_dst.cpu()


def check_untouched(out, rows, n_lang):
    probs, tok, conf, nsp, _ = out
    assert (probs[:rows, n_lang:] == SENT).all(), "lang_probs columns at or beyond n_lang were written"
    assert (probs[rows:] == SENT).all() and (tok[rows:] == SENT_I).all(), "rows beyond `rows` were written"
    assert (conf[rows:] == SENT).all() and (nsp[rows:] == SENT).all(), "rows beyond `rows` were written"


def written(out, rows, n_lang):
    probs, tok, conf, nsp, _ = out
    return probs[:rows, :n_lang], tok[:rows], conf[:rows], nsp[:rows]


@pytest.mark.parametrize("kind", ["all", "half", "one"])
@pytest.mark.parametrize("rows", [1, 5, 64])
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_probe_matches_the_f64_oracle(name, rows, kind):
    layout = LAYOUTS[name]
    n_lang = layout[2]
    allow, ref = ref_of(name, kind)
    rng = np.random.default_rng(rows)
    # every other row is patched into a distinct entry of tok_dst, the rest are not (-1)
    dst = [int(d) if r % 2 == 0 else -1 for r, d in enumerate(rng.permutation(70)[:rows])]
    out = run(logits_of(name)[1], rows, layout, allow, dst=dst)
    check_untouched(out, rows, n_lang)
    so.check_probe(written(out, rows, n_lang), tuple(t[:rows] for t in ref), f"{name} rows={rows} allow={kind}")
    tok, tok_dst = out[1], out[4]
    want = torch.full((70,), SENT_I, dtype=I32)
    for r, d in enumerate(dst):
        if d >= 0:
            want[d] = tok[r]
    assert torch.equal(tok_dst, want), "tok_dst differs from lang_tok scattered through dst_rows"
    if kind == "one":
        only = layout[1] + so.allow_ids(allow, n_lang)[0]
        assert (tok[:rows] == only).all() and (out[2][:rows] == 1.0).all()
        assert (out[0][:rows, only - layout[1]] == 1.0).all(), "the single allowed language must have probability 1"


def test_tok_dst_is_untouched_when_no_row_is_patched_or_a_row_is_out_of_range():
    layout = LAYOUTS["v200"]
    xd = logits_of("v200")[1]
    out = run(xd, 5, layout, (1 << 65) - 1, dst=[-1] * 5)
    assert (out[4] == SENT_I).all(), "tok_dst written with dst_rows all -1"
    # entries at or beyond len(tok_dst) are dropped by the kernel's own range check
    out = run(xd, 5, layout, (1 << 65) - 1, dst=[-1, 3, 70, 1 << 30, -7], n_dst=70)
    want = torch.full((70,), SENT_I, dtype=I32)
    want[3] = out[1][1]
    assert torch.equal(out[4], want)


def _edit(name: str, rows: int, fn):
    """A copy of the layout's first rows with fn(x, layout) applied to the [rows, vocab] part."""
    layout = LAYOUTS[name]
    x = logits_of(name)[0][:rows].clone()
    fn(x, layout)
    return x, layout


@pytest.mark.parametrize("name", ["v51865", "v200", "v300"])
def test_ties_take_the_lower_id_and_maxima_outside_the_set_are_ignored(name):
    vocab, lang0, n_lang, ns = LAYOUTS[name]
    allow = ((1 << n_lang) - 1) & ~(1 << 3) & ~(1 << 0)   # languages 0 and 3 are not allowed
    hi, lo = n_lang - 2, 5                               # two allowed ids that will share the maximum

    def fn(x, _):
        x[0, lang0 + hi] = x[0, lang0 + lo] = 50.0       # row 0: a tie -> the lower id
        x[1, lang0 + 3] = 80.0                           # row 1: the global maximum on a disallowed language
        x[2, lang0 + n_lang] = 80.0                      # row 2: ... on the id right after the languages
        x[2, lang0 - 1] = 90.0                           #        and right before them
        x[3, lang0 + hi] = x[3, lang0 + lo] = 50.0       # row 3: the tie below a disallowed maximum
        x[3, lang0 + 0] = 60.0

    x, layout = _edit(name, 4, fn)
    out = run(x.to(DEV), 4, layout, allow)
    ref = so.probe64(x, vocab, lang0, n_lang, allow, ns)
    check_untouched(out, 4, n_lang)
    so.check_probe(written(out, 4, n_lang), ref, f"{name} ties and masks")
    tok = out[1][:4].tolist()
    assert tok[0] == lang0 + lo and tok[3] == lang0 + lo, tok
    assert tok[1] != lang0 + 3 and tok[2] not in (lang0 + n_lang, lang0 - 1), tok
    assert (out[0][:4, 3] == 0).all() and (out[0][:4, 0] == 0).all()


@pytest.mark.parametrize("name", ["v51866", "v200"])
def test_logits_times_50_stay_finite(name):
    """Logits of +-600 and more: exp without the maximum subtracted overflows."""
    x, layout = _edit(name, 5, lambda x, l: x[:, : l[0]].mul_(50.0))
    vocab, lang0, n_lang, ns = layout
    allow = (1 << n_lang) - 1
    out = run(x.to(DEV), 5, layout, allow)
    so.check_probe(written(out, 5, n_lang), so.probe64(x, vocab, lang0, n_lang, allow, ns), f"{name} x50")


@pytest.mark.parametrize("name", ["v51865", "v300"])
def test_minus_infinity_entries_get_probability_zero(name):
    def fn(x, l):
        vocab, lang0, n_lang, ns = l
        x[:, lang0 + 1 : lang0 + n_lang : 3] = float("-inf")   # a third of the languages
        x[:, 0:vocab:7] = float("-inf")                        # and a seventh of everything
        x[1, ns] = float("-inf")                               # row 1: the no-speech id itself

    x, layout = _edit(name, 3, fn)
    vocab, lang0, n_lang, ns = layout
    allow = (1 << n_lang) - 1
    out = run(x.to(DEV), 3, layout, allow)
    ref = so.probe64(x, vocab, lang0, n_lang, allow, ns)
    so.check_probe(written(out, 3, n_lang), ref, f"{name} -inf entries")
    dead = torch.isinf(x[:, lang0 : lang0 + n_lang])
    assert dead.any() and (out[0][:3, :n_lang][dead] == 0).all()
    assert out[3][1] == 0.0


@pytest.mark.parametrize("name", ["v51865", "v200", "v40"])
def test_all_allowed_logits_minus_infinity_give_the_lowest_allowed_id_and_nan(name):
    vocab, lang0, n_lang, ns = LAYOUTS[name]
    allow = (1 << n_lang) - 1 if n_lang == 1 else ((1 << n_lang) - 1) & ~0b101   # lowest allowed: 0 or 1
    ids = so.allow_ids(allow, n_lang)

    def fn(x, _):
        x[0, lang0 + ids] = float("-inf")   # row 0 only; row 1 stays ordinary

    x, layout = _edit(name, 2, fn)
    out = run(x.to(DEV), 2, layout, allow, dst=[4, 9])
    probs, tok, conf, nsp, tok_dst = out
    check_untouched(out, 2, n_lang)
    assert tok[0] == lang0 + ids[0], "the lowest allowed id"
    assert torch.isnan(probs[0, ids]).all() and torch.isnan(conf[0])
    off = np.setdiff1d(np.arange(n_lang), ids)
    assert (probs[0, off] == 0).all(), "disallowed languages stay exactly 0"
    assert tok_dst[4] == lang0 + ids[0] and lang0 <= tok_dst[9] < lang0 + n_lang, "the patched token is a valid id"
    ref = so.probe64(x, vocab, lang0, n_lang, allow, ns)
    so.check_probe(tuple(t[1:2] for t in written(out, 2, n_lang)), tuple(t[1:2] for t in ref), f"{name} row beside")
    assert abs(float(nsp[0]) - ref[3][0]) <= so.prob_bound(ref[3][0])


BAD = {
    "no rows": dict(rows=0),
    "n_lang 0": dict(n_lang=0),
    "n_lang 129": dict(n_lang=129, lang0=0),
    "lang0 < 0": dict(lang0=-1),
    "languages past the vocabulary": dict(lang0=200 - 64),
    "vocab > ld": dict(vocab=209),
    "no_speech_id < 0": dict(no_speech_id=-1),
    "no_speech_id = vocab": dict(no_speech_id=200),
    "ldp < n_lang": dict(ldp=64),
    "allow empty": dict(allow=0),
    "allow only at or beyond n_lang": dict(allow=1 << 65),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_the_wrapper_rejects_what_the_launcher_rejects(what):
    vocab, lang0, n_lang, ns = LAYOUTS["v200"]
    k = dict(rows=2, vocab=vocab, lang0=lang0, n_lang=n_lang, no_speech_id=ns, allow=(1 << n_lang) - 1, ldp=n_lang + 3)
    k.update(BAD[what])
    xd = logits_of("v200")[1][: k["rows"]]
    probs = torch.full((2, k["ldp"]), SENT, dtype=F32, device=DEV)
    tok = torch.full((2,), SENT_I, dtype=I32, device=DEV)
    with pytest.raises((ValueError, RuntimeError)) as ei:
        ops.sot_probe(xd, k["vocab"], k["lang0"], k["n_lang"], k["no_speech_id"], k["allow"], lang_probs=probs,
                      lang_tok=tok)
    assert "HIP error" not in str(ei.value)
    torch.cuda.synchronize()
    assert (probs == SENT).all() and (tok == SENT_I).all(), "a rejected call wrote its outputs"


@pytest.mark.parametrize("what", sorted(set(BAD) - {"no rows"}))
def test_the_binding_rejects_what_the_launcher_rejects(what):
    """The library's own validation (the wrapper's checks bypassed): nothing reaches the kernel."""
    vocab, lang0, n_lang, ns = LAYOUTS["v200"]
    k = dict(vocab=vocab, lang0=lang0, n_lang=n_lang, no_speech_id=ns, allow=(1 << n_lang) - 1, ldp=n_lang + 3)
    k.update(BAD[what])
    xd = logits_of("v200")[1][:2]
    probs = torch.full((2, k["ldp"]), SENT, dtype=F32, device=DEV)
    tok = torch.full((2,), SENT_I, dtype=I32, device=DEV)
    vec = torch.full((2,), SENT, dtype=F32, device=DEV)
    words = [(k["allow"] >> (32 * i)) & 0xFFFFFFFF for i in range(4)]
    with pytest.raises(RuntimeError) as ei:
        ops.sot_ext().sot_probe(xd, k["vocab"], k["lang0"], k["n_lang"], words, k["no_speech_id"], probs, tok, vec,
                                vec.clone(), None, None)
    assert "HIP error" not in str(ei.value)
    torch.cuda.synchronize()
    assert (probs == SENT).all() and (tok == SENT_I).all()
