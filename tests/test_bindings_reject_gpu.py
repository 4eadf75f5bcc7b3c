"""The kernel bindings (csrc/bindings.cpp) reject one wrong argument in one slot, every other
argument valid and on the GPU, with a RuntimeError that names the argument.

Safety: a MISSED check must fail the test ("DID NOT RAISE"), never fault the card.  Every wrong
argument here is device-accessible (a GPU tensor, or pinned host memory for the "not on the GPU"
cases) and holds at least as many bytes as the right one: a wider dtype at the same shape, a larger
but mismatching shape, or a misaligned view of a larger buffer.  No pageable host tensor, no short
tensor, no out-of-range index, no shrunken cache.

Each good argument set is also run once as it stands and compared with ops.reference at the
tolerance of the op's test in test_kernels_gpu.py, so a rejection cannot pass because the baseline
arguments were wrong all along."""
import dataclasses
import functools
import math

import pytest
import torch

import voice_enabled_browser_automation_amd.ops as ops
from voice_enabled_browser_automation_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, I32, I64 = torch.bfloat16, torch.float32, torch.int32, torch.int64


@pytest.fixture(scope="module", autouse=True)
def _native():
    ops.ext()  # fail loudly if the extension is missing


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * len(shape) + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)


def close(a, b, atol, rtol=2e-2):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs().max().item()
    tol = atol + rtol * b.abs().max().item()
    assert err <= tol, f"max err {err} > tol {tol}"


def pinned(t):
    return t.cpu().pin_memory()


def wider(t):
    """The same shape in the next wider dtype (f32 for bf16, int64 for int32)."""
    return t.to({BF: F32, I32: I64}[t.dtype])


def rejects(fn, args, name, **replace):
    """fn(**args) with ``replace`` swapped in raises a RuntimeError naming ``name``."""
    with pytest.raises(RuntimeError, match=rf"\b{name}\b"):
        fn(**{**args, **replace})


# ----------------------------------------------------------------------------- QKV operands
NQ, NKV, HD, K = 2, 1, 16, 128
H = NQ + 2 * NKV
QKV_CONSUMERS = {"skinny_gemm_qkv": 1, "gemm_qkv": 17, "rope_kv_write": 17}  # consumer -> rows M


def _qkv_inputs(M):
    x = rnd(M, K)
    w = ops.permute_qkv_rows(rnd(H * HD, K, scale=K ** -0.5), H, HD)
    return x, w


def _qkv_operands(M):
    return dict(positions=(torch.arange(M, dtype=I32, device=DEV) * 3) % 32,
                slots=torch.arange(M, dtype=I64, device=DEV) + 5, rope=ops.rope_table(32, HD, 1e4, device=DEV),
                q_out=torch.zeros(M, NQ * HD, dtype=BF, device=DEV),
                k_cache=torch.zeros(2, NKV, 16, HD, dtype=BF, device=DEV),
                v_cache=torch.zeros(2, NKV, 16, HD, dtype=BF, device=DEV))


def _qkv_call(consumer, **o):
    E = ops.ext()
    M = QKV_CONSUMERS[consumer]
    x, w = _qkv_inputs(M)
    tail = (NQ, NKV, HD, True, o["positions"], o["slots"], o["rope"], o["q_out"], o["k_cache"], o["v_cache"])
    if consumer == "skinny_gemm_qkv":
        E.skinny_gemm_qkv(x, w, None, False, 1e-5, *tail)
    elif consumer == "gemm_qkv":
        E.gemm_qkv(x, None, w, None, None, None, False, torch.zeros(1 << 16, device=DEV), *tail)
    else:
        qkv = (x.float().cpu() @ w.float().cpu().t()).to(BF).to(DEV)
        E.rope_kv_write(qkv, *tail)


@functools.lru_cache(maxsize=None)
def _qkv_reference(M):
    x, w = _qkv_inputs(M)
    o = {k: v.cpu() for k, v in _qkv_operands(M).items()}
    ref.qkv_rope_write(x.cpu(), w.cpu(), None, fuse_rms=False, eps=1e-5, n_q_heads=NQ, n_kv_heads=NKV, head_dim=HD,
                       rope=o["rope"], positions=o["positions"], slots=o["slots"], q_out=o["q_out"],
                       k_cache=o["k_cache"], v_cache=o["v_cache"])
    return o["q_out"], o["k_cache"], o["v_cache"]


def _two_kv_heads(cache):
    """A [2, 2, 16, HD] view (two kv heads where one is stated) with the good cache's strides, over a
    buffer one block longer: a consumer that missed the check would still write in bounds."""
    return torch.zeros(3, NKV, 16, HD, dtype=BF, device=DEV).as_strided((2, 2, 16, HD), cache.stride())


QKV_WRONG = {
    "positions_int64": ("positions", lambda o: wider(o["positions"])),
    "slots_int32_2M": ("slots", lambda o: torch.cat([o["slots"], o["slots"]]).to(I32)),
    "q_out_f32": ("q_out", lambda o: wider(o["q_out"])),
    "k_cache_2_kv_heads": ("k_cache", lambda o: _two_kv_heads(o["k_cache"])),
    "v_cache_head_dim_32": ("v_cache", lambda o: torch.zeros(2, NKV, 16, 32, dtype=BF, device=DEV)),
    "rope_table_16_pairs": ("rope", lambda o: ops.rope_table(32, 32, 1e4, device=DEV)),
    "positions_pinned": ("positions", lambda o: pinned(o["positions"])),
}


@pytest.mark.parametrize("consumer", sorted(QKV_CONSUMERS))
def test_qkv_good_operands_match_reference(consumer):
    M = QKV_CONSUMERS[consumer]
    o = _qkv_operands(M)
    _qkv_call(consumer, **o)
    for got, exp in zip((o["q_out"], o["k_cache"], o["v_cache"]), _qkv_reference(M)):
        close(got, exp, 3e-2)


@pytest.mark.parametrize("case", sorted(QKV_WRONG))
@pytest.mark.parametrize("consumer", sorted(QKV_CONSUMERS))
def test_qkv_wrong_operand_is_rejected(consumer, case):
    name, make = QKV_WRONG[case]
    o = _qkv_operands(QKV_CONSUMERS[consumer])
    rejects(functools.partial(_qkv_call, consumer), o, name, **{name: make(o)})


# ----------------------------------------------------------------------------- tiled GEMM operands
GM, GN = 17, 16


def _gemm_args():
    x = rnd(GM, K)
    rstd = torch.empty(GM, device=DEV)
    ops.ext().row_rstd(x, rstd, 1e-5)
    return dict(x=x, w=rnd(GN, K, scale=K ** -0.5), bias=rnd(GN, scale=0.1), rstd=rstd, residual=rnd(GM, GN),
                y=torch.empty(GM, GN, dtype=BF, device=DEV), ws=torch.zeros(1 << 16, device=DEV))


def _gemm_call(kind, *, x, w, bias, rstd, residual, y, ws):
    E = ops.ext()
    if kind == "gemm":
        E.gemm(x, w, bias, y, 1, rstd, residual, False, ws)
    else:  # W8A16: bf16 x, fp8 tiled weight
        w8 = ops.FP8Weight.quantize(w)
        assert w8.tiled
        E.gemm_fp8(x, None, w8.w8, w8.scale, bias, y, 1, rstd, residual, ws)


def _misaligned_rows(t):
    """t's values in a column-sliced view of a wider buffer: rows start 2 bytes off a 16-byte boundary."""
    wide = torch.zeros(t.shape[0], t.shape[1] + 8, dtype=t.dtype, device=t.device)
    view = wide[:, 1 : 1 + t.shape[1]]
    view.copy_(t)
    return view


GEMM_WRONG = {
    "bias_f32": ("bias", lambda a: wider(a["bias"])),
    "rstd_bf16_2M": ("rstd", lambda a: torch.ones(2 * GM, dtype=BF, device=DEV)),
    "residual_f32": ("residual", lambda a: wider(a["residual"])),
    "y_misaligned_view": ("y", lambda a: _misaligned_rows(a["y"])),
    "ws_bf16": ("ws", lambda a: torch.zeros(2 * a["ws"].numel(), dtype=BF, device=DEV)),
    "bias_pinned": ("bias", lambda a: pinned(a["bias"])),
}


@pytest.mark.parametrize("kind", ["gemm", "gemm_fp8"])
def test_gemm_good_operands_match_reference(kind):
    a = _gemm_args()
    _gemm_call(kind, **a)
    w = a["w"].cpu() if kind == "gemm" else ops.FP8Weight.quantize(a["w"]).to("cpu").dequant()
    exp = torch.empty(GM, GN, dtype=BF)
    ref.linear(a["x"].cpu(), w, a["bias"].cpu(), out=exp, residual=a["residual"].cpu(), fuse_rms=True, eps=1e-5)
    close(a["y"], exp, 3e-2)


@pytest.mark.parametrize("case", sorted(GEMM_WRONG))
@pytest.mark.parametrize("kind", ["gemm", "gemm_fp8"])
def test_gemm_wrong_operand_is_rejected(kind, case):
    name, make = GEMM_WRONG[case]
    a = _gemm_args()
    rejects(functools.partial(_gemm_call, kind), a, name, **{name: make(a)})


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible GPUs")
def test_gemm_rejects_a_tensor_on_another_device():
    a = _gemm_args()
    rejects(functools.partial(_gemm_call, "gemm"), a, "w", w=a["w"].to("cuda:1"))


# ----------------------------------------------------------------------------- elementwise and the rest
# op -> (good-argument builder, call, positive control, {case: (argument, wrong-value maker)})
def _norm_args():
    return dict(x=rnd(3, K), w=rnd(K) + 1, b=rnd(K, scale=0.2), y=torch.empty(3, K, dtype=BF, device=DEV))


def _layernorm_ok(a):
    exp = ref.layernorm(a["x"].cpu(), a["w"].cpu(), a["b"].cpu(), eps=1e-5, out=torch.empty(3, K, dtype=BF))
    close(a["y"], exp, 3e-2)


def _rmsnorm_ok(a):
    close(a["y"], ref.rmsnorm(a["x"].cpu(), a["w"].cpu(), eps=1e-5, out=torch.empty(3, K, dtype=BF)), 3e-2)


def _bias_act_args():
    return dict(x=rnd(5, 64), bias=rnd(64, seed=1), residual=rnd(5, 64, seed=2),
                y=torch.empty(5, 64, dtype=BF, device=DEV))


def _bias_act_ok(a):
    close(a["y"], torch.nn.functional.gelu(a["x"].float() + a["bias"].float()) + a["residual"].float(), 2e-2)


def _swiglu_args():
    return dict(gu=rnd(3, 64), h=torch.empty(3, 32, dtype=BF, device=DEV))


def _swiglu_ok(a):
    t = a["gu"].float().view(3, 2, 2, 16)  # per 32-column tile: 16 gate | 16 up
    close(a["h"], (torch.nn.functional.silu(t[:, :, 0]) * t[:, :, 1]).reshape(3, 32), 2e-2)


def _embedding_args():
    return dict(ids=torch.tensor([3, 99, 0, 150], dtype=I32, device=DEV), table=rnd(100, 64),
                pos_table=rnd(50, 64, seed=1), positions=torch.arange(4, dtype=I32, device=DEV),
                out=torch.empty(4, 64, dtype=BF, device=DEV))


def _embedding_ok(a):
    c = {k: v.cpu() for k, v in a.items()}
    close(a["out"], ref.embedding(c["ids"], c["table"], pos_table=c["pos_table"], positions=c["positions"],
                                  out=torch.empty(4, 64, dtype=BF)), 1e-2)


def _flash_args():
    B, S, Hq, D = 1, 33, 1, 64
    kv = ops.KVLayout.contiguous(rnd(B, S, Hq, D, seed=1), rnd(B, S, Hq, D, seed=2),
                                 torch.arange(B, dtype=I32, device=DEV)[:, None].contiguous())
    return dict(q=rnd(B, S, Hq, D), kv=kv, out=torch.empty(B, S, Hq, D, dtype=BF, device=DEV),
                k_lens=torch.full((B,), S, dtype=I32, device=DEV))


def _flash_call(*, q, kv, out, k_lens):
    ops.ext().flash_attention(q, kv.k, kv.v, kv.table, kv.block_size, kv.sb, kv.sh, kv.st, out, q.shape[1], q.shape[2],
                              False, 0, None, k_lens, q.shape[3] ** -0.5)


def _flash_ok(a):
    q, kv = a["q"], a["kv"]
    exp = ref.flash_attention(q.cpu(), ops.KVLayout.contiguous(kv.k.cpu(), kv.v.cpu(), kv.table.cpu()), Sk=q.shape[1],
                              n_kv_heads=q.shape[2], causal=False, scale=q.shape[3] ** -0.5,
                              out=torch.empty(q.shape, dtype=BF), k_lens=a["k_lens"].cpu())
    close(a["out"], exp, 2e-2)


DA = dict(nq=2, nkv=2, hd=64, rows=2)


def _decode_args():
    nq, nkv, hd, rows = DA["nq"], DA["nkv"], DA["hd"], DA["rows"]
    return dict(q=rnd(rows, nq * hd), k=rnd(4, nkv, 16, hd, seed=1), v=rnd(4, nkv, 16, hd, seed=2),
                table=torch.tensor([[1, 0, 3, 2]], dtype=I32, device=DEV),
                ctx_lens=torch.tensor([5, 40], dtype=I32, device=DEV), seq_ids=torch.zeros(rows, dtype=I32, device=DEV),
                out=torch.empty(rows, nq * hd, dtype=BF, device=DEV))


def _decode_call(*, q, k, v, table, ctx_lens, seq_ids, out):
    nq, nkv, hd, rows = DA["nq"], DA["nkv"], DA["hd"], DA["rows"]
    ops.ext().decode_attention(q, k, v, table, 16, k.stride(0), k.stride(1), k.stride(2), ctx_lens, seq_ids, nq, nkv,
                               hd, hd ** -0.5, 1, torch.empty(rows * nq * hd, device=DEV),
                               torch.empty(rows * nq * 2, device=DEV), torch.zeros(rows * nkv, dtype=I32, device=DEV),
                               out, None)


def _decode_ok(a):
    c = {k: v.cpu() for k, v in a.items()}
    exp = ref.decode_attention(c["q"], ops.KVLayout.paged(c["k"], c["v"], c["table"]), c["ctx_lens"], c["seq_ids"],
                               n_q_heads=DA["nq"], n_kv_heads=DA["nkv"], head_dim=DA["hd"], scale=DA["hd"] ** -0.5,
                               out=torch.empty(a["out"].shape, dtype=BF))
    close(a["out"], exp, 2e-2)


def _quant_args():
    return dict(x=rnd(3, K), q=torch.empty(3, K, dtype=torch.float8_e4m3fn, device=DEV),
                scale=torch.empty(3, device=DEV), rstd=torch.empty(3, device=DEV))


def _quant_ok(a):
    xf = a["x"].float()
    torch.testing.assert_close(a["rstd"], torch.rsqrt(xf.pow(2).mean(-1) + 1e-5), rtol=1e-4, atol=0)
    # the codes dequantise to the reference's e4m3 rounding of x, give or take one step of the top
    # binade (32 of 448 = amax / 14) where the two divisions round a tie differently
    deq = (a["q"].float() * a["scale"][:, None]).cpu()
    err = (deq - ops.quant_rows_fp8(a["x"].cpu())).abs().amax(-1)
    assert bool((err <= xf.abs().amax(-1).cpu() / 14).all()), err


def _sample_args():
    rows, V = 2, 4096
    g = torch.Generator().manual_seed(7)
    return dict(logits=torch.randn(rows, V, generator=g).to(DEV), temperature=torch.full((rows,), 0.7, device=DEV),
                seed=torch.tensor([1234], dtype=I64, device=DEV), step=torch.zeros(1, dtype=I32, device=DEV),
                out_tokens=torch.empty(rows, dtype=I32, device=DEV))


def _sample_call(*, logits, temperature, seed, step, out_tokens):
    n = logits.shape[0] * 64
    ops.ext().sample(logits, None, temperature, seed, step, out_tokens, torch.empty(n, device=DEV),
                     torch.empty(n, dtype=I32, device=DEV))


def _sample_ok(a):
    exp = torch.empty(2, dtype=I32)
    ref.sample(a["logits"].cpu(), mask=None, temperature=a["temperature"].cpu(), seed=a["seed"].cpu(),
               step=torch.zeros(1, dtype=I32), out_tokens=exp)
    assert a["out_tokens"].cpu().tolist() == exp.tolist()


def _pcm_args():
    pcm = (torch.sin(torch.arange(320) * 2 * math.pi * 440 / 16000) * 8000).to(torch.int16).to(DEV)
    return dict(pcm=pcm, out=torch.empty(320, device=DEV))


def _log_mel_args():
    n_frames, n_mels = 16, 80
    audio = (torch.sin(torch.arange(n_frames * 160) * 2 * math.pi * 440 / 16000) * 0.25).to(DEV)
    fb = ref.mel_filterbank(n_mels=n_mels).to(DEV)
    basis, fbf = ops.logmel_tables(fb)
    return dict(audio=audio, window=torch.hann_window(400, periodic=True, device=DEV), fb=fb, basis=basis, fb_frag=fbf,
                out=torch.empty(n_frames, n_mels, dtype=BF, device=DEV))


def _log_mel_call(*, audio, window, fb, basis, fb_frag, out):
    n_frames, n_mels = out.shape
    ops.ext().log_mel(audio, n_frames, window, basis, fb_frag, n_mels, torch.empty(n_frames * n_mels, device=DEV),
                      torch.empty(1, device=DEV), out)


def _log_mel_ok(a):
    exp = ref.log_mel(a["audio"].cpu(), n_frames=a["out"].shape[0], window=a["window"].cpu(), mel_fb=a["fb"].cpu(),
                      out=torch.empty(a["out"].shape, dtype=BF))
    close(a["out"], exp, 3e-2)


def _E(name, order):
    """The raw binding ``name`` called with the named good arguments in positional ``order``
    (a string of names, or literal values)."""
    return lambda **a: getattr(ops.ext(), name)(*[a[o] if isinstance(o, str) else o for o in order])


OPS = {
    "layernorm": (_norm_args, _E("layernorm", ["x", None, None, "w", "b", "y", 1e-5]), _layernorm_ok,
                  {"y_f32": ("y", wider), "w_f32": ("w", wider), "b_f32": ("b", wider)}),
    "rmsnorm": (_norm_args, _E("rmsnorm", ["x", None, None, "w", "y", 1e-5]), _rmsnorm_ok, {"w_f32": ("w", wider)}),
    "bias_act": (_bias_act_args, _E("bias_act", ["x", "bias", "residual", "y", 1]), _bias_act_ok,
                 {"y_f32": ("y", wider), "bias_f32": ("bias", wider), "residual_f32": ("residual", wider)}),
    "swiglu": (_swiglu_args, _E("swiglu", ["gu", "h"]), _swiglu_ok, {"h_f32": ("h", wider)}),
    "embedding": (_embedding_args, _E("embedding", ["ids", "table", "pos_table", "positions", "out", 0]),
                  _embedding_ok, {"out_f32": ("out", wider), "ids_pinned": ("ids", pinned)}),
    "flash_attention": (_flash_args, _flash_call, _flash_ok,
                        {"out_f32": ("out", wider), "k_lens_pinned": ("k_lens", pinned)}),
    "decode_attention": (_decode_args, _decode_call, _decode_ok,
                         {"out_f32": ("out", wider), "ctx_lens_pinned": ("ctx_lens", pinned),
                          "table_pinned": ("table", pinned)}),
    "quant_fp8_rows": (_quant_args, _E("quant_fp8_rows", ["x", "q", "scale", "rstd", 1e-5]), _quant_ok,
                       {"scale_pinned": ("scale", pinned)}),
    "sample": (_sample_args, _sample_call, _sample_ok, {"temperature_pinned": ("temperature", pinned)}),
    "pcm16_to_f32": (_pcm_args, _E("pcm16_to_f32", ["pcm", "out", 1.0]),
                     lambda a: close(a["out"], a["pcm"].float() / 32768, 1e-6), {"out_pinned": ("out", pinned)}),
    "log_mel": (_log_mel_args, _log_mel_call, _log_mel_ok, {"window_pinned": ("window", pinned)}),
}


@pytest.mark.parametrize("op", sorted(OPS))
def test_good_arguments_match_reference(op):
    build, call, verify, _ = OPS[op]
    a = build()
    call(**a)
    verify(a)


@pytest.mark.parametrize("op,case", [(op, case) for op in sorted(OPS) for case in sorted(OPS[op][3])])
def test_wrong_argument_is_rejected(op, case):
    build, call, _, wrong = OPS[op]
    name, make = wrong[case]
    a = build()
    rejects(call, a, name, **{name: make(a[name])})


# ----------------------------------------------------------------------------- persistent Whisper decoder
class _Recorder:
    """The kernel library with wdec_run's argument lists kept."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name != "wdec_run":
            return fn

        def wdec_run(*args):
            self.calls.append(args)
            return fn(*args)

        return wdec_run


def test_wdec_run_rejects_an_int64_index_buffer(monkeypatch):
    """bufs[6] (seq_ids, int32) given as int64.  The good argument list is the model's own, recorded
    from one persistent decoder step that is first checked against the per-kernel path."""
    from voice_enabled_browser_automation_amd.asr.engine import WhisperRunner
    from voice_enabled_browser_automation_amd.models.config import get_config
    from voice_enabled_browser_automation_amd.models.whisper import WhisperModel

    rec = _Recorder(ops.ext())
    monkeypatch.setattr(ops, "_EXT", rec)
    cfg = dataclasses.replace(get_config("whisper-tiny"), n_enc_layers=1, n_dec_layers=2)
    m = WhisperModel(cfg, device=DEV, seed=3)
    enc = rnd(1, cfg.n_audio_ctx, cfg.d_model)
    logits = {}
    for persist in ("0", "1"):
        monkeypatch.setenv("VWA_ASR_PERSIST", persist)
        r = WhisperRunner(m, max_sessions=1, use_graphs=False)
        r.set_cross(0, enc)
        logits[persist] = r.step([(0, 5, 0)]).float().cpu().clone()
    assert rec.calls and not m.chain_error()
    err = (logits["1"] - logits["0"]).abs().max().item()
    assert err < 0.02 * (1 + logits["0"].abs().max().item()), err
    args = list(rec.calls[-1])
    bufs = list(args[2])
    assert bufs[6].dtype == I32
    bufs[6] = wider(bufs[6])
    with pytest.raises(RuntimeError, match=r"\bbufs\[6\]"):
        rec.real.wdec_run(args[0], args[1], bufs, *args[3:])
