"""Per-element float64 oracle for the small kernels (norms, element-wise, embedding, rope, PCM, sampler)
and, in its last part, the per-key oracle for the attention kernels.

A plain helper module (no fixtures, no pytest hooks).  The comparator asks, per element,

    |got - ref64| <= h * |ref64| + slack

where ``ref64`` is the operation computed in float64 from the very bf16 / f32 inputs the kernel
read, ``h`` is half an ulp of the output type under round-to-nearest-even (2^-8 for bf16: what
``f2bf`` does; 0 for f32) and ``slack`` is what the kernel's f32 arithmetic may add, given per call.
Nothing here scales a tolerance by the largest value of the whole tensor.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

from voice_enabled_browser_automation_amd import ops
from voice_enabled_browser_automation_amd.ops import reference as ref

BF = torch.bfloat16
F64 = torch.float64
HALF_ULP = {torch.bfloat16: 2.0 ** -8, torch.float32: 0.0}
# f32 arithmetic alone (norms, embedding, bias add, rope): relative to the row's largest |ref64|
F32_SLACK = 2.0 ** -18
SENTINEL = -12288.0  # exactly representable in bf16, f32 and int32; no case here produces it

# Where an approximate intrinsic sits in the path the slack is MEASURED, not guessed: 4 x the
# kernel's largest deviation from the float64 reference (deviation() below: what the output
# rounding lets through) over every case of tests/test_small_kernels_gpu.py on an MI355X; the
# tests print the figures (MEASURED ...).  All are 4 to 6 orders of magnitude below what the
# whole-tensor close() of tests/test_kernels_gpu.py allowed for the same kernels.
#   silu via __expf (swiglu), relative to |ref64|: measured 2.14e-8 (F = 14336, 70 rows)
C_SILU = 4 * 2.14e-8
#   gelu_erf (bias_act, act 1), relative to max(1, |x + bias|) -- erff's absolute error times
#   x / 2: measured 4.46e-8 (N = 5120)
C_GELU = 4 * 4.46e-8
#   rsqrtf, eps-dominated rows included (row_rstd, quant_fp8_rows' rstd: f32 outputs, so this also
#   holds their rounding), relative to |ref64|: measured 1.42e-7 (D = 8192)
C_RSQRT = 4 * 1.42e-7
#   __logf twice in the sampler's Gumbel key (f32 output), absolute: measured 1.28e-6 (V = 1000)
C_KEY = 4 * 1.28e-6


# ----------------------------------------------------------------------------- comparator
def rne(ref64: torch.Tensor, dtype) -> torch.Tensor:
    """float64 -> ``dtype`` in ONE round-to-nearest-even step (torch's double -> bf16 goes through
    f32: two roundings).  bf16: 8 significand bits, ulp exponent floored at the subnormal spacing."""
    if dtype == torch.float32:
        return ref64.to(torch.float32)
    assert dtype == torch.bfloat16
    _, e = torch.frexp(ref64)  # |x| = m 2^e, m in [0.5, 1)
    ue = (e - 8).clamp(min=-133).to(F64)
    q = torch.round(ref64 * torch.exp2(-ue)) * torch.exp2(ue)  # torch.round: half to even
    return torch.where(torch.isfinite(ref64), q, ref64).to(torch.bfloat16)  # q is exact in bf16


def deviation(got: torch.Tensor, ref64: torch.Tensor, out_dtype) -> torch.Tensor:
    """What can be seen of the kernel's own error through the output rounding, per element: the
    unrounded result lies within half the spacing at ``got``, so it is at least
    |got - ref64| - spacing(got) / 2 away from ref64 (f32 outputs: |got - ref64| itself, h is 0).
    The measured slack constants are 4 x the largest value of this over the GPU cases."""
    g = got.detach().to("cpu", F64)
    if out_dtype == torch.float32:
        return (g - ref64).abs()
    _, e = torch.frexp(g)
    half = torch.exp2((e - 9).clamp(min=-134).to(F64))  # bf16: spacing 2^(e - 8) for |g| in [2^(e-1), 2^e)
    return ((g - ref64).abs() - half).clamp(min=0.0)


def assert_elementwise(got: torch.Tensor, ref64: torch.Tensor, *, slack, out_dtype, what: str = "") -> None:
    assert got.dtype == out_dtype, f"{what}: output dtype {got.dtype}, expected {out_dtype}"
    assert ref64.dtype == F64 and tuple(got.shape) == tuple(ref64.shape), f"{what}: {tuple(got.shape)} vs {tuple(ref64.shape)}"
    g = got.detach().to("cpu", F64)
    bound = HALF_ULP[out_dtype] * ref64.abs() + torch.as_tensor(slack, dtype=F64)
    bound = bound.expand_as(ref64)
    err = (g - ref64).abs()
    same = (g == ref64)  # (equal infinities: inf - inf is NaN)
    bad = ~((err <= bound) | same)  # a NaN in got or err is bad
    if bool(bad.any()):
        over = torch.where(bad, torch.nan_to_num(err / bound.clamp(min=1e-300), nan=math.inf, posinf=math.inf),
                           torch.zeros_like(err))
        flat = int(over.argmax())
        idx = tuple(int(i) for i in np.unravel_index(flat, tuple(ref64.shape))) if ref64.dim() else ()
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {ref64.numel()} elements out of bound; worst at {idx}: got {float(g[idx])!r}, "
            f"ref64 {float(ref64[idx])!r}, |err| {float(err[idx]):.6g} = {float(over[idx]):.4g} x bound "
            f"{float(bound[idx]):.6g}")


def assert_bitwise(got: torch.Tensor, ref64: torch.Tensor, *, out_dtype, what: str = "") -> None:
    """got == the single RNE rounding of ref64, bit for bit (residual_out, plain copies)."""
    want = rne(ref64, out_dtype)
    g = got.detach().cpu()
    assert g.dtype == out_dtype and g.shape == want.shape, what
    it = torch.int16 if out_dtype == torch.bfloat16 else torch.int32
    ne = g.contiguous().view(it) != want.contiguous().view(it)
    if bool(ne.any()):
        idx = tuple(int(i) for i in ne.nonzero()[0])
        raise AssertionError(f"{what}: {int(ne.sum())} elements differ from RNE(ref64); first at {idx}: got "
                             f"{float(g[idx])!r}, want {float(want[idx])!r} (ref64 {float(ref64[idx])!r})")


def row_slack(ref64: torch.Tensor) -> torch.Tensor:
    """F32_SLACK x the row's largest |ref64| ([..., 1], broadcasts over the row)."""
    return F32_SLACK * ref64.abs().amax(dim=-1, keepdim=True)


def bias_act_slack(y64: torch.Tensor, pre64: torch.Tensor, act: int) -> torch.Tensor:
    """act 0: f32 adds alone (row_slack); act 1 (gelu_erf): C_GELU x max(1, |x + bias|) per element."""
    return C_GELU * pre64.abs().clamp(min=1.0) if act == 1 else row_slack(y64)


def old_close_accepts(a: torch.Tensor, b: torch.Tensor, atol: float, rtol: float = 2e-2) -> bool:
    """The whole-tensor criterion of tests/test_kernels_gpu.py close(): kept to record what it lets through."""
    a, b = a.double().cpu(), b.double().cpu()
    return bool((a - b).abs().max() <= atol + rtol * b.abs().max())


# ----------------------------------------------------------------------------- canary
def canary(shape, rows: Tuple[int, int] = (2, 3), cols: Tuple[int, int] = (0, 0), *, dtype=BF, device="cpu",
           fill: float = SENTINEL):
    """An output view of ``shape`` ([R, C]) inside a larger buffer filled with ``fill``: ``rows``
    guard rows above / below and ``cols`` guard columns left / right (keep them multiples of 8 for
    16-byte rows; (0, 0) leaves the view contiguous).  Returns (view, check); ``check()`` asserts that
    nothing outside the view changed."""
    R, C = shape
    buf = torch.full((rows[0] + R + rows[1], cols[0] + C + cols[1]), fill, dtype=dtype, device=device)
    view = buf[rows[0]: rows[0] + R, cols[0]: cols[0] + C]

    def check(what: str = "") -> None:
        b = buf.detach().cpu().clone().double()
        b[rows[0]: rows[0] + R, cols[0]: cols[0] + C] = fill
        bad = b != fill
        assert not bool(bad.any()), f"{what}: wrote outside the output view at {[tuple(i) for i in bad.nonzero()[:4].tolist()]}"

    return view, check


def untouched(t: torch.Tensor, fill: float = SENTINEL) -> torch.Tensor:
    """Elementwise: still holds the sentinel."""
    return t.detach().cpu().double() == fill


# ----------------------------------------------------------------------------- float64 references
def _d(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None else t.detach().to("cpu", F64)


def rmsnorm64(x, w, eps, residual=None):
    """-> (y64, resid64 or None).  y uses the unrounded x + residual, as the kernel does."""
    v = _d(x) if residual is None else _d(x) + _d(residual)
    y = v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps)
    return (y if w is None else y * _d(w)), (None if residual is None else v)


def layernorm64(x, w, b, eps, residual=None):
    v = _d(x) if residual is None else _d(x) + _d(residual)
    mu = v.mean(-1, keepdim=True)
    var = (v - mu).pow(2).mean(-1, keepdim=True)
    return (v - mu) * torch.rsqrt(var + eps) * _d(w) + _d(b), (None if residual is None else v)


def rstd64(x, eps):
    return torch.rsqrt(_d(x).pow(2).mean(-1) + eps)


def swiglu64(gu):
    """gu [rows, 2F] in [16 gate | 16 up] tiles -> silu(gate) * up [rows, F]."""
    g = _d(gu)
    t = g.view(g.shape[0], g.shape[1] // 32, 2, 16)
    gate, up = t[:, :, 0, :], t[:, :, 1, :]
    return (gate * torch.sigmoid(gate) * up).reshape(g.shape[0], g.shape[1] // 2)


def bias_act64(x, bias, residual, act):
    """-> (y64, pre64): act(x + bias) + residual and the pre-activation x + bias."""
    v = _d(x) if bias is None else _d(x) + _d(bias)
    y = 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0))) if act == 1 else v
    return (y if residual is None else y + _d(residual)), v


def embedding64(ids, table, vocab_start=0, pos_table=None, positions=None, rows=None):
    n = ids.numel() if rows is None else rows
    idl = ids.detach().cpu()[:n].long() - vocab_start
    ok = (idl >= 0) & (idl < table.shape[0])
    e = _d(table)[idl.clamp(0, table.shape[0] - 1)]
    e = torch.where(ok[:, None], e, torch.zeros_like(e))  # (+0 rows, as the kernel writes them)
    if pos_table is not None:
        e = e + _d(pos_table)[positions.detach().cpu()[:n].long()]
    return e


def rope64(qkv, n_q, n_kv, hd, positions, rope, k_sin_sign: float = 1.0):
    """qkv [M, (n_q + 2 n_kv) hd] in the per-head permuted layout (ops.qkv_row_perm) -> natural-layout
    (q [M, n_q, hd], k [M, n_kv, hd], v [M, n_kv, hd]) in float64, q and k rotated (rotate-half) when
    ``rope`` ([max_pos, hd/2, 2] cos / sin) is given.  k_sin_sign = -1 builds the K-only mutation."""
    M, H = qkv.shape[0], n_q + 2 * n_kv
    y = ops.unpermute_qkv_cols(_d(qkv), H, hd).view(M, H, hd)
    q, k, v = y[:, :n_q], y[:, n_q: n_q + n_kv], y[:, n_q + n_kv:]
    if rope is not None:
        cs = _d(rope)[positions.detach().cpu()[:M].long()]
        c, s = cs[..., 0][:, None, :], cs[..., 1][:, None, :]
        half = hd // 2

        def rot(x, sg):
            x1, x2 = x[..., :half], x[..., half:]
            return torch.cat([x1 * c - x2 * (sg * s), x2 * c + x1 * (sg * s)], dim=-1)

        q, k = rot(q, 1.0), rot(k, k_sin_sign)
    return q, k, v


def pcm64(pcm, in_rate: int, n_out: int, pos_dtype=np.float64):
    """Linear resampling to 16 kHz in float64 (read position i * in_rate / 16000, clamped taps).
    pos_dtype = np.float32 computes the read position as an f32 product: the mutation."""
    p = pcm.detach().cpu().numpy().astype(np.float64)
    if in_rate == 16000:
        return torch.from_numpy(p[:n_out] / 32768.0)
    i = np.arange(n_out)
    if pos_dtype is np.float32:
        src = (i.astype(np.float32) * np.float32(in_rate / 16000.0)).astype(np.float64)
    else:
        src = i.astype(np.float64) * (in_rate / 16000.0)
    j = np.floor(src).astype(np.int64)
    f = src - j
    j1 = np.minimum(j + 1, p.size - 1)
    j = np.minimum(j, p.size - 1)
    return torch.from_numpy(((1.0 - f) * p[j] + f * p[j1]) / 32768.0)


# ----------------------------------------------------------------------------- inputs
# The CPU test shows these inputs are fair (an honest f32 computation passes the comparator on
# them); the GPU test feeds the very same tensors to the kernels.
REGIMES = ("unit", "tiny", "zero_row", "offset", "outlier")
EPS = 1e-5


def _gen(*key) -> torch.Generator:
    s = 17
    for k in key:
        s = (s * 1000003 + int(k)) % 0x7FFFFFFF
    return torch.Generator().manual_seed(s)


def regime_rows(regime: str, rows: int, D: int, gen: torch.Generator) -> torch.Tensor:
    x = torch.randn(rows, D, generator=gen)
    if regime == "tiny":  # mean(x^2) ~ 1e-6 < eps: eps decides the scale
        x = x * 2.0 ** -10
    elif regime == "zero_row":
        x[rows // 2] = 0.0
    elif regime == "offset":
        x = 30.0 + 0.5 * x
    elif regime == "outlier":
        x[:, D // 3] = 200.0
    else:
        assert regime == "unit", regime
    return x.to(BF)


def norm_case(regime: str, rows: int, D: int):
    """x, residual, w, b (bf16, CPU) of one norm case; the residual is unit-scale except on the
    tiny and zero-row regimes, where it keeps the regime (x + residual stays tiny / zero)."""
    g = _gen(REGIMES.index(regime), rows, D)
    x = regime_rows(regime, rows, D, g)
    if regime == "tiny":
        r = regime_rows("tiny", rows, D, g)
    elif regime == "zero_row":
        r = regime_rows("zero_row", rows, D, g)
    else:
        r = regime_rows("unit", rows, D, g)
    w = (1.0 + 0.5 * torch.randn(D, generator=g)).to(BF)
    b = torch.randn(D, generator=g).to(BF)
    return x, r, w, b


SWIGLU_GATES = (30.0, -30.0, 1e4, -1e4, 0.0)


def swiglu_case(rows: int, F: int) -> torch.Tensor:
    """gu [rows, 2F] ([16 gate | 16 up] tiles): unit values, the first gates of every row replaced
    by the saturating ones."""
    g = _gen(7, rows, F)
    gu = torch.randn(rows, 2 * F, generator=g)
    k = min(len(SWIGLU_GATES), 16)
    gu[:, :k] = torch.tensor(SWIGLU_GATES[:k])
    return gu.to(BF)


def bias_act_case(rows: int, N: int):
    g = _gen(8, rows, N)
    x = (2.0 * torch.randn(rows, N, generator=g)).to(BF)
    x[:, 0], x[:, 1] = -9.0, 9.0  # gelu tails
    return x, torch.randn(N, generator=g).to(BF), torch.randn(rows, N, generator=g).to(BF)


def embedding_case(D: int, vocab_start: int = 1000, shard: int = 40, n_pos: int = 12):
    """A table shard [shard, D] for ids vocab_start .. vocab_start + shard - 1, a position table,
    ids around both shard edges (and -1), positions."""
    g = _gen(9, D)
    table = torch.randn(shard, D, generator=g).to(BF)
    pos_table = torch.randn(n_pos, D, generator=g).to(BF)
    ve = vocab_start + shard
    ids = torch.tensor([vocab_start - 1, vocab_start, ve - 1, ve, -1, vocab_start + 7, 0, ve + 5, vocab_start + 1],
                       dtype=torch.int32)
    positions = torch.tensor([3, 0, n_pos - 1, 5, 1, 2, 7, 4, 6], dtype=torch.int32)
    return table, pos_table, ids, positions


def rope_case(hd: int, n_q: int, n_kv: int, M: int = 7, max_pos: int = 50):
    """qkv (permuted layout, bf16), unordered positions with 0 and the table's last row, the table."""
    g = _gen(10, hd, n_q, n_kv)
    qkv = torch.randn(M, (n_q + 2 * n_kv) * hd, generator=g).to(BF)
    positions = torch.tensor([max_pos - 1, 0, 17, 3, max_pos - 1, 1, 30][:M], dtype=torch.int32)
    return qkv, positions, ops.rope_table(max_pos, hd, 10000.0)


PCM_OUT = 480000  # one 30 s window at 16 kHz


def pcm_case(in_rate: int, n_out: int = PCM_OUT) -> torch.Tensor:
    """A 3 kHz tone at half scale plus noise, sampled at in_rate; exactly as many input samples as
    make the last output's second tap fall off the end (it is clamped)."""
    n_in = int(math.floor((n_out - 1) * (in_rate / 16000.0))) + 1
    g = _gen(11, in_rate)
    t = torch.arange(n_in, dtype=F64)
    s = 16384.0 * torch.sin(2.0 * math.pi * 3000.0 * t / in_rate) + 300.0 * torch.randn(n_in, generator=g, dtype=F64)
    return s.round().clamp(-32768, 32767).to(torch.int16)


# ----------------------------------------------------------------------------- sampler
_M64 =(1 << 64) - 1
NO_TOKEN = 0x7FFFFFFF  # part_idx of a chunk with no admitted token (its part_val is -inf)


def uniforms(seed: int, step: int, row: int, ids: np.ndarray) -> np.ndarray:
    """The sampler's u in (0, 1) for global token ids (float64; exact: 23 bits + 0.5)."""
    base = ref._splitmix64((seed & _M64) ^ ref._splitmix64((step * 0x100000001B3 + row) & _M64))
    x = np.uint64(base) ^ ids.astype(np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return ((x >> np.uint64(41)).astype(np.float64) + 0.5) / 8388608.0


def gumbel_keys64(logits_row: torch.Tensor, T: float, seed: int, step: int, row: int, v_offset: int = 0) -> torch.Tensor:
    """logit / T - log(-log(u)) in float64; plain logits for T <= 0 (greedy)."""
    lg = _d(logits_row)
    if T <= 0:
        return lg
    u = uniforms(seed, step, row, np.arange(v_offset, v_offset + lg.numel()))
    return lg / float(T) - torch.from_numpy(np.log(-np.log(u)))


def mask_bits(mask_row: torch.Tensor, n: int, v_offset: int = 0) -> torch.Tensor:
    """int32 mask words -> bool [n] for tokens v_offset .. v_offset + n - 1."""
    words = mask_row.detach().cpu().to(torch.int64) & 0xFFFFFFFF
    return ((words[:, None] >> torch.arange(32)[None, :]) & 1).reshape(-1)[v_offset: v_offset + n].bool()


def pack_mask(bits: torch.Tensor) -> torch.Tensor:
    """bool [rows, n] -> int32 mask words [rows, ceil(n / 32)]."""
    rows, n = bits.shape
    words = (n + 31) // 32
    b = torch.zeros(rows, words * 32, dtype=torch.int64)
    b[:, :n] = bits.long()
    w = (b.view(rows, words, 32) << torch.arange(32)[None, None, :]).sum(-1)
    return ((w + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)


def chi2_quantile(df: int, z: float = 3.7190164854556804) -> float:
    """Wilson-Hilferty chi-square quantile; the default z is the normal 1 - 1e-4 quantile."""
    a = 2.0 / (9.0 * df)
    return df * (1.0 - a + z * math.sqrt(a)) ** 3


def pearson_chi2(counts: torch.Tensor, probs: torch.Tensor, min_expected: float = 5.0):
    """-> (chi2, cells): Pearson statistic of observed counts against probabilities; cells whose
    expected count is under ``min_expected`` are pooled into one."""
    c, p = counts.double().cpu(), probs.double().cpu()
    n = float(c.sum())
    e = p * n
    small = e < min_expected
    obs, exp = c[~small], e[~small]
    if bool(small.any()):
        obs = torch.cat([obs, c[small].sum()[None]])
        exp = torch.cat([exp, e[small].sum()[None]])
    return float(((obs - exp) ** 2 / exp).sum()), int(obs.numel())


# ============================================================================= attention oracle
# Per-key oracle of decode_mq_kernel ("mq"), decode_attn_kernel ("split") and flash_attn_kernel.
#
#     |got - o64| <= 2^-8 |o64| + c * A64        o64 = sum_t p_t v_t,   A64 = sum_t p_t |v_t|
#
# o64 is a float64 softmax attention over an explicit per-row key weighting (0: invisible,
# 1: visible) on the kernel's own score operand: mq and flash fold scale * log2(e) into Q and
# round it to bf16 before the MFMA (mq_attention.h make_qf, attention.hip flash Q^T fragments);
# the reference takes that very operand (f32 multiply, RNE: the same bits in torch on the CPU).
# The split kernel reads Q unrounded (f32 q * scale).  c from the code:
#   mq, flash: P is rounded to bf16 for the P.V MFMA (2^-9 per weight; the row sum l adds the
#              unrounded f32 P) + 2^-16 for the f32 accumulation and exp2f
#   split:     all-f32 VALU: 2^-16
# The 2^-9 is the rounding error of a weight just below a power of two; just above one it is 2^-8.
# So c holds where many keys share the weight (the errors are independent) and where the top key's
# P is exactly 1 (mq: the running max is the true max); it is NOT a worst case for a row whose
# weight sits on two or three keys of large |v|.  The input families keep away from such rows
# (SPIKE_W, RETRIEVAL_MISS_GAIN below say how and what was measured before they did); c is not
# raised for them.
# Largest deviation / A64 (deviation(): what the output rounding lets through) over every case of
# tests/test_attention_oracle_gpu.py on an MI355X (MEASURED attn_<kernel>_<family>), c = 1.97e-3
# for mq and flash, 1.53e-5 for split:
#             counting   retrieval   spiked
#   mq        0          1.16e-3     1.52e-3
#   flash     0          1.61e-3     1.37e-3
#   split     0          0           8.25e-8
# (counting: p = 1 exactly, every output the bf16 rounding of a ratio of counts; retrieval: the rows
# aiming at an invisible key, the others equal V[t*] bit for bit in mq and split)
# The folded-Q reference sits 1.7e-3 (hd 64) to 3.0e-3 (hd 128) x A64 from the exact-Q one on the
# spiked family (test_attention_oracle_cpu.py prints it): larger than everything else in the bound.
ATTN_C = {"mq": 2.0 ** -9 + 2.0 ** -16, "flash": 2.0 ** -9 + 2.0 ** -16, "split": 2.0 ** -16}
ATTN_FOLD = {"mq": True, "flash": True, "split": False}
LOG2E = 1.4426950408889634
FAMILIES = ("counting", "retrieval", "spiked")
BS = 16  # tokens per block of every paged case here


def q_operand(q: torch.Tensor, scale: float, fold: bool) -> torch.Tensor:
    """The score operand in log2 units (p = 2^(s - max)), float64.  fold: bf16_rne(f32(q) *
    (f32(scale) * 1.4426950408889634f)) as the MFMA kernels build it; else q * scale exactly."""
    if fold:
        qs = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
        return (q.detach().cpu().float() * qs).to(BF).double()
    return q.detach().cpu().double() * (float(scale) * LOG2E)


def _batches(kv_rows):
    """Runs of consecutive rows that share one (K, V) pair (rows of one sequence / one batch)."""
    i, n = 0, len(kv_rows)
    while i < n:
        j = i + 1
        while j < n and kv_rows[j][0] is kv_rows[i][0]:
            j += 1
        yield i, j, kv_rows[i][0], kv_rows[i][1]
        i = j


def _w3(w, i, j, Hq, T):
    ww = w[i:j, ..., :T]
    if ww.shape[-1] < T:
        ww = torch.nn.functional.pad(ww, (0, T - ww.shape[-1]))
    return (ww[:, None, :] if ww.dim() == 2 else ww).expand(j - i, Hq, T)


def attention64(qop: torch.Tensor, kv_rows, w: torch.Tensor, hmap):
    """Float64 softmax attention.  qop [R, Hq, D]: score operand in log2 units (q_operand);
    kv_rows: per row a (K, V) pair of float64 [Hkv, T, D] (gather64; rows of one sequence share
    the pair); w [R, T] or [R, Hq, T]: key weights (0 invisible, 1 visible, 2 counted twice);
    hmap [Hq]: kv head of each q head.  -> (o64, A64 [R, Hq, D], p64 [R, Hq, Tmax]); a row without
    a visible key gives zeros."""
    R, Hq, D = qop.shape
    hmap = torch.as_tensor(hmap, dtype=torch.long)
    Tmax = max(k.shape[1] for k, _ in kv_rows)
    o = torch.zeros(R, Hq, D, dtype=F64)
    A = torch.zeros(R, Hq, D, dtype=F64)
    p64 = torch.zeros(R, Hq, Tmax, dtype=F64)
    for i, j, K, V in _batches(kv_rows):
        T = K.shape[1]
        Kh, Vh = K[hmap], V[hmap]
        ww = _w3(w.to(F64), i, j, Hq, T)
        s = torch.einsum("nhd,htd->nht", qop[i:j], Kh).masked_fill(ww <= 0, -math.inf)
        m = s.amax(-1, keepdim=True)
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        p = ww * torch.exp2(s - m)
        l = p.sum(-1, keepdim=True)
        p = torch.where(l > 0, p / l.clamp(min=1e-300), torch.zeros_like(p))
        o[i:j] = torch.einsum("nht,htd->nhd", p, Vh)
        A[i:j] = torch.einsum("nht,htd->nhd", p, Vh.abs())
        p64[i:j, :, :T] = p
    return o, A, p64


def attention_emulated(qop: torch.Tensor, kv_rows, w: torch.Tensor, hmap, *, p_bf16: bool, n_chunks: int) -> torch.Tensor:
    """An honest f32 kernel: the given score operand, an online softmax over 32-key steps inside
    each of ``n_chunks`` key chunks (multiples of 32 keys), P rounded to bf16 for P.V when
    ``p_bf16`` (the row sum keeps the f32 P), f32 sums, the chunks merged in f32, one RNE rounding
    to bf16.  w holds 0 / 1 only.  -> bf16 [R, Hq, D]."""
    R, Hq, D = qop.shape
    hmap = torch.as_tensor(hmap, dtype=torch.long)
    f32 = torch.float32
    out = torch.zeros(R, Hq, D, dtype=f32)
    ninf = torch.tensor(-math.inf, dtype=f32)
    for i, j, K, V in _batches(kv_rows):
        T = K.shape[1]
        Kh, Vh = K[hmap].to(f32), V[hmap].to(f32)
        vis = _w3(w, i, j, Hq, T) > 0
        s = torch.einsum("nhd,htd->nht", qop[i:j].to(f32), Kh).masked_fill(~vis, -math.inf)
        n = j - i
        last = int(vis.any(0).any(0).nonzero().max()) + 1 if bool(vis.any()) else 0
        CL = max(32, -(-(-(-last // n_chunks)) // 32) * 32)
        M = torch.full((n, Hq, 1), -math.inf, dtype=f32)
        L = torch.zeros(n, Hq, 1, dtype=f32)
        O = torch.zeros(n, Hq, D, dtype=f32)
        for c0 in range(0, last, CL):
            m = torch.full((n, Hq, 1), -math.inf, dtype=f32)
            l = torch.zeros(n, Hq, 1, dtype=f32)
            acc = torch.zeros(n, Hq, D, dtype=f32)
            for k0 in range(c0, min(last, c0 + CL), 32):
                st = s[:, :, k0: k0 + 32]
                mn = torch.maximum(m, st.amax(-1, keepdim=True))
                ms = torch.where(torch.isfinite(mn), mn, torch.zeros_like(mn))
                alpha = torch.where(torch.isfinite(m), torch.exp2(m - ms), torch.zeros_like(m))
                p = torch.exp2(st - ms)  # exp2(-inf) = 0 for masked keys
                l = l * alpha + p.sum(-1, keepdim=True)
                pb = p.to(BF).to(f32) if p_bf16 else p
                acc = acc * alpha + torch.einsum("nht,htd->nhd", pb, Vh[:, k0: k0 + 32])
                m = mn
            Mn = torch.maximum(M, m)
            Ms = torch.where(torch.isfinite(Mn), Mn, torch.zeros_like(Mn))
            fo = torch.where(torch.isfinite(M), torch.exp2(M - Ms), torch.zeros_like(M))
            fc = torch.where(torch.isfinite(m), torch.exp2(m - Ms), torch.zeros_like(m))
            L = L * fo + l * fc
            O = O * fo + acc * fc
            M = Mn
        out[i:j] = torch.where(L > 0, O * (1.0 / L.clamp(min=1e-38)), torch.zeros_like(O))
    return out.to(BF)


def attn_slack(family: str, kernel: str, o64: torch.Tensor, A64: torch.Tensor) -> torch.Tensor:
    """The slack next to the output half-ulp: counting has p = 1 exactly (no P rounding): f32
    arithmetic alone, relative to the element; otherwise c * A64."""
    return F32_SLACK * o64.abs() if family == "counting" else ATTN_C[kernel] * A64


def attn_ratio(got: torch.Tensor, o64: torch.Tensor, slack: torch.Tensor) -> torch.Tensor:
    """[R, Hq]: the largest |got - o64| / bound over a (row, head)'s elements (inf for a NaN, or
    for a miss where the bound is 0)."""
    g = got.detach().to("cpu", F64).reshape(o64.shape)
    err = (g - o64).abs()
    bound = HALF_ULP[BF] * o64.abs() + slack
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    return torch.nan_to_num(r, nan=math.inf, posinf=math.inf).amax(-1)


def attn_measured(got: torch.Tensor, o64: torch.Tensor, A64: torch.Tensor) -> float:
    """Largest deviation / A64 (0 where A64 is 0)."""
    d = deviation(got.reshape(o64.shape), o64, BF)
    return float(torch.where(A64 > 0, d / A64.clamp(min=1e-300), torch.zeros_like(d)).max()) if d.numel() else 0.0


# ----------------------------------------------------------------------------- attention inputs
class AttnCase:
    """One set of inputs (CPU tensors; the GPU tests move the same tensors to the device).
    rows: ctx[r] visible keys of row r over sequence seqs[r]; Klog / Vlog[s]: the sequence's logical
    keys [nkv, cap_s, hd] (cap_s >= its longest context + 2: the keys past a context exist and carry
    the family's code, so a leak reads something); kc / vc / table: the same keys in a paged cache
    (16-token blocks in a random permutation; blocks no sequence owns and unused table entries hold
    a sentinel code, never zeros).  P / n_real: shared-prefix form (the first P keys of every
    session are the same physical blocks).  target[r, h]: the retrieval key (may be == ctx[r]: the
    first invisible key, which must NOT win)."""

    def paged(self, dev="cpu"):
        return ops.KVLayout.paged(self.kc.to(dev), self.vc.to(dev), self.table.to(dev))

    def contiguous(self, dev="cpu"):
        """[B, S, H, D] tensors (one block per sequence), S = the longest capacity; shorter
        sequences are padded with the sentinel code."""
        S = max(k.shape[1] for k in self.Klog)
        B = len(self.Klog)
        k = torch.empty(B, S, self.nkv, self.hd, dtype=BF)
        v = torch.empty(B, S, self.nkv, self.hd, dtype=BF)
        sk, sv = _sentinel_kv(self.family, self.nkv, S, self.hd, _gen(31, *self.key))
        for s in range(B):
            k[s], v[s] = sk.permute(1, 0, 2), sv.permute(1, 0, 2)
            n = self.Klog[s].shape[1]
            k[s, :n], v[s, :n] = self.Klog[s].permute(1, 0, 2), self.Vlog[s].permute(1, 0, 2)
        table = torch.arange(B, dtype=torch.int32).view(B, 1)
        return ops.KVLayout.contiguous(k.to(dev), v.to(dev), table.to(dev))

    @property
    def hmap(self):
        return torch.arange(self.nq) // (self.nq // self.nkv)

    def weights(self, ctx=None) -> torch.Tensor:
        """[R, Tmax] 0 / 1: key t of row r is visible when t < ctx[r]."""
        ctx = self.ctx if ctx is None else ctx
        T = max(k.shape[1] for k in self.Klog)
        return (torch.arange(T)[None, :] < torch.tensor(ctx)[:, None]).to(F64)

    def kv_rows(self, kv=None, seqs=None):
        """Per row (K, V) float64 [nkv, cap, hd], gathered on the CPU through the layout."""
        kv = self.paged() if kv is None else kv
        cache = {}
        for s in sorted(set(self.seqs if seqs is None else seqs)):
            cache[s] = gather64(kv, s, self.Klog[s].shape[1], self.nkv)
        return [cache[s] for s in (self.seqs if seqs is None else seqs)]

    def qop(self, kernel: str) -> torch.Tensor:
        return q_operand(self.q.view(len(self.ctx), self.nq, self.hd), self.scale, ATTN_FOLD[kernel])

    def reference(self, kernel: str, kv=None):
        """-> (o64, A64, p64) of the honest operation on this kernel's score operand."""
        return attention64(self.qop(kernel), self.kv_rows(kv), self.weights(), self.hmap)


def gather64(kv, seq: int, n: int, heads: int):
    K, V = ref._gather_kv_heads(kv, seq, n, heads)
    return K.double(), V.double()


def _count_code(t: torch.Tensor, D: int, shift: int) -> torch.Tensor:
    """[n, D] 0 / 1: the lower half of the dims counts 32-key steps, V[t][d] = 1 if (t // 32 + shift)
    % (D/2) == d; the upper half counts keys, V[t][D/2 + d] = 1 if (t + shift) % (D/2) == d."""
    half = D // 2
    v = torch.zeros(t.numel(), D)
    idx = torch.arange(t.numel())
    v[idx, (t // 32 + shift) % half] = 1.0
    v[idx, half + (t + shift) % half] = 1.0
    return v


def _pm1(shape, g):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def _sentinel_kv(family: str, nkv: int, n: int, hd: int, g):
    """What lies where no row may read: finite keys, and values in a code of their own (3 in the
    last bin of each half for counting, 5 elsewhere): never zeros."""
    if family == "spiked":
        k = torch.randn(nkv, n, hd, generator=g)
    else:
        k = _pm1((nkv, n, hd), g)
    if family == "counting":
        v = torch.zeros(nkv, n, hd)
        v[..., hd // 2 - 1] = 3.0
        v[..., hd - 1] = 3.0
    else:
        v = torch.full((nkv, n, hd), 5.0)
    return k.to(BF), v.to(BF)


def _family_kv(family: str, nkv: int, t0: int, t1: int, hd: int, code: int, g):
    """Keys t0 .. t1-1 of one sequence: K, V [nkv, t1 - t0, hd] (f32).  code: the sequence's own
    counting code (0: the shared prefix)."""
    n = t1 - t0
    t = torch.arange(t0, t1)
    if family == "counting":
        k = _pm1((nkv, n, hd), g)
        v = torch.stack([_count_code(t, hd, 5 * code + 3 * h) for h in range(nkv)])
    elif family == "retrieval":
        k = _pm1((nkv, n, hd), g)
        v = (torch.randint(1, 4, (nkv, n, hd), generator=g) * _pm1((nkv, n, hd), g)).float()
    else:
        assert family == "spiked", family
        k = torch.randn(nkv, n, hd, generator=g)
        v = torch.randn(nkv, n, hd, generator=g)
    return k, v


def retrieval_targets(ctx: int, P: int = 0):
    """Candidate keys of a row with ``ctx`` visible keys: the last visible key, the first invisible
    one (== ctx), key 0, 31, 32, both sides of every multiple of 128 below ctx (and of P)."""
    c = [ctx - 1, ctx, 0, 31, 32]
    for m in list(range(128, ctx, 128)) + ([P] if 0 < P < ctx else []):
        c += [m - 1, m]
    out = []
    for t in c:
        if 0 <= t <= ctx and t not in out:
            out.append(t)
    return out


SPIKE_W = 32.0
RETRIEVAL_GAIN = 16.0  # q = 16 K[t*]: a power of two, so q and the folded operand stay +-one value
# A target that is the first INVISIBLE key gets q = 1 K[t*]: were it read it would still take most of
# the weight (its score: sqrt(hd) log2(e) >= 11 in log2 units, against a spread of 1.4 among the
# others), but the honest softmax over the rest stays broad.  With the gain of 16 the rest is one
# or two random keys holding all the weight, and then the bf16 rounding of P alone (up to 2^-8
# relative, against c = 2^-9) decides: flash_attn_kernel, whose deferred max leaves even the top
# key's P off a power of two, measured 1.09 x the bound on such rows.
RETRIEVAL_MISS_GAIN = 1.0


def attn_case(family: str, hd: int, nq: int, nkv: int, ctx, seqs, *, key, P: int = 0, n_real=None,
              spare_blocks: int = 8) -> AttnCase:
    """Build one case.  ctx / seqs: per row.  key: ints that seed it (with family and shape)."""
    assert family in FAMILIES and P % BS == 0
    c = AttnCase()
    key = (FAMILIES.index(family), hd, nq, nkv) + tuple(key)
    g = _gen(21, *key)
    R = len(ctx)
    n_real = R if n_real is None else n_real
    nseq = max(seqs) + 1
    c.family, c.hd, c.nq, c.nkv, c.ctx, c.seqs, c.P, c.n_real, c.key = family, hd, nq, nkv, list(ctx), list(seqs), P, n_real, key
    c.scale = hd ** -0.5
    cmax = [max([P] + [n for n, s in zip(ctx, seqs) if s == q]) for q in range(nseq)]
    cmin = [min([n for n, s in zip(ctx, seqs) if s == q] or [P]) for q in range(nseq)]
    cap = [-(-(m + 2) // BS) * BS for m in cmax]
    # ---- logical keys
    pk, pv = _family_kv(family, nkv, 0, P, hd, 0, g) if P else (None, None)
    c.Klog, c.Vlog, c.edges = [], [], []
    for s in range(nseq):
        k, v = _family_kv(family, nkv, P, cap[s], hd, s + 1, g)
        if P:
            k, v = torch.cat([pk, k], 1), torch.cat([pv, v], 1)
        c.Klog.append(k)
        c.Vlog.append(v)
    if family == "spiked":
        # The edge keys: K[e, 0] = ln(max(ctx, SPIKE_W) / SPIKE_W) / (4 scale) against q[..., 0] = 4 and
        # V[e] = +-4, so one edge key carries about 1 / (1.8 SPIKE_W) of the weight (the unit-normal
        # keys average e^0.6 each) and moves an output by about 0.07 when it is lost: 5 to 10 x what
        # the bound allows.  Why not 1/8 of the weight each: P is rounded to bf16 with a relative error
        # of up to 2^-8 (mantissa just above a power of two; 2^-9 only just below the next one).  The
        # bound's c = 2^-9 is met on average over many keys, but the few edge keys' errors add
        # coherently in a quarter of the dims, so they must hold well under half of A64
        # (sum_e p_e |v_e| <= 0.4 x the rest) for an honest kernel to pass whatever its roundings.
        # Own keys only (>= P): the prefix is shared.
        for s in range(nseq):
            E = []
            for e in (0, 31, 32, cmin[s] - 1, cmin[s], cmax[s] - 2, cmax[s] - 1, cmax[s], cmax[s] + 1):
                if P <= e < cap[s] and e not in E and len(E) < 8:
                    E.append(e)
            c.edges.append(E)
            for e in E:
                # a quarter of the score noise on an edge key: its weight, which the mutants' margin
                # rests on, stays within about 1.6 x of the above (with none, all edge keys would share
                # one P and one rounding error of it)
                c.Klog[s][:, e] *= 0.25
                c.Klog[s][:, e, 0] = math.log(max(cmax[s], SPIKE_W) / SPIKE_W) / (4.0 * c.scale)
                c.Vlog[s][:, e] = 4.0 * _pm1((nkv, hd), g)
    c.Klog = [k.to(BF) for k in c.Klog]
    c.Vlog = [v.to(BF) for v in c.Vlog]
    # ---- queries
    G = nq // nkv
    c.target = None
    if family == "counting":
        q = torch.zeros(R, nq, hd)
    elif family == "spiked":
        q = torch.randn(R, nq, hd, generator=g)
        q[..., 0] = 4.0
    else:
        q = torch.empty(R, nq, hd)
        c.target = torch.empty(R, nq, dtype=torch.long)
        for r in range(R):
            cand = retrieval_targets(ctx[r], P) if ctx[r] > 0 else [0]
            for h in range(nq):
                t = cand[(r + h) % len(cand)]
                c.target[r, h] = t
                gain = RETRIEVAL_GAIN if t < ctx[r] else RETRIEVAL_MISS_GAIN
                q[r, h] = gain * c.Klog[seqs[r]][h // G, t].float()
    c.q = q.to(BF).reshape(R, nq * hd)
    # ---- the paged cache: shared prefix blocks, each sequence's own blocks, spare blocks
    n_own = [(cap[s] - P) // BS for s in range(nseq)]
    nblk = P // BS + sum(n_own) + spare_blocks
    perm = torch.randperm(nblk, generator=g)
    sk, sv = _sentinel_kv(family, nkv, nblk * BS, hd, g)
    c.kc = sk.view(nkv, nblk, BS, hd).permute(1, 0, 2, 3).contiguous()
    c.vc = sv.view(nkv, nblk, BS, hd).permute(1, 0, 2, 3).contiguous()
    width = max(cap) // BS
    c.table = torch.empty(nseq, width, dtype=torch.int32)
    nxt = P // BS
    for s in range(nseq):
        ids = torch.cat([perm[: P // BS], perm[nxt: nxt + n_own[s]]])
        nxt += n_own[s]
        c.table[s, : ids.numel()] = ids.to(torch.int32)
        c.table[s, ids.numel():] = perm[nblk - 1 - (s % spare_blocks)].to(torch.int32)  # a spare block
        first = 0 if s == 0 else P // BS  # (the shared blocks are written once, from session 0)
        for b in range(first, ids.numel()):
            c.kc[ids[b]] = c.Klog[s][:, b * BS: (b + 1) * BS]
            c.vc[ids[b]] = c.Vlog[s][:, b * BS: (b + 1) * BS]
    return c


# ----------------------------------------------------------------------------- attention case tables
# Shared by tests/test_attention_oracle_cpu.py (an honest emulation passes, mutants fail, on these
# very inputs) and tests/test_attention_oracle_gpu.py (the kernels), so the two cannot drift.
ATTN_SHAPES = ((128, 8, 2), (64, 2, 2), (64, 16, 2), (128, 16, 1))  # (hd, nq, nkv); G = 4, 1, 8, 16
SWEEP_CTX = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513)
GROUP_STARTS = (30, 126, 254)
GROUP_PARTS = (0, 1)  # run lengths (RG - 1, RG, RG + 1) | (2 RG + 1,): <= 64 rows per launch
ZERO_SHAPES = ((128, 8, 2), (64, 2, 2))
ZERO_KINDS = ("inside", "group")
ROWS_SLICED = (65, 130)
SHARED_SHAPES = ((128, 8, 2), (64, 16, 2))
SHARED_P = (32, 160, 512)
SHARED_SESS = (3, 17)
SHARED_OWN = (0, 1, 33, 129)  # own keys past P, by session (0: the context ends exactly at P)
SHARED_MAX_CTX = 1024  # 8 partial slots > RG: the cascade is on
FLASH_SHAPES = ((64, 2, 2), (128, 4, 1))
FLASH_NONCAUSAL = ((1, 1), (31, 63), (33, 64), (127, 65), (128, 129), (129, 193), (1, 193), (129, 1))  # (Sq, Sk)
FLASH_CAUSAL = ((1, 1), (65, 65), (129, 129), (200, 200), (77, 300), (1, 129), (64, 192))  # q_offset = Sk - Sq
# ("direct": k_lens below q_offset + run length, so k_lens and not the causal mask ends runs 0 and 1)
FLASH_RUNS = {"direct": dict(S=40, lens=(40, 17, 1), q_offsets=(60, 20, 0), k_lens=(90, 30, 1)),
              "runs": dict(S=40, lens=(40, 17, 1), q_offsets=(60, 0, 0), k_lens=(100, 17, 1))}


def shape_id(shape) -> str:
    return "hd%d-q%d-kv%d" % tuple(shape)


def sweep_case(family, shape) -> AttnCase:
    """20 single-row sequences, each with its own blocks."""
    return attn_case(family, *shape, SWEEP_CTX, range(len(SWEEP_CTX)), key=(1,))


def group_case(family, shape, start, part) -> AttnCase:
    """Runs of one sequence with consecutive contexts from ``start`` (rows of one group differ in
    which keys of the last step / last wave range they see), a single-row sequence between runs."""
    RG = 16 // (shape[1] // shape[2])
    ctx, seqs, s = [], [], 0
    for n in ((RG - 1, RG, RG + 1) if part == 0 else (2 * RG + 1,)):
        if n < 1:
            continue
        ctx += list(range(start, start + n))
        seqs += [s] * n
        ctx.append(start + 47)
        seqs.append(s + 1)
        s += 2
    assert len(ctx) <= 64
    return attn_case(family, *shape, ctx, seqs, key=(2, start, part))


def zero_case(family, shape, kind) -> AttnCase:
    """ctx_len == 0: a zero-context row inside a group of live rows | a group of such rows only."""
    if kind == "inside":
        ctx, seqs = [33, 0, 34, 20], [0, 0, 0, 1]
    else:
        ctx, seqs = [20, 0, 0, 33], [0, 1, 1, 2]
    return attn_case(family, *shape, ctx, seqs, key=(3, ZERO_KINDS.index(kind)))


def multi_item_case(family) -> AttnCase:
    """64 single-row sequences x 20 kv heads: 1280 work items on the mq kernel's 512 workgroups."""
    return attn_case(family, 64, 20, 20, [1 + (i * 199) // 63 for i in range(64)], range(64), key=(4,))


def sliced_case(rows: int) -> AttnCase:
    """More rows than one launch takes (decode_attention_rows slices at 64)."""
    return attn_case("counting", 128, 8, 2, [1 + (i * 37) % 400 for i in range(rows)], range(rows), key=(5, rows))


def shared_case(family, shape, P, n_sess) -> AttnCase:
    """Sessions over one cached prefix of P keys (the same physical blocks).  Session 2 is a
    jump-forward run of 3 rows (rows 2..4: it straddles the 4-row group cut of G = 4); 3 padded rows
    (sequence 0, one key) behind the n_real real ones."""
    ctx, seqs = [], []
    for s in range(n_sess):
        own = SHARED_OWN[s % 4]
        for o in ((own, own + 1, own + 2) if s == 2 else (own,)):
            ctx.append(P + o)
            seqs.append(s)
    n_real = len(ctx)
    return attn_case(family, *shape, ctx + [1, 1, 1], seqs + [0, 0, 0], key=(6, P, n_sess), P=P, n_real=n_real)


def flash_case(family, shape, Sq, Sk, causal, B=2) -> AttnCase:
    """Flash attention as rows: row b * Sq + i is query i of batch b over sequence b; it sees Sk keys,
    or under the causal mask with q_offset = Sk - Sq the keys 0 .. q_offset + i."""
    ctx = [(Sk - Sq + i + 1) if causal else Sk for _ in range(B) for i in range(Sq)]
    seqs = [b for b in range(B) for _ in range(Sq)]
    c = attn_case(family, *shape, ctx, seqs, key=(7, Sq, Sk, int(causal)))
    c.B, c.Sq, c.Sk, c.causal, c.q_offset = B, Sq, Sk, causal, (Sk - Sq if causal else 0)
    return c


def flash_runs_case(family, shape, form) -> AttnCase:
    """Per-batch causal form: B = 3 runs in an S-query block, run b at absolute offset q_offsets[b]
    with k_lens[b] keys; queries past lens[b] are padding (computed, never compared)."""
    f = FLASH_RUNS[form]
    S, B = f["S"], len(f["lens"])
    ctx = [min(f["k_lens"][b], f["q_offsets"][b] + i + 1) for b in range(B) for i in range(S)]
    seqs = [b for b in range(B) for _ in range(S)]
    c = attn_case(family, *shape, ctx, seqs, key=(8, list(FLASH_RUNS).index(form)))
    c.B, c.Sq, c.Sk, c.causal = B, S, max(f["k_lens"]), True
    c.q_offsets, c.k_lens, c.lens = list(f["q_offsets"]), list(f["k_lens"]), list(f["lens"])
    c.real = torch.tensor([i < f["lens"][b] for b in range(B) for i in range(S)])
    return c


def decode_kernels(shape):
    """The split kernel has no G = 16."""
    return ("mq",) if shape[1] // shape[2] == 16 else ("mq", "split")


def attn_cases():
    """Every case of the GPU file: id -> (kernels that run it, builder).  The GPU tests take their
    parameters from these ids; the CPU test walks all of them."""
    out = {}

    def add(cid, kernels, fn, *a):
        out[cid] = (kernels, lambda: fn(*a))

    for sh in ATTN_SHAPES:
        for fam in FAMILIES:
            add(f"sweep-{fam}-{shape_id(sh)}", decode_kernels(sh), sweep_case, fam, sh)
        for fam in ("counting", "spiked"):
            for st in GROUP_STARTS:
                for part in GROUP_PARTS:
                    add(f"group-{fam}-{shape_id(sh)}-{st}-{part}", decode_kernels(sh), group_case, fam, sh, st, part)
    for sh in ZERO_SHAPES:
        for fam in ("counting", "spiked"):
            for kind in ZERO_KINDS:
                add(f"zero-{fam}-{shape_id(sh)}-{kind}", decode_kernels(sh), zero_case, fam, sh, kind)
    for fam in ("counting", "retrieval"):
        add(f"multi-{fam}", ("mq",), multi_item_case, fam)
    for n in ROWS_SLICED:
        add(f"sliced-{n}", ("mq", "split"), sliced_case, n)
    for sh in SHARED_SHAPES:
        for fam in ("counting", "retrieval"):
            for P in SHARED_P:
                for ns in SHARED_SESS:
                    add(f"shared-{fam}-{shape_id(sh)}-P{P}-s{ns}", ("mq",), shared_case, fam, sh, P, ns)
    for sh in FLASH_SHAPES:
        for fam in FAMILIES:
            for sq, sk in FLASH_NONCAUSAL:
                add(f"flash-{fam}-{shape_id(sh)}-{sq}x{sk}", ("flash",), flash_case, fam, sh, sq, sk, False)
            if fam == "spiked":  # (its edge keys are sized for ONE context per sequence)
                continue
            for sq, sk in FLASH_CAUSAL:
                add(f"causal-{fam}-{shape_id(sh)}-{sq}x{sk}", ("flash",), flash_case, fam, sh, sq, sk, True)
            for form in FLASH_RUNS:
                add(f"runs-{fam}-{shape_id(sh)}-{form}", ("flash",), flash_runs_case, fam, sh, form)
    return out


def attn_ids(prefix: str):
    return [k for k in attn_cases() if k.startswith(prefix + "-")]


def check_attention(c: AttnCase, kernel: str, got: torch.Tensor, what: str, rows=None, refs=None) -> float:
    """Compare one kernel output [R, nq * hd] with the oracle under the family's rule and return
    the largest deviation / A64: counting and spiked under the elementwise bound; retrieval rows
    whose target is visible must equal V[t*] bit for bit in the decode kernels (the winner's P is
    exp2(0) = 1), under the elementwise bound in flash (deferred max: P is no power of two) and
    where the target is the first invisible key (it must not win).  rows: bool mask of the rows
    that are compared."""
    o64, A64, _ = c.reference(kernel) if refs is None else refs
    R = len(c.ctx)
    g = got.detach().cpu().reshape(R, c.nq, c.hd)
    keep = torch.ones(R, dtype=torch.bool) if rows is None else rows
    slack = attn_slack(c.family, kernel, o64, A64)
    if c.family == "retrieval" and kernel != "flash":
        hit = (c.target < torch.tensor(c.ctx)[:, None]) & keep[:, None]  # [R, nq]
        if bool(hit.any()):
            assert_bitwise(g[hit], o64[hit], out_dtype=BF, what=what + " (visible targets, bitwise)")
        keep2 = (~hit) & keep[:, None]
        if bool(keep2.any()):
            assert_elementwise(g[keep2], o64[keep2], slack=slack[keep2], out_dtype=BF, what=what + " (invisible targets)")
    else:
        assert_elementwise(g[keep], o64[keep], slack=slack[keep], out_dtype=BF, what=what)
    return attn_measured(g[keep], o64[keep], A64[keep])
