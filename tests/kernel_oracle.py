"""Per-element float64 oracle for the small kernels (norms, element-wise, embedding, rope, PCM, sampler).

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
