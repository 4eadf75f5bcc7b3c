"""The per-element oracle (tests/kernel_oracle.py) is itself tested, without a GPU.

* Honest outputs pass: for every kernel family and input regime of tests/test_small_kernels_gpu.py
  the plain float32 computation, rounded to the output type, passes ``assert_elementwise`` against
  the float64 reference.  That is the condition that the chosen inputs and slacks are fair.
* Mutated references fail: each subtly wrong kernel of the second half of this file is rejected.

OLD_CLOSE_ACCEPTS records which of those mutations the whole-tensor criterion of
tests/test_kernels_gpu.py (``close``: atol + 2e-2 * max|ref| for every element) lets through; the
table is asserted, so it cannot go stale.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_oracle as ko
from voice_enabled_browser_automation_amd import ops
from voice_enabled_browser_automation_amd.ops import reference as ref

BF = torch.bfloat16
EPS = ko.EPS
DS = (8, 384, 520, 1280, 4096, 8192)

# mutation -> accepted by the old close() at the atol the old test of that family used
OLD_CLOSE_ACCEPTS = {
    "rmsnorm_eps_dropped": False,       # (the tiny regime triples every output: even close() sees it)
    "layernorm_eps_dropped": False,
    "rmsnorm_mean_div_512": False,      # (D = 1280 -> 1536: every output 9.5 % large)
    "layernorm_mean_div_512": True,     # (a unit row's mean is near 0: the error is a small shift)
    "w_shifted_8_in_chunk": False,
    "one_element_1pct": True,
    "last_row_unwritten": False,
    "swiglu_gate_up_swapped": True,     # (one saturated gate makes max|ref| 1e4: the tolerance is 200)
    "rope_k_sin_flipped": False,
    "embedding_off_by_one_row": False,
    "pcm_positions_f32_22050": False,   # (over a whole 30 s window; the old test ran ratio 1 only)
    "pcm_positions_f32_44100": False,
}


def rejected(got, ref64, *, slack, out_dtype) -> bool:
    try:
        ko.assert_elementwise(got, ref64, slack=slack, out_dtype=out_dtype)
    except AssertionError:
        return True
    return False


# ----------------------------------------------------------------------------- the comparator itself
def test_rne_is_a_single_rounding():
    # 1 + 2^-8 + 2^-30: above the bf16 midpoint; f32 rounds it onto the midpoint, then half-to-even goes down
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.0, 3e-40, math.inf],
                     dtype=torch.float64)
    got = ko.rne(x, BF).double()
    assert got.tolist()[:3] == [1.0 + 2.0 ** -7, 1.0, 1.0 + 2.0 ** -6]
    assert x.float().to(BF).double()[0] == 1.0  # the double rounding this avoids
    assert got[4] == 2.0 ** -133 * round(3e-40 / 2.0 ** -133) and got[5] == math.inf


def test_assert_elementwise_bounds_and_report():
    r = torch.tensor([[1.0, -2.0, 0.0, 100.0]], dtype=torch.float64)
    ko.assert_elementwise(ko.rne(r, BF), r, slack=0.0, out_dtype=BF)
    ko.assert_elementwise(r.float(), r, slack=0.0, out_dtype=torch.float32)
    g = r.clone()
    g[0, 3] = 100.5  # > 2^-8 * 100
    with pytest.raises(AssertionError, match=r"worst at \(0, 3\).*100\.5.*ref64 100\.0"):
        ko.assert_elementwise(g.to(BF), r, slack=0.0, out_dtype=BF)
    ko.assert_elementwise(g.to(BF), r, slack=torch.tensor([[0, 0, 0, 0.2]]), out_dtype=BF)  # per-element slack
    g = r.float().clone()
    g[0, 2] = math.nan
    assert rejected(g, r, slack=1e9, out_dtype=torch.float32)  # a NaN never passes
    g[0, 2] = 1e-7
    assert rejected(g, r, slack=0.0, out_dtype=torch.float32) and not rejected(g, r, slack=2e-7, out_dtype=torch.float32)
    with pytest.raises(AssertionError, match="dtype"):
        ko.assert_elementwise(r.float(), r, slack=0.0, out_dtype=BF)
    inf = torch.tensor([-math.inf], dtype=torch.float64)
    ko.assert_elementwise(inf.float(), inf, slack=0.0, out_dtype=torch.float32)
    assert rejected(torch.zeros(1), inf, slack=0.0, out_dtype=torch.float32)


def test_canary_sees_writes_outside_the_view():
    for cols in ((0, 0), (8, 16)):
        view, check = ko.canary((3, 16), rows=(2, 1), cols=cols)
        assert view.shape == (3, 16) and bool(ko.untouched(view).all())
        view.fill_(1.0)
        check()
        base = view._base
        base[view.shape[0] + 2, cols[0]] = 0.0  # the row after the view
        with pytest.raises(AssertionError, match="outside"):
            check()
    view, check = ko.canary((3, 16))
    assert view.is_contiguous()


# ----------------------------------------------------------------------------- honest f32 outputs pass
def _f32_rmsnorm(x, r, w, with_res, with_w):
    D = x.shape[1]
    ro = torch.empty_like(x) if with_res else None
    y = ref.rmsnorm(x, w if with_w else None, eps=EPS, residual=r if with_res else None, residual_out=ro,
                    out=torch.empty(x.shape[0], D, dtype=BF))
    return y, ro


def _f32_layernorm(x, r, w, b, with_res):
    """Two-pass f32 mean / variance, as the kernel computes them."""
    v = x.float() + r.float() if with_res else x.float()
    mu = v.mean(-1, keepdim=True)
    d = v - mu
    y = d * torch.rsqrt(d.pow(2).mean(-1, keepdim=True) + EPS) * w.float() + b.float()
    return y.to(BF), (v.to(BF) if with_res else None)


@pytest.mark.parametrize("regime", ko.REGIMES)
@pytest.mark.parametrize("D", DS)
def test_honest_norms_pass(regime, D):
    for rows in (1, 4, 5, 9):
        x, r, w, b = ko.norm_case(regime, rows, D)
        for with_res in (False, True):
            y, ro = _f32_rmsnorm(x, r, w, with_res, True)
            y64, r64 = ko.rmsnorm64(x, w, EPS, r if with_res else None)
            ko.assert_elementwise(y, y64, slack=ko.row_slack(y64), out_dtype=BF, what="rmsnorm")
            y, ro2 = _f32_layernorm(x, r, w, b, with_res)
            y64, _ = ko.layernorm64(x, w, b, EPS, r if with_res else None)
            ko.assert_elementwise(y, y64, slack=ko.row_slack(y64), out_dtype=BF, what="layernorm")
            if with_res:
                ko.assert_bitwise(ro, r64, out_dtype=BF, what="rmsnorm residual_out")
                ko.assert_bitwise(ro2, r64, out_dtype=BF, what="layernorm residual_out")
        y, _ = _f32_rmsnorm(x, r, w, False, False)
        y64, _ = ko.rmsnorm64(x, None, EPS)
        ko.assert_elementwise(y, y64, slack=ko.row_slack(y64), out_dtype=BF, what="rmsnorm w=None")
        rs = torch.rsqrt(x.float().pow(2).mean(-1) + EPS)
        r64 = ko.rstd64(x, EPS)
        ko.assert_elementwise(rs, r64, slack=ko.C_RSQRT * r64.abs(), out_dtype=torch.float32, what="rstd")


def test_zero_rows_are_exact_in_the_reference():
    x, r, w, b = ko.norm_case("zero_row", 5, 520)
    y64, _ = ko.rmsnorm64(x, w, EPS)
    assert bool((y64[2] == 0).all())
    y64, _ = ko.layernorm64(x, w, b, EPS)
    assert torch.equal(y64[2], b.double())


@pytest.mark.parametrize("F_", [16, 48, 14336])
def test_honest_swiglu_passes(F_):
    for rows in (1, 3, 70):
        gu = ko.swiglu_case(rows, F_)
        t = gu.float().view(rows, F_ // 16, 2, 16)
        h = (F.silu(t[:, :, 0, :]) * t[:, :, 1, :]).reshape(rows, F_).to(BF)
        h64 = ko.swiglu64(gu)
        assert bool(torch.isfinite(h64).all()) and bool(torch.isfinite(h.float()).all())
        ko.assert_elementwise(h, h64, slack=ko.C_SILU * h64.abs(), out_dtype=BF, what="swiglu")


@pytest.mark.parametrize("N", [8, 24, 5120])
def test_honest_bias_act_passes(N):
    for rows in (1, 5, 70):
        x, b, r = ko.bias_act_case(rows, N)
        _honest_bias_act(x, b, r)


def _honest_bias_act(x, b, r):
    for act in (0, 1):
        for wb in (False, True):
            for wr in (False, True):
                v = x.float() + b.float() if wb else x.float()
                y = F.gelu(v) if act else v
                y = (y + r.float() if wr else y).to(BF)
                y64, pre = ko.bias_act64(x, b if wb else None, r if wr else None, act)
                ko.assert_elementwise(y, y64, slack=ko.bias_act_slack(y64, pre, act), out_dtype=BF,
                                      what=f"bias_act act={act} bias={wb} residual={wr}")
                if not act and not (wb and wr):
                    ko.assert_bitwise(y, y64, out_dtype=BF)  # a copy or one exact f32 sum


@pytest.mark.parametrize("D", [8, 384, 4096])
def test_honest_embedding_passes_and_shards_sum(D):
    table, pos_table, ids, positions = ko.embedding_case(D)
    for pt in (None, pos_table):
        out = ref.embedding(ids, table, pos_table=pt, positions=positions, vocab_start=1000,
                            out=torch.empty(ids.numel(), D, dtype=BF))
        e64 = ko.embedding64(ids, table, 1000, pt, positions)
        ko.assert_elementwise(out, e64, slack=ko.row_slack(e64), out_dtype=BF, what="embedding")
        # (ref.embedding multiplies the rows outside the shard by 0: -0 where the kernel writes +0)
        ko.assert_bitwise(out + torch.zeros((), dtype=BF), e64, out_dtype=BF)
    assert bool((ko.embedding64(ids, table, 1000)[[0, 3, 4, 6, 7]] == 0).all())  # ids outside the shard


@pytest.mark.parametrize("hd,nq,nkv", [(64, 8, 2), (128, 6, 6)])
def test_honest_rope_passes(hd, nq, nkv):
    qkv, positions, rope = ko.rope_case(hd, nq, nkv)
    M, H = qkv.shape[0], nq + 2 * nkv
    y = ops.unpermute_qkv_cols(qkv.float(), H, hd).view(M, H, hd)
    q = ref._apply_rope(y[:, :nq], positions, rope).to(BF)
    k = ref._apply_rope(y[:, nq: nq + nkv], positions, rope).to(BF)
    q64, k64, v64 = ko.rope64(qkv, nq, nkv, hd, positions, rope)
    for got, want in ((q, q64), (k, k64)):
        ko.assert_elementwise(got.reshape(M, -1), want.reshape(M, -1), slack=ko.row_slack(want.reshape(M, -1)),
                              out_dtype=BF, what="rope")
    q0, k0, v0 = ko.rope64(qkv, nq, nkv, hd, positions, None)
    ko.assert_bitwise(y[:, nq + nkv:].to(BF), v64, out_dtype=BF)
    assert torch.equal(q0, y[:, :nq].double()) and torch.equal(v0, v64)


@pytest.mark.parametrize("rate", [8000, 22050, 44100, 48000])
def test_honest_pcm_passes(rate):
    pcm = ko.pcm_case(rate, 48000)
    out = ref.pcm16_to_f32(pcm, rate / 16000.0, torch.empty(48000))
    p64 = ko.pcm64(pcm, rate, 48000)
    ko.assert_elementwise(out, p64, slack=1e-6, out_dtype=torch.float32, what="pcm")
    last = (48000 - 1) * (rate / 16000.0)
    assert int(last) == pcm.numel() - 1  # the last output's second tap is clamped


def test_honest_sampler_keys_pass():
    g = torch.Generator().manual_seed(3)
    lg = torch.randn(1000, generator=g) * 3
    for row, step in ((0, 0), (5, 77)):
        k32 = ref.gumbel_keys(lg, 0.7, 1234, step, row)
        k64 = ko.gumbel_keys64(lg, 0.7, 1234, step, row)
        ko.assert_elementwise(k32, k64, slack=ko.C_KEY, out_dtype=torch.float32, what="gumbel keys")
    shard = ko.gumbel_keys64(lg[320:672], 0.7, 1234, 0, 0, v_offset=320)
    assert torch.equal(shard, ko.gumbel_keys64(lg, 0.7, 1234, 0, 0)[320:672])  # noise follows the global id
    bits = torch.rand(3, 1000, generator=g) < 0.3
    m = ko.pack_mask(bits)
    assert m.shape == (3, 32) and torch.equal(ko.mask_bits(m[1], 1000), bits[1])
    assert torch.equal(ko.mask_bits(m[1], 352, 320), bits[1, 320:672])


def test_chi2_reference_distribution():
    """The distribution test's statistic on the CPU reference sampler: V = 37, 64 identical rows,
    T = 0.7, 2000 steps.  The honest sampler is accepted; one that draws at T = 0.8, and one whose
    rows share their noise, are not."""
    V, rows, steps, T = 37, 64, 2000, 0.7
    lg = torch.randn(V, generator=torch.Generator().manual_seed(5)) * 2
    probs = torch.softmax(lg.double() / T, 0)
    ids = np.arange(V)
    u = np.stack([ko.uniforms(1234, s, r, ids) for s in range(steps) for r in range(rows)])  # [steps * rows, V]
    noise = torch.from_numpy(-np.log(-np.log(u)))
    toks = (lg.double()[None] / T + noise).argmax(-1)
    chi2, cells = ko.pearson_chi2(torch.bincount(toks, minlength=V), probs)
    limit = ko.chi2_quantile(cells - 1)
    print(f"reference chi2 {chi2:.2f} over {cells} cells, limit {limit:.2f}")
    assert cells == 26 and 59.0 < limit < 62.0
    assert abs(chi2 - 36.96) < 0.01, chi2
    assert chi2 < limit
    wrong_t = (lg.double()[None] / 0.8 + noise).argmax(-1)
    assert ko.pearson_chi2(torch.bincount(wrong_t, minlength=V), probs)[0] > limit
    shared = (lg.double()[None] / T + noise.view(steps, rows, V)[:, :1].expand(steps, rows, V).reshape(-1, V)).argmax(-1)
    assert ko.pearson_chi2(torch.bincount(shared, minlength=V), probs)[0] > limit


# ----------------------------------------------------------------------------- mutated references fail
def _mut_norm(kind, D, regime="unit", rows=5):
    """-> (mutant bf16, honest bf16, ref64, slack) for rmsnorm / layernorm mutations."""
    x, r, w, b = ko.norm_case(regime, rows, D)
    xf = x.float()
    if kind.startswith("rmsnorm"):
        y64, _ = ko.rmsnorm64(x, w, EPS)
        honest, _ = _f32_rmsnorm(x, r, w, False, True)
        if kind == "rmsnorm_eps_dropped":
            m = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True)) * w.float()
        elif kind == "rmsnorm_mean_div_512":
            Dp = (D + 511) // 512 * 512
            m = xf * torch.rsqrt(xf.pow(2).sum(-1, keepdim=True) / Dp + EPS) * w.float()
    else:
        y64, _ = ko.layernorm64(x, w, b, EPS)
        honest, _ = _f32_layernorm(x, r, w, b, False)
        mu = xf.mean(-1, keepdim=True)
        if kind == "layernorm_eps_dropped":
            d = xf - mu
            m = d * torch.rsqrt(d.pow(2).mean(-1, keepdim=True)) * w.float() + b.float()
        elif kind == "layernorm_mean_div_512":
            Dp = (D + 511) // 512 * 512
            d = xf - xf.sum(-1, keepdim=True) / Dp
            m = d * torch.rsqrt(d.pow(2).mean(-1, keepdim=True) + EPS) * w.float() + b.float()
    return m.to(BF), honest, y64, ko.row_slack(y64)


def _check_mutation(name, mutant, honest, ref64, slack, *, out_dtype=BF, old_atol=3e-2):
    assert not rejected(honest, ref64, slack=slack, out_dtype=out_dtype), f"{name}: the honest output must pass"
    assert rejected(mutant, ref64, slack=slack, out_dtype=out_dtype), f"{name}: mutation not rejected"
    assert ko.old_close_accepts(mutant, honest, old_atol) == OLD_CLOSE_ACCEPTS[name], \
        f"{name}: the record of what close() accepts is out of date"


@pytest.mark.parametrize("name", ["rmsnorm_eps_dropped", "layernorm_eps_dropped"])
def test_mutation_eps_dropped(name):
    _check_mutation(name, *_mut_norm(name, 1280, regime="tiny"))


@pytest.mark.parametrize("name", ["rmsnorm_mean_div_512", "layernorm_mean_div_512"])
def test_mutation_mean_divided_by_padded_d(name):
    for D in (8, 520, 1280):  # (384 -> 512 and 520 -> 1024 likewise; 4096 and 8192 are multiples of 512)
        for regime in ("unit", "offset"):
            m, h, y64, s = _mut_norm(name, D, regime)
            assert rejected(m, y64, slack=s, out_dtype=BF), (name, D, regime)
    _check_mutation(name, *_mut_norm(name, 1280, "unit"))


def test_mutation_w_shifted_by_8_columns_in_one_chunk():
    x, r, w, b = ko.norm_case("unit", 5, 1280)
    wm = w.clone()
    wm[512:1024] = torch.roll(w[512:1024], 8)
    y64, _ = ko.rmsnorm64(x, w, EPS)
    honest, _ = _f32_rmsnorm(x, r, w, False, True)
    mutant, _ = _f32_rmsnorm(x, r, wm, False, True)
    _check_mutation("w_shifted_8_in_chunk", mutant, honest, y64, ko.row_slack(y64))


def test_mutation_one_element_off_by_one_percent():
    x, r, w, b = ko.norm_case("unit", 9, 4096)
    y64, _ = ko.rmsnorm64(x, w, EPS)
    honest, _ = _f32_rmsnorm(x, r, w, False, True)
    f = ref.rmsnorm(x, w, eps=EPS, out=torch.empty(9, 4096))  # f32 output
    # a typical element (|y| about 1), a large and a small one: 1 % is 2.6 half-ulps of bf16 at any size
    for (i, j) in ((4, 100), (0, int(y64[0].abs().argmax())), (8, int((y64[8].abs() - 0.05).abs().argmin()))):
        m = f.clone()
        m[i, j] *= 1.01
        assert rejected(m.to(BF), y64, slack=ko.row_slack(y64), out_dtype=BF), (i, j)
    m = f.clone()
    m[4, 100] *= 1.01
    _check_mutation("one_element_1pct", m.to(BF), honest, y64, ko.row_slack(y64))


def test_mutation_last_row_left_unwritten():
    x, r, w, b = ko.norm_case("unit", 5, 384)
    y64, _ = ko.layernorm64(x, w, b, EPS)
    honest, _ = _f32_layernorm(x, r, w, b, False)
    for stale in (ko.SENTINEL, 0.0):
        mutant = honest.clone()
        mutant[-1] = stale
        assert rejected(mutant, y64, slack=ko.row_slack(y64), out_dtype=BF)
    _check_mutation("last_row_unwritten", mutant, honest, y64, ko.row_slack(y64))


def test_mutation_swiglu_gate_and_up_swapped_in_one_tile():
    gu = ko.swiglu_case(3, 48)
    gm = gu.clone().view(3, 3, 2, 16)
    gm[:, 1] = gm[:, 1].flip(1)  # tile 1: [up | gate]
    h64 = ko.swiglu64(gu)
    honest = ko.rne(h64, BF)
    mutant = ko.rne(ko.swiglu64(gm.view(3, 96)), BF)
    _check_mutation("swiglu_gate_up_swapped", mutant, honest, h64, ko.C_SILU * h64.abs())


def test_mutation_rope_sin_sign_flipped_for_k_only():
    hd, nq, nkv = 64, 8, 2
    qkv, positions, rope = ko.rope_case(hd, nq, nkv)
    M = qkv.shape[0]
    q64, k64, _ = ko.rope64(qkv, nq, nkv, hd, positions, rope)
    qm, km, _ = ko.rope64(qkv, nq, nkv, hd, positions, rope, k_sin_sign=-1.0)
    assert torch.equal(qm, q64)
    k64, km = k64.reshape(M, -1), km.reshape(M, -1)
    _check_mutation("rope_k_sin_flipped", ko.rne(km, BF), ko.rne(k64, BF), k64, ko.row_slack(k64))
    # position 0 rotates nothing: only the rows at other positions can tell
    assert torch.equal(km[1], k64[1]) and not torch.equal(km[0], k64[0])


def test_mutation_embedding_off_by_one_row_at_the_shard_edge():
    table, pos_table, ids, positions = ko.embedding_case(384)
    e64 = ko.embedding64(ids, table, 1000, pos_table, positions)
    # a kernel that admits vs < id <= ve and reads row id - vs - 1
    m64 = ko.embedding64(ids - 1, table, 1000, pos_table, positions)
    _check_mutation("embedding_off_by_one_row", ko.rne(m64, BF), ko.rne(e64, BF), e64, ko.row_slack(e64), old_atol=1e-2)


def test_mutation_resample_positions_in_float32():
    """What pcm_kernel computed before the read position moved to f64: over a 30 s window the f32
    product i * ratio is up to 0.1 sample off at 44.1 kHz, a few per cent of a 3 kHz tone."""
    worst = {}
    for rate in (8000, 22050, 44100, 48000):
        pcm = ko.pcm_case(rate)
        p64 = ko.pcm64(pcm, rate, ko.PCM_OUT)
        m = ko.pcm64(pcm, rate, ko.PCM_OUT, pos_dtype=np.float32).float()
        worst[rate] = float((m.double() - p64).abs().max())
        if rate in (22050, 44100):
            honest = ref.pcm16_to_f32(pcm, rate / 16000.0, torch.empty(ko.PCM_OUT))
            _check_mutation(f"pcm_positions_f32_{rate}", m, honest, p64, 1e-6, out_dtype=torch.float32, old_atol=1e-6)
            # the error grows with the index: a short buffer shows a small fraction of it
            assert float((m[:2000].double() - p64[:2000]).abs().max()) < worst[rate] / 20
        else:  # i / 2 and 3 i are exact in f32
            assert not rejected(m, p64, slack=1e-6, out_dtype=torch.float32)
    print("f32 read positions, worst output error:", worst)
    assert worst[44100] > 5e-3 and worst[22050] > 2e-3
