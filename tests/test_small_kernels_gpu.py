"""Per-element oracle tests of the small kernels: norms, swiglu, bias_act, embedding, rope_kv_write,
decode_advance, fp8 row quantiser, PCM resampler and the sampler.

Every output is compared element by element with a float64 computation of the same operation on
the same inputs (tests/kernel_oracle.py: |got - ref64| <= half an ulp of the output type + a slack
from f32 arithmetic, or a measured constant where an approximate intrinsic sits in the path).
tests/test_kernel_oracle_cpu.py shows, without a GPU, that honest f32 outputs pass on exactly
these inputs and that subtly wrong kernels do not.  Each test prints the figures it measures
(``MEASURED name value``; run with -s) before it asserts.
"""
import math

import pytest
import torch

import kernel_oracle as ko
import voice_enabled_browser_automation_amd.ops as ops
from voice_enabled_browser_automation_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
F32 = torch.float32
I32 = torch.int32
EPS = ko.EPS


@pytest.fixture(scope="module", autouse=True)
def _native():
    ops.ext()  # fail loudly if the extension is missing


def measured(name: str, value: float) -> None:
    print(f"MEASURED {name} {value:.6g}")


def strided(t: torch.Tensor, pad=(8, 8)) -> torch.Tensor:
    """t's values as a column slice of a wider device buffer (row stride and offset multiples of 8)."""
    wide = torch.full((t.shape[0], pad[0] + t.shape[1] + pad[1]), 7.0, dtype=t.dtype, device=DEV)
    wide[:, pad[0]: pad[0] + t.shape[1]] = t.to(DEV)
    return wide[:, pad[0]: pad[0] + t.shape[1]]


# ----------------------------------------------------------------------------- rmsnorm / layernorm
def _run_norm(kind, x, r, w, b, *, res, strided_x, inplace=False):
    """One launch; -> (y, residual_out or None, canary checks)."""
    E = ops.ext()
    rows, D = x.shape
    xd = strided(x) if strided_x else x.to(DEV)
    rd = r.to(DEV) if res else None
    checks = []
    if inplace:
        y, ro = xd, rd
    else:
        y, c = ko.canary((rows, D), device=DEV)
        checks.append(c)
        ro = None
        if res:
            ro, c = ko.canary((rows, D), device=DEV)
            checks.append(c)
    wd = None if w is None else w.to(DEV)
    if kind == "rmsnorm":
        E.rmsnorm(xd, rd, ro, wd, y, EPS)
    else:
        E.layernorm(xd, rd, ro, wd, b.to(DEV), y, EPS)
    torch.cuda.synchronize()
    for c in checks:
        c(kind)
    return y, ro


@pytest.mark.parametrize("regime", ko.REGIMES)
@pytest.mark.parametrize("D", [8, 384, 520, 1280, 4096, 8192])
def test_norms_per_element(regime, D):
    for rows in (1, 4, 5, 9):
        x, r, w, b = ko.norm_case(regime, rows, D)
        zero = rows // 2 if regime == "zero_row" else None
        for res in (False, True):
            rr = r if res else None
            refs = {"rmsnorm": ko.rmsnorm64(x, w, EPS, rr), "layernorm": ko.layernorm64(x, w, b, EPS, rr)}
            variants = [dict(strided_x=False), dict(strided_x=True)]
            if rows == 5:
                variants.append(dict(strided_x=False, inplace=True))  # out is x, residual_out is residual
            for kind, (y64, r64) in refs.items():
                for var in variants:
                    what = f"{kind} {regime} rows={rows} D={D} residual={res} {var}"
                    y, ro = _run_norm(kind, x, r, w, b, res=res, **var)
                    ko.assert_elementwise(y, y64, slack=ko.row_slack(y64), out_dtype=BF, what=what)
                    if res:
                        ko.assert_bitwise(ro, r64, out_dtype=BF, what=what + " residual_out")
                    if zero is not None:  # an all-zero row: exact 0 (rmsnorm) or exactly b (layernorm), no NaN
                        want = torch.zeros(D, dtype=BF) if kind == "rmsnorm" else b
                        assert torch.equal(y[zero].cpu(), want), what + " zero row"
        y64, _ = ko.rmsnorm64(x, None, EPS)
        y, _ = _run_norm("rmsnorm", x, r, None, b, res=False, strided_x=False)
        ko.assert_elementwise(y, y64, slack=ko.row_slack(y64), out_dtype=BF, what=f"rmsnorm w=None {regime} {rows}x{D}")


def test_norms_reject_unsupported_widths():
    E = ops.ext()
    for D in (8200, 12, 4100):  # wider than the 16 register chunks of a lane; not a multiple of 8
        x = torch.zeros(2, D, dtype=BF, device=DEV)
        w = torch.ones(D, dtype=BF, device=DEV)
        y, check = ko.canary((2, D), device=DEV)
        with pytest.raises(RuntimeError):
            E.rmsnorm(x, None, None, w, y, EPS)
        with pytest.raises(RuntimeError):
            E.layernorm(x, None, None, w, w, y, EPS)
        torch.cuda.synchronize()
        check()
        assert bool(ko.untouched(y).all())


# ----------------------------------------------------------------------------- swiglu / bias_act
@pytest.mark.parametrize("F_", [16, 48, 14336])
def test_swiglu_per_element(F_):
    E = ops.ext()
    worst = 0.0
    for rows in (1, 3, 70):
        gu = ko.swiglu_case(rows, F_)
        h64 = ko.swiglu64(gu)
        h, check = ko.canary((rows, F_), device=DEV)
        E.swiglu(gu.to(DEV), h)
        torch.cuda.synchronize()
        check("swiglu")
        assert bool(torch.isfinite(h.float()).all()), "swiglu: saturated gates must stay finite"
        nz = h64 != 0
        worst = max(worst, float((ko.deviation(h, h64, BF)[nz] / h64[nz].abs()).max()))
        measured(f"silu_rel F={F_} rows={rows}", worst)
        ko.assert_elementwise(h, h64, slack=ko.C_SILU * h64.abs(), out_dtype=BF, what=f"swiglu {rows}x{F_}")
        # the saturated gates (ko.SWIGLU_GATES: 30, -30, 1e4, -1e4, 0): silu -> g, ~0, g, -0, 0
        up = gu[:, 16:21].double()
        assert torch.equal(h[:, 2].cpu().double(), ko.rne(gu[:, 2].double() * up[:, 2], BF).double())
        assert bool((h[:, 3].cpu() == 0).all()) and bool((h[:, 4].cpu() == 0).all())


@pytest.mark.parametrize("N", [8, 24, 5120])
def test_bias_act_all_combinations(N):
    E = ops.ext()
    worst = 0.0
    for rows in (1, 5, 70):
        x, b, r = ko.bias_act_case(rows, N)
        for act in (0, 1):
            for wb in (False, True):
                for wr in (False, True):
                    what = f"bias_act {rows}x{N} act={act} bias={wb} residual={wr}"
                    y64, pre = ko.bias_act64(x, b if wb else None, r if wr else None, act)
                    slack = ko.bias_act_slack(y64, pre, act)
                    for inplace in ((False, True) if rows == 5 else (False,)):  # in place: y is x
                        xd = x.to(DEV)
                        y, check = (xd, None) if inplace else ko.canary((rows, N), device=DEV)
                        E.bias_act(xd, b.to(DEV) if wb else None, r.to(DEV) if wr else None, y, act)
                        torch.cuda.synchronize()
                        if check:
                            check(what)
                        if act == 1:
                            worst = max(worst, float((ko.deviation(y, y64, BF) / pre.abs().clamp(min=1.0)).max()))
                        ko.assert_elementwise(y, y64, slack=slack, out_dtype=BF, what=what)
                        if act == 0 and not (wb and wr):  # a plain copy, or one f32 sum of two bf16 values
                            ko.assert_bitwise(y, y64, out_dtype=BF, what=what)
    measured(f"gelu_abs_over_max1x N={N}", worst)


# ----------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("D", [8, 384, 4096])
def test_embedding_vocab_shard(D):
    table, pos_table, ids, positions = ko.embedding_case(D)  # shard of ids 1000 .. 1039
    idd, posd = ids.to(DEV), positions.to(DEV)
    for rows in (ids.numel(), 7):  # rows smaller than ids.numel(): only the first 7 are looked up
        for pt in (None, pos_table):
            out, check = ko.canary((rows, D), device=DEV)
            ops.embedding(idd, table.to(DEV), pos_table=None if pt is None else pt.to(DEV),
                          positions=None if pt is None else posd, vocab_start=1000, out=out, rows=rows)
            torch.cuda.synchronize()
            check("embedding")
            e64 = ko.embedding64(ids, table, 1000, pt, positions, rows=rows)
            ko.assert_elementwise(out, e64, slack=ko.row_slack(e64), out_dtype=BF, what=f"embedding D={D} rows={rows}")
            ko.assert_bitwise(out, e64, out_dtype=BF, what="embedding (a copy, or one f32 sum)")
            if pt is None:  # ids below the shard, at its end, -1, 0: exact zero rows
                outside = [i for i in (0, 3, 4, 6, 7) if i < rows]
                assert bool((out[outside].cpu() == 0).all())
    # the sum over all shards equals the full-table lookup, bitwise
    g = torch.Generator().manual_seed(D)
    full = torch.randn(120, D, generator=g).to(BF)  # ids 960 .. 1079
    full[40:80] = table
    fd = full.to(DEV)
    whole = ops.embedding(idd, fd, vocab_start=960)
    parts = [ops.embedding(idd, fd[s: s + 40], vocab_start=960 + s) for s in (0, 40, 80)]
    assert torch.equal((parts[0].float() + parts[1].float() + parts[2].float()).to(BF), whole)
    ko.assert_bitwise(whole, ko.embedding64(ids, full, 960), out_dtype=BF, what="full-table embedding")


# ----------------------------------------------------------------------------- rope_kv_write
@pytest.mark.parametrize("use_rope", [True, False])
@pytest.mark.parametrize("nq,nkv", [(8, 2), (6, 6)])
@pytest.mark.parametrize("hd", [64, 128])
def test_rope_kv_write_direct(hd, nq, nkv, use_rope):
    E = ops.ext()
    qkv, positions, rope = ko.rope_case(hd, nq, nkv)
    M, blocks, bs = qkv.shape[0], 4, 16
    slots = torch.tensor([5, -1, 33, 16, -1, 0, 63], dtype=torch.int64)
    qd = strided(qkv, pad=(8, 16))
    q_out, q_check = ko.canary((M, nq * hd), rows=(1, 2), cols=(8, 8), device=DEV)
    # caches: views of a larger allocation (guard blocks before / after, guard columns in every token row)
    big_k = torch.full((blocks + 2, nkv, bs, hd + 16), ko.SENTINEL, dtype=BF, device=DEV)
    big_v = torch.full_like(big_k, ko.SENTINEL)
    k_cache, v_cache = big_k[1: 1 + blocks, :, :, 8: 8 + hd], big_v[1: 1 + blocks, :, :, 8: 8 + hd]
    E.rope_kv_write(qd, nq, nkv, hd, use_rope, positions.to(DEV), slots.to(DEV), rope.to(DEV) if use_rope else None,
                    q_out, k_cache, v_cache)
    torch.cuda.synchronize()
    q_check("q_out")
    q64, k64, v64 = ko.rope64(qkv, nq, nkv, hd, positions, rope if use_rope else None)
    q64 = q64.reshape(M, -1)
    ko.assert_elementwise(q_out, q64, slack=ko.row_slack(q64), out_dtype=BF, what="rope q")
    # every cache element: a written line holds the rotated K / the copied V, anything else the sentinel
    for name, big, want64 in (("k", big_k, k64), ("v", big_v, v64)):
        exp = torch.full(tuple(big.shape), ko.SENTINEL, dtype=torch.float64)
        written = torch.zeros(tuple(big.shape), dtype=torch.bool)
        for m in range(M):
            s = int(slots[m])
            if s < 0:
                continue
            exp[1 + s // bs, :, s % bs, 8: 8 + hd] = want64[m]
            written[1 + s // bs, :, s % bs, 8: 8 + hd] = True
        got = big.cpu()
        assert bool((got.double()[~written] == ko.SENTINEL).all()), f"{name}_cache: wrote outside the slots' lines"
        lines64 = exp[written].view(-1, hd)
        ko.assert_elementwise(got[written].view(-1, hd), lines64, slack=ko.row_slack(lines64), out_dtype=BF,
                              what=f"rope {name}_cache")
        if name == "v" or not use_rope:
            ko.assert_bitwise(got[written].view(-1, hd), lines64, out_dtype=BF, what=f"{name}_cache copy")
    if not use_rope:
        ko.assert_bitwise(q_out, q64, out_dtype=BF, what="q copy")


# ----------------------------------------------------------------------------- decode_advance
def test_decode_advance_model():
    E = ops.ext()
    bs, base, pos0, S = 16, 2, 13, -7  # two tokens before the block boundary at position 16
    for max_out in (8, 3):
        i32 = lambda v: torch.tensor([v], dtype=I32, device=DEV)
        tokens, positions, ctx, counter = i32(11), i32(pos0), i32(pos0 + 1), i32(0)
        slots = torch.tensor([(base + pos0 // bs) * bs + pos0 % bs], dtype=torch.int64, device=DEV)
        sampled = i32(0)
        big = torch.full((8,), S, dtype=I32, device=DEV)
        out = big[:max_out]
        pos, rec = pos0, []
        for call in range(5):
            tok = 100 + 7 * call
            sampled.fill_(tok)
            E.decode_advance(tokens, positions, ctx, slots, sampled, out, counter, base, bs)
            pos += 1  # the model: the sampled token becomes the input, one position on
            rec.append(tok)
            want_slot = (base + pos // bs) * bs + pos % bs
            assert (int(tokens), int(positions), int(ctx), int(slots), int(counter)) == (tok, pos, pos + 1, want_slot,
                                                                                         call + 1)
        n = min(max_out, 5)  # out[max_out:] keeps the sentinel while the counter goes on
        assert big.tolist() == rec[:n] + [S] * (8 - n)
        assert int(counter) == 5


# ----------------------------------------------------------------------------- quant_fp8_rows / row_rstd
@pytest.mark.parametrize("D", [8, 2056, 8192])
def test_quant_fp8_rows_and_rstd(D):
    E = ops.ext()
    g = torch.Generator().manual_seed(D)
    x = torch.randn(6, D, generator=g)
    x[1] = 0.0                 # zero row: scale 1, all-zero bytes
    x[2, D // 2] = 200.0       # single-outlier rows: the outlier maps to +-448 exactly
    x[3, D - 1] = -200.0
    x[4] *= 2.0 ** -10         # tiny: eps decides rstd
    x = x.to(BF)
    worst = 0.0
    for xd in (x.to(DEV), strided(x)):
        q, q_check = ko.canary((6, D), device=DEV, dtype=torch.uint8, fill=0x55)
        scale = torch.full((8,), ko.SENTINEL, device=DEV)
        rstd = torch.full((8,), ko.SENTINEL, device=DEV)
        rstd1 = torch.full((8,), ko.SENTINEL, device=DEV)
        E.quant_fp8_rows(xd, q.view(torch.float8_e4m3fn), scale[:6], rstd[:6], EPS)
        E.row_rstd(xd, rstd1[:6], EPS)
        torch.cuda.synchronize()
        q_check("quant_fp8_rows")
        for t in (scale, rstd, rstd1):
            assert bool(ko.untouched(t[6:]).all())
        x64 = x.double()
        amax = x64.abs().amax(-1)
        s64 = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
        ko.assert_elementwise(scale[:6], s64, slack=ko.F32_SLACK * s64, out_dtype=F32, what="fp8 scale")
        qb = q.cpu()
        assert float(scale[1]) == 1.0 and bool((qb[1] == 0).all())
        deq = qb.view(torch.float8_e4m3fn).double()
        assert float(deq[2, D // 2]) == 448.0 and float(deq[3, D - 1]) == -448.0
        # every code: e4m3 has 3 mantissa bits (half an ulp = 2^-4 relative) and subnormal spacing 2^-9
        xs = x64 / s64[:, None]
        bound = 2.0 ** -4 * xs.abs() + 2.0 ** -10 + ko.F32_SLACK * 448.0
        assert bool(((deq - xs).abs() <= bound).all()), f"fp8 codes: worst {float(((deq - xs).abs() - bound).max())}"
        r64 = ko.rstd64(x, EPS)
        for name, got in (("quant rstd", rstd[:6]), ("row_rstd", rstd1[:6])):
            worst = max(worst, float((ko.deviation(got, r64, F32) / r64).max()))
            ko.assert_elementwise(got, r64, slack=ko.C_RSQRT * r64, out_dtype=F32, what=name)
    measured(f"rsqrt_rel D={D}", worst)


@pytest.mark.parametrize("regime", ["tiny", "unit"])
def test_row_rstd_regimes(regime):
    E = ops.ext()
    worst = 0.0
    for D in (8, 520, 1280, 8192):
        x, _, _, _ = ko.norm_case(regime, 9, D)
        r64 = ko.rstd64(x, EPS)
        for xd in (x.to(DEV), strided(x)):
            got = torch.empty(9, device=DEV)
            E.row_rstd(xd, got, EPS)
            worst = max(worst, float((ko.deviation(got, r64, F32) / r64).max()))
            ko.assert_elementwise(got, r64, slack=ko.C_RSQRT * r64, out_dtype=F32, what=f"row_rstd {regime} D={D}")
    measured(f"rsqrt_rel {regime}", worst)


# ----------------------------------------------------------------------------- pcm16_to_f32
@pytest.mark.parametrize("rate", [8000, 22050, 44100, 48000])
def test_pcm_resample_whole_window(rate):
    """One 30 s window (480 000 outputs): the read position i * rate / 16000 needs more than the 24
    bits of an f32 at 22.05 and 44.1 kHz, and its error grows with i.  With the f32 read position
    pcm_kernel had before, the worst output error was 0.0109 (22.05 kHz) and 0.0122 (44.1 kHz) on
    these inputs, on nearly every sample; with the f64 position it is 6.0e-8.  8 and 48 kHz were
    and are exact."""
    pcm = ko.pcm_case(rate)
    out = torch.full((ko.PCM_OUT + 8,), ko.SENTINEL, device=DEV)
    ops.pcm16_to_f32(pcm.to(DEV), in_rate=rate, out=out[: ko.PCM_OUT])
    torch.cuda.synchronize()
    assert bool(ko.untouched(out[ko.PCM_OUT:]).all())
    p64 = ko.pcm64(pcm, rate, ko.PCM_OUT)
    got = out[: ko.PCM_OUT]
    err = (got.cpu().double() - p64).abs()
    measured(f"pcm_abs rate={rate} (worst at {int(err.argmax())})", float(err.max()))
    assert int((ko.PCM_OUT - 1) * (rate / 16000.0)) == pcm.numel() - 1  # the last sample's second tap is clamped
    ko.assert_elementwise(got, p64, slack=1e-6, out_dtype=F32, what=f"pcm16_to_f32 {rate} Hz")


# ----------------------------------------------------------------------------- sample
SEED = 1234


def _sample(logits, mask, temperature, step, *, out=None, n_chunks=64, fail_word=None, v_offset=0, seed=None):
    """ext().sample with its partial buffers sized for n_chunks; -> (tokens, part_val, part_idx)."""
    rows = logits.shape[0]
    seed = torch.tensor([SEED], dtype=torch.int64, device=DEV) if seed is None else seed
    out = torch.full((rows,), -9, dtype=I32, device=DEV) if out is None else out
    pv = torch.empty(rows * n_chunks, dtype=F32, device=DEV)
    pi = torch.empty(rows * n_chunks, dtype=I32, device=DEV)
    ops.ext().sample(logits, mask, temperature, seed, step, out, pv, pi, fail_word, v_offset)
    return out, pv.view(rows, n_chunks), pi.view(rows, n_chunks)


def _step(v=0):
    return torch.tensor([v], dtype=I32, device=DEV)


def _keys64(lg, temps, step, mask=None, v_offset=0):
    """[rows, V] float64 keys of the reference (masked tokens -inf)."""
    out = []
    for r in range(lg.shape[0]):
        k = ko.gumbel_keys64(lg[r], float(temps[r]) if temps is not None else 0.0, SEED, step, r, v_offset)
        if mask is not None:
            k = k.masked_fill(~ko.mask_bits(mask[r], lg.shape[1], v_offset), -math.inf)
        out.append(k)
    return torch.stack(out)


def _tokens64(keys):
    """First maximum per row (the lowest id wins ties), -1 when nothing is admitted; and the top-two gap."""
    top = keys.topk(2, dim=-1).values
    tok = torch.where(torch.isinf(top[:, 0]) & (top[:, 0] < 0), torch.full((keys.shape[0],), -1), keys.argmax(-1))
    return tok, top[:, 0] - top[:, 1]


@pytest.mark.parametrize("masked", [False, True])
def test_sample_every_key(masked):
    """n_chunks == V: one token per chunk, so part_val / part_idx hold every token's key and id."""
    rows, V, step0 = 4, 1000, 3
    g = torch.Generator().manual_seed(21)
    lg = torch.randn(rows, V, generator=g) * 3
    temps = torch.tensor([0.7, 0.0, 1.3, 0.7])
    mask = ko.pack_mask(torch.rand(rows, V, generator=g) < 0.5) if masked else None
    step = _step(step0)
    _, pv, pi = _sample(lg.to(DEV), None if mask is None else mask.to(DEV), temps.to(DEV), step, n_chunks=V)
    torch.cuda.synchronize()
    k64 = _keys64(lg, temps, step0, mask)
    fin = torch.isfinite(k64)
    measured(f"key_abs masked={masked}", float((pv.cpu().double() - k64)[fin].abs().max()))
    ko.assert_elementwise(pv, k64, slack=ko.C_KEY, out_dtype=F32, what="sampler keys")
    assert torch.equal(pv[1].cpu()[fin[1]], lg[1][fin[1]])  # T = 0: the logit itself
    want_idx = torch.where(fin, torch.arange(V)[None].expand(rows, V), torch.full((rows, V), ko.NO_TOKEN))
    assert torch.equal(pi.cpu().long(), want_idx)
    for r in range(rows):  # the CPU reference's f32 keys sit in the same band
        if temps[r] > 0:
            ko.assert_elementwise(ref.gumbel_keys(lg[r], float(temps[r]), SEED, step0, r), _keys64(lg, temps, step0)[r],
                                  slack=ko.C_KEY, out_dtype=F32, what="ref.gumbel_keys")
    assert int(step) == step0 + 1


def test_sample_greedy_edges():
    V, C = 51865, 64  # Whisper's vocabulary: no multiple of 32; 811 tokens per chunk, not word aligned
    per = (V + C - 1) // C
    assert per == 811
    words = (V + 31) // 32
    g = torch.Generator().manual_seed(22)
    rows = 9
    lg = torch.randn(rows, V, generator=g)
    bits = torch.ones(rows, words * 32, dtype=torch.bool)  # (pad bits past V set on purpose)
    want = [0] * rows
    lg[0] = 0.0                                   # all equal: the lowest id wins
    lg[1] = -1.0
    lg[1, [7 * per - 1, 7 * per]] = 5.0           # a tie across a chunk border
    want[1] = 7 * per - 1
    lg[2] = -1.0
    lg[2, [900 + 256, 900, 900 + 3 * 256 + 1]] = 5.0  # a tie across the 256-thread stride and across threads
    want[2] = 900
    lg[3] = 2.0                                   # all equal under a mask: the lowest admitted id wins
    bits[3] = False
    bits[3, [40001, 40000 + per, V - 1]] = True
    want[3] = 40001
    bits[4] = False                               # only the last token admitted
    bits[4, V - 1] = True
    want[4] = V - 1
    bits[5] = False                               # only bit 31 of a word admitted
    bits[5, 32 * 700 + 31] = True
    want[5] = 32 * 700 + 31
    bits[6] = False                               # empty mask -> -1 in this row only
    bits[6, V:] = True                            # (pad bits do not count)
    want[6] = -1
    lg[7] = -math.inf                             # nothing finite -> -1
    want[7] = -1
    bits[8] = False
    adm = torch.randint(0, V, (50,), generator=g)
    bits[8, adm] = True
    want[8] = int(adm[lg[8, adm].argmax()])
    mask = ko.pack_mask(bits)
    assert mask.shape == (rows, words)
    step = _step(0)
    lgd, md = lg.to(DEV), mask.to(DEV)
    out, _, _ = _sample(lgd, md, None, step, n_chunks=C)
    assert out.tolist() == want
    assert int(step) == 1  # one step per call, whatever the rows
    out3, _, _ = _sample(lgd[:3], md[:3], None, step, n_chunks=C)
    assert out3.tolist() == want[:3] and int(step) == 2
    # T = 0 rows are greedy whatever the temperature of the others
    temps = torch.zeros(rows, device=DEV)
    out, _, _ = _sample(lgd, md, temps, step, n_chunks=C)
    assert out.tolist() == want and int(step) == 3
    # a set fail word: -2 in every row, the step still advances
    fail = torch.tensor([1], dtype=torch.int64, device=DEV)
    out, _, _ = _sample(lgd, md, None, step, n_chunks=C, fail_word=fail)
    assert out.tolist() == [-2] * rows and int(step) == 4
    fail.zero_()
    out, _, _ = _sample(lgd, md, None, step, n_chunks=C, fail_word=fail)
    assert out.tolist() == want
    # the same tokens with the mask and out_tokens in pinned host memory
    pm = mask.clone().pin_memory()
    po = torch.full((rows,), -9, dtype=I32).pin_memory()
    _sample(lgd, pm, None, step, out=po, n_chunks=C)
    torch.cuda.synchronize()
    assert po.tolist() == want


def test_sample_mixed_temperatures_one_call():
    rows, V, step0 = 6, 5003, 9
    g = torch.Generator().manual_seed(23)
    lg = torch.randn(rows, V, generator=g) * 3
    mask = ko.pack_mask(torch.rand(rows, V, generator=g) < 0.2)
    temps = torch.tensor([0.0, 0.7, 0.0, 1.3, 0.7, 0.0])
    tok, gap = _tokens64(_keys64(lg, temps, step0, mask))
    assert float(gap.min()) >= 1e-3, gap  # the reference's choice is not a near tie
    out = torch.full((rows,), -9, dtype=I32, device=DEV)
    ops.sample(lg.to(DEV), mask=mask.to(DEV), temperature=temps.to(DEV),
               seed=torch.tensor([SEED], dtype=torch.int64, device=DEV), step=_step(step0), out_tokens=out)
    assert out.tolist() == tok.tolist()
    exp = torch.empty(rows, dtype=I32)
    ref.sample(lg, mask=mask, temperature=temps, seed=torch.tensor([SEED]), step=torch.tensor([step0], dtype=I32),
               out_tokens=exp)
    assert exp.tolist() == tok.tolist()  # the f32 CPU reference agrees with the float64 one


def test_sample_token_equality_whisper_vocab():
    rows, V = 16, 51865
    lg = torch.randn(rows, V, generator=torch.Generator().manual_seed(1234)) * 3
    temps = torch.full((rows,), 0.7)
    tok, gap = _tokens64(_keys64(lg, temps, 0))
    measured("top_two_key_gap_min", float(gap.min()))
    assert float(gap.min()) >= 1e-3, gap
    out, _, _ = _sample(lg.to(DEV), None, temps.to(DEV), _step(0), n_chunks=64)
    assert out.tolist() == tok.tolist()  # exact, no excused rows


@pytest.mark.parametrize("T", [0.0, 0.7])
def test_sample_shard_invariance(T):
    """V = 1000 as shards of 320 / 352 / 328 columns: the merged shard partials give the full-vocab token."""
    rows, V, C = 5, 1000, 8
    g = torch.Generator().manual_seed(24)
    lg = torch.randn(rows, V, generator=g) * 3
    lg[4] = 1.0  # all equal: the lowest admitted id has to win across shards too
    bits = torch.rand(rows, V, generator=g) < 0.3
    bits[3] = False
    bits[3, 700:] = True  # a row whose admitted tokens all sit in the last shard
    mask = ko.pack_mask(bits)
    temps = torch.full((rows,), T)
    tok, gap = _tokens64(_keys64(lg, temps, 5, mask))
    assert float((gap if T > 0 else gap[:4]).min()) >= 1e-3, gap  # (row 4 at T = 0 is the all-equal tie)
    lgd, md, td = lg.to(DEV), mask.to(DEV), temps.to(DEV)
    full, _, _ = _sample(lgd, md, td, _step(5), n_chunks=64)
    assert full.tolist() == tok.tolist()
    vals, idx = [], []
    for off, n in ((0, 320), (320, 352), (672, 328)):
        shard_tok, pv, pi = _sample(lgd[:, off: off + n], md, td, _step(5), n_chunks=C, v_offset=off)
        pv, pi = pv.cpu(), pi.cpu().long()
        k64 = _keys64(lg[:, off: off + n], temps, 5, mask, v_offset=off)  # this shard alone
        st, _ = _tokens64(k64)
        assert shard_tok.tolist() == [int(t) + off if t >= 0 else -1 for t in st]
        vals.append(pv.t())
        idx.append(torch.where(pi == ko.NO_TOKEN, torch.full_like(pi, -1), pi).t())
    merged = ref.merge_partials(torch.cat(vals), torch.cat(idx))
    assert merged.tolist() == tok.tolist()


def test_sample_distribution_chi_square():
    """64 identical rows x 2000 steps at T = 0.7 over V = 37 follow softmax(logits / T): Pearson
    chi-square below the 1 - 1e-4 quantile (the CPU reference gives 36.96 on this input, limit 60.4:
    tests/test_kernel_oracle_cpu.py)."""
    V, rows, steps, T = 37, 64, 2000, 0.7
    lg = torch.randn(V, generator=torch.Generator().manual_seed(5)) * 2
    probs = torch.softmax(lg.double() / T, 0)
    lgd = lg.to(DEV)[None].expand(rows, V).contiguous()
    td = torch.full((rows,), T, device=DEV)
    seed = torch.tensor([SEED], dtype=torch.int64, device=DEV)
    pv = torch.empty(rows * 4, dtype=F32, device=DEV)
    pi = torch.empty(rows * 4, dtype=I32, device=DEV)
    E = ops.ext()

    def run(n):
        toks = torch.full((n, rows), -9, dtype=I32, device=DEV)
        step = _step(0)
        for s in range(n):
            E.sample(lgd, None, td, seed, step, toks[s], pv, pi, None, 0)
        assert int(step) == n
        return toks

    toks = run(steps)
    counts = torch.bincount(toks.flatten().long(), minlength=V)  # accumulated on the device
    assert int(counts.sum()) == rows * steps and int(toks.min()) >= 0 and int(toks.max()) < V
    chi2, cells = ko.pearson_chi2(counts, probs)
    limit = ko.chi2_quantile(cells - 1)
    measured(f"chi2 ({cells} cells, limit {limit:.2f})", chi2)
    assert chi2 < limit
    assert torch.unique(toks.t().cpu(), dim=0).shape[0] == rows  # no two rows draw the same sequence
    assert torch.equal(run(50), toks[:50])  # the same (seed, step) replays the same tokens
