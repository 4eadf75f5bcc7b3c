"""Non-temporal weight loads (VWA_CHAIN_WNT: skinny_stream.hip chain_wnt_kernel; VWA_STREAM_WNT:
SkinnyParams::w_nt, the AUX = 2 streaming GEMMs) change how the weight bytes are requested, not which
bytes or in what order they are used: every output must be the same BITS with the policy on and off.

Chained launch: test_chain_pack_gpu.py's configuration (hidden 512, FFN 1024, 3 layers, 8 query / 2 kv
heads of 128, context 40, steps of 1, 4 and 1 rows) -- logits, hidden rows and every layer's K/V, for
packed and bf16 weights, one launch per layer and one for all layers, the flagged-block variant and
fp8 once each.  Streaming GEMMs: the store, residual, SwiGLU and QKV epilogues on tiled weights
(N 64, K 512, 1 / 5 / 16 rows, at the 8-wave split that has the nt instantiation), the smallest
shape that streams X with the weights (K 14336, 6 rows, N 32), and the LM head under a grammar mask
that admits two non-adjacent tiles.  A row-major weight cannot take the policy: both entry points raise."""
import os

import pytest
import torch

from test_chain_pack_gpu import CFG, _bits, _flag
from voice_enabled_browser_automation_amd import ops
from voice_enabled_browser_automation_amd.models.llama import LlamaModel
from voice_enabled_browser_automation_amd.runtime.engine import LLMEngine

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------ chained launch
def _run(model, toks, pack: bool, multi: bool, wnt: bool):
    """Prefill 40 tokens, then steps of 1, 4 and 1 rows through the chained launch with the weight
    policy `wnt` (both knobs: the chain's and the streaming GEMMs'); per step the logits and hidden
    rows, at the end every layer's K/V -- all as integer bit patterns."""
    env = {"VWA_CHAIN": "1", "VWA_CHAIN_ATTN": "1", "VWA_CHAIN_PACK": "1" if pack else "0",
           "VWA_CHAIN_MULTI": "1" if multi else "0", "VWA_CHAIN_WNT": "1" if wnt else "0"}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        model.set_stream_nt(wnt)
        model.reset_chains()
        e = LLMEngine(model, max_seqs=2, max_model_len=256, kv_blocks=20, block_size=16)
        s = e.new_sequence(toks[:40], use_prefix_cache=False)
        e.prefill(s)
        steps, i = [], 40
        for n in (1, 4, 1):
            logits = e.run_rows([(s, t) for t in toks[i:i + n]])
            steps.append((n, _bits(logits.float()).cpu().clone(), _bits(e.bufs.hidden[:n]).cpu().clone()))
            i += n
        torch.cuda.synchronize()
        kv = [(_bits(k).cpu().clone(), _bits(v).cpu().clone()) for k, v in zip(e.kv.k, e.kv.v)]
        descs = [v for v in model.chain_descs() if v is not None]
        multis = [v for d in model._chains.values() for k, v in d.items() if k[0] == "multi" and v is not None]
        assert not model.chain_error(), "chain error word set"
        return dict(steps=steps, kv=kv, n_desc=len(descs), multi=bool(multis),
                    packed=[bool((v[2] >> 28) & 1) for v in descs], fp8=[bool((v[2] >> 25) & 1) for v in descs],
                    nt=[bool((v[2] >> 29) & 1) for v in descs])
    finally:
        model.set_stream_nt(False)
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def world():
    """The models (built on first use) and, per (variant, packed, multi), the default-policy run:
    the reference, computed once."""
    ops.ext()
    torch.manual_seed(0)
    toks = torch.randint(0, CFG.vocab_size, (48,)).tolist()
    models, refs = {}, {}

    def model(variant):
        if variant not in models:
            os.environ["VWA_CHAIN_PACK"] = "1"
            try:
                m = LlamaModel(CFG, device="cuda", seed=3, wdtype="fp8" if variant == "fp8" else "bf16")
            finally:
                os.environ.pop("VWA_CHAIN_PACK", None)
            if variant == "flagged":
                _flag(m)
            models[variant] = m
        return models[variant]

    def ref(variant, pack, multi):
        key = (variant, pack, multi)
        if key not in refs:
            refs[key] = _run(model(variant), toks, pack, multi, False)
        return refs[key]

    return dict(toks=toks, model=model, ref=ref)


CHAIN_CASES = [("plain", True, True), ("plain", True, False), ("plain", False, True), ("plain", False, False),
               ("flagged", True, True), ("fp8", False, True)]


@pytest.mark.parametrize("variant,pack,multi", CHAIN_CASES,
                         ids=["packed-multi", "packed-per-layer", "bf16-multi", "bf16-per-layer", "flagged", "fp8"])
def test_chain_nt_weight_stream_gives_the_same_bits(world, variant, pack, multi):
    ref = world["ref"](variant, pack, multi)
    got = _run(world["model"](variant), world["toks"], pack, multi, True)
    # the launches really were the nt / the default-policy form of the same instantiation
    assert got["n_desc"] and all(got["nt"]) and ref["n_desc"] == got["n_desc"] and not any(ref["nt"])
    assert got["multi"] == multi and ref["multi"] == multi
    assert all(got["packed"]) == pack and got["packed"] == ref["packed"]
    assert all(got["fp8"]) == (variant == "fp8") and got["fp8"] == ref["fp8"]
    for (n, lg, hd), (n2, lg2, hd2) in zip(got["steps"], ref["steps"]):
        assert n == n2
        assert torch.equal(hd, hd2), f"hidden rows differ at a {n}-row step"
        assert torch.equal(lg, lg2), f"logits differ at a {n}-row step"
    for li, ((k, v), (k2, v2)) in enumerate(zip(got["kv"], ref["kv"])):
        assert torch.equal(k, k2) and torch.equal(v, v2), f"layer {li} K/V differ"


def test_chain_refuses_nt_on_row_major_weights():
    E = ops.ext()
    bf, dev = torch.bfloat16, "cuda"
    M, d, F = 1, 512, 1024
    mk = lambda *s: (torch.randn(*s, device=dev) * 0.02).to(bf)  # noqa: E731
    bar, _, work = ops.chain_buffers(torch.device(dev))
    args = (mk(M, d), mk(M, d), mk(M, F), mk(d, d), mk(2 * F, d), mk(d, F), 1e-5, None, 4, 1, 128, None, None, None,
            None, None, None, bar, work)
    with pytest.raises(RuntimeError, match="w_nt"):
        E.chain_make(*args, w_tiled=False, w_nt=True)


# ------------------------------------------------------------------------------ streaming GEMMs
@pytest.fixture
def ks8():
    """The 8-wave split of K for every shape (by default K < 2048 runs 4 waves, which has no nt
    instantiation and would make on-vs-off the same kernel)."""
    E = ops.ext()
    E.set_skinny_mode(1, 256, 8, 2)
    yield
    E.set_skinny_mode(1, 256, 0, 2)


def _w(N, K, seed, nt):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return ops.TiledWeight((torch.randn(N, K, device="cuda", generator=g) * 0.05).to(torch.bfloat16), nt=nt)


def _x(M, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)


def _gemm(epi: int, M: int, N: int, K: int, nt: bool, mask=None):
    """One streaming GEMM with epilogue `epi` on a tiled weight; every tensor it wrote, as bits."""
    w, x = _w(N, K, 1, nt), _x(M, K, 2)
    if epi == 0:
        out = torch.full((M, N), -7.0, dtype=torch.float32, device="cuda")  # (masked tiles stay as they are)
        ops.linear(x, w, out=out, fuse_rms=True, eps=1e-5, col_mask=mask)
        outs = [out]
    elif epi == 1:
        h = _x(M, N, 3)
        ops.linear(x, w, out=h, residual=h)
        outs = [h]
    elif epi == 2:
        outs = [ops.linear_swiglu(x, w, fuse_rms=True, eps=1e-5)]
    else:
        hd, nq, nkv = 16, N // 16 - 2, 1
        q = torch.zeros(M, nq * hd, dtype=torch.bfloat16, device="cuda")
        kc = torch.zeros(4, nkv, 16, hd, dtype=torch.bfloat16, device="cuda")
        vc = torch.zeros_like(kc)
        ops.qkv_rope_write(x, w, None, fuse_rms=True, eps=1e-5, n_q_heads=nq, n_kv_heads=nkv, head_dim=hd,
                           rope=ops.rope_table(64, hd, 1e4, device="cuda"),
                           positions=torch.arange(3, 3 + M, dtype=torch.int32, device="cuda"),
                           slots=torch.arange(5, 5 + M, dtype=torch.int64, device="cuda"), q_out=q, k_cache=kc, v_cache=vc)
        outs = [q, kc, vc]
    torch.cuda.synchronize()
    return [_bits(o).cpu() for o in outs]


@pytest.mark.parametrize("M", [1, 5, 16])
@pytest.mark.parametrize("epi", [0, 1, 2, 4], ids=["store", "resid", "swiglu", "qkv"])
def test_stream_gemm_nt_gives_the_same_bits(ks8, epi, M):
    off, on = _gemm(epi, M, 64, 512, False), _gemm(epi, M, 64, 512, True)
    assert all(torch.equal(a, b) for a, b in zip(off, on))
    assert any(bool(a.ne(0).any()) for a in on), "nothing was written"


def test_stream_gemm_nt_with_streamed_x_gives_the_same_bits():
    # 6 rows of K = 14336 do not fit LDS next to the scratch: X is streamed with the weights (XG)
    off, on = _gemm(1, 6, 32, 14336, False), _gemm(1, 6, 32, 14336, True)
    assert torch.equal(off[0], on[0])


def test_masked_lm_head_nt_gives_the_same_bits(ks8):
    # tokens 3 and 37: the 16-column tiles 0 and 2 of 4 are computed, tiles 1 and 3 left as they were
    mask = torch.tensor([[1 << 3, 1 << 5]], dtype=torch.int32, device="cuda")
    off, on = _gemm(0, 1, 64, 512, False, mask), _gemm(0, 1, 64, 512, True, mask)
    assert torch.equal(off[0], on[0])
    f = on[0].view(torch.float32).view(1, 4, 16)
    assert bool((f[0, 1] == -7.0).all()) and bool((f[0, 3] == -7.0).all()), "a masked tile was written"
    assert bool((f[0, 0] != -7.0).all()) and bool((f[0, 2] != -7.0).all()), "an admitted tile was not written"


def test_fp8_stream_gemm_nt_gives_the_same_bits(ks8):
    w = ops.FP8Weight.quantize((torch.randn(64, 512, device="cuda") * 0.05).to(torch.bfloat16), tiled=True)
    x = _x(5, 512, 2)
    outs = []
    for nt in (False, True):
        w.nt = nt
        outs.append(_bits(ops.linear_swiglu(x, w, fuse_rms=True, eps=1e-5)).cpu())
    assert torch.equal(*outs) and bool(outs[0].ne(0).any())


def test_stream_gemm_refuses_nt_on_a_row_major_weight():
    x, w = _x(1, 512, 2), (torch.randn(64, 512, device="cuda") * 0.05).to(torch.bfloat16)
    out = torch.empty(1, 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="w_nt"):
        ops.ext().skinny_gemm(x, w, None, out, 0, False, 1e-5, None, w_nt=True)
