"""The chained decode layer over packed weights (VWA_CHAIN_PACK: ops.pack_weight, skinny_stream.hip
chain_kernel PK) against the same launch over the bf16 weights: the packed form is lossless and the
MFMA sequence is the same, so the hidden rows, the logits and the K/V written are the same BITS --
for steps of 1 and 4 rows, one launch per layer and one launch for all layers, and with k-groups
that the codes cannot express (read from the bf16 copy on the flagged path).

Shapes: hidden 512, FFN 1024, 3 layers, context 40, 8 query / 2 kv heads of 128 -- a GQA group of 4,
the smallest the chained attention phase (the only launch form that decodes packed weights) takes."""
import os

import pytest
import torch

from voice_enabled_browser_automation_amd import ops
from voice_enabled_browser_automation_amd.models.config import LlamaConfig
from voice_enabled_browser_automation_amd.models.llama import LlamaModel
from voice_enabled_browser_automation_amd.runtime.engine import LLMEngine

pytestmark = pytest.mark.gpu

CFG = LlamaConfig(name="tpk", vocab_size=4096, hidden=512, n_layers=3, n_heads=8, n_kv_heads=2, head_dim=128,
                  ffn=1024, max_pos=2048)
ZERO_CH = 77  # FFN channel whose activation is exactly zero in the flagged variant


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t.contiguous().view(torch.int32)


def _run(model, toks, pack: bool, multi: bool):
    """Prefill 40 tokens, then steps of 1, 4 and 1 rows through the chained launch; per step the
    logits and hidden rows, at the end every layer's K/V -- all as integer bit patterns."""
    env = {"VWA_CHAIN": "1", "VWA_CHAIN_ATTN": "1", "VWA_CHAIN_PACK": "1" if pack else "0",
           "VWA_CHAIN_MULTI": "1" if multi else "0"}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
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
        descs = list(model.chain_descs())
        multis = [v for d in model._chains.values() for k, v in d.items() if k[0] == "multi" and v is not None]
        assert not model.chain_error(), "chain error word set"
        return dict(steps=steps, kv=kv, packed=[bool((v[2] >> 28) & 1) for v in descs if v is not None],
                    n_desc=len(descs), multi=bool(multis), engine=e)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _flag(model):
    """Two k-groups no code can express: 1e-30 in layer 1's o_proj, and +Inf in the last layer's down
    projection in a column whose X is zero (the FFN channel's gate and up rows are zeroed, so its
    activation silu(0) * 0 is exactly 0).  The K/V of every layer stay finite; the last hidden rows
    carry the NaN of 0 x Inf in both forms."""
    def put(L, name, w):
        tw = ops.TiledWeight(w)
        tw.pk = ops.pack_weight(tw.t)
        setattr(L, name, tw)
        return tw

    o = model.layers[1].o.dense().clone()
    o[5, 300] = 1e-30
    assert put(model.layers[1], "o", o).pk.n_flagged == 1
    L = model.layers[-1]
    gu = L.gu.dense().clone()
    t, q = divmod(ZERO_CH, 16)  # (ops.interleave_gate_up: gate rows 32 t + q, up rows 32 t + 16 + q of tile t)
    gu[32 * t + q] = 0
    gu[32 * t + 16 + q] = 0
    put(L, "gu", gu)
    dn = L.down.dense().clone()
    dn[9, ZERO_CH] = float("inf")
    assert put(L, "down", dn).pk.n_flagged == 1


@pytest.fixture(scope="module")
def world():
    ops.ext()
    torch.manual_seed(0)
    toks = torch.randint(0, CFG.vocab_size, (48,)).tolist()
    out = {}
    for variant in ("plain", "flagged"):
        os.environ["VWA_CHAIN_PACK"] = "1"
        try:
            model = LlamaModel(CFG, device="cuda", seed=3)
        finally:
            os.environ.pop("VWA_CHAIN_PACK", None)
        assert all(w.pk is not None for L in model.layers for w in (L.qkv, L.o, L.gu, L.down))
        # (the random weights themselves may hold a few exact zeros -- about 2^-24 of a float32 normal
        # draw -- whose blocks are flagged in both variants)
        if variant == "flagged":
            _flag(model)
        # the reference: the same launches over the bf16 weights, computed once per variant
        out[variant] = dict(model=model, toks=toks, ref={m: _run(model, toks, False, m) for m in (False, True)})
    return out


@pytest.mark.parametrize("multi", [False, True], ids=["per-layer", "multi-layer"])
@pytest.mark.parametrize("variant", ["plain", "flagged"])
def test_packed_chain_gives_the_bf16_chains_bits(world, variant, multi):
    w = world[variant]
    ref = w["ref"][multi]
    got = _run(w["model"], w["toks"], True, multi)
    # the launches really were the packed / the bf16 form, and one launch for all layers where asked
    assert got["n_desc"] and all(got["packed"]) and not any(ref["packed"])
    assert got["multi"] == multi and ref["multi"] == multi
    for (n, lg, hd), (n2, lg2, hd2) in zip(got["steps"], ref["steps"]):
        assert n == n2
        assert torch.equal(hd, hd2), f"hidden rows differ at a {n}-row step"
        assert torch.equal(lg, lg2), f"logits differ at a {n}-row step"
    for li, ((k, v), (k2, v2)) in enumerate(zip(got["kv"], ref["kv"])):
        assert torch.equal(k, k2) and torch.equal(v, v2), f"layer {li} K/V differ"
    if variant == "plain":  # (the flagged variant's 0 x Inf is a NaN in both forms: compared as bits above)
        assert all(torch.isfinite(lg.view(torch.float32)).all() for _, lg, _ in got["steps"])


def test_flagged_activation_column_is_zero(world):
    """The flagged variant's construction holds: the zeroed FFN channel's activation is exactly 0
    in the last chained step, so the +Inf weight met X = 0."""
    e = world["flagged"]["ref"][False]["engine"]
    assert float(e.bufs.act[:1, ZERO_CH].float().abs().max()) == 0.0
