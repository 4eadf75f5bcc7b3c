"""Packed chained layer, flagged k-groups in every item position (skinny_stream.hip chain_phase
compute: an item with a flagged k-group runs the loop with the bf16-copy loads, every other item
the loop without loads).  Against the same launches over the bf16 weights the hidden rows, logits
and K/V are the same BITS.

Shape: hidden 1024, FFN 2048, 3 layers, 8 query / 2 kv heads of 128, context 40, on 16 workgroups
(VWA_CHAIN_GRID_DIV) -- every workgroup then holds 8 gate/up, 4 down, 6 QKV and >= 2 o_proj items
(asserted below from the phases' unit counts), so each phase has items issued ahead of a barrier
wait (items 0 and 1, gate/up's item 0 in o_proj's free register set), the item read back from LDS
(index 2) and mid-phase items (>= 3).  Every 16-row tile of every chained weight carries one
unrepresentable value (1e-30) in a k-group that rotates with the tile: each item of each phase
then has a wave whose k-group is flagged in one of the item's tiles and not in the other, and
seven waves that take the loop without loads.  The last layer's down projection also holds one
+Inf against an exactly zero activation, as tests/test_chain_pack_gpu.py."""
import os

import pytest
import torch

from voice_enabled_browser_automation_amd import ops
from voice_enabled_browser_automation_amd.models.config import LlamaConfig
from voice_enabled_browser_automation_amd.models.llama import LlamaModel
from voice_enabled_browser_automation_amd.runtime.engine import LLMEngine

pytestmark = pytest.mark.gpu

CFG = LlamaConfig(name="tpkf", vocab_size=4096, hidden=1024, n_layers=3, n_heads=8, n_kv_heads=2, head_dim=128,
                  ffn=2048, max_pos=2048)
WGS = 16
ZERO_CH = 77  # FFN channel whose activation is exactly zero


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t.contiguous().view(torch.int32)


def _items_per_workgroup():
    """Items of the smallest workgroup range per phase, by chain_range's arithmetic: the contiguous
    range [units b / n, units (b + 1) / n) of ntiles x nb units, nb = ceil(ceil(K / 128 / 8 waves) / U)."""
    out = {}
    d, f, nqkv = CFG.hidden, CFG.ffn, (CFG.n_heads + 2 * CFG.n_kv_heads) * CFG.head_dim
    for name, n, k, nt in (("o", d, CFG.n_heads * CFG.head_dim, 2), ("gu", 2 * f, d, 2), ("down", d, f, 1), ("qkv", nqkv, d, 1)):
        per_wave = -(-(k // 128) // 8)
        nb = -(-per_wave // (4 // nt))
        units = n // (16 * nt) * nb
        out[name] = min(units * (b + 1) // WGS - units * b // WGS for b in range(WGS))
    return out


def _run(model, toks, pack: bool, multi: bool, div: int):
    env = {"VWA_CHAIN": "1", "VWA_CHAIN_ATTN": "1", "VWA_CHAIN_PACK": "1" if pack else "0",
           "VWA_CHAIN_MULTI": "1" if multi else "0", "VWA_CHAIN_GRID_DIV": str(div)}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        model.reset_chains()
        e = LLMEngine(model, max_seqs=2, max_model_len=256, kv_blocks=20, block_size=16)
        s = e.new_sequence(toks[:40], use_prefix_cache=False)
        e.prefill(s)
        steps, i = [], 40
        for n in (1, 2, 4, 1):
            logits = e.run_rows([(s, t) for t in toks[i:i + n]])
            torch.cuda.synchronize()
            assert not model.chain_error(), f"chain error word set after the {n}-row step"
            steps.append((n, _bits(logits.float()).cpu().clone(), _bits(e.bufs.hidden[:n]).cpu().clone()))
            i += n
        kv = [(_bits(k).cpu().clone(), _bits(v).cpu().clone()) for k, v in zip(e.kv.k, e.kv.v)]
        descs = list(model.chain_descs())
        multis = [v for d in model._chains.values() for k, v in d.items() if k[0] == "multi" and v is not None]
        return dict(steps=steps, kv=kv, packed=[bool((v[2] >> 28) & 1) for v in descs if v is not None],
                    n_desc=len(descs), multi=bool(multis), zero_act=float(e.bufs.act[:1, ZERO_CH].float().abs().max()))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _flag_every_tile(model):
    """1e-30 in tile t of every chained weight, k-group (5 t + layer) mod (K / 128); the last layer's
    down projection: +Inf in the zeroed FFN channel's column.  Returns the blocks planted."""
    planted = 0
    for li, L in enumerate(model.layers):
        for name in ("qkv", "o", "gu", "down"):
            w = getattr(L, name).dense().clone()
            n, k = w.shape
            if li == len(model.layers) - 1 and name == "gu":
                t, q = divmod(ZERO_CH, 16)  # (ops.interleave_gate_up: gate rows 32 t + q, up rows 32 t + 16 + q)
                w[32 * t + q] = 0
                w[32 * t + 16 + q] = 0
            rows = torch.arange(n // 16, device=w.device)
            kg = (5 * rows + li) % (k // 128)
            w[16 * rows + 3, 128 * kg + 7] = 1e-30
            if li == len(model.layers) - 1 and name == "down":
                w[9, ZERO_CH] = float("inf")
            tw = ops.TiledWeight(w)
            tw.pk = ops.pack_weight(tw.t)
            # every planted block is flagged (the zeroed gate/up rows and the random draw may add more)
            assert tw.pk.n_flagged >= n // 16
            flags = tw.pk.data[-(n // 16) * (k // 128):].view(n // 16, k // 128)
            assert bool((flags[rows, kg] != 0).all()), f"layer {li} {name}: a planted block is not flagged"
            if li == len(model.layers) - 1 and name == "down":
                assert int(flags[0, ZERO_CH // 128]) != 0
            setattr(L, name, tw)
            planted += n // 16
    return planted


@pytest.fixture(scope="module")
def world():
    ops.ext()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus % WGS == 0
    div = cus // WGS
    torch.manual_seed(0)
    toks = torch.randint(0, CFG.vocab_size, (48,)).tolist()
    os.environ["VWA_CHAIN_PACK"] = "1"
    try:
        model = LlamaModel(CFG, device="cuda", seed=3)
    finally:
        os.environ.pop("VWA_CHAIN_PACK", None)
    planted = _flag_every_tile(model)
    return dict(model=model, toks=toks, div=div, planted=planted,
                ref={m: _run(model, toks, False, m, div) for m in (False, True)})


def test_every_phase_has_pre_issued_lds_and_mid_phase_items():
    n = _items_per_workgroup()
    assert n["gu"] >= 4 and n["down"] >= 3 and n["qkv"] >= 3 and n["o"] >= 2, n


@pytest.mark.parametrize("multi", [False, True], ids=["per-layer", "multi-layer"])
def test_flagged_items_give_the_bf16_chains_bits(world, multi):
    ref = world["ref"][multi]
    got = _run(world["model"], world["toks"], True, multi, world["div"])
    assert world["planted"] == 3 * (96 + 64 + 256 + 64)
    assert got["n_desc"] and all(got["packed"]) and not any(ref["packed"])
    assert got["multi"] == multi and ref["multi"] == multi
    assert got["zero_act"] == 0.0 and ref["zero_act"] == 0.0  # the +Inf weight met X = 0
    for (n, lg, hd), (n2, lg2, hd2) in zip(got["steps"], ref["steps"]):
        assert n == n2
        assert torch.equal(hd, hd2), f"hidden rows differ at a {n}-row step"
        assert torch.equal(lg, lg2), f"logits differ at a {n}-row step"
    for li, ((k, v), (k2, v2)) in enumerate(zip(got["kv"], ref["kv"])):
        assert torch.equal(k, k2) and torch.equal(v, v2), f"layer {li} K/V differ"
