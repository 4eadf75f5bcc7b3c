"""Per-key oracle tests of the three standalone attention kernels, as reached through
ops.decode_attention, ops.decode_attention_rows, ops.flash_attention and ops.flash_attention_runs:
decode_mq_kernel ("mq"), decode_attn_kernel ("split") and flash_attn_kernel.

Every output element is compared with a float64 softmax attention over an explicit visible-key
mask on the kernel's own score operand (tests/kernel_oracle.py: |got - o64| <= 2^-8 |o64| + c A64),
on three input families built so that ONE key going wrong is seen: counting (q = 0, V a 0/1 code:
outputs are key counts), retrieval (one key wins by >= 40 in log2 units: the output is that key's
V row, bit for bit in the decode kernels) and spiked random (the numerics case; a few heavy edge
keys).  tests/test_attention_oracle_cpu.py shows without a GPU that an honest kernel passes on
exactly these inputs (the case table ko.attn_cases() is shared) and that a key dropped, leaked,
counted twice or read from the wrong place fails by at least 4 x the bound.

Common to every test: 16-token blocks in a random permutation, blocks nobody owns hold a sentinel
code (never zeros), the output is a canary view (guard rows, a row stride wider than the row), the
decode partial buffers are oversized and sentinel-filled (their tails are checked), and the chunk
tickets must be zero after two back-to-back launches.  Each test prints the largest deviation / A64
it saw (``MEASURED attn_<kernel>_<family>``; run with -s) before it asserts.

Out of scope: the chained launch's attention phase (mq_body FINE, 8 waves, plan modes) cannot be
run apart from its GEMM phases; nothing here covers it.
"""
import contextlib
import functools
from types import SimpleNamespace

import pytest
import torch

import kernel_oracle as ko
import voice_enabled_browser_automation_amd.ops as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
I32 = torch.int32
CASES = ko.attn_cases()


@pytest.fixture(scope="module", autouse=True)
def _native():
    ops.ext()  # fail loudly if the extension is missing
    yield
    ops.set_attention_impl("mq")


def measured(name: str, value: float) -> None:
    print(f"MEASURED {name} {value:.6g}")


@functools.lru_cache(maxsize=None)
def case(cid):
    return CASES[cid][1]()


@functools.lru_cache(maxsize=None)
def reference(cid, kernel, layout="paged"):
    """Computed once per (case, score operand, layout) and shared; nothing changes it."""
    c = case(cid)
    return c.reference(kernel, c.contiguous() if layout == "contiguous" else None)


def params(prefix):
    """(case id, kernel) pairs of one group of the shared table (the split kernel has no G = 16)."""
    return [(cid, k) for cid in ko.attn_ids(prefix) for k in CASES[cid][0]]


@contextlib.contextmanager
def launches(what: str):
    """A device error (a fault, not a wrong value) ends the session: nothing more is launched on a
    device that has faulted."""
    try:
        yield
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory" in str(e) or "hipError" in str(e):
            pytest.exit(f"device error in {what}: {e}", returncode=3)
        raise


def strided(t: torch.Tensor, pad=(8, 8)) -> torch.Tensor:
    wide = torch.full((t.shape[0], pad[0] + t.shape[1] + pad[1]), 7.0, dtype=t.dtype, device=DEV)
    wide[:, pad[0]: pad[0] + t.shape[1]] = t.to(DEV)
    return wide[:, pad[0]: pad[0] + t.shape[1]]


# ----------------------------------------------------------------------------- decode
def run_decode(c, kernel, *, max_ctx, n_splits=None, shared=False, sliced=False):
    """Two back-to-back launches -> the output [R, nq * hd]; canary, partial tails and tickets checked."""
    ops.set_attention_impl(kernel)
    R, W = len(c.ctx), c.nq * c.hd
    q = strided(c.q)
    kv = c.paged(DEV)
    ctx_lens = torch.tensor(c.ctx, dtype=I32, device=DEV)
    seq_ids = torch.tensor(c.seqs, dtype=I32, device=DEV)
    ns = min(n_splits or 1 << 30, ops.decode_n_splits(max_ctx))
    rl = min(R, 64) if sliced else R  # rows per launch
    used_o = rl * ns * W if ns > 1 else 0  # (n_splits == 1: no partials at all)
    used_ml = rl * ns * c.nq * 2 if ns > 1 else 0
    part_o = torch.full((rl * ns * W + 4096,), ko.SENTINEL, dtype=torch.float32, device=DEV)
    part_ml = torch.full((rl * ns * c.nq * 2 + 4096,), ko.SENTINEL, dtype=torch.float32, device=DEV)
    counters = torch.zeros(max(R, 64) * c.nkv + 64, dtype=I32, device=DEV)
    out, check = ko.canary((R, W), cols=(8, 8), device=DEV)
    sh = torch.tensor([c.P, c.n_real], dtype=I32, device=DEV) if shared else None
    fn = ops.decode_attention_rows if sliced else ops.decode_attention
    kw = dict(n_q_heads=c.nq, n_kv_heads=c.nkv, head_dim=c.hd, scale=c.scale, max_ctx=max_ctx, out=out,
              part_o=part_o, part_ml=part_ml, counters=counters, n_splits=n_splits)
    if shared:
        kw["shared"] = sh
    what = f"{kernel} max_ctx={max_ctx} n_splits={n_splits} shared={shared}"
    with launches(what):
        fn(q, kv, ctx_lens, seq_ids, **kw)
        first = out.clone()
        fn(q, kv, ctx_lens, seq_ids, **kw)
    check(what)
    assert int(counters.abs().sum()) == 0, f"{what}: chunk tickets left non-zero"
    assert bool(ko.untouched(part_o[used_o:]).all()), f"{what}: wrote past the partial outputs"
    assert bool(ko.untouched(part_ml[used_ml:]).all()), f"{what}: wrote past the partial (m, l)"
    assert torch.equal(first, out), f"{what}: the second launch differs from the first"
    return out


def check_decode(cid, kernel, **kw):
    c = case(cid)
    out = run_decode(c, kernel, **kw)
    m = ko.check_attention(c, kernel, out, f"{cid} {kernel} {kw}", refs=reference(cid, kernel))
    measured(f"attn_{kernel}_{c.family}", m)


@pytest.mark.parametrize("n_splits", [1, 3])
@pytest.mark.parametrize("max_ctx", [640, 2048])
@pytest.mark.parametrize("cid,kernel", params("sweep"))
def test_decode_context_sweep(cid, kernel, max_ctx, n_splits):
    """20 single-row sequences with contexts around every 32-key step, wave range and chunk edge;
    n_splits = 1 writes every row directly (no partials), 3 merges chunks; max_ctx changes the grid."""
    check_decode(cid, kernel, max_ctx=max_ctx, n_splits=n_splits)


@pytest.mark.parametrize("cid,kernel", params("group"))
def test_decode_row_groups(cid, kernel):
    """Runs of RG - 1 .. 2 RG + 1 rows of one sequence with consecutive contexts from 30, 126, 254."""
    check_decode(cid, kernel, max_ctx=640)


@pytest.mark.parametrize("cid,kernel", params("zero"))
def test_decode_zero_context_rows_are_zeros(cid, kernel):
    """A row without keys gets zeros (DecodeAttnParams::out), beside live rows of its group and in a
    group of such rows only: the canary view would still hold the sentinel where nothing was stored."""
    check_decode(cid, kernel, max_ctx=640)
    check_decode(cid, kernel, max_ctx=640, n_splits=1)


@pytest.mark.parametrize("cid,kernel", params("multi"))
def test_decode_mq_multi_item_loop(cid, kernel):
    """64 rows x 20 kv heads: 1280 items on 512 workgroups (mq_body's item += grid loop)."""
    check_decode(cid, kernel, max_ctx=256)


@pytest.mark.parametrize("cid,kernel", params("sliced"))
def test_decode_rows_beyond_one_launch(cid, kernel):
    """decode_attention_rows: 65 and 130 rows in 64-row slices that reuse the partial buffers."""
    check_decode(cid, kernel, max_ctx=640, sliced=True)


@pytest.mark.parametrize("cid,kernel", params("shared"))
def test_decode_shared_prefix(cid, kernel):
    """The shared-prefix cascade and the per-session grouping, each against the oracle: every
    session's own blocks carry its own code, so keys of another session are seen exactly."""
    check_decode(cid, kernel, max_ctx=ko.SHARED_MAX_CTX, shared=True)
    check_decode(cid, kernel, max_ctx=ko.SHARED_MAX_CTX, shared=False)


# ----------------------------------------------------------------------------- flash
def run_flash(c, layout, **kw):
    """q: a strided view of a fused QKV buffer; out: a canary view.  -> [B * Sq, Hq * D]"""
    B, Sq, W = c.B, c.Sq, c.nq * c.hd
    fused = torch.full((B * Sq, W + 2 * c.nkv * c.hd), 7.0, dtype=BF, device=DEV)
    fused[:, :W] = c.q.to(DEV)
    q = fused[:, :W].view(B, Sq, c.nq, c.hd)
    kv = c.contiguous(DEV) if layout == "contiguous" else c.paged(DEV)
    out2, check = ko.canary((B * Sq, W), cols=(8, 8), device=DEV)
    with launches(f"flash {layout} {kw}"):
        ops.flash_attention(q, kv, Sk=c.Sk, n_kv_heads=c.nkv, causal=c.causal, scale=c.scale,
                            out=out2.view(B, Sq, c.nq, c.hd), **kw)
    check(f"flash {layout} {kw}")
    return out2


@pytest.mark.parametrize("cid,kernel", params("flash"))
def test_flash_non_causal(cid, kernel):
    """Sq around the 32-query wave and 128-query block, Sk around the 64-key tile; contiguous K/V
    physically longer than Sk (the keys past Sk carry the family's code)."""
    c = case(cid)
    out = run_flash(c, "contiguous")
    m = ko.check_attention(c, kernel, out, cid, refs=reference(cid, kernel, "contiguous"))
    measured(f"attn_flash_{c.family}", m)


@pytest.mark.parametrize("cid,kernel", params("causal"))
def test_flash_causal_paged(cid, kernel):
    """q_offset = Sk - Sq (0, and the prefix form), paged: counting gives every query's key count,
    retrieval aims at the diagonal key and at the first masked one."""
    c = case(cid)
    out = run_flash(c, "paged", q_offset=c.q_offset)
    m = ko.check_attention(c, kernel, out, cid, refs=reference(cid, kernel))
    measured(f"attn_flash_{c.family}", m)


@pytest.mark.parametrize("cid,kernel", params("runs"))
def test_flash_per_batch_lengths(cid, kernel):
    """B = 3 with distinct k_lens / q_offsets, one run shorter than S (its padding queries are
    computed, stay inside out[b] and are not compared), one with a single key."""
    c = case(cid)
    R, W = len(c.ctx), c.nq * c.hd
    k_lens = torch.tensor(c.k_lens, dtype=I32, device=DEV)
    q_offsets = torch.tensor(c.q_offsets, dtype=I32, device=DEV)
    if cid.endswith("-direct"):
        out = run_flash(c, "paged", k_lens=k_lens, q_offsets=q_offsets)
    else:
        dst = c.real.nonzero().flatten().to(DEV)
        runs = SimpleNamespace(B=c.B, S=c.Sq, dst=dst, q_offsets=q_offsets, k_lens=k_lens, table=c.table.to(DEV),
                               max_k=c.Sk)
        got = torch.full((int(c.real.sum()), W), ko.SENTINEL, dtype=BF, device=DEV)
        with launches("flash_attention_runs"):
            ops.flash_attention_runs(c.q.to(DEV)[dst].contiguous(), c.kc.to(DEV), c.vc.to(DEV), runs, n_q_heads=c.nq,
                                     n_kv_heads=c.nkv, head_dim=c.hd, scale=c.scale, out=got)
        out = torch.zeros(R, W, dtype=BF)
        out[c.real] = got.cpu()
    m = ko.check_attention(c, kernel, out, cid, rows=c.real, refs=reference(cid, kernel))
    measured(f"attn_flash_{c.family}", m)
