"""The lossless 13-bit weight form of the chained decode layer (ops.pack_weight, vwa_kernels.h
SkinnyParams::w_pack) on the CPU: every block that is not flagged decodes to its bf16 bits -- with a
decoder written here from the format's description, element by element, not with the packer's own
unpack -- and the flagged blocks are exactly those that hold a value the codes cannot express."""
import numpy as np
import pytest
import torch

from voice_enabled_browser_automation_amd import ops

N, K = 256, 512  # 16 tiles x 4 k-groups = 64 blocks of 2048 weights


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).numpy().astype(np.int64) & 0xFFFF


def _decode(pw: ops.PackedWeight) -> np.ndarray:
    """bf16 bits [blocks, s, lane, e] of every block, from the documented layout."""
    data = pw.data.numpy().astype(np.int64)
    body = data[:pw.blocks * ops.PACK_BLOCK].reshape(pw.blocks, ops.PACK_BLOCK)
    s, lane, e = np.meshgrid(np.arange(4), np.arange(64), np.arange(8), indexing="ij")
    q, i = e >> 2, e & 3
    lo = body[:, (s >> 1) * 1024 + lane * 16 + (s & 1) * 8 + e]
    code = (body[:, 2048 + lane * 16 + s * 4 + i] >> (4 * q)) & 15
    sign = (body[:, 3072 + lane * 4 + i] >> (2 * s + q)) & 1
    return lo | ((pw.base + code) << 8) | (sign << 15)


def _check(w: torch.Tensor, expect_flagged=None):
    t = ops.tile_weight(w)
    pw = ops.pack_weight(t)
    want = _bits(t).reshape(-1, 4, 64, 8)
    hi7 = (want >> 8) & 0x7F
    finite = ((want >> 7) & 0xFF) != 0xFF
    base = max(0, int(np.where(finite, hi7, 0).max()) - (ops.PACK_WINDOW - 1))
    assert pw.base == base and 0 <= base <= 112
    bad = ((hi7 < base) | (hi7 > base + ops.PACK_WINDOW - 1)).reshape(pw.blocks, -1).any(axis=1)
    flags = pw.flags.numpy() != 0
    assert np.array_equal(flags, bad), "flagged blocks are not exactly those with an inexpressible value"
    assert pw.n_flagged == int(bad.sum())
    got = _decode(pw)
    assert np.array_equal(got[~bad], want[~bad])
    # the packer's own unpack (the kernel's arithmetic) agrees, and the tiling round-trips
    back = ops.unpack_weight(pw, t.shape)
    assert np.array_equal(_bits(back).reshape(-1, 4, 64, 8)[~bad], want[~bad])
    assert torch.equal(ops.untile_weight(t).view(torch.int16), w.view(torch.int16))
    assert pw.data.numel() == pw.blocks * (ops.PACK_BLOCK + 1)  # 13 bits per weight + one flag byte per block
    if expect_flagged is not None:
        assert int(bad.sum()) == expect_flagged
    return pw, bad


@pytest.mark.parametrize("std,seed", [(0.02, 1), (0.006, 2)])
def test_normal_weights_pack_without_a_flagged_block(std, seed):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) * std).to(torch.bfloat16)
    _check(w, expect_flagged=0)


def _block_of(row: int, col: int) -> int:
    return (row // 16) * (K // 128) + col // 128


def test_zeros_denormals_inf_and_nan_are_flagged_and_nothing_else():
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16)
    bits = w.view(torch.int16)
    spots = {(0, 0): 0x0000, (17, 130): -0x8000, (40, 300): 0x0001, (40, 301): -0x7F81,  # +-0, +-denormal
             (100, 5): 0x7F80, (101, 200): -0x80, (200, 500): 0x7FC1, (255, 511): -0x3F}  # +-Inf, NaNs
    for (r, c), v in spots.items():
        bits[r, c] = v
    pw, bad = _check(w)
    assert set(np.nonzero(bad)[0]) == {_block_of(r, c) for r, c in spots}


def test_sixty_binades_keep_the_top_window_and_flag_the_rest():
    # column c holds +-2^(10 - c % 60): every 128-wide k-group spans all 60 binades
    e = 10 - (torch.arange(K) % 60)
    w = (torch.pow(2.0, e.float())[None, :] * torch.where(torch.arange(N)[:, None] % 2 == 0, 1.0, -1.0)).to(torch.bfloat16)
    pw, bad = _check(w)
    assert bad.all()
    # and a tensor whose small values sit in one k-group only: the others stay packed
    w2 = torch.full((N, K), 0.5, dtype=torch.bfloat16)
    w2[:, 128:256] = w[:, 128:256]
    pw2, bad2 = _check(w2)
    assert set(np.nonzero(bad2)[0]) == {t * (K // 128) + 1 for t in range(N // 16)}


def test_all_zero_tensor_packs_with_base_zero():
    pw, bad = _check(torch.zeros(N, K, dtype=torch.bfloat16), expect_flagged=0)
    assert pw.base == 0


def test_every_bf16_bit_pattern_survives_pack_or_flag():
    """All 65536 patterns (twice over, shuffled): each is either decoded to itself or sits in a
    flagged block, whatever the base."""
    g = torch.Generator().manual_seed(4)
    v = torch.arange(N * K, dtype=torch.int32) % 65536
    v = v[torch.randperm(N * K, generator=g)]
    w = (((v ^ 0x8000) - 0x8000).to(torch.int16)).view(torch.bfloat16).view(N, K)
    _check(w)
