"""The kernel bindings reject host tensors in their own validation (csrc/bindings.cpp), before
anything reaches the HIP runtime: every exported entry point that takes tensors is called with
well-shaped, right-dtype CPU tensors at the smallest legal shapes and must raise a RuntimeError
that names the offending argument.

Runs only where there is NO GPU: on a GPU machine a missed device check would hand a host pointer
to a kernel, and this file must never be the thing that does that."""
import os
import re

import pytest
import torch

import voice_enabled_browser_automation_amd.ops as ops
from voice_enabled_browser_automation_amd.ops.build import KERNEL_SO

BF, F32, I32, I64 = torch.bfloat16, torch.float32, torch.int32, torch.int64
NQ, NKV, HD, K = 2, 1, 16, 128  # the smallest QKV geometry: 64 projection rows


def z(*shape, dtype=BF):
    return torch.zeros(*shape, dtype=dtype)


def _qkv(M):
    """(n_q_heads .. v_cache): the QKV-epilogue operand tail of the three QKV entry points."""
    return (NQ, NKV, HD, True, z(M, dtype=I32), z(M, dtype=I64), z(32, HD // 2, 2, dtype=F32), z(M, NQ * HD),
            z(2, NKV, 16, HD), z(2, NKV, 16, HD))


def _conv_x():
    buf = z(1, 6, 128)
    return buf[:, 1:5]


def _wdec_bufs():
    # ints: n_layers, d, H, ffn, T, block_size, bt_stride, nch, ch_len, sessions, grid
    return [z(128), z(128), z(128), z(128), z(512), z(2 * 1 * 68 + 3 * 128, dtype=F32), z(1, dtype=I32),
            z(1, dtype=I32), z(1, dtype=I64), z(1, dtype=I32), z(1, dtype=I32), z(2 * (1280 + 32), dtype=I32)]


X1, X17 = (1, K), (17, K)
# entry point -> (the argument its message must name -- alternatives where which of two host tensors is
# seen first is incidental -- and a builder of CPU arguments)
CASES = {
    "quant_fp8_rows": ("x", lambda: (z(*X1), z(*X1, dtype=torch.float8_e4m3fn), z(1, dtype=F32))),
    "ar_allreduce": ("in", lambda: (0, z(8), z(8))),
    "ar_gather": ("in", lambda: (0, z(4, dtype=I32), z(8, dtype=I32))),
    "skinny_gemm": ("x", lambda: (z(*X1), z(16, K), None, z(1, 16), 0, False, 1e-5, None)),
    "skinny_gemm_swiglu": ("x", lambda: (z(*X1), z(32, K), None, z(1, 16), False, 1e-5)),
    "skinny_gemm_qkv": ("x", lambda: (z(*X1), z(64, K), None, False, 1e-5) + _qkv(1)),
    "chain_make": ("h|bar", lambda: (z(*X1), z(*X1), z(*X1), z(K, K), z(2 * K, K), z(K, K), 1e-5, None, NQ, NKV, HD,
                                     None, None, None, None, None, None, z(384, dtype=I32), z(12289, dtype=I32))),
    "chain_make_seq": ("X|bar", lambda: (1, [z(*X1)] * 2, [z(K, K)] * 2, [None] * 2, [None] * 2, [z(*X1)] * 2, [0, 0],
                                         1e-5, 2, 64, None, None, None, None, z(384, dtype=I32),
                                         z(12289, dtype=I32))),
    "chain_run": ("like|desc", lambda: (z(64, dtype=torch.uint8), 3, 0, z(1))),
    "alloc_uncached_i32": ("like", lambda: (4, z(1))),
    "device_cus": ("like", lambda: (z(1),)),
    "wdec_layers": ("like|flat", lambda: ([z(K, K), None, None] * 7 + [z(16)] * 4, 1, z(1))),
    "wdec_run": ("bufs|layers", lambda: (z(8, dtype=torch.uint8), z(32, dtype=I32), _wdec_bufs(),
                                         [1, 128, 2, 512, 4, 16, 1, 1, 4, 1, 1], 1e-5, 0.125, [1] * 8)),
    "decode_advance": ("tokens", lambda: (z(1, dtype=I32), z(1, dtype=I32), z(1, dtype=I32), z(1, dtype=I64),
                                          z(1, dtype=I32), z(4, dtype=I32), z(1, dtype=I32), 0, 16)),
    "gemm": ("x", lambda: (z(*X17), z(16, K), None, z(17, 16), 0)),
    "row_rstd": ("x", lambda: (z(*X17), z(17, dtype=F32), 1e-5)),
    "gemm_qkv": ("x", lambda: (z(*X17), None, z(64, K), None, None, None, False, z(4096, dtype=F32)) + _qkv(17)),
    "gemm_fp8": ("x8", lambda: (z(*X17), None, z(16, K, dtype=torch.float8_e4m3fn), z(16, dtype=F32), None,
                                z(17, 16), 0)),
    "rmsnorm": ("x", lambda: (z(*X1), None, None, z(K), z(*X1), 1e-5)),
    "layernorm": ("x", lambda: (z(*X1), None, None, z(K), z(K), z(*X1), 1e-5)),
    "rope_kv_write": ("qkv", lambda: (z(1, 64),) + _qkv(1)),
    "swiglu": ("gu", lambda: (z(1, 32), z(1, 16))),
    "bias_act": ("x", lambda: (z(1, 16), None, None, z(1, 16), 0)),
    "decode_attention": ("q", lambda: (z(1, 128), z(1, 1, 16, 64), z(1, 1, 16, 64), z(1, 1, dtype=I32), 16, 1024, 1024,
                                       64, z(1, dtype=I32), z(1, dtype=I32), 2, 1, 64, 0.125, 1, z(128, dtype=F32),
                                       z(4, dtype=F32), z(1, dtype=I32), z(1, 128), None)),
    "flash_attention": ("q", lambda: (z(1, 1, 1, 64), z(1, 1, 16, 64), z(1, 1, 16, 64), z(1, 1, dtype=I32), 16, 1024,
                                      1024, 64, z(1, 1, 1, 64), 1, 1, False, 0, None, None, 0.125)),
    "embedding": ("ids|table", lambda: (z(1, dtype=I32), z(4, 16), None, None, z(1, 16), 0)),
    "sample": ("logits", lambda: (z(1, 32, dtype=F32), None, None, z(1, dtype=I64), z(1, dtype=I32), z(1, dtype=I32),
                                  z(1, dtype=F32), z(1, dtype=I32))),
    "sample_tp": ("logits", lambda: (z(1, 32, dtype=F32), None, None, z(1, dtype=I64), z(1, dtype=I32),
                                     z(1, dtype=I32), z(2, dtype=I32), z(2, dtype=I32), 1, None, 0, 1, 1)),
    "pcm16_to_f32": ("pcm", lambda: (z(8, dtype=torch.int16), z(8, dtype=F32), 1.0)),
    "log_mel": ("audio", lambda: (z(480, dtype=F32), 1, z(400, dtype=F32), z(26 * 25 * 64 * 4, dtype=F32),
                                  z(13 * 64 * 4, dtype=F32), 16, z(16, dtype=F32), z(1, dtype=F32), z(1, 16))),
    "conv1d_gelu": ("x", lambda: (_conv_x(), z(16, 384), None, None, z(1, 4, 16), 1, False)),
}
# tensor-taking entry points that take HOST tensors by contract (nothing to reject)
HOST_ONLY = {"ar_open_peer"}  # (the peer's IPC handle bytes)


@pytest.fixture(scope="module")
def E():
    if not os.path.exists(KERNEL_SO):
        pytest.skip("kernel library not built here (python -c 'import __graft_entry__ as g; g.build()')")
    if torch.cuda.is_available():
        pytest.skip("host tensors are only ever offered to the bindings where there is no GPU to launch on")
    return ops.ext()


@pytest.mark.parametrize("name", sorted(CASES))
def test_cpu_tensors_are_rejected_by_the_binding(E, name):
    arg, build = CASES[name]
    with pytest.raises(RuntimeError) as ei:
        getattr(E, name)(*build())
    msg = str(ei.value).splitlines()[0]
    assert "HIP error" not in str(ei.value) and "no ROCm-capable device" not in str(ei.value), msg
    assert re.search(rf"\b({arg})\b", msg), f"{name}: message does not name {arg!r}: {msg}"


def test_every_tensor_taking_entry_point_has_a_case(E):
    """A binding added later without a case here fails: the pybind signature (first docstring
    line, arguments only) of every public callable is searched for tensor parameters."""
    takes = {n for n in dir(E) if not n.startswith("_") and callable(getattr(E, n))
             and "Tensor" in (getattr(E, n).__doc__ or "").splitlines()[0].split("->")[0]}
    assert takes == set(CASES) | HOST_ONLY, (sorted(takes - set(CASES) - HOST_ONLY), sorted(set(CASES) - takes))
