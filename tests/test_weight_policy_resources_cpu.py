"""Register budget of the non-temporal weight-stream instantiations (skinny_stream.hip
chain_wnt_kernel = chain_body WA 2; skinny_stream_kernel / skinny_fp8_kernel AUX 2; CPU: the gfx950
code object metadata of the in-tree build).  The policy is two bits of each weight load's encoding:
every nt kernel must exist, use no scratch, and allocate exactly the VGPRs of its default-policy
twin -- and nothing but what a Llama decode step launches has an nt form.

The fp8 streaming kernel's twins are its tiled-only forms (TILED): with the run-time layout branch the
compiler merges the tiled and the row-major load of a k-group only when both have one policy, and
the nt form then allocated one VGPR more (159 / 160 / 165 vs 158 / 159 / 164); tiled fp8 weights now
run the form without the row-major branch under either policy."""
import pytest

from test_kernel_resources_cpu import _kernels


def _chain_pairs():
    """(nt kernel, default-policy twin) mangled-name tails: packed, bf16 with o_nt2 and fp8 (F8, O2,
    PK) x one launch for all layers, 4- and 3-phase single layers (MULTI, NPH) x GQA group 4 and 8."""
    out = []
    for f8, o2, pk in ((0, 1, 1), (0, 1, 0), (1, 0, 0)):
        for multi, nph in ((1, 4), (0, 4), (0, 3)):
            for g in (4, 8):
                out.append((f"16chain_wnt_kernelILi{nph}ELi{g}ELb{f8}ELb{o2}ELb{multi}ELb{pk}EEEvPK11ChainParamsi",
                            f"12chain_kernelILi8ELi0ELi{nph}ELi{g}ELi0ELb0ELb{f8}ELb{o2}ELb0ELb{multi}ELb{pk}EEEvPK11ChainParamsi"))
    return out


def _stream_pairs():
    """Store, residual (X in LDS and streamed with the weights), SwiGLU and QKV at 8 waves."""
    return [tuple(f"20skinny_stream_kernelILi{epi}ELi{nt}ELi8ELb{xg}ELi1ELi{aux}EEEv12SkinnyParamsiii" for aux in (2, 0))
            for epi, nt, xg in ((0, 1, 0), (1, 1, 0), (1, 1, 1), (2, 2, 0), (4, 1, 0))]


def _fp8_pairs():
    """The fp8 twin kernel (its tiled-only form): store, residual, SwiGLU, QKV at 8 waves."""
    return [tuple(f"17skinny_fp8_kernelILi{epi}ELi{nt}ELi8ELi{aux}ELb1EEEv12SkinnyParamsii" for aux in (2, 0))
            for epi, nt in ((0, 1), (1, 1), (2, 2), (4, 1))]


FAMILIES = {"chain": _chain_pairs, "bf16-stream": _stream_pairs, "fp8-stream": _fp8_pairs}


def _find(ks, tail):
    hit = [k for k in ks if k.endswith(tail)]
    assert len(hit) == 1, (tail, hit)
    return ks[hit[0]]


def test_nt_kernels_exist_and_do_not_spill():
    ks = _kernels("skinny_stream.hip.o")
    pairs = [p for f in FAMILIES.values() for p in f()]
    assert len(pairs) == 18 + 5 + 4
    bad = {nt: _find(ks, nt) for nt, _ in pairs if _find(ks, nt)[0] > 0}
    assert not bad, f"nt kernels use scratch (spills): {bad}"
    assert all(_find(ks, nt)[1] <= 256 for nt, _ in pairs)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_nt_vgprs_equal_the_default_policy_twins(family):
    ks = _kernels("skinny_stream.hip.o")
    got = {nt: (_find(ks, nt)[1], _find(ks, twin)[1]) for nt, twin in FAMILIES[family]()}
    print(got)
    diff = {k: v for k, v in got.items() if v[0] != v[1]}
    assert not diff, f"(nt VGPRs, default-policy twin's VGPRs) differ: {diff}"


def test_only_the_llama_decode_forms_have_an_nt_instantiation():
    ks = _kernels("skinny_stream.hip.o")
    chain = [k for k in ks if "chain_wnt_kernel" in k]
    assert len(chain) == 18, sorted(chain)
    stream = [k for k in ks if ("skinny_stream_kernel" in k and k.endswith("Li2EEEv12SkinnyParamsiii"))
              or ("skinny_fp8_kernel" in k and k.endswith("Li2ELb1EEEv12SkinnyParamsii"))]
    assert len(stream) == 9, sorted(stream)
