"""Register budget of the packed-weight chain (skinny_stream.hip chain_kernel PK, CPU: the gfx950
code object metadata of the in-tree build): its register sets are 14 instead of 16 registers of 16
bytes, which leaves room for the decode temporaries -- every packed instantiation (3- and 4-phase
tails, GQA 4 and 8, one launch per layer and one for all layers) must use no scratch."""
from test_kernel_resources_cpu import _kernels


def _packed(name: str) -> bool:
    # chain_kernel<KS, SEQ, NPH, AG, WA, XG2, F8, O2, D2, MULTI, PK>: the last template argument
    return "chain_kernel" in name and name.endswith("Lb1EEEvPK11ChainParamsi")


def test_packed_chain_kernels_do_not_spill():
    ks = {k: v for k, v in _kernels("skinny_stream.hip.o").items() if _packed(k)}
    assert len(ks) == 6, sorted(ks)
    bad = {k: v for k, v in ks.items() if v[0] > 0}
    assert not bad, f"packed chain kernels use scratch (spills): {bad}"
    assert all(v[1] <= 256 for v in ks.values()), ks
