"""Diagnostic builds of the kernel library for the packed-decode timing cells (skinny_stream.hip
CHAIN_PK_DIAG: WRONG RESULTS by design, timing only).

    python tools/pk_diag_build.py            # after the normal build: gpu_alt/_vwa_kernels_pkdiag{1,2}.so
    VWA_KERNEL_SO=gpu_alt/_vwa_kernels_pkdiag1.so python tools/chain_probe.py --attn --multi 8 --no-stamps --wnt 1 --pack
    VWA_KERNEL_SO=gpu_alt/_vwa_kernels_pkdiag2.so python tools/chain_probe.py --attn --multi 8 --no-stamps --wnt 1

Only skinny_stream.hip is recompiled (with the macro it holds four chained instantiations: about a
minute); every other object is the normal build's.  Nothing the project's build makes changes.
"""
import concurrent.futures as cf
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voice_enabled_browser_automation_amd.ops import build as b  # noqa: E402


def build_one(cell: int) -> str:
    out_dir = os.path.join(b.REPO, "gpu_alt")
    obj_dir = os.path.join(b.BUILD, "pkdiag")
    os.makedirs(out_dir, exist_ok=True)
    os.makedirs(obj_dir, exist_ok=True)
    src = os.path.join(b.CSRC, "kernels", "skinny_stream.hip")
    obj = os.path.join(obj_dir, f"skinny_stream.pkdiag{cell}.o")
    so = os.path.join(out_dir, f"_vwa_kernels_pkdiag{cell}.so")
    b._run([b.HIPCC, f"--offload-arch={b.ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-I", b.CSRC,
            f"-DCHAIN_PK_DIAG={cell}", "-c", src, "-o", obj])
    others = [o for o in sorted(glob.glob(os.path.join(b.BUILD, "*.o"))) if os.path.basename(o) != "skinny_stream.hip.o"]
    assert any(os.path.basename(o) == "bindings.o" for o in others), "run the normal build first"
    _, lib, _ = b._torch_paths()
    b._run([b.HIPCC, f"--offload-arch={b.ARCH}", "-shared", "-fPIC", "-o", so, obj] + others + [
        "-L", lib, "-ltorch", "-ltorch_cpu", "-ltorch_python", "-lc10", "-lc10_hip", "-ltorch_hip", f"-Wl,-rpath,{lib}"])
    return so


if __name__ == "__main__":
    cells = [int(x) for x in sys.argv[1:]] or [1, 2]
    with cf.ThreadPoolExecutor(max_workers=len(cells)) as ex:
        print(list(ex.map(build_one, cells)))
