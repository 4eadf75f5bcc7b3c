"""Native build driver (no setuptools/hipify involved).

The gfx950 HIP kernel libraries, one row of ``KERNEL_LIBS`` each:

================  ====================  ===============================================
sources           library               what
================  ====================  ===============================================
``csrc/kernels``  ``_vwa_kernels.so``   the main kernel library (GEMMs, attention, ...)
``csrc/align``    ``_vwa_align.so``     word alignment
``csrc/sot``      ``_vwa_sot.so``       start-of-transcript probe
``csrc/beam``     ``_vwa_beam.so``      beam search steps
``csrc/boost``    ``_vwa_boost.so``     keyterm boosting step
``csrc/tsrules``  ``_vwa_tsrules.so``   timestamp rules step
``csrc/score``    ``_vwa_score.so``     transcript score step
``csrc/turn``     ``_vwa_turn.so``      set log-probability (turn-completion probe)
``csrc/nucleus``  ``_vwa_nucleus.so``   repetition penalty, top-k / top-p mask step
``csrc/ingest``   ``_vwa_ingest.so``    wire audio: G.711 / PCM16 decode, downmix, resample
``csrc/rescore``  ``_vwa_rescore.so``   per-sequence log-probabilities (n-best rescoring)
================  ====================  ===============================================

Every ``*.hip`` of a library's directory is compiled with ``hipcc --offload-arch=gfx950`` into its
own object (parallel, incremental), its ``bindings.cpp`` (the main library's: ``csrc/bindings.cpp``)
is compiled against the torch headers, and the lot is linked against torch's own HIP runtime (same
``libamdhip64.so.7`` soname, so one HIP runtime per process).

``_vwa_native.so`` is the CPU runtime library (grammar engine, KV block manager): plain C++17 with
pybind11, built with g++.

All land in-tree next to this file so they travel with the repo snapshot to the GPU box.
Run: ``python -m voice_enabled_browser_automation_amd.ops.build [--force]``.
"""
from __future__ import annotations

import concurrent.futures as cf
import glob
import os
import subprocess
import sys
import sysconfig

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(REPO, "csrc")
BUILD = os.path.join(REPO, "build", "native")
ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# (source directory under csrc/, extension name); the first row is the main library
KERNEL_LIBS = (("kernels", "_vwa_kernels"), ("align", "_vwa_align"), ("sot", "_vwa_sot"), ("beam", "_vwa_beam"),
               ("boost", "_vwa_boost"), ("tsrules", "_vwa_tsrules"), ("score", "_vwa_score"), ("turn", "_vwa_turn"),
               ("nucleus", "_vwa_nucleus"), ("ingest", "_vwa_ingest"), ("rescore", "_vwa_rescore"))
(KERNEL_SO, ALIGN_SO, SOT_SO, BEAM_SO, BOOST_SO, TSRULES_SO, SCORE_SO, TURN_SO, NUCLEUS_SO, INGEST_SO,
 RESCORE_SO) = (
    os.path.join(HERE, ext_name + ".so") for _, ext_name in KERNEL_LIBS)
NATIVE_SO = os.path.join(HERE, "_vwa_native.so")
# headers any library's sources may include, besides those of its own directory
SHARED_HEADERS = [os.path.join(CSRC, "torch_checks.h"), os.path.join(CSRC, "kernels", "common.h"),
                  os.path.join(CSRC, "kernels", "logit_row.h")]


def _torch_paths():
    import torch

    root = os.path.dirname(torch.__file__)
    inc = [os.path.join(root, "include"), os.path.join(root, "include", "torch", "csrc", "api", "include")]
    lib = os.path.join(root, "lib")
    abi = int(torch._C._GLIBCXX_USE_CXX11_ABI)
    return inc, lib, abi


def _py_include():
    return sysconfig.get_paths()["include"]


def _pybind_include():
    import pybind11

    return pybind11.get_include()


def _newer(target: str, deps: list[str]) -> bool:
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(d) <= t for d in deps)


def _run(cmd: list[str]) -> None:
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout)
        raise RuntimeError("build step failed: " + " ".join(cmd[:6]) + " ...")


def _build_kernel_lib(sub: str, ext_name: str, force: bool, jobs: int) -> str:
    """One row of KERNEL_LIBS: csrc/<sub>/*.hip + csrc/<sub>/bindings.cpp -> <ext_name>.so, objects under
    build/native/<sub>.  The main library's bindings are csrc/bindings.cpp and its objects build/native."""
    main = sub == KERNEL_LIBS[0][0]
    so = os.path.join(HERE, ext_name + ".so")
    bdir = BUILD if main else os.path.join(BUILD, sub)
    os.makedirs(bdir, exist_ok=True)
    inc, lib, abi = _torch_paths()
    headers = glob.glob(os.path.join(CSRC, sub, "*.h")) + SHARED_HEADERS
    common = [HIPCC, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result",
              "-I", os.path.join(CSRC)] + os.environ.get("VWA_HIPCC_EXTRA", "").split()  # (utils/env.py Settings documents it; build.py stays import-light)
    jobs_list = []
    objs = []
    for src in sorted(glob.glob(os.path.join(CSRC, sub, "*.hip"))):
        obj = os.path.join(bdir, os.path.basename(src) + ".o")
        objs.append(obj)
        if force or not _newer(obj, [src] + headers):
            jobs_list.append(common + ["-c", src, "-o", obj])
    bind_src = os.path.join(CSRC, "bindings.cpp") if main else os.path.join(CSRC, sub, "bindings.cpp")
    bind_obj = os.path.join(bdir, "bindings.o")
    objs.append(bind_obj)
    if force or not _newer(bind_obj, [bind_src] + headers):
        cmd = common + ["-c", bind_src, "-o", bind_obj, f"-D_GLIBCXX_USE_CXX11_ABI={abi}",
                        f"-DTORCH_EXTENSION_NAME={ext_name}", "-DUSE_ROCM=1", "-I", _py_include()]
        for i in inc:
            cmd += ["-I", i]
        jobs_list.append(cmd)
    with cf.ThreadPoolExecutor(max_workers=jobs) as ex:
        list(ex.map(_run, jobs_list))
    if force or jobs_list or not _newer(so, objs):
        _run([HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", so] + objs + [
            "-L", lib, "-ltorch", "-ltorch_cpu", "-ltorch_python", "-lc10", "-lc10_hip", "-ltorch_hip",
            f"-Wl,-rpath,{lib}"])
    return so


def build_kernels(force: bool = False, jobs: int = 8) -> str:
    """The main kernel library: csrc/kernels + csrc/bindings.cpp -> _vwa_kernels.so."""
    return _build_kernel_lib(*KERNEL_LIBS[0], force, jobs)


def build_native(force: bool = False) -> str:
    """CPU runtime library (grammar engine + block manager) -- g++ / pybind11."""
    srcs = sorted(glob.glob(os.path.join(CSRC, "runtime", "*.cpp")))
    hdrs = glob.glob(os.path.join(CSRC, "runtime", "*.h"))
    if not srcs:
        return ""
    if not force and _newer(NATIVE_SO, srcs + hdrs):
        return NATIVE_SO
    ext = sysconfig.get_config_var("EXT_SUFFIX")  # noqa: F841 (plain .so name is importable)
    cmd = ["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-fvisibility=hidden", "-I", _py_include(),
           "-I", _pybind_include(), "-I", os.path.join(CSRC, "runtime"), "-o", NATIVE_SO] + srcs
    _run(cmd)
    return NATIVE_SO


def build_all(force: bool = False) -> list[str]:
    # the libraries build side by side: the main library's longest source (skinny_stream.hip, all the
    # chained-layer instantiations in one translation unit) takes minutes on one core, and the ten
    # small libraries and the CPU runtime, a few minutes one after the other, fit beside it
    with cf.ThreadPoolExecutor(max_workers=len(KERNEL_LIBS) + 1) as ex:
        native = ex.submit(build_native, force)
        libs = [ex.submit(_build_kernel_lib, sub, ext_name, force, 8 if i == 0 else 2)
                for i, (sub, ext_name) in enumerate(KERNEL_LIBS)]
        n = native.result()
        return ([n] if n else []) + [f.result() for f in libs]


if __name__ == "__main__":
    print(build_all(force="--force" in sys.argv))
