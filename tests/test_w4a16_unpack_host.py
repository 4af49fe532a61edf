"""Host-side check of the fp16 GEMV family's int4 -> fp16 unpack (tinychatengine_amd/csrc/w4a16_unpack16.hpp): compiled as plain C++ with the
clang++ that hipcc drives (the header computes in _Float16, which the system g++ does not have on the host) and run here, no GPU involved."""
import os
import shutil
import subprocess

from tinychatengine_amd import build as tce_build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rocm_clang() -> str:
    hipcc = os.path.realpath(tce_build._hipcc())
    roots = [os.path.dirname(os.path.dirname(hipcc)), os.environ.get("ROCM_PATH", "/opt/rocm")]
    for cand in [os.path.join(r, sub, "clang++") for r in roots for sub in (os.path.join("llvm", "bin"), os.path.join("lib", "llvm", "bin"))] + [shutil.which("amdclang++")]:
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError(f"no clang++ next to {hipcc}")


def test_w4a16_unpack_is_exact_and_pair_ordered(tmp_path):
    exe = tmp_path / "test_w4a16_unpack"
    subprocess.check_call([_rocm_clang(), "-std=c++17", "-O1", "-Wall", "-I", os.path.join(REPO, "tinychatengine_amd", "csrc"),
                           os.path.join(REPO, "tests", "host", "test_w4a16_unpack.cc"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "w4a16 unpack ok" in r.stdout, r.stdout + r.stderr
