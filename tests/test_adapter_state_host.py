"""CPU (no GPU): the adapter's host state -- three maps under one mutex, pinned verdict words, the generation counter, the lock-free front cache -- on a model of the
C ABI (tests/host/test_adapter_state.cc: it #includes tinychatengine_amd/adapter/matmul_operator_hip.cc and defines the tce_* functions the adapter calls; nothing of
libtce_hip.so or HIP is linked).  The program is a stand-alone executable, compiled with g++ and run here three times: plain, -fsanitize=address,undefined,
-fsanitize=thread.  Nothing is loaded into this Python process; the environment passes through untouched but for TCE_ADAPTER_PACK.  DESIGN.md 4.6 has the stand-in's rules and the scenarios."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIOS = ("steady state:", "M classes:", "identity:", "forget:", "prepare:", "awq:", "int8 members:", "collisions: 2 tensors", "collisions: 3 tensors", "collisions: 4 tensors",
             "collisions: 9 tensors", "threads:")


def _links(tmp_path, flags):
    """Whether this toolchain links a program with `flags` (a sanitiser's runtime may be missing)."""
    src = tmp_path / "probe.cc"
    src.write_text("int main() { return 0; }\n")
    return subprocess.run(["g++", *flags, str(src), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0


def _build_and_run(tmp_path, name, flags):
    exe = tmp_path / f"test_adapter_state_{name}"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-pthread", *flags, "-I", os.path.join(REPO, "include"),
                           "-I", os.path.join(REPO, "tinychatengine_amd", "adapter"), os.path.join(REPO, "tests", "host", "test_adapter_state.cc"), "-o", str(exe)])
    env = {k: v for k, v in os.environ.items() if k != "TCE_ADAPTER_PACK"}  # (the program's rules are those of the default; everything else passes through)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "adapter state: ok (0 violations)" in r.stdout and "VIOLATION" not in r.stdout
    for s in SCENARIOS:  # every scenario printed its line, and said ok
        lines = [l for l in r.stdout.splitlines() if l.startswith(s)]
        assert len(lines) == 1 and lines[0].endswith(": ok"), (s, lines)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def _sanitiser_flags(tmp_path, flags, static, name):
    """The sanitiser's runtime linked statically where the toolchain can: the program then starts whatever else the environment loads into it.  With only the shared
    runtime, which insists on being the first library of the process, the build is skipped by name where the environment preloads a library of its own."""
    if _links(tmp_path, flags + static):
        return flags + static
    if not _links(tmp_path, flags):
        pytest.skip(f"this toolchain cannot link {flags[0]} ({name})")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip(f"{flags[0]} links only its shared runtime here, which cannot start beside the environment's preloaded library ({name})")
    return flags


def test_adapter_state_plain(tmp_path):
    _build_and_run(tmp_path, "plain", [])


def test_adapter_state_address_undefined(tmp_path):
    """No use of a freed packed copy or workspace (the stand-in's tce_free really frees in this build), no overflow, no undefined behaviour."""
    flags = _sanitiser_flags(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], ["-static-libasan", "-static-libubsan"],
                             "test_adapter_state_address_undefined")
    _build_and_run(tmp_path, "asan_ubsan", flags)


def test_adapter_state_thread(tmp_path):
    """No data race between four calling threads, a forgetting thread and the model's device."""
    flags = _sanitiser_flags(tmp_path, ["-fsanitize=thread"], ["-static-libtsan"], "test_adapter_state_thread")
    _build_and_run(tmp_path, "tsan", flags)
