"""CPU (no GPU): the table of tce_w4a16_set_debug_mode (tinychatengine_amd/csrc/tuning_modes.hpp) against the chain of range checks it replaced.
tests/host/test_tuning_modes.cc includes the table with recording stand-ins for the setters (nothing of libtce_hip.so or HIP is linked) and holds every mode of
-16 .. 70000, INT_MIN and INT_MAX to tests/golden/tuning_modes_{product,lab}.txt -- the parent's function recorded mode by mode, both builds -- and to at most one
accepting row.  The program is a stand-alone executable, compiled with g++ and run here twice: plain, -fsanitize=address,undefined.  Nothing is loaded into this
Python process."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _links(tmp_path, flags):
    """Whether this toolchain links a program with `flags` (a sanitiser's runtime may be missing)."""
    src = tmp_path / "probe.cc"
    src.write_text("int main() { return 0; }\n")
    return subprocess.run(["g++", *flags, str(src), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0


def _build_and_run(tmp_path, name, flags):
    exe = tmp_path / f"test_tuning_modes_{name}"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", *flags, "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "tinychatengine_amd", "csrc"),
                           os.path.join(REPO, "tests", "host", "test_tuning_modes.cc"), "-o", str(exe)])
    r = subprocess.run([str(exe), os.path.join(REPO, "tests", "golden")], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "tuning modes: ok (0 differences)" in r.stdout and "MISMATCH" not in r.stdout
    for build in ("product", "lab"):  # both builds swept every mode and said so
        lines = [l for l in r.stdout.splitlines() if l.startswith(f"tuning modes, {build} build:")]
        assert len(lines) == 1 and "70019 modes swept" in lines[0] and lines[0].endswith(" 0 differences"), (build, lines)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_tuning_modes_plain(tmp_path):
    _build_and_run(tmp_path, "plain", [])


def test_tuning_modes_address_undefined(tmp_path):
    """No read past the table or a golden line, no shift or overflow on INT_MIN / INT_MAX."""
    flags, static = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], ["-static-libasan", "-static-libubsan"]
    # the sanitiser's runtime linked statically where the toolchain can: the program then starts whatever else the environment loads into it
    if _links(tmp_path, flags + static):
        flags = flags + static
    elif not _links(tmp_path, flags):
        pytest.skip("this toolchain cannot link -fsanitize=address,undefined")
    elif os.environ.get("LD_PRELOAD"):
        pytest.skip("-fsanitize=address links only its shared runtime here, which cannot start beside the environment's preloaded library")
    _build_and_run(tmp_path, "asan_ubsan", flags)
