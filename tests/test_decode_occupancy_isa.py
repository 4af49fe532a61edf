"""The registers of the int8 decode kernels, held on the compiled gfx950 object without a GPU (csrc/w4a16_gemv_i8.hip section 3, profiles/decode_occupancy/).

A wave of the plain decode kernel keeps 8 KiB of weights in flight in 32 vector registers; what else is live across the contraction decides how many waves a SIMD holds
(512 registers, allocated in eights) and with that whether the 1792 workgroups of the gate+up launch are resident at once: 7 waves per SIMD (<= 72 registers) -- all of
them -- against 5 (84 registers, 1280 workgroups) in the parent.  The contraction's B operand is staged two units ahead in a ring of two register sets instead of a
whole pass of four.

Held here, on the code object's own metadata (register counts, spill count, the private segment's size) and nothing else:
  * the two plain zero-point-8 instantiations (plain and residual + next-norm) and the NORM twin use at most 72 vector registers;
  * they spill nothing and use no scratch;
  * no instantiation listed in the parent's table (profiles/decode_occupancy/kernel_resources.txt, second section) holds fewer waves per SIMD than it did, and none spills.
"""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from tinychatengine_amd import build as tce_build
from tinychatengine_amd import isa_lint

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = os.path.join(isa_lint.LLVM_BIN, "llvm-readelf")
TABLE = os.path.join(REPO, "profiles", "decode_occupancy", "kernel_resources.txt")
# <MB, GPU, ROWS, UW, Z8, MAXT, NORM, RNORM, COMB, STAMPS>
TARGETS = {
    "plain": "w4a16_gemv_i8_kernel<1, 1, 1, 8, true, 1024, false, false, 0, false>",
    "residual + next norm": "w4a16_gemv_i8_kernel<1, 1, 1, 8, true, 1024, false, true, 0, false>",
    "NORM": "w4a16_gemv_i8_kernel<1, 1, 1, 8, true, 1024, true, false, 0, false>",
}
VGPR_TARGET = 72  # 512 / 7 = 73.1, allocated in eights


def waves_per_simd(vgprs, agprs):
    """gfx950: one file of 512 registers per SIMD lane, the accumulation registers behind the vector registers rounded up to four, the total allocated in eights"""
    total = (vgprs + 3) // 4 * 4 + agprs if agprs else vgprs
    total = max(8, (total + 7) // 8 * 8)
    return min(8, 512 // total)


@pytest.fixture(scope="module")
def resources():
    """demangled kernel name -> {vgpr, agpr, spill, scratch} from the metadata note of the product build's w4a16_gemv_i8 object"""
    tce_build.build()
    obj = os.path.join(tce_build.LIB_DIR, "w4a16_gemv_i8.o")
    d = tempfile.mkdtemp(prefix="tce_occ_")
    try:
        shutil.copy(obj, os.path.join(d, "x.o"))
        subprocess.run([isa_lint.OBJDUMP, "--offloading", "x.o"], cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=False)
        co = [f for f in os.listdir(d) if "gfx950" in f]
        assert co, "no gfx950 code object in " + obj
        notes = subprocess.run([READELF, "--notes", os.path.join(d, co[0])], capture_output=True, text=True, check=True).stdout
    finally:
        shutil.rmtree(d, ignore_errors=True)
    rows, cur = [], None
    for ln in notes.splitlines():
        m = re.match(r"\s*(- )?\.(\w+):\s*(.*)$", ln)
        if not m:
            continue
        if m.group(1) and ln.startswith("  - "):  # a new kernel's record (the argument records sit deeper)
            cur = {}
            rows.append(cur)
        if cur is not None and ln.startswith("    ") and not ln.startswith("      "):
            cur[m.group(2)] = m.group(3).strip().strip("'")
    rows = [r for r in rows if "name" in r and "vgpr_count" in r]
    names = isa_lint.demangle([r["name"] for r in rows])
    out = {}
    for r, n in zip(rows, names):
        n = re.sub(r"tce::\(anonymous namespace\)::", "", n).split("(")[0]
        n = n[5:] if n.startswith("void ") else n
        out[n] = {"vgpr": int(r["vgpr_count"]), "agpr": int(r.get("agpr_count", 0)), "spill": int(r.get("vgpr_spill_count", 0)) + int(r.get("sgpr_spill_count", 0)),
                  "scratch": int(r.get("private_segment_fixed_size", 0))}
    assert len(out) >= 20, sorted(out)
    return out


def parent_table():
    """kernel -> waves per SIMD of the parent commit's source: the second section of the committed table"""
    text = open(TABLE).read()
    parent = text[text.index("# the parent commit's source"):]
    rows = {}
    for ln in parent.splitlines():
        m = re.match(r"^(?:void )?(\S.*?>)\s+vgpr\s+(\d+) agpr\s+(\d+) spill\s+(\d+) scratch\s+(\d+) sgpr\s+\d+ occ\s+(\d+)", ln)
        if m:
            rows[m.group(1)] = int(m.group(6))
    assert len(rows) >= 20, len(rows)
    return rows


@pytest.mark.parametrize("form", sorted(TARGETS))
def test_the_plain_forms_fit_seven_waves_per_simd(resources, form):
    r = resources[TARGETS[form]]
    assert r["agpr"] == 0 and r["vgpr"] <= VGPR_TARGET, f"{form}: {r['vgpr']} vector registers (+ {r['agpr']}), more than {VGPR_TARGET}"
    assert waves_per_simd(r["vgpr"], r["agpr"]) >= 7, (form, r)


@pytest.mark.parametrize("form", sorted(TARGETS))
def test_the_plain_forms_spill_nothing(resources, form):
    r = resources[TARGETS[form]]
    assert r["spill"] == 0 and r["scratch"] == 0, f"{form}: {r['spill']} spilled registers, {r['scratch']} bytes of scratch per lane"


def test_no_instantiation_lost_occupancy(resources):
    parent = parent_table()
    missing = sorted(set(parent) - set(resources))
    assert not missing, f"instantiations of the parent's table that the object no longer holds: {missing}"
    lost = {k: (occ, waves_per_simd(resources[k]["vgpr"], resources[k]["agpr"]), resources[k]["vgpr"]) for k, occ in parent.items()
            if waves_per_simd(resources[k]["vgpr"], resources[k]["agpr"]) < occ}
    assert not lost, f"(parent's waves per SIMD, now, vector registers now): {lost}"
    spilled = {k: resources[k] for k in parent if resources[k]["spill"] or resources[k]["scratch"]}
    assert not spilled, spilled
