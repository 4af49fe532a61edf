#!/usr/bin/env python3
"""Are a build's objects what another build's were?  For every translation unit of tinychatengine_amd.build.HIP_SOURCES: the object of PARENT_LIB_DIR (the objects
of a build of the parent commit, copied aside) against the object of this tree's build, by byte; where the bytes differ, the gfx950 code objects' disassembly
(isa_lint.disassemble, file names stripped); where that differs too -- kernels renamed or reordered --, kernel by kernel with the symbol names ignored: the multiset of
instruction lists (the values of isa_lint.kernels) and the kernel counts.  One JSON line per object; a unit PARENT_LIB_DIR does not have is a new one.  Needs no GPU.
Both builds must have been made by the same compiler in directories of the same path.

    python scripts/objects_unchanged.py PARENT_LIB_DIR [OUT.jsonl] [--resources PARENT.txt BRANCH.txt]
                                                             (profiles/lora/objects_unchanged.jsonl, profiles/attn_forms/objects_unchanged.jsonl)
        --resources: two files written by the mode below; an object whose unit they list also gets "resources_equal": the multisets of the compiler's per-kernel
        resource lines (registers, LDS, scratch, spills, occupancy) with the name column dropped
    python scripts/objects_unchanged.py --write-resources OUT.txt [UNIT.hip ...]
        compiles the units (default: the two attention units) of THIS tree as the build does, with the compiler's resource remarks on -- what build._check_spills
        reads --, into a scratch object, and writes one line per kernel: unit, symbol, the remarks' fields
    python scripts/objects_unchanged.py --write-digests OUT.json [LIB_DIR]
        tests/golden/attn_forms_parent.json: per attention object of LIB_DIR (default: this tree's build) the sorted SHA-256 digests of its kernels' instruction lists,
        and the compiler's version string
"""
import collections
import hashlib
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ATTENTION_UNITS = ("attention_fast.hip", "attention_prefill.hip")


def compiler_version():
    """the clang line of hipcc --version"""
    from tinychatengine_amd import build as B
    text = subprocess.run([B._hipcc(), "--version"], capture_output=True, text=True, check=True).stdout
    return next(ln.strip() for ln in text.splitlines() if "clang version" in ln)


def kernel_bodies(obj):
    """the instruction lists of an object's kernels, as tuples, in no particular order"""
    from tinychatengine_amd import isa_lint
    return [tuple(v) for v in isa_lint.kernels(isa_lint.disassemble(obj)).values()]


def kernel_digests(obj):
    return sorted(hashlib.sha256("\n".join(body).encode()).hexdigest() for body in kernel_bodies(obj))


def resource_lines(unit):
    """[(symbol, "SGPRs: .. ; VGPRs: .. ; ...")] from the compiler's resource remarks on one unit"""
    from tinychatengine_amd import build as B
    with tempfile.TemporaryDirectory(prefix="tce_res_") as d:
        cmd = [B._hipcc(), *B.HIPCC_FLAGS, *B.EXTRA_FLAGS.get(unit, []), "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(REPO, "include"), "-I", B.CSRC, "-c",
               os.path.join(B.CSRC, unit), "-o", os.path.join(d, "x.o")]
        err = subprocess.run(cmd, stderr=subprocess.PIPE, text=True, check=True).stderr
    rows = []
    for ln in err.splitlines():
        if "remark:" not in ln or "kernel-resource-usage" not in ln:
            continue
        field = ln.split("remark:", 1)[1].split("[-Rpass-analysis")[0].strip()
        if field.startswith("Function Name:"):
            rows.append((field.split("Function Name:")[1].strip(), []))
        elif rows:
            rows[-1][1].append(field)
    return [(name, "; ".join(fields)) for name, fields in rows]


def read_resources(path):
    """unit -> multiset of resource lines, names dropped"""
    out = collections.defaultdict(collections.Counter)
    for ln in open(path):
        if ln.strip() and not ln.startswith("#"):
            unit, _, fields = ln.rstrip("\n").split("\t")
            out[unit][fields] += 1
    return out


def main():
    from tinychatengine_amd import build as B
    from tinychatengine_amd import isa_lint
    argv = sys.argv[1:]
    if argv and argv[0] == "--write-resources":
        with open(argv[1], "w") as f:
            f.write(f"# {compiler_version()}\n# unit, symbol, the resource remarks' fields\n")
            for unit in argv[2:] or ATTENTION_UNITS:
                f.writelines(f"{unit}\t{name}\t{fields}\n" for name, fields in resource_lines(unit))
        return
    if argv and argv[0] == "--write-digests":
        lib_dir = argv[2] if len(argv) > 2 else B.LIB_DIR
        rec = {"compiler": compiler_version()}
        for unit in ATTENTION_UNITS:
            o = unit.replace(".hip", ".o")
            rec[o] = kernel_digests(os.path.join(lib_dir, o))
        with open(argv[1], "w") as f:
            json.dump(rec, f, indent=0)
            f.write("\n")
        return
    res = None
    if "--resources" in argv:
        i = argv.index("--resources")
        res = (read_resources(argv[i + 1]), read_resources(argv[i + 2]))
        del argv[i:i + 3]
    parent_dir = argv[0]
    out_path = argv[1] if len(argv) > 1 else None
    strip = lambda text: "\n".join(ln for ln in text.splitlines() if "file format" not in ln and not ln.startswith("/"))
    lines = []
    for src in B.HIP_SOURCES:
        o = src.replace(".hip", ".o")
        pp, cp = os.path.join(parent_dir, o), os.path.join(B.LIB_DIR, o)
        if not os.path.exists(pp):
            rec = {"object": o, "parent": None, "note": "new translation unit"}
        else:
            a, b = open(pp, "rb").read(), open(cp, "rb").read()
            rec = {"object": o, "parent_sha256": hashlib.sha256(a).hexdigest(), "branch_sha256": hashlib.sha256(b).hexdigest(), "bytes_equal": a == b}
            if a != b:
                da, db = isa_lint.disassemble(pp), isa_lint.disassemble(cp)
                rec["device_disassembly_equal"] = strip(da) == strip(db)
                rec["device_kernels"] = len(isa_lint.kernels(da))
                if not rec["device_disassembly_equal"]:
                    ka, kb = kernel_bodies(pp), kernel_bodies(cp)
                    rec["kernel_bodies_equal"] = collections.Counter(ka) == collections.Counter(kb)
                    rec["kernel_counts"] = [len(ka), len(kb)]
            if res and (src in res[0] or src in res[1]):
                rec["resources_equal"] = res[0][src] == res[1][src]
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec) + "\n")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.writelines(lines)


if __name__ == "__main__":
    main()
