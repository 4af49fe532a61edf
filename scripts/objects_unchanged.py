#!/usr/bin/env python3
"""Are a build's objects what another build's were?  For every translation unit of tinychatengine_amd.build.HIP_SOURCES: the object of PARENT_LIB_DIR (the objects
of a build of the parent commit, copied aside) against the object of this tree's build, by byte; where the bytes differ, the gfx950 code objects' disassembly
(isa_lint.disassemble, file names stripped).  One JSON line per object; a unit PARENT_LIB_DIR does not have is a new one.  Needs no GPU.

    python scripts/objects_unchanged.py PARENT_LIB_DIR [OUT.jsonl]       (profiles/lora/objects_unchanged.jsonl)
"""
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    from tinychatengine_amd import build as B
    from tinychatengine_amd import isa_lint
    parent_dir = sys.argv[1]
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
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
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec) + "\n")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.writelines(lines)


if __name__ == "__main__":
    main()
