"""The attention kernels' instructions, held on the compiled gfx950 objects without a GPU ("The paged attention forms"; profiles/attn_forms/).

The paged attention family's scaffolding -- argument structs, wrappers, builders, the launchers' dispatch -- was rewritten around kernels whose device text did not
change: every instantiation of csrc/attention_fast.hip and csrc/attention_prefill.hip must compile to the instruction stream it had before.  The fixture
tests/golden/attn_forms_parent.json holds, from a build of the commit BEFORE that rewrite (scripts/objects_unchanged.py --write-digests), per object the sorted SHA-256
digests of its kernels' instruction lists (isa_lint.kernels: mnemonics and operands, symbol names not included) and the compiler's version string.  Held here: the
built objects give the same sorted lists -- no kernel added, none dropped, none changed.

Another compiler makes other instructions from the same source: the comparison says nothing then, and the test skips (only then).
"""
import importlib.util
import json
import os

import pytest

from tinychatengine_amd import build as tce_build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, "tests", "golden", "attn_forms_parent.json")
OBJECTS = ("attention_fast.o", "attention_prefill.o")


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("objects_unchanged", os.path.join(REPO, "scripts", "objects_unchanged.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded(tool):
    rec = json.load(open(FIXTURE))
    now = tool.compiler_version()
    if now != rec["compiler"]:
        pytest.skip(f"the fixture was recorded with another compiler ({rec['compiler']}; here: {now})")
    tce_build.build()
    return rec


def test_every_kernel_is_the_parents(tool, recorded):
    for obj in OBJECTS:
        want = recorded[obj]
        got = tool.kernel_digests(os.path.join(tce_build.LIB_DIR, obj))
        assert len(got) == len(want), f"{obj}: {len(got)} kernels, the parent had {len(want)}"
        changed = sorted(set(got) - set(want))
        assert got == want, f"{obj}: {len(changed)} kernel(s) whose instructions the parent's build does not have"
