"""Records tests/golden/layer_trace_parent.json: the calls a decoder layer issues, per case of tests/layer_trace_cases.py (no device needed).

Run it on the commit BEFORE a change to the host code that issues a decoder layer's launches; tests/test_layer_trace_host.py then holds the changed tree to the file.

    python scripts/layer_trace_record.py [OUT]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main() -> int:
    import layer_trace_cases as lt
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "layer_trace_parent.json")
    traces = {}
    for name, fn in lt.cases().items():
        traces[name] = lt.run(fn)
        assert traces[name] == lt.run(fn), f"{name}: two runs gave different traces"
        print(f"{name}: {len(traces[name])} events")
    with open(out, "w") as f:
        json.dump(traces, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
