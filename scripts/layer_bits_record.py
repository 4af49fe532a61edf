"""Records tests/golden/layer_bits_parent.json: a SHA-256 of the residual rows' bytes for every case of tests/layer_bits_cases.py (needs the GPU).

Run it on the commit BEFORE a change to the host code that issues a decoder layer's launches (batch_decode.py, decoder_block.py, paged_kv.py, speculative.py);
tests/test_gpu_layer_bits.py then holds the changed tree to the file.  Every case runs twice on fresh decoders; a case whose two runs differ is NOT written (its name
goes to "unstable" with both digests, and the script exits 1 after writing the rest), so the file only holds what the device reproduces.

    python scripts/layer_bits_record.py [OUT]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main() -> int:
    import torch

    import layer_bits_cases as lb
    from tinychatengine_amd import capi
    assert torch.cuda.is_available(), "layer_bits_record needs cuda:0"
    capi.lib()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "layer_bits_parent.json")
    model = lb.Model(torch.device("cuda:0"))
    digests, unstable = {}, {}
    for name in lb.cases():
        a, b = lb.run(model, name), lb.run(model, name)
        if a == b:
            digests.update(a)
        else:
            unstable[name] = [a, b]
        print(name, "ok" if a == b else "UNSTABLE", flush=True)
    with open(out, "w") as f:
        json.dump({"digests": digests, "unstable": unstable}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} digests, {len(unstable)} unstable cases -> {out}")
    return 1 if unstable else 0


if __name__ == "__main__":
    sys.exit(main())
