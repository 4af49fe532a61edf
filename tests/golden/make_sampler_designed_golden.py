"""Records tests/golden/sampler_designed_golden.npz: the reference's own sampling code on the designed cases of tests/sampler_cases.py.

    python tests/golden/make_sampler_designed_golden.py REFERENCE_TREE

make_sampling_golden.build_harness compiles llm/src/Generate.cc of the reference tree with tests/golden/sampling_harness.cc (unchanged) into a TEMPORARY directory
and every recordable case (sampler_cases.recordable: finite logits, vocab <= 8200, k <= vocab) runs through it as a one-row configuration whose recent window is
the case's penalty window.  Inputs are NOT stored -- the case table rebuilds them --; the file holds, per case, the greedy id, n, the k sorted penalised logits with
their ids, p and the final p, and one SHA-256 over the inputs of all recorded cases, which the test checks before it compares anything.
"""
from __future__ import annotations

import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sampler_cases as S  # noqa: E402
from sampling_rules import maker  # noqa: E402  (make_sampling_golden, loaded by path)

OUT = os.path.join(HERE, "sampler_designed_golden.npz")


def main() -> None:
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    cs = [c for c in S.cases() if S.recordable(c)]
    out = {"digest": np.array(S.digest(cs)), "names": np.array([c.name for c in cs])}
    with tempfile.TemporaryDirectory() as tmp:
        exe = maker.build_harness(ref, tmp)
        for c in cs:
            k, w = c.k, c.window.astype(np.int32)
            fin, fout = os.path.join(tmp, c.name + ".in"), os.path.join(tmp, c.name + ".out")
            with open(fin, "wb") as f:
                f.write(np.array([1, c.vocab, k, w.size], np.int32).tobytes())
                f.write(np.array([c.prm.top_p, c.prm.temp, c.prm.repeat_penalty, c.prm.alpha_frequency, c.prm.alpha_presence], np.float32).tobytes())
                f.write(c.logits.astype(np.float32).tobytes())  # half2float: exact
                f.write(w.tobytes())
            subprocess.check_call([exe, fin, fout])
            rec = np.fromfile(fout, dtype=np.int32)
            assert rec.size == 2 + 4 * k
            out[c.name + "/greedy"] = rec[0].copy()
            if c.prm.temp > 0:
                out[c.name + "/n"] = rec[1].copy()
                out[c.name + "/ids"] = rec[2:2 + k].copy()
                out[c.name + "/logit"] = rec[2 + k:2 + 2 * k].copy().view(np.float32)
                out[c.name + "/p"] = rec[2 + 2 * k:2 + 3 * k].copy().view(np.float32)
                out[c.name + "/final_p"] = rec[2 + 3 * k:2 + 4 * k].copy().view(np.float32)
            print(f"{c.name}: k = {k}, n = {rec[1]}, greedy {rec[0]}", flush=True)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
