"""Records tests/golden/sampling_golden.npz from the reference's own sampling code.

    python tests/golden/make_sampling_golden.py [REFERENCE_TREE]

llm/src/Generate.cc of the reference tree is compiled, together with tests/golden/sampling_harness.cc (ours: it only calls the reference's sample_* functions in
LLaMA3Generate.cc's order), into a TEMPORARY directory -- nothing of the reference enters the repository -- and run on the inputs of CONFIGS.  Generate.h includes
nlohmann/json.hpp, which the sampling functions do not use: a one-line stub of our own on the include path stands in for it.  -ffp-contract=off: the reference's
arithmetic as written.

Inputs are NOT stored: config_rows() regenerates them from the configuration's seed -- fp16(N(0, sigma)) logits over a 128256-token vocabulary and a 64-entry recent
window that starts as zeros (the reference's last_n_tokens) and has taken a random number of tokens, half of them drawn from the row's strongest logits (so the
penalties move candidates) and with repeats.  The file holds, per configuration and row: the greedy id, the k sorted penalised logits with their ids, their p, n after
top-p, the final p after temperature -- and a SHA-256 of the regenerated inputs, which the tests check before they compare anything.
"""
from __future__ import annotations

import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "sampling_golden.npz")
VOCAB = 128256
NRECENT = 64

# name: (k, top_p, temp, sigma, repeat_penalty, alpha_frequency, alpha_presence, rows, seed)
CONFIGS = {
    "defaults": (40, 0.95, 0.8, 2.5, 1.1, 0.0, 0.0, 100, 1001),      # the reference's defaults (Generate.h:60-68)
    "k256": (256, 0.9, 0.7, 2.5, 1.1, 0.0, 0.0, 80, 1002),
    "wide": (40, 0.95, 0.8, 4.0, 1.0, 0.0, 0.0, 100, 1003),          # sigma 4: inf-free but steep; repeat penalty off
    "k1": (1, 0.95, 0.8, 2.5, 1.1, 0.0, 0.0, 60, 1004),
    "k64_hot": (64, 0.5, 1.3, 3.0, 1.1, 0.0, 0.0, 100, 1005),
    "freq_presence": (40, 0.95, 0.8, 2.5, 1.1, 0.3, 0.2, 100, 1006),
    "greedy": (40, 0.95, 0.0, 2.5, 1.1, 0.0, 0.0, 100, 1007),        # temp <= 0
    "top_p_off": (40, 1.0, 0.8, 2.5, 1.0, 0.0, 0.0, 40, 1008),
}


def config_rows(name: str):
    """Yields (logits fp16 [VOCAB], recent int32 [NRECENT]) for every row of configuration `name`, from its seed alone."""
    k, top_p, temp, sigma, rp, af, ap, rows, seed = CONFIGS[name]
    rng = np.random.default_rng(seed)
    for _ in range(rows):
        logits = (rng.standard_normal(VOCAB, dtype=np.float32) * np.float32(sigma)).astype(np.float16)
        strongest = np.argsort(-logits.astype(np.float32), kind="stable")[:50]
        ring = np.zeros(NRECENT, np.int32)
        for t in range(int(rng.integers(3, 90))):
            tok = int(strongest[rng.integers(0, 50)]) if rng.random() < 0.5 else int(rng.integers(0, VOCAB))
            ring[t % NRECENT] = tok
        yield logits, ring  # (the window is a set with counts: the order of its entries does not matter)


def config_digest(name: str) -> str:
    h = hashlib.sha256()
    for logits, recent in config_rows(name):
        h.update(logits.tobytes())
        h.update(recent.tobytes())
    return h.hexdigest()


def build_harness(ref: str, tmp: str) -> str:
    inc = os.path.join(tmp, "stub", "nlohmann")
    os.makedirs(inc)
    with open(os.path.join(inc, "json.hpp"), "w") as f:
        f.write("namespace nlohmann { struct json {}; }\n")
    exe = os.path.join(tmp, "sampling_harness")
    llm = os.path.join(ref, "llm")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-w", "-I", os.path.join(tmp, "stub"), "-I", os.path.join(llm, "include"), "-I", os.path.join(llm, "include", "nn_modules"),
           "-I", os.path.join(llm, "include", "ops"), "-I", os.path.join(ref, "kernels"), "-I", os.path.join(llm, "half-2.2.0", "include"), "-I", llm,
           os.path.join(llm, "src", "Generate.cc"), os.path.join(HERE, "sampling_harness.cc"), "-o", exe, "-lpthread"]
    subprocess.check_call(cmd)
    return exe


def main() -> None:
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_harness(ref, tmp)
        for name, (k, top_p, temp, sigma, rp, af, ap, rows, seed) in CONFIGS.items():
            fin, fout = os.path.join(tmp, name + ".in"), os.path.join(tmp, name + ".out")
            h = hashlib.sha256()
            with open(fin, "wb") as f:
                f.write(np.array([rows, VOCAB, k, NRECENT], np.int32).tobytes())
                f.write(np.array([top_p, temp, rp, af, ap], np.float32).tobytes())
                for logits, recent in config_rows(name):
                    h.update(logits.tobytes())
                    h.update(recent.tobytes())
                    f.write(logits.astype(np.float32).tobytes())  # half2float: exact
                    f.write(recent.tobytes())
            subprocess.check_call([exe, fin, fout])
            rec = np.fromfile(fout, dtype=np.int32).reshape(rows, 2 + 4 * k)
            out[name + "/greedy"] = rec[:, 0].copy()
            out[name + "/n"] = rec[:, 1].copy()
            if temp > 0:
                out[name + "/ids"] = rec[:, 2:2 + k].copy()
                out[name + "/logit"] = rec[:, 2 + k:2 + 2 * k].copy().view(np.float32)
                out[name + "/p"] = rec[:, 2 + 2 * k:2 + 3 * k].copy().view(np.float32)
                out[name + "/final_p"] = rec[:, 2 + 3 * k:2 + 4 * k].copy().view(np.float32)
            out[name + "/digest"] = np.array(h.hexdigest())
            print(f"{name}: {rows} rows, k = {k}, n in [{rec[:, 1].min()}, {rec[:, 1].max()}]", flush=True)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
