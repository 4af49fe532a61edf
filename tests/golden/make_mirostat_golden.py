"""Records tests/golden/mirostat_golden.npz from the reference's own sampling code: the mirostat branches of its chain.

    python tests/golden/make_mirostat_golden.py [REFERENCE_TREE]

As make_sampler_stages_golden.py: llm/src/Generate.cc of the reference tree is compiled, together with tests/golden/mirostat_harness.cc (ours: it only calls the
reference's sample_* functions -- penalties, sample_top_k(k, 1), sample_temperature, sample_token_mirostat[_v2] -- and records what they leave), into a TEMPORARY
directory -- nothing of the reference enters the repository --, with the one-line json stub and -ffp-contract=off.  mu is carried from row to row as the reference's
function-static is; every row records the mu it started from, so a row can be checked on its own.

Inputs are NOT stored: config_rows() regenerates them from the configuration's seed (fp16(N(0, sigma)) logits over the configuration's vocabulary, a 64-entry recent
window: make_sampling_golden.config_rows' generator with the vocabulary as a parameter).  The file holds, per configuration and row: mu_in, the k sorted penalised
logits with their ids, the softmax over logit / temp, the count the reference kept, its final p, the token X it drew (std::discrete_distribution on its own
default-seeded mt19937), mu_out -- and a SHA-256 of the regenerated inputs.

Two configurations have vocab <= k: sample_top_k removes nothing there and the recorded chain is the reference's unmodified one (penalties -> temperature -> mirostat
over the whole vocabulary).
"""
from __future__ import annotations

import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "mirostat_golden.npz")
NRECENT = 64
REPEAT_PENALTY = 1.1  # every configuration: the reference's default (Generate.h:63), no frequency / presence penalty
M = 100               # the reference's mirostat_m (LLaMA3Generate.cc:164)

# name: (mode, vocab, k, sigma, temp, tau, eta, rows, seed).  tau is chosen per configuration so that the counts the reference keeps vary and so that at most 10 % of
# its rows are undecided by tests/mirostat_rules.py (at k = 256 a k_f between about 25 and 256 is undecided: the rule's relative delta_k times k_f exceeds 1 / 2).
CONFIGS = {
    "v1_k40_sharp": (1, 128256, 40, 2.5, 0.8, 5.0, 0.1, 48, 3001),
    "v1_k40_flat": (1, 128256, 40, 1.0, 0.8, 3.0, 0.1, 48, 3002),
    "v1_k256_sharp": (1, 128256, 256, 2.5, 0.8, 3.0, 0.1, 32, 3003),
    "v1_k256_flat": (1, 128256, 256, 1.0, 0.8, 3.0, 0.1, 32, 3004),
    "v2_k40_sharp": (2, 128256, 40, 2.5, 0.8, 5.0, 0.1, 48, 3005),
    "v2_k40_flat": (2, 128256, 40, 1.0, 0.8, 3.0, 0.1, 48, 3006),
    "v2_k256_sharp": (2, 128256, 256, 2.5, 0.8, 3.0, 0.1, 32, 3007),
    "v2_k256_flat": (2, 128256, 256, 1.0, 1.0, 5.0, 0.1, 32, 3008),
    "v1_whole_vocab": (1, 200, 200, 2.0, 0.8, 3.0, 0.1, 48, 3009),   # vocab <= k: the reference's unmodified chain
    "v2_whole_vocab": (2, 200, 200, 2.0, 0.8, 3.0, 0.1, 48, 3010),
}


def config_rows(name: str) -> list:
    """[(logits fp16 [vocab], recent int32 [NRECENT])] of configuration `name`, from its seed alone."""
    mode, vocab, k, sigma, temp, tau, eta, rows, seed = CONFIGS[name]
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(rows):
        logits = (rng.standard_normal(vocab, dtype=np.float32) * np.float32(sigma)).astype(np.float16)
        strongest = np.argsort(-logits.astype(np.float32), kind="stable")[:50]
        ring = np.zeros(NRECENT, np.int32)
        for t in range(int(rng.integers(3, 90))):
            tok = int(strongest[rng.integers(0, 50)]) if rng.random() < 0.5 else int(rng.integers(0, vocab))
            ring[t % NRECENT] = tok
        out.append((logits, ring))  # (the window is a set with counts: the order of its entries does not matter)
    return out


def build_harness(ref: str, tmp: str) -> str:
    inc = os.path.join(tmp, "stub", "nlohmann")
    os.makedirs(inc)
    with open(os.path.join(inc, "json.hpp"), "w") as f:
        f.write("namespace nlohmann { struct json {}; }\n")
    exe = os.path.join(tmp, "mirostat_harness")
    llm = os.path.join(ref, "llm")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-w", "-I", os.path.join(tmp, "stub"), "-I", os.path.join(llm, "include"), "-I", os.path.join(llm, "include", "nn_modules"),
           "-I", os.path.join(llm, "include", "ops"), "-I", os.path.join(ref, "kernels"), "-I", os.path.join(llm, "half-2.2.0", "include"), "-I", llm,
           os.path.join(llm, "src", "Generate.cc"), os.path.join(HERE, "mirostat_harness.cc"), "-o", exe, "-lpthread"]
    subprocess.check_call(cmd)
    return exe


def main() -> None:
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_harness(ref, tmp)
        for name, (mode, vocab, k, sigma, temp, tau, eta, rows, seed) in CONFIGS.items():
            fin, fout = os.path.join(tmp, name + ".in"), os.path.join(tmp, name + ".out")
            h = hashlib.sha256()
            with open(fin, "wb") as f:
                f.write(np.array([rows, vocab, k, NRECENT, mode, M], np.int32).tobytes())
                f.write(np.array([temp, REPEAT_PENALTY, 0.0, 0.0, tau, eta], np.float32).tobytes())
                for logits, recent in config_rows(name):
                    h.update(logits.tobytes())
                    h.update(recent.tobytes())
                    f.write(logits.astype(np.float32).tobytes())  # half2float: exact
                    f.write(recent.tobytes())
            subprocess.check_call([exe, fin, fout])
            rec = np.fromfile(fout, dtype=np.int32).reshape(rows, 4 + 4 * k)
            col = 0
            for key, width, is_float in (("mu_in", 1, True), ("ids", k, False), ("logit", k, True), ("p", k, True), ("kept", 1, False), ("final_p", k, True), ("X", 1, False),
                                         ("mu_out", 1, True)):
                a = rec[:, col:col + width].copy()
                a = a.view(np.float32) if is_float else a
                out[f"{name}/{key}"] = a[:, 0].copy() if width == 1 else a
                col += width
            out[name + "/digest"] = np.array(h.hexdigest())
            kept, mu = out[name + "/kept"], out[name + "/mu_out"]
            print(f"{name}: {rows} rows, k = {k}, kept in [{kept.min()}, {kept.max()}], mu_out in [{mu.min():.3f}, {mu.max():.3f}]", flush=True)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
