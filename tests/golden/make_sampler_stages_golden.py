"""Records tests/golden/sampler_stages_golden.npz from the reference's own sampling code: the chain WITH tail-free and typical sampling.

    python tests/golden/make_sampler_stages_golden.py [REFERENCE_TREE]

As make_sampling_golden.py: llm/src/Generate.cc of the reference tree is compiled, together with tests/golden/sampler_stages_harness.cc (ours: it only calls the
reference's sample_* functions in LLaMA3Generate.cc's order and records the candidates after every stage), into a TEMPORARY directory -- nothing of the reference
enters the repository --, with the one-line json stub and -ffp-contract=off.

Inputs are NOT stored: config_rows() regenerates them from the configuration's seed through make_sampling_golden.config_rows (fp16(N(0, sigma)) logits over 128256
ids, a 64-entry recent window).  The file holds, per configuration and row: the greedy id, n_tfs, n_typ, n, the k sorted penalised logits with their ids and the softmax
over them, the ids and p as sample_typical left them, the softmax top-p walked, the final p after temperature -- and a SHA-256 of the regenerated inputs.
"""
from __future__ import annotations

import hashlib
import importlib.util
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "sampler_stages_golden.npz")
_spec = importlib.util.spec_from_file_location("make_sampling_golden_for_stages", os.path.join(HERE, "make_sampling_golden.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)
VOCAB = base.VOCAB
NRECENT = base.NRECENT
TOP_P, TEMP, REPEAT_PENALTY = 0.95, 0.8, 1.1  # every configuration: the reference's defaults (Generate.h:60-68), no frequency / presence penalty

# name: (k, sigma, tfs_z, typical_p, rows, seed)
CONFIGS = {
    "tfs_only": (40, 2.5, 0.95, 1.0, 60, 2001),
    "typical_only": (40, 2.5, 1.0, 0.9, 60, 2002),
    "both": (40, 2.5, 0.95, 0.9, 60, 2003),
    "flat_both": (40, 1.0, 0.97, 0.5, 60, 2004),
    "tight": (40, 2.5, 0.5, 0.2, 60, 2005),
}


def config_rows(name: str) -> list:
    """[(logits fp16 [VOCAB], recent int32 [NRECENT])] of configuration `name`, from its seed alone: make_sampling_golden.config_rows' generator on (k, sigma, rows, seed)."""
    k, sigma, z, typ, rows, seed = CONFIGS[name]
    key = "sampler_stages/" + name
    base.CONFIGS[key] = (k, TOP_P, TEMP, sigma, REPEAT_PENALTY, 0.0, 0.0, rows, seed)
    try:
        return list(base.config_rows(key))
    finally:
        del base.CONFIGS[key]


def build_harness(ref: str, tmp: str) -> str:
    inc = os.path.join(tmp, "stub", "nlohmann")
    os.makedirs(inc)
    with open(os.path.join(inc, "json.hpp"), "w") as f:
        f.write("namespace nlohmann { struct json {}; }\n")
    exe = os.path.join(tmp, "sampler_stages_harness")
    llm = os.path.join(ref, "llm")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-w", "-I", os.path.join(tmp, "stub"), "-I", os.path.join(llm, "include"), "-I", os.path.join(llm, "include", "nn_modules"),
           "-I", os.path.join(llm, "include", "ops"), "-I", os.path.join(ref, "kernels"), "-I", os.path.join(llm, "half-2.2.0", "include"), "-I", llm,
           os.path.join(llm, "src", "Generate.cc"), os.path.join(HERE, "sampler_stages_harness.cc"), "-o", exe, "-lpthread"]
    subprocess.check_call(cmd)
    return exe


def main() -> None:
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_harness(ref, tmp)
        for name, (k, sigma, z, typ, rows, seed) in CONFIGS.items():
            fin, fout = os.path.join(tmp, name + ".in"), os.path.join(tmp, name + ".out")
            h = hashlib.sha256()
            with open(fin, "wb") as f:
                f.write(np.array([rows, VOCAB, k, NRECENT], np.int32).tobytes())
                f.write(np.array([TOP_P, TEMP, REPEAT_PENALTY, 0.0, 0.0, z, typ], np.float32).tobytes())
                for logits, recent in config_rows(name):
                    h.update(logits.tobytes())
                    h.update(recent.tobytes())
                    f.write(logits.astype(np.float32).tobytes())  # half2float: exact
                    f.write(recent.tobytes())
            subprocess.check_call([exe, fin, fout])
            rec = np.fromfile(fout, dtype=np.int32).reshape(rows, 4 + 7 * k)
            for j, key in enumerate(("greedy", "n_tfs", "n_typ", "n")):
                out[f"{name}/{key}"] = rec[:, j].copy()
            for j, (key, is_float) in enumerate((("ids", False), ("logit", True), ("p", True), ("ids_typ", False), ("p_typ", True), ("p_top", True), ("final_p", True))):
                a = rec[:, 4 + j * k:4 + (j + 1) * k].copy()
                out[f"{name}/{key}"] = a.view(np.float32) if is_float else a
            out[name + "/digest"] = np.array(h.hexdigest())
            print(f"{name}: {rows} rows, k = {k}, n_tfs in [{rec[:, 1].min()}, {rec[:, 1].max()}], n_typ in [{rec[:, 2].min()}, {rec[:, 2].max()}], "
                  f"n in [{rec[:, 3].min()}, {rec[:, 3].max()}]", flush=True)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
