"""Host time of the decoder layer's callers, this tree against an earlier commit's batch_decode.py / decoder_block.py loaded beside it (needs the GPU).

The library is the same .so and both versions issue the same launches on the same weights, so only what the host does between launches can differ:

  block_prefill    DecoderBlock.prefill at bench.py's prefill shape (one Llama-3-8B layer, 512 rows), 20 calls per repeat
  step / step+pool an eager BatchedDecoder.step at the tiny shape (hidden 512, 4 / 1 heads, ffn 1408, batch 4), without and with a LoraPool, 300 calls per repeat

A repeat is timed by the host clock around the calls and the synchronise that ends them; the two versions alternate, REPEATS repeats each after a warm-up of both.
The margin is the parent's own spread (max - min over its repeats), measured in this run: a case is "within_margin" when median(branch) - median(parent) <= spread.

    python scripts/layer_body_host_time.py PARENT_DIR [OUT]      PARENT_DIR holds the earlier commit's batch_decode.py and decoder_block.py
"""
import json
import os
import statistics
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
REPEATS = 7


def load_parent(parent_dir: str):
    """the earlier commit's two modules as tinychatengine_amd.parent_decoder_block / parent_batch_decode (every other module is this tree's)"""
    def load(name, path, edit=lambda s: s):
        mod = types.ModuleType(f"tinychatengine_amd.{name}")
        mod.__package__, mod.__file__ = "tinychatengine_amd", path
        sys.modules[mod.__name__] = mod
        with open(path) as f:
            exec(compile(edit(f.read()), path, "exec"), mod.__dict__)
        return mod
    db = load("parent_decoder_block", os.path.join(parent_dir, "decoder_block.py"))
    bd = load("parent_batch_decode", os.path.join(parent_dir, "batch_decode.py"), lambda s: s.replace("from .decoder_block import", "from .parent_decoder_block import"))
    return db, bd


def main() -> int:
    import numpy as np
    import torch

    from tinychatengine_amd import batch_decode, capi, decoder_block
    from tinychatengine_amd.lora import LoraPool
    parent_db, parent_bd = load_parent(sys.argv[1])
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "layer_body", "host_time.jsonl")
    assert torch.cuda.is_available(), "layer_body_host_time needs cuda:0"
    capi.lib()
    dev = torch.device("cuda:0")

    def tables(keys):
        ang = np.random.default_rng(0).uniform(0, 2 * np.pi, (keys, 64))
        return [torch.from_numpy(np.concatenate([f(ang), f(ang)], axis=1).astype(np.float16)).to(dev) for f in (np.cos, np.sin)]

    cases = {}
    # DecoderBlock.prefill: ONE block (its weights, its cache, its _pf rows) under both versions of the method
    big = decoder_block.DecoderBlock(4096, 32, 14336, 2048, dev, *tables(2048), seed=100, kv_heads=8)
    rows0 = torch.randn(512, 4096, device=dev).to(torch.float16)
    rows = rows0.clone()

    def prefill(method):
        def run():
            for _ in range(20):
                rows.copy_(rows0)
                method(big, rows, 0)
            return 20
        return run
    cases["block_prefill"] = {"parent": prefill(parent_db.DecoderBlock.prefill), "branch": prefill(decoder_block.DecoderBlock.prefill)}
    # BatchedDecoder.step, eager: the same block under a decoder of each version (caches and buffers of their own)
    tiny = decoder_block.DecoderBlock(512, 4, 1408, 64, dev, *tables(64), seed=7, kv_heads=1)
    pool = LoraPool(tiny, 1, 4, 8, dev)
    hidden0 = torch.randn(4, 512, device=dev).to(torch.float16)
    hidden, pos = hidden0.clone(), torch.zeros(4, dtype=torch.int32, device=dev)

    def step(dec):
        def run():
            hidden.copy_(hidden0)
            for _ in range(300):
                dec.step(hidden, pos, 63)
            return 300
        return run
    for name, view in (("step", None), ("step+pool", pool.layer(0))):
        cases[name] = {"parent": step(parent_bd.BatchedDecoder(tiny, 4, lora=view)), "branch": step(batch_decode.BatchedDecoder(tiny, 4, lora=view))}
    if pool.row_adapter is not None:
        pool.row_adapter.copy_(torch.tensor([0, -1, 1, 2], dtype=torch.int32))

    lines, ok = [], True
    for name, versions in cases.items():
        for run in versions.values():  # warm-up: both versions, every shape
            run()
        torch.cuda.synchronize()
        us = {"parent": [], "branch": []}
        for _ in range(REPEATS):
            for version, run in versions.items():
                t0 = time.perf_counter()
                n = run()
                torch.cuda.synchronize()
                us[version].append((time.perf_counter() - t0) * 1e6 / n)
        med = {v: statistics.median(t) for v, t in us.items()}
        spread = max(us["parent"]) - min(us["parent"])
        within = med["branch"] - med["parent"] <= spread
        ok = ok and within
        lines.append({"case": name, "repeats": REPEATS, "us_per_call": {v: [round(t, 2) for t in ts] for v, ts in us.items()},
                      "median_us": {v: round(m, 2) for v, m in med.items()}, "parent_spread_us": round(spread, 2), "within_margin": within})
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        for l in lines:
            f.write(json.dumps(l) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
