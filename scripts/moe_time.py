#!/usr/bin/env python3
"""The mixture-of-experts FFN on the clock, in ONE process, on Mixtral-8x7B's FFN shapes (hidden 4096, ffn 14336, E = 8, k = 2), B = 1 / 4 / 16 rows, the routing
FORCED to 2, 4 and 8 distinct active experts (the router is the identity on the first 8 columns and the rows carry 2 and 1 there: the real route kernel picks them).

    moe       the five launches (MoeFFN.forward) and each stage alone: REPS copies captured in one graph, device events around REPLAYS replays, after a warm-up
    dense     the yardstick: tce_w4a16_forward gate_up (pair epilogue) + down at M = B on as many DISTINCT experts' weights as are active -- the same weight bytes
              through the existing dense kernels
    readback  the only form the library could serve before: ids copied to the host, then per chosen expert a gather of its rows and one dense launch pair (eager,
              host clock around a synchronise: the read-back is the point)
    floor     each stage's bytes (distinct active experts x the expert's bytes of that stage + activations) over 8 TB/s

The forms alternate, REPEATS times; the median and the spread are written.  No speed bar is set: the numbers say where the kernels stand.

    python scripts/moe_time.py [OUT.jsonl]        (default profiles/moe/moe_time.jsonl)
"""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HIDDEN, FFN, E, K_TOP = 4096, 14336, 8, 2
BATCHES, ACTIVE = (1, 4, 16), (2, 4, 8)
REPS, REPLAYS, WARMUP, REPEATS = 200, 10, 3, 3  # a timed window is one replay of REPS copies: 20 .. 100 ms at these shapes
HBM_BYTES_PER_US = 8e6


def forced_rows(torch, B, active, dev):
    """Gaussian rows whose first 8 columns force the routing: row i takes experts (2 i) % active (logit 8) and (2 i + 1) % active (logit 4), the others 0"""
    x = torch.empty(B, HIDDEN, device=dev).normal_(0, 1, generator=torch.Generator(device=dev).manual_seed(B * 16 + active)).half()
    x[:, :E] = 0
    for i in range(B):
        x[i, (2 * i) % active], x[i, (2 * i + 1) % active] = 2.0, 1.0
    return x


def graph_us(torch, fn):
    """median microseconds of one fn() among REPS captured copies, over REPLAYS replays"""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(REPS):
                fn()
    for _ in range(WARMUP):
        g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPLAYS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / REPS)
    return statistics.median(out)


def main():
    import torch
    from tinychatengine_amd import capi, moe
    from tinychatengine_amd.linear import Linear_half_int4, _stream
    assert torch.cuda.is_available(), "no GPU: nothing is measured (there is no fallback)"
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "moe", "moe_time.jsonl")
    dev = torch.device("cuda:0")
    ffn = moe.MoeFFN(HIDDEN, FFN, E, K_TOP, dev, seed=3)
    ffn.Wr.zero_()
    ffn.Wr[:, :E] = 4.0 * torch.eye(E, device=dev, dtype=torch.float16)
    dense = [(Linear_half_int4(*(a[e] for a in ffn.gate_up)), Linear_half_int4(*(a[e] for a in ffn.down))) for e in range(E)]  # views of the stacked arrays: no copy
    stage_bytes = [sum(t.numel() * t.element_size() for t in arrs) // E for arrs in (ffn.gate_up, ffn.down)]
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        for B in BATCHES:
            for active in ACTIVE:
                x, C = forced_rows(torch, B, active, dev), torch.zeros(B, HIDDEN, dtype=torch.float16, device=dev)
                ws = ffn.workspace(B)
                ffn.forward(x, C)
                torch.cuda.synchronize()
                ids = ws.ids.cpu().numpy()
                distinct = sorted(set(ids.reshape(-1).tolist()))
                act, y = torch.empty(B, FFN, dtype=torch.float16, device=dev), torch.empty(B, HIDDEN, dtype=torch.float16, device=dev)

                def dense_pairs():
                    st = _stream()
                    for e in distinct:
                        capi.check(capi.w4a16_forward(dense[e][0].desc(x, act, flags=capi.TCE_W4_SILU_MUL_PAIRS), st))
                        capi.check(capi.w4a16_forward(dense[e][1].desc(act, y), st))

                def readback():
                    st, chosen = _stream(), ws.ids.cpu()  # the synchronising copy the captured graph cannot contain
                    for e in sorted(set(chosen.reshape(-1).tolist())):
                        idx = (chosen == e).any(dim=1).nonzero().reshape(-1).to(dev)
                        xe = x.index_select(0, idx).contiguous()
                        ae, ye = act[:len(idx)], y[:len(idx)]
                        capi.check(capi.w4a16_forward(dense[e][0].desc(xe, ae, flags=capi.TCE_W4_SILU_MUL_PAIRS), st))
                        capi.check(capi.w4a16_forward(dense[e][1].desc(ae, ye), st))
                    torch.cuda.synchronize()

                forms = {"moe_all": lambda: ffn.forward(x, C), "route": lambda: moe.route(x, ffn.Wr, ws), "gate_up": lambda: moe.gate_up(x, ffn.gate_up, ws, ffn.flags),
                         "down": lambda: moe.down(ffn.down, ws, ffn.flags), "combine": lambda: moe.combine_add(C, ws), "dense": dense_pairs}
                times = {name: [] for name in list(forms) + ["readback"]}
                for _ in range(REPEATS):  # the forms alternate
                    for name, fn in forms.items():
                        times[name].append(graph_us(torch, fn))
                    readback()
                    t0 = time.perf_counter()
                    for _ in range(REPS):
                        readback()
                    times["readback"].append((time.perf_counter() - t0) * 1e6 / REPS)
                rec = {"B": B, "active_forced": active, "active": len(distinct), "reps": REPS, "replays": REPLAYS, "repeats": REPEATS,
                       "us": {n: round(statistics.median(v), 2) for n, v in times.items()}, "spread_us": {n: round(max(v) - min(v), 2) for n, v in times.items()},
                       "floor_us": {"gate_up": round((len(distinct) * stage_bytes[0] + B * HIDDEN * 2 + B * K_TOP * FFN * 2) / HBM_BYTES_PER_US, 2),
                                    "down": round((len(distinct) * stage_bytes[1] + B * K_TOP * (FFN * 2 + HIDDEN * 4)) / HBM_BYTES_PER_US, 2)}}
                f.write(json.dumps(rec) + "\n")
                f.flush()
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
