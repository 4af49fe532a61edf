#!/usr/bin/env python3
"""The two forms of the expert contractions on the clock at prompt sizes, in ONE process: Mixtral-8x7B's FFN shapes (hidden 4096, ffn 14336, E = 8, k = 2) at rows 16,
64, 128, 256, 512 and 2048, and one many-expert point (E = 64, k = 8, hidden 2048, ffn 1408) at rows 512.  Gaussian rows through the real router (random Wr): the
routing is what the route kernel picks; the experts' counts are written with the times.

    passes / tiled   gate_up and down in each form (moe.gate_up / moe.down(tiled=)): REPS copies captured in one graph, device events around REPLAYS replays, warmed
    dense            scripts/moe_time.py's yardstick: tce_w4a16_forward gate_up (pair epilogue) + down at M = the expert's pair count, once per ACTIVE expert -- the
                     same weight bytes through the dense kernels (the gather they would need is not charged)
    route            the two route launches at this P (the grouping is one wave that walks every pair)

The forms alternate, REPEATS times; medians and spreads (max - min over the repeats) are written.  `tiled_from` at the end: the smallest measured P from which the
tiled pair of launches is faster than the pass pair at every larger measured Mixtral point by more than both spreads -- MoeFFN.TILED_FROM_PAIRS is set from it.

    python scripts/moe_tiled_time.py [OUT.jsonl]        (default profiles/moe_tiled/moe_tiled_time.jsonl)
"""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MIXTRAL = [(4096, 14336, 8, 2, rows) for rows in (16, 64, 128, 256, 512, 2048)]
POINTS = MIXTRAL + [(2048, 1408, 64, 8, 512)]
REPLAYS, WARMUP, REPEATS = 5, 2, 3
WINDOW_US = 20000.0  # a timed window (one replay) is REPS copies sized to about this long from a first eager measurement, 2 <= REPS <= 200


def graph_us(torch, fn, reps):
    """median microseconds of one fn() among `reps` captured copies, over REPLAYS replays"""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(reps):
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
        out.append(a.elapsed_time(b) * 1000.0 / reps)
    return statistics.median(out)


def eager_us(torch, fn):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0


def main():
    import torch
    from tinychatengine_amd import capi, moe
    from tinychatengine_amd.linear import Linear_half_int4, _stream
    assert torch.cuda.is_available(), "no GPU: nothing is measured (there is no fallback)"
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "moe_tiled", "moe_tiled_time.jsonl")
    dev, layers, recs = torch.device("cuda:0"), {}, []
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        for hidden, ffn_n, E, k, rows in POINTS:
            if (hidden, ffn_n, E, k) not in layers:
                layers.clear()  # (one layer's experts at a time on the device)
                layers[(hidden, ffn_n, E, k)] = moe.MoeFFN(hidden, ffn_n, E, k, dev, seed=3)
            ffn = layers[(hidden, ffn_n, E, k)]
            x = torch.empty(rows, hidden, device=dev).normal_(0, 1, generator=torch.Generator(device=dev).manual_seed(rows)).half()
            ws = ffn.workspace(rows)
            moe.route(x, ffn.Wr, ws, ffn.renormalize)
            moe.gate_up(x, ffn.gate_up, ws, ffn.flags)  # (act holds real values for both down forms)
            torch.cuda.synchronize()
            count = ws.count.cpu().numpy().tolist()
            dense = [(e, c, Linear_half_int4(*(a[e] for a in ffn.gate_up)), Linear_half_int4(*(a[e] for a in ffn.down))) for e, c in enumerate(count) if c > 0]
            xd, ad, yd = x, torch.empty(max(count), ffn_n, dtype=torch.float16, device=dev), torch.empty(max(count), hidden, dtype=torch.float16, device=dev)

            def dense_pairs():
                st = _stream()
                for _, c, gu, dn in dense:
                    capi.check(capi.w4a16_forward(gu.desc(xd[:c], ad[:c], flags=capi.TCE_W4_SILU_MUL_PAIRS), st))
                    capi.check(capi.w4a16_forward(dn.desc(ad[:c], yd[:c]), st))

            forms = {"gate_up_passes": lambda: moe.gate_up(x, ffn.gate_up, ws, ffn.flags), "gate_up_tiled": lambda: moe.gate_up(x, ffn.gate_up, ws, ffn.flags, tiled=True),
                     "down_passes": lambda: moe.down(ffn.down, ws, ffn.flags), "down_tiled": lambda: moe.down(ffn.down, ws, ffn.flags, tiled=True),
                     "dense": dense_pairs, "route": lambda: moe.route(x, ffn.Wr, ws, ffn.renormalize)}
            try:  # (a shape the dense dispatcher refuses is reported, not measured)
                dense_pairs()
                torch.cuda.synchronize()
                dense_note = None
            except Exception as err:
                dense_note = str(err)[:200]
                del forms["dense"]
            reps = {n: int(min(200, max(2, WINDOW_US / max(eager_us(torch, fn), 1.0)))) for n, fn in forms.items()}
            times = {n: [] for n in forms}
            for _ in range(REPEATS):  # the forms alternate
                for n, fn in forms.items():
                    times[n].append(graph_us(torch, fn, reps[n]))
            rec = {"dense_refused": dense_note, "hidden": hidden, "ffn": ffn_n, "E": E, "k": k, "rows": rows, "P": rows * k, "count": count, "reps": reps, "replays": REPLAYS, "repeats": REPEATS,
                   "us": {n: round(statistics.median(v), 2) for n, v in times.items()}, "spread_us": {n: round(max(v) - min(v), 2) for n, v in times.items()}}
            recs.append(rec)
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)
        pair = lambda r, form: r["us"]["gate_up_" + form] + r["us"]["down_" + form]
        wins = [(r["P"], pair(r, "passes") - pair(r, "tiled") > sum(r["spread_us"][n] for n in ("gate_up_passes", "gate_up_tiled", "down_passes", "down_tiled")))
                for r in recs[:len(MIXTRAL)]]
        frm = None
        for P, won in reversed(wins):
            if not won:
                break
            frm = P
        f.write(json.dumps({"tiled_from": frm, "tiled_faster_by_more_than_the_spreads": wins}) + "\n")
        print({"tiled_from": frm}, flush=True)


if __name__ == "__main__":
    main()
