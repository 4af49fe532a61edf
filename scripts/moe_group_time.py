#!/usr/bin/env python3
"""The two groupings of the routed pairs on the clock, in ONE process: Mixtral routing (E = 8, k = 2) and a many-expert router (E = 64, k = 8), hidden 4096 / 2048, at
P = rows * k in 32, 128, 256, 512, 1024, 4096, 16384, 65536.  Gaussian rows through the real router (random Wr): the routing is what the route kernel picks.

    route            tce_moe_route_f16: the selection, then the one-wave grouping (two launches)
    route_parallel   tce_moe_route_parallel_f16: the selection, then the parallel grouping (three launches)
    group_parallel   tce_moe_group_parallel alone, on the ids the route left
    (group_one_wave  derived, not timed: route - (route_parallel - group_parallel); the one-wave grouping has no entry point of its own)
    ffn / ffn_parallel   at 4096 pairs only: MoeFFN.forward (route, tiled contractions, combine) with parallel_group_from never reached / 0

Each form: REPS copies captured in one graph, device events around REPLAYS replays, warmed.  The forms alternate, REPEATS times; medians and spreads (max - min over
the repeats) are written.  Before a point is timed, count and the live part of the lists of the two routes are compared (a difference ends the run).
`parallel_group_from` at the end: the smallest measured P from which route_parallel is faster than route at every larger measured point OF BOTH ROUTERS by more than
both spreads -- MoeFFN.PARALLEL_GROUP_FROM_PAIRS is set from it.

    python scripts/moe_group_time.py [OUT.jsonl]        (default profiles/moe_group/moe_group_time.jsonl)
"""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from moe_tiled_time import eager_us, graph_us  # noqa: E402

PAIRS = (32, 128, 256, 512, 1024, 4096, 16384, 65536)
ROUTERS = [(4096, 8, 2), (2048, 64, 8)]  # hidden, E, k
FFN = {(4096, 8, 2): 14336, (2048, 64, 8): 1408}  # the whole layer at 4096 pairs
REPEATS, WINDOW_US = 3, 20000.0


def main():
    import torch
    from tinychatengine_amd import moe
    assert torch.cuda.is_available(), "no GPU: nothing is measured (there is no fallback)"
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "moe_group", "moe_group_time.jsonl")
    dev, recs = torch.device("cuda:0"), []
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        for hidden, E, k in ROUTERS:
            Wr = torch.empty(E, hidden, device=dev).normal_(0, 1, generator=torch.Generator(device=dev).manual_seed(E)).half()
            for P in PAIRS:
                rows = P // k
                x = torch.empty(rows, hidden, device=dev).normal_(0, 1, generator=torch.Generator(device=dev).manual_seed(P)).half()
                ws, wp = moe.MoeWorkspace(rows, k, E, 128, dev), moe.MoeWorkspace(rows, k, E, 128, dev)
                moe.route(x, Wr, ws)
                moe.route(x, Wr, wp, parallel=True)
                torch.cuda.synchronize()
                count, lst, plst = ws.count.cpu().numpy(), ws.list.cpu().numpy(), wp.list.cpu().numpy()
                assert (count == wp.count.cpu().numpy()).all() and all((lst[e, :count[e]] == plst[e, :count[e]]).all() for e in range(E)), "the groupings differ"
                forms = {"route": lambda: moe.route(x, Wr, ws), "route_parallel": lambda: moe.route(x, Wr, wp, parallel=True), "group_parallel": lambda: moe.group_parallel(wp)}
                if P == 4096:
                    ffn, C = moe.MoeFFN(hidden, FFN[(hidden, E, k)], E, k, dev, seed=3), torch.zeros_like(x)
                    at = lambda frm: (setattr(ffn, "parallel_group_from", frm), ffn.forward(x, C))  # (the threshold is read when the launches are issued or captured)
                    forms.update({"ffn": lambda: at(1 << 30), "ffn_parallel": lambda: at(0)})
                reps = {n: int(min(200, max(2, WINDOW_US / max(eager_us(torch, fn), 1.0)))) for n, fn in forms.items()}
                times = {n: [] for n in forms}
                for _ in range(REPEATS):  # the forms alternate
                    for n, fn in forms.items():
                        times[n].append(graph_us(torch, fn, reps[n]))
                us = {n: round(statistics.median(v), 2) for n, v in times.items()}
                us["group_one_wave_derived"] = round(us["route"] - (us["route_parallel"] - us["group_parallel"]), 2)
                rec = {"hidden": hidden, "E": E, "k": k, "rows": rows, "P": P, "count_max": int(count.max()), "reps": reps, "repeats": REPEATS, "us": us,
                       "spread_us": {n: round(max(v) - min(v), 2) for n, v in times.items()}}
                recs.append(rec)
                f.write(json.dumps(rec) + "\n")
                f.flush()
                print(json.dumps(rec), flush=True)
                forms.clear()
        won = {P: all(r["us"]["route"] - r["us"]["route_parallel"] > r["spread_us"]["route"] + r["spread_us"]["route_parallel"] for r in recs if r["P"] == P) for P in PAIRS}
        frm = None
        for P in reversed(PAIRS):
            if not won[P]:
                break
            frm = P
        f.write(json.dumps({"parallel_group_from": frm, "parallel_faster_by_more_than_the_spreads": sorted(won.items())}) + "\n")
        print({"parallel_group_from": frm}, flush=True)


if __name__ == "__main__":
    main()
