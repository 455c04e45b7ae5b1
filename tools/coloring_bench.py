#!/usr/bin/env python3
"""Graph colouring, fused path (mgx_color_run) against the operator path (mgx_color_enact), to completion (max_iter = 0).
usage: coloring_bench.py SCALE [--graph rmat|uniform|grid2d] [--seeds K] [--edgefactor EF] [--no-layout]

Prints one JSON line: ms per colouring of both paths (HIP events on the context's stream, one warm-up run each, the median over
K seeds), rounds, colours used, host waits, the active vertices at the start of every round, and a byte floor for the fused
path: per round the row offsets (8 bytes) of every active vertex and one pass over the uncoloured bitmap (n / 8 bytes).  It is
a lower bound only: how many entries a row scans depends on where its early exit falls."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mini_amd  # noqa: E402
from mini_amd import rmat  # noqa: E402

SEED0 = 15485863


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scale", type=int)
    ap.add_argument("--graph", choices=["rmat", "uniform", "grid2d"], default="rmat")
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--no-layout", action="store_true", help="do not build the hub-first layout (the operator path's fast reduce needs it)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("coloring_bench.py needs a GPU")

    stream = torch.cuda.current_stream()
    ctx = mini_amd.Context(0, stream.cuda_stream)
    if args.graph == "rmat":
        d = rmat.rmat_csr(ctx, args.scale, args.edgefactor, seed=args.scale)
    elif args.graph == "uniform":
        d = rmat.uniform_csr(ctx, args.scale, args.edgefactor)
    else:
        d = rmat.grid2d_csr(ctx, args.scale)
    g = mini_amd.Graph.from_device(ctx, d["n"], d["m"], d["row_offsets"], d["col_indices"])
    if not args.no_layout:
        g.build_layout()
    cp = mini_amd.ColorProblem(g)

    def timed(fn, seed):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        st = fn(seed, 0)
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), st

    seeds = [SEED0 + k for k in range(args.seeds)]
    cp.run(seeds[0], 0)                      # warm-up: code objects, the state's allocations
    cp.enact(seeds[0], 0)
    torch.cuda.synchronize()
    fused, oper, runs = [], [], []
    for s in seeds:
        ms, st = timed(cp.run, s)
        fused.append(ms)
        colours = cp.colors()
        trace = cp.round_trace()
        runs.append((st, int(colours.max()) if len(colours) else 0, int(len(set(colours.tolist()))), trace))
        ms, sto = timed(cp.enact, s)
        oper.append(ms)
        if not (cp.colors() == colours).all() or sto["rounds"] != st["rounds"]:
            sys.exit("fused and operator path differ at seed %d" % s)
        runs[-1] = runs[-1] + (sto,)
    st, top, used, trace, sto = runs[0]
    n = d["n"]
    floor = int(sum(8 * int(a) + (n + 7) // 8 for a in trace))
    f_ms, o_ms = statistics.median(fused), statistics.median(oper)
    out = {
        "tool": "coloring_bench", "graph": args.graph, "scale": args.scale, "n": n, "m": d["m"], "layout": not args.no_layout,
        "seeds": seeds, "fused_ms": round(f_ms, 4), "operator_ms": round(o_ms, 4), "speedup": round(o_ms / f_ms, 2),
        "fused_ms_all": [round(x, 4) for x in fused], "operator_ms_all": [round(x, 4) for x in oper],
        "rounds": st["rounds"], "colors_used": used, "max_color": top, "uncolored": st["uncolored"],
        "host_waits_fused": st["host_waits"], "host_waits_operator": sto["host_waits"],
        "fused_us_per_round": round(f_ms * 1e3 / max(st["rounds"], 1), 2),
        "operator_us_per_round": round(o_ms * 1e3 / max(st["rounds"], 1), 2),
        "active_per_round": [int(a) for a in trace],
        "byte_floor": floor, "byte_floor_note": "per round: 8 B of row offsets per active vertex + n/8 B of bitmap; entries scanned not counted",
        "floor_GBps_at_fused": round(floor / (f_ms * 1e-3) / 1e9, 2),
    }
    print(json.dumps(out), flush=True)
    cp.close()
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
