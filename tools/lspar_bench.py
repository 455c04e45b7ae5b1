#!/usr/bin/env python3
"""Local sparsification, fused path (mgx_lspar_run) against the operator path (mgx_lspar_enact).
usage: lspar_bench.py SCALE [--graph rmat|uniform] [--k K] [--e E] [--seeds S] [--edgefactor EF] [--no-layout]

Prints one JSON line: ms per sparsification of both paths (HIP events on the context's stream, one warm-up run each, the
median over S seeds), kept entries, rows cut, host waits, and a byte FLOOR for the fused path with its fraction of 8 TB/s:
8 (n + 1) + 8 m (two reads of the row structure) + 4 k m (the neighbours' minhashes) + 8 k n (the table written and read)
+ 12 sum(t) + 4 (n + 1) (the output).  It is a lower bound: the gathers of the neighbours' minhashes move whole lines."""
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
HBM = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scale", type=int)
    ap.add_argument("--graph", choices=["rmat", "uniform"], default="rmat")
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--e", type=float, default=0.5)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--no-layout", action="store_true", help="do not build the hub-first layout (the operator path's fast reduce needs it)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lspar_bench.py needs a GPU")

    stream = torch.cuda.current_stream()
    ctx = mini_amd.Context(0, stream.cuda_stream)
    if args.graph == "rmat":
        d = rmat.rmat_csr(ctx, args.scale, args.edgefactor, seed=args.scale)
    else:
        d = rmat.uniform_csr(ctx, args.scale, args.edgefactor)
    g = mini_amd.Graph.from_device(ctx, d["n"], d["m"], d["row_offsets"], d["col_indices"])
    if not args.no_layout:
        g.build_layout()
    lp = mini_amd.LsparProblem(g)

    def timed(fn, seed):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        st = fn(seed, args.k, args.e)
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), st

    seeds = [SEED0 + s for s in range(args.seeds)]
    lp.run(seeds[0], args.k, args.e)                     # warm-up: code objects, the states' allocations
    lp.enact(seeds[0], args.k, args.e)
    torch.cuda.synchronize()
    fused, oper, stats = [], [], []
    for s in seeds:
        ms, st = timed(lp.run, s)
        fused.append(ms)
        ms, sto = timed(lp.enact, s)
        oper.append(ms)
        if (st["kept"], st["rows_cut"]) != (sto["kept"], sto["rows_cut"]):
            sys.exit("fused and operator path differ at seed %d" % s)
        stats.append((st, sto))
    st, sto = stats[0]
    n, m, k, kept = d["n"], d["m"], args.k, st["kept"]
    floor = 8 * (n + 1) + 8 * m + 4 * k * m + 8 * k * n + 12 * kept + 4 * (n + 1)
    f_ms, o_ms = statistics.median(fused), statistics.median(oper)
    out = {
        "tool": "lspar_bench", "graph": args.graph, "scale": args.scale, "n": n, "m": m, "k": k, "e": args.e,
        "layout": not args.no_layout, "seeds": seeds,
        "fused_ms": round(f_ms, 4), "operator_ms": round(o_ms, 4), "speedup": round(o_ms / f_ms, 2),
        "fused_ms_all": [round(x, 4) for x in fused], "operator_ms_all": [round(x, 4) for x in oper],
        "kept": kept, "rows_cut": st["rows_cut"], "host_waits_fused": st["host_waits"], "host_waits_operator": sto["host_waits"],
        "byte_floor": floor, "byte_floor_ms_at_8TBps": round(floor / HBM * 1e3, 4),
        "fused_fraction_of_8TBps": round(floor / HBM * 1e3 / f_ms, 3),
    }
    print(json.dumps(out), flush=True)
    lp.close()
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
