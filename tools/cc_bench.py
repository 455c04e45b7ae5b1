#!/usr/bin/env python3
"""Connected components, fused path (mgx_cc_run) against the operator path (mgx_cc_enact).
usage: cc_bench.py SCALE [--graph rmat|uniform|grid2d] [--directed [--csc]] [--seeds K] [--edgefactor EF]

Prints one JSON line: ms per run of both paths (HIP events on the context's stream, one warm-up run each, the median over K
seeds; the operator path takes no seed and is simply run K times), the stats of both, and a byte floor for the fused path.
--directed builds the R-MAT graph without the swapped copies and runs the fused path with symmetric = 0; --csc gives it a
genuine CSC as well.  The floor counts per vertex 4 B of labels in each of the eight passes that touch them (init, two
neighbour rounds, three compresses, the work list, the sizes), 4 B of row offsets in the three passes that read them and 4 B of
one entry in each neighbour round: 52 B a vertex.  The final link's entries are not counted, since which rows it reads depends on
the sample."""
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
FLOOR_BYTES_PER_VERTEX = 4 * 8 + 4 * 3 + 4 * 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scale", type=int)
    ap.add_argument("--graph", choices=["rmat", "uniform", "grid2d"], default="rmat")
    ap.add_argument("--directed", action="store_true", help="R-MAT without the swapped copies; the fused path runs with symmetric = 0")
    ap.add_argument("--csc", action="store_true", help="with --directed: build the genuine CSC the fused final pass reads")
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--edgefactor", type=int, default=16)
    args = ap.parse_args()
    if args.directed and args.graph != "rmat":
        sys.exit("--directed needs --graph rmat")
    if args.csc and not args.directed:
        sys.exit("--csc needs --directed")
    if not torch.cuda.is_available():
        sys.exit("cc_bench.py needs a GPU")

    stream = torch.cuda.current_stream()
    ctx = mini_amd.Context(0, stream.cuda_stream)
    if args.graph == "rmat":
        d = rmat.rmat_csr(ctx, args.scale, args.edgefactor, seed=args.scale, undirected=not args.directed)
    elif args.graph == "uniform":
        d = rmat.uniform_csr(ctx, args.scale, args.edgefactor)
    else:
        d = rmat.grid2d_csr(ctx, args.scale)
    g = mini_amd.Graph.from_device(ctx, d["n"], d["m"], d["row_offsets"], d["col_indices"])
    if args.csc:
        g.build_csc()
    cp = mini_amd.CcProblem(g)
    symmetric = not args.directed

    def timed(fn, *a):
        x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        x.record(stream)
        st = fn(*a)
        y.record(stream)
        y.synchronize()
        return x.elapsed_time(y), st

    seeds = [SEED0 + k for k in range(args.seeds)]
    cp.run(symmetric, seeds[0])                 # warm-up: code objects, the state's allocations
    cp.enact()
    torch.cuda.synchronize()
    fused, oper, runs = [], [], []
    labels = None
    for s in seeds:
        ms, st = timed(cp.run, symmetric, s)
        fused.append(ms)
        lab = cp.labels()
        if labels is not None and not (lab == labels).all():
            sys.exit("fused labels depend on the seed at seed %d" % s)
        labels = lab
        ms, sto = timed(cp.enact)
        oper.append(ms)
        if not (cp.labels() == labels).all():
            sys.exit("fused and operator path differ at seed %d" % s)
        runs.append((st, sto))
    st, sto = runs[0]
    n = d["n"]
    floor = FLOOR_BYTES_PER_VERTEX * n
    f_ms, o_ms = statistics.median(fused), statistics.median(oper)
    out = {
        "tool": "cc_bench", "graph": args.graph, "scale": args.scale, "n": n, "m": d["m"], "directed": args.directed,
        "csc": args.csc, "seeds": seeds, "fused_ms": round(f_ms, 4), "operator_ms": round(o_ms, 4), "speedup": round(o_ms / f_ms, 2),
        "fused_ms_all": [round(x, 4) for x in fused], "operator_ms_all": [round(x, 4) for x in oper],
        "components": st["components"], "largest": st["largest"], "largest_label": st["largest_label"],
        "skipped": [r[0]["skipped"] for r in runs], "host_waits_fused": st["host_waits"], "host_waits_operator": sto["host_waits"],
        "byte_floor": floor, "byte_floor_note": "52 B a vertex: labels in 8 passes, row offsets in 3, one entry in each neighbour round",
        "floor_GBps_at_fused": round(floor / (f_ms * 1e-3) / 1e9, 2),
    }
    print(json.dumps(out), flush=True)
    cp.close()
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
