#!/usr/bin/env python3
"""PageRank to convergence, fused path (mgx_pagerank_run) against the operator path (mgx_pagerank_enact).
usage: pagerank_bench.py SCALE [--graph rmat|uniform|grid2d] [--directed --csc] [--iters T] [--no-layout] [--edgefactor EF]

Prints one JSON line:
  * ms per iteration of both paths at tol = 0, max_iter = T (HIP events on the context's stream around the whole run, divided by
    the iterations it made; one warm-up run each, the median of 5 and all five);
  * ms of ONE full-frontier neighbour-reduce call on the same graph (mini_amd.segreduce, f32_plus: what bench.py --mode pr times),
    median of 5 after a warm-up -- the comparator of a fused iteration;
  * a run to tol = 1e-6 on both paths: iterations, ms, host waits;
  * a byte floor for one iteration: 4 B an entry (its neighbour id; the values it gathers are counted once per vertex) plus 24 B a
    vertex (contribution read by the reduce, S written and read, offsets, old rank in; rank and contribution out).
--directed builds the R-MAT graph without the swapped copies and needs --csc (the in-entries come from the genuine CSC); such a run
takes the general reduce, as does --no-layout."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mini_amd  # noqa: E402
from mini_amd import rmat  # noqa: E402

REPS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scale", type=int)
    ap.add_argument("--graph", choices=["rmat", "uniform", "grid2d"], default="rmat")
    ap.add_argument("--directed", action="store_true", help="R-MAT without the swapped copies; runs with symmetric = 0")
    ap.add_argument("--csc", action="store_true", help="build the genuine CSC (needed with --directed)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--alpha", type=float, default=0.85)
    ap.add_argument("--no-layout", action="store_true", help="no hub-first layout: the general reduce")
    ap.add_argument("--edgefactor", type=int, default=16)
    args = ap.parse_args()
    if args.directed and args.graph != "rmat":
        sys.exit("--directed needs --graph rmat")
    if args.directed and not args.csc:
        sys.exit("--directed needs --csc: the in-entries come from the graph's genuine CSC")
    if not torch.cuda.is_available():
        sys.exit("pagerank_bench.py needs a GPU")

    stream = torch.cuda.current_stream()
    ctx = mini_amd.Context(0, stream.cuda_stream)
    if args.graph == "rmat":
        d = rmat.rmat_csr(ctx, args.scale, args.edgefactor, seed=args.scale, undirected=not args.directed)
    elif args.graph == "uniform":
        d = rmat.uniform_csr(ctx, args.scale, args.edgefactor)
    else:
        d = rmat.grid2d_csr(ctx, args.scale)
    n, m = d["n"], d["m"]
    g = mini_amd.Graph.from_device(ctx, n, m, d["row_offsets"], d["col_indices"])
    if args.csc:
        g.build_csc()
    if not args.no_layout:
        g.build_layout()
    pp = mini_amd.PageRankProblem(g)
    symmetric = not args.directed

    def timed(fn, *a):
        x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        x.record(stream)
        st = fn(*a)
        y.record(stream)
        y.synchronize()
        return x.elapsed_time(y), st

    T = args.iters
    pp.run(args.alpha, 0.0, T, symmetric)            # warm-up: code objects, the state's allocations, the layout's slices
    pp.enact(args.alpha, 0.0, T, symmetric)
    torch.cuda.synchronize()
    fused, oper = [], []
    ranks = None
    for _ in range(REPS):
        ms, sf = timed(pp.run, args.alpha, 0.0, T, symmetric)
        fused.append(ms / max(sf["iterations"], 1))
        r = pp.ranks()
        if ranks is not None and not (r == ranks).all():
            sys.exit("two fused runs gave different ranks")
        ranks = r
        ms, so = timed(pp.enact, args.alpha, 0.0, T, symmetric)
        oper.append(ms / max(so["iterations"], 1))
    conv = {}
    for name, fn in (("fused", pp.run), ("operator", pp.enact)):
        ms, st = timed(fn, args.alpha, 1e-6, 1000, symmetric)
        conv[name] = {"iterations": st["iterations"], "converged": st["converged"], "ms": round(ms, 4), "host_waits": st["host_waits"],
                      "launches": st["launches"], "residual": st["residual"]}

    # one full-frontier neighbour-reduce call, as bench.py --mode pr times it (push: the CSR's rows, what a symmetric run reduces over)
    f = mini_amd.Frontier(ctx, n).fill_iota(n)
    vals = torch.rand(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(args.scale))
    red = torch.empty(n, device="cuda")
    mini_amd.segreduce(g, f, vals, 0.0, red, "f32_plus")
    torch.cuda.synchronize()
    reduce_ms = [timed(mini_amd.segreduce, g, f, vals, 0.0, red, "f32_plus")[0] for _ in range(REPS)]

    f_ms, o_ms, r_ms = statistics.median(fused), statistics.median(oper), statistics.median(reduce_ms)
    floor = 4 * m + 24 * n
    out = {
        "tool": "pagerank_bench", "graph": args.graph, "scale": args.scale, "n": n, "m": m, "directed": args.directed, "csc": args.csc,
        "layout": not args.no_layout, "layout_path": sf["layout_path"], "alpha": args.alpha, "iters": T,
        "fused_ms_per_iter": round(f_ms, 4), "operator_ms_per_iter": round(o_ms, 4), "reduce_call_ms": round(r_ms, 4),
        "fused_over_reduce": round(f_ms / r_ms, 3), "operator_over_fused": round(o_ms / f_ms, 2),
        "fused_ms_per_iter_all": [round(x, 4) for x in fused], "operator_ms_per_iter_all": [round(x, 4) for x in oper],
        "reduce_call_ms_all": [round(x, 4) for x in reduce_ms],
        "host_waits_fused": sf["host_waits"], "host_waits_operator": so["host_waits"], "launches_fused": sf["launches"],
        "dangling": sf["dangling"], "to_tol_1e-6": conv,
        "byte_floor": floor, "byte_floor_note": "4 B an entry + 24 B a vertex per iteration",
        "floor_GBps_at_fused": round(floor / (f_ms * 1e-3) / 1e9, 2),
    }
    print(json.dumps(out), flush=True)
    f.close()
    pp.close()
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
