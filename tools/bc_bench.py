#!/usr/bin/env python3
"""Betweenness centrality, fused path (mgx_bc_run) against the operator path (mgx_bc_enact).
usage: bc_bench.py SCALE [--graph rmat|uniform|grid2d] [--directed --csc] [--sources K] [--operator] [--no-layout] [--edgefactor EF]

Prints one JSON line.  HIP events on the context's stream, one warm-up, the median of 5 runs (and all five):
  * ms per source of the fused path over K sources (bench.py's sources: rmat.pick_sources), and its split into traversal, list
    build (clears, keys, sort, bounds), forward and backward launches -- from a run of its own with the library's phase events on
    (mgx_bc_set_timing: a few microseconds of stream gap per event, so the split is not taken from the timed runs);
  * with --operator the ms per source of the operator path (its traversal and its forward pass are one loop: no split);
  * the ms per source of ONE bench.py-style batched BFS of the same sources on the same graph (mgx_bfs_run_many, push mode);
  * the ms of ONE full-frontier neighbour-reduce call on the same graph (mini_amd.segreduce, f32_plus: what bench.py --mode pr times);
  * the ratio t_bc / (t_bfs + 2 t_nreduce): that sum is the price of one traversal plus two gather sweeps before this path existed
    (the gathers here are 8 bytes where the neighbour-reduce's are 4).
--directed builds the R-MAT graph without the swapped copies and needs --csc (the in-entries come from the genuine CSC)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
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
    ap.add_argument("--sources", type=int, default=8)
    ap.add_argument("--operator", action="store_true", help="time the operator path as well")
    ap.add_argument("--no-layout", action="store_true", help="no hub-first layout under the traversal")
    ap.add_argument("--edgefactor", type=int, default=16)
    args = ap.parse_args()
    if args.directed and args.graph != "rmat":
        sys.exit("--directed needs --graph rmat")
    if args.directed and not args.csc:
        sys.exit("--directed needs --csc: the in-entries come from the graph's genuine CSC")
    if not torch.cuda.is_available():
        sys.exit("bc_bench.py needs a GPU")

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
    symmetric = not args.directed
    K = args.sources
    src = np.array(rmat.pick_sources(d["row_offsets"].cpu().numpy(), K, args.scale), dtype=np.int32)

    def timed(fn, *a):
        x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        x.record(stream)
        st = fn(*a)
        y.record(stream)
        y.synchronize()
        return x.elapsed_time(y), st

    bp = mini_amd.BcProblem(g)
    bp.run(src, symmetric)                                     # warm-up: code objects, the handle's state, the row classes
    torch.cuda.synchronize()
    fused, bc0 = [], None
    for _ in range(REPS):
        ms, sf = timed(bp.run, src, symmetric)
        fused.append(ms / K)
        bc = bp.centrality()
        if bc0 is not None and not np.array_equal(bc, bc0):
            sys.exit("two fused runs gave different centralities")
        bc0 = bc
    bp.set_timing(True)
    bp.run(src, symmetric)
    split = {k: (round(v, 4) if k != "sources_timed" else v) for k, v in bp.phase_ms().items()}
    bp.set_timing(False)
    info = bp.info()
    oper, so = [], None
    if args.operator:
        bp.enact(src, symmetric)
        torch.cuda.synchronize()
        for _ in range(REPS):
            ms, so = timed(bp.enact, src, symmetric)
            oper.append(ms / K)

    # the same sources as one batched BFS, as bench.py times it
    bfs = mini_amd.BfsProblem(g, int(src[0]))
    prepared = mini_amd.BfsProblem.prepare_many(src)
    bfs.run_many(src, prepared=prepared)
    torch.cuda.synchronize()
    bfs_ms = [timed(lambda: bfs.run_many(src, prepared=prepared))[0] / K for _ in range(REPS)]

    # one full-frontier neighbour-reduce call, as bench.py --mode pr times it
    f = mini_amd.Frontier(ctx, n).fill_iota(n)
    vals = torch.rand(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(args.scale))
    red = torch.empty(n, device="cuda")
    mini_amd.segreduce(g, f, vals, 0.0, red, "f32_plus")
    torch.cuda.synchronize()
    reduce_ms = [timed(mini_amd.segreduce, g, f, vals, 0.0, red, "f32_plus")[0] for _ in range(REPS)]

    f_ms, b_ms, r_ms = statistics.median(fused), statistics.median(bfs_ms), statistics.median(reduce_ms)
    out = {
        "tool": "bc_bench", "graph": args.graph, "scale": args.scale, "n": n, "m": m, "directed": args.directed, "csc": args.csc,
        "layout": not args.no_layout, "sources": K,
        "fused_ms_per_source": round(f_ms, 4), "fused_ms_per_source_all": [round(x, 4) for x in fused], "fused_split_ms": split,
        "bfs_ms_per_source": round(b_ms, 4), "bfs_ms_per_source_all": [round(x, 4) for x in bfs_ms],
        "reduce_call_ms": round(r_ms, 4), "reduce_call_ms_all": [round(x, 4) for x in reduce_ms],
        "fused_over_bfs_plus_two_reduces": round(f_ms / (b_ms + 2.0 * r_ms), 3),
        "levels": sf["levels"], "reached": sf["reached"], "host_waits": sf["host_waits"], "traversal_waits": sf["traversal_waits"],
        "launches": sf["launches"], "chain_launches": sf["chain_launches"], "inexact": sf["inexact"], "info": info,
    }
    if args.operator:
        o_ms = statistics.median(oper)
        out.update({"operator_ms_per_source": round(o_ms, 4), "operator_ms_per_source_all": [round(x, 4) for x in oper],
                    "operator_over_fused": round(o_ms / f_ms, 2), "operator_over_bfs_plus_two_reduces": round(o_ms / (b_ms + 2.0 * r_ms), 3),
                    "host_waits_operator": so["host_waits"]})
    print(json.dumps(out), flush=True)
    f.close()
    bfs.close()
    bp.close()
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
