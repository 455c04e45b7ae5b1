#!/usr/bin/env python3
"""k-truss decomposition, fused path (mgx_ktruss_run), optionally against the operator path (mgx_ktruss_enact).
usage: ktruss_bench.py SCALE [--graph rmat|uniform|grid2d] [--directed] [--operator] [--rounds K] [--edgefactor EF]

Prints one JSON line, HIP events on the context's stream, one warm-up handle, the median, minimum and maximum over K rounds (a fresh
handle each):
  * ms of the fused path's first run on a fresh handle (builds of the oriented graph and of the adjacency with edge ids, supports,
    peel) and of its repeat run (supports and peel only);
  * the repeat run's support launches and its peel separately, from one more run with the library's own events
    (mgx_ktruss_set_timing: a few microseconds of stream gap per event, so the split is not taken from the timed runs);
  * levels, passes, launches and host waits of the repeat run;
  * beside them mgx_tc_run's repeat run on the same graph, and support / triangle count: what sending the adds to the three
    entries of a triangle, one of them un-aggregated, costs over adding to its three vertices;
  * with --operator the same two figures for the operator path (ONE round: it makes three host waits a pass).
--directed builds the R-MAT graph without the swapped copies and runs with symmetric = 0."""
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


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scale", type=int)
    ap.add_argument("--graph", choices=["rmat", "uniform", "grid2d"], default="rmat")
    ap.add_argument("--directed", action="store_true", help="R-MAT without the swapped copies; symmetric = 0")
    ap.add_argument("--operator", action="store_true", help="time the operator path as well (one round)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--edgefactor", type=int, default=16)
    args = ap.parse_args()
    if args.directed and args.graph != "rmat":
        sys.exit("--directed needs --graph rmat")
    if not torch.cuda.is_available():
        sys.exit("ktruss_bench.py needs a GPU")

    stream = torch.cuda.current_stream()
    ctx = mini_amd.Context(0, stream.cuda_stream)
    if args.graph == "rmat":
        d = rmat.rmat_csr(ctx, args.scale, args.edgefactor, seed=args.scale, undirected=not args.directed)
    elif args.graph == "uniform":
        d = rmat.uniform_csr(ctx, args.scale, args.edgefactor)
    else:
        d = rmat.grid2d_csr(ctx, args.scale)
    g = mini_amd.Graph.from_device(ctx, d["n"], d["m"], d["row_offsets"], d["col_indices"])
    symmetric = not args.directed

    def timed(fn, *a):
        x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        x.record(stream)
        st = fn(*a)
        y.record(stream)
        y.synchronize()
        return x.elapsed_time(y), st

    def one_handle(cls, method):
        """(ms of the first run, ms of the repeat run, stats of the repeat run, the handle) of a fresh handle"""
        h = cls(g)
        first, _ = timed(getattr(h, method), symmetric)
        again, st = timed(getattr(h, method), symmetric)
        return first, again, st, h

    def rounds_of(cls, method, rounds):
        one_handle(cls, method)[3].close()          # warm-up: code objects, allocator
        firsts, repeats = [], []
        for _ in range(rounds):
            f, r, st, h = one_handle(cls, method)
            firsts.append(f)
            repeats.append(r)
            if _ < rounds - 1:
                h.close()
        return firsts, repeats, st, h

    out = {"tool": "ktruss_bench", "graph": args.graph, "scale": args.scale, "n": d["n"], "m": d["m"], "directed": args.directed,
           "rounds": args.rounds}
    firsts, repeats, st, kp = rounds_of(mini_amd.KtrussProblem, "run", args.rounds)
    out.update({"fused_first_ms": spread(firsts), "fused_repeat_ms": spread(repeats)})
    out.update({k: st[k] for k in ("max_truss", "edges", "triangles", "levels", "passes")})
    out.update({"launches_repeat": st["launches"], "host_waits_repeat": st["host_waits"]})
    kp.set_timing(True)
    kp.run(symmetric)
    out["fused_phase_ms"] = {k: round(v, 4) for k, v in kp.phase_ms().items()}
    kp.set_timing(False)
    truss = kp.edges()[2]
    kp.close()
    _, tc_repeats, tst, tp = rounds_of(mini_amd.TcProblem, "run", args.rounds)
    tp.close()
    if tst["triangles"] != st["triangles"]:
        sys.exit("the supports' total and the triangle count differ")
    out["tc_repeat_ms"] = spread(tc_repeats)
    out["support_over_tc"] = round(out["fused_phase_ms"]["support"] / out["tc_repeat_ms"]["median"], 2)
    if args.operator:
        f, r, sto, ko = one_handle(mini_amd.KtrussProblem, "enact")
        same = np.array_equal(ko.edges()[2], truss) and all(sto[k] == st[k] for k in ("max_truss", "edges", "triangles", "levels", "passes"))
        ko.close()
        if not same:
            sys.exit("fused and operator path differ")
        out.update({"operator_first_ms": round(f, 4), "operator_repeat_ms": round(r, 4), "host_waits_operator": sto["host_waits"],
                    "repeat_speedup": round(r / out["fused_repeat_ms"]["median"], 2)})
    print(json.dumps(out), flush=True)
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
