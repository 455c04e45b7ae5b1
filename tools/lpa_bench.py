#!/usr/bin/env python3
"""Label propagation, fused path (mgx_lpa_run), optionally against the operator path (mgx_lpa_enact), and the modularity of what it
returns.
usage: lpa_bench.py SCALE [--graph rmat|uniform|grid2d] [--directed --csc] [--sync] [--operator] [--rounds K] [--edgefactor EF]
                          [--max-iter N]

The graph is symmetric (R-MAT with the swapped copies, edge factor 16; the uniform and grid generators' graphs as they are) and the
run is told so; with --directed the R-MAT pairs are kept as they are, the run counts every entry at both of its ends
(symmetric = 0) and needs --csc: the genuine CSC, built on the device first and not timed.  Prints one JSON line, HIP events on
the context's stream, one warm-up handle, the median, minimum and maximum over K rounds (a fresh handle each):
  * ms of the fused path's first run on a fresh handle (its allocations included) and of its repeat run;
  * the repeat run's phases (setup, evaluations, long rows, applies) from one more run with the device's wall clock
    (mgx_lpa_set_timing), ms per iteration from them, its launches, host waits and kinds;
  * the rows evaluated beside n x (iterations + 1), the vertices per body, the rows that overflowed their table;
  * communities and Q (mgx_modularity of the labels, its ms);
  * one full-frontier neighbour-reduce call (mgx_segreduce_f32_plus) on the same graph: a DENSE iteration reads the same entries once;
  * with --operator the operator path's first and repeat run (ONE round), and repeat / repeat."""
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

STATS = ("communities", "largest", "largest_label", "iterations", "converged", "unstable")


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scale", type=int)
    ap.add_argument("--graph", choices=["rmat", "uniform", "grid2d"], default="rmat")
    ap.add_argument("--directed", action="store_true", help="R-MAT without the swapped copies, symmetric = 0 (needs --csc)")
    ap.add_argument("--csc", action="store_true", help="build the genuine CSC first")
    ap.add_argument("--sync", action="store_true", help="the synchronous rule instead of the lazy one")
    ap.add_argument("--operator", action="store_true", help="time the operator path as well (one round)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--max-iter", type=int, default=100)
    args = ap.parse_args()
    if args.directed and (args.graph != "rmat" or not args.csc):
        sys.exit("--directed is for --graph rmat and needs --csc")
    if not torch.cuda.is_available():
        sys.exit("lpa_bench.py needs a GPU")

    stream = torch.cuda.current_stream()
    ctx = mini_amd.Context(0, stream.cuda_stream)
    if args.graph == "rmat":
        d = rmat.rmat_csr(ctx, args.scale, args.edgefactor, seed=args.scale, undirected=not args.directed)
    elif args.graph == "uniform":
        d = rmat.uniform_csr(ctx, args.scale, args.edgefactor)
    else:
        d = rmat.grid2d_csr(ctx, args.scale)
    n = d["n"]
    g = mini_amd.Graph.from_device(ctx, n, d["m"], d["row_offsets"], d["col_indices"])
    if args.csc:
        g.build_csc()
    run_args = dict(symmetric=not args.directed, mode=mini_amd.LpaProblem.SYNC if args.sync else mini_amd.LpaProblem.LAZY,
                    max_iter=args.max_iter)

    def timed(fn, *a, **kw):
        x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        x.record(stream)
        st = fn(*a, **kw)
        y.record(stream)
        y.synchronize()
        return x.elapsed_time(y), st

    def one_handle(method):
        """(ms of the first run, ms of the repeat run, stats of the repeat run, the handle) of a fresh handle"""
        h = mini_amd.LpaProblem(g)
        first, _ = timed(getattr(h, method), **run_args)
        again, st = timed(getattr(h, method), **run_args)
        return first, again, st, h

    one_handle("run")[3].close()                      # warm-up: code objects, allocator
    firsts, repeats = [], []
    for i in range(args.rounds):
        f, r, st, lp = one_handle("run")
        firsts.append(f)
        repeats.append(r)
        if i < args.rounds - 1:
            lp.close()
    out = {"tool": "lpa_bench", "graph": args.graph, "scale": args.scale, "n": n, "m": d["m"], "symmetric": int(not args.directed),
           "mode": "sync" if args.sync else "lazy", "rounds_timed": args.rounds}
    out.update({"fused_first_ms": spread(firsts), "fused_repeat_ms": spread(repeats)})
    out.update({k: st[k] for k in STATS})
    iters = st["iterations"] + 1
    out.update({"rows_evaluated": st["evaluated"], "rows_if_every_row": n * iters, "overflowed": st["overflowed"],
                "launches_repeat": st["launches"], "host_waits_repeat": st["host_waits"], "bins": lp.bins()})
    kinds = lp.step_kinds()
    out["launches_by_kind"] = {name: int((kinds == code).sum()) for code, name in mini_amd.LpaProblem.STEP_KINDS.items()}
    lp.set_timing(True)
    lp.run(**run_args)
    ms = lp.phase_ms()
    out["fused_phase_ms"] = {k: round(v, 4) for k, v in ms.items()}
    out["ms_per_iteration"] = round((ms["evaluate"] + ms["long_rows"] + ms["apply"]) / iters, 4)
    dense = int((kinds == 2).sum())
    out["dense_iterations"] = dense
    lp.set_timing(False)
    labels = lp.labels()
    mod_ms = [timed(lp.modularity)[0] for _ in range(args.rounds)]
    q = lp.modularity()
    out.update({"modularity": round(q[0], 6), "modularity_ms": spread(mod_ms)})
    lp.close()

    fr = mini_amd.Frontier(ctx, n).fill_iota(n)
    vals = torch.rand(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(args.scale))
    red = torch.empty(n, device="cuda")
    mini_amd.segreduce(g, fr, vals, 0.0, red, "f32_plus")
    out["segreduce_ms"] = spread([timed(mini_amd.segreduce, g, fr, vals, 0.0, red, "f32_plus")[0] for _ in range(args.rounds)])

    if args.operator:
        f, r, sto, lo = one_handle("enact")
        same = np.array_equal(lo.labels(), labels) and all(sto[k] == st[k] for k in STATS)
        lo.close()
        if not same:
            sys.exit("fused and operator path differ")
        out.update({"operator_first_ms": round(f, 4), "operator_repeat_ms": round(r, 4), "host_waits_operator": sto["host_waits"],
                    "repeat_speedup": round(r / out["fused_repeat_ms"]["median"], 2)})
    print(json.dumps(out), flush=True)
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
