#!/usr/bin/env python3
"""Louvain community detection, fused path (mgx_louvain_run), beside three yardsticks on the same graph.
usage: louvain_bench.py SCALE [--graph rmat|uniform|grid2d] [--directed --csc] [--operator] [--rounds K] [--edgefactor EF]
                              [--max-iter N] [--max-levels L] [--tol T]

The graph is symmetric (R-MAT with the swapped copies, edge factor 16; the uniform and grid generators' graphs as they are) and the
run is told so; with --directed the R-MAT pairs are kept as they are, the run counts every entry at both of its ends
(symmetric = 0) and needs --csc: the genuine CSC, built on the device first and not timed.  Prints one JSON line, HIP events on
the context's stream, one warm-up handle, the median, minimum and maximum over K rounds (a fresh handle each):
  * ms of the fused path's first run on a fresh handle (its allocations included) and of its repeat run;
  * per level: vertices, entries, iterations, accepted iterations, communities and Q after it;
  * the repeat run's phases (setup, evaluations, long rows, applies, Qnum launches on the device's wall clock, aggregation on the
    host's) from one more run (mgx_louvain_set_timing), the long rows' share of level 0 ... of the whole run, ms per iteration,
    launches, host waits, the vertices per body and the long rows' items;
  * communities and Q of the result;
  * the yardsticks: LpaProblem's lazy run (its repeat ms and Q), one mgx_modularity call, one full-frontier neighbour-reduce call
    (mgx_segreduce_f32_plus: an EVAL and a QNUM launch each read the same entries once);
  * with --operator the operator path's first and repeat run (ONE round), checked against the fused labels, and repeat / repeat."""
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
    ap.add_argument("--directed", action="store_true", help="R-MAT without the swapped copies, symmetric = 0 (needs --csc)")
    ap.add_argument("--csc", action="store_true", help="build the genuine CSC first")
    ap.add_argument("--operator", action="store_true", help="time the operator path as well (one round)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--max-levels", type=int, default=32)
    ap.add_argument("--tol", type=float, default=0.0)
    args = ap.parse_args()
    if args.directed and (args.graph != "rmat" or not args.csc):
        sys.exit("--directed is for --graph rmat and needs --csc")
    if not torch.cuda.is_available():
        sys.exit("louvain_bench.py needs a GPU")

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
    symmetric = not args.directed
    run_args = dict(symmetric=symmetric, max_iter=args.max_iter, max_levels=args.max_levels, tol=args.tol)

    def timed(fn, *a, **kw):
        x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        x.record(stream)
        st = fn(*a, **kw)
        y.record(stream)
        y.synchronize()
        return x.elapsed_time(y), st

    def one_handle(cls, **kw):
        """(ms of the first run, ms of the repeat run, stats of the repeat run, the handle) of a fresh handle"""
        h = cls(g)
        first, _ = timed(h.run, **kw)
        again, st = timed(h.run, **kw)
        return first, again, st, h

    one_handle(mini_amd.LouvainProblem, **run_args)[3].close()                      # warm-up: code objects, allocator
    firsts, repeats = [], []
    for i in range(args.rounds):
        f, r, st, lp = one_handle(mini_amd.LouvainProblem, **run_args)
        firsts.append(f)
        repeats.append(r)
        if i < args.rounds - 1:
            lp.close()
    out = {"tool": "louvain_bench", "graph": args.graph, "scale": args.scale, "n": n, "m": d["m"], "symmetric": int(symmetric),
           "rounds_timed": args.rounds, "fused_first_ms": spread(firsts), "fused_repeat_ms": spread(repeats)}
    out.update({k: st[k] for k in ("communities", "largest", "levels", "iterations", "launches", "host_waits")})
    w = st["w"]
    out["modularity"] = round(lp.modularity(), 6)
    out["levels_run"] = [dict(lv, q=round(lv["qnum"] / (w * w), 6) if w else 0.0) for lv in lp.levels()]
    out["bins"] = lp.bins()
    kinds = lp.step_kinds()
    out["launches_by_kind"] = {name: int((kinds == code).sum()) for code, name in mini_amd.LouvainProblem.STEP_KINDS.items()}
    lp.set_timing(True)
    lp.run(**run_args)
    ms = lp.phase_ms()
    out["fused_phase_ms"] = {k: round(v, 4) for k, v in ms.items()}
    device = sum(v for k, v in ms.items() if k != "aggregate")
    out["long_rows_share"] = round(ms["long_rows"] / device, 4) if device > 0 else 0.0
    out["ms_per_iteration"] = round((device - ms["setup"]) / max(st["iterations"], 1), 4)
    out["eval_plus_qnum_ms_per_iteration"] = round((ms["evaluate"] + ms["long_rows"] + ms["qnum"]) / max(st["iterations"], 1), 4)
    lp.run(symmetric=symmetric, max_iter=args.max_iter, max_levels=1, tol=args.tol)      # level 0 alone: its long rows' share
    ms0 = lp.phase_ms()
    device0 = sum(v for k, v in ms0.items() if k != "aggregate")
    out["level0_phase_ms"] = {k: round(v, 4) for k, v in ms0.items()}
    out["level0_long_rows_share"] = round(ms0["long_rows"] / device0, 4) if device0 > 0 else 0.0
    lp.set_timing(False)
    lp.run(**run_args)
    labels = lp.labels()
    if args.operator:
        f, _ = timed(lp.enact, **run_args)
        r, sto = timed(lp.enact, **run_args)
        if not (np.array_equal(lp.labels(), labels) and all(sto[k] == st[k] for k in ("communities", "levels", "s_in", "s_sq", "w"))):
            sys.exit("fused and operator path differ")
        out.update({"operator_first_ms": round(f, 4), "operator_repeat_ms": round(r, 4), "host_waits_operator": sto["host_waits"],
                    "repeat_speedup": round(r / out["fused_repeat_ms"]["median"], 2)})
        lp.run(**run_args)
    labels_ptr = lp.labels_device_ptr()
    out["modularity_call_ms"] = spread([timed(mini_amd.modularity, g, labels_ptr, symmetric)[0] for _ in range(args.rounds)])
    lp.close()

    lpa_args = dict(symmetric=symmetric, mode=mini_amd.LpaProblem.LAZY, max_iter=100)
    one_handle(mini_amd.LpaProblem, **lpa_args)[3].close()
    lpa_ms = []
    for i in range(args.rounds):
        f, r, lst, la = one_handle(mini_amd.LpaProblem, **lpa_args)
        lpa_ms.append(r)
        if i < args.rounds - 1:
            la.close()
    out.update({"lpa_repeat_ms": spread(lpa_ms), "lpa_modularity": round(la.modularity()[0], 6), "lpa_communities": lst["communities"],
                "lpa_iterations": lst["iterations"]})
    la.close()

    fr = mini_amd.Frontier(ctx, n).fill_iota(n)
    vals = torch.rand(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(args.scale))
    red = torch.empty(n, device="cuda")
    mini_amd.segreduce(g, fr, vals, 0.0, red, "f32_plus")
    out["segreduce_ms"] = spread([timed(mini_amd.segreduce, g, fr, vals, 0.0, red, "f32_plus")[0] for _ in range(args.rounds)])
    print(json.dumps(out), flush=True)
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
