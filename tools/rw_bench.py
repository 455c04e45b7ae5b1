#!/usr/bin/env python3
"""Random walks and node2vec sampling, fused path (mgx_rw_run), optionally against the operator path (mgx_rw_enact).
usage: rw_bench.py SCALE [--graph rmat|uniform|grid2d] [--length L] [--walks R] [--weighted] [--p P --q Q] [--restart A]
                         [--no-paths] [--visits] [--operator] [--edgefactor EF] [--rounds N]

The graph is symmetric (R-MAT with the swapped copies, edge factor 16; the uniform and grid generators' graphs as they are); every
vertex is a start, R walks each (default 1), of L steps (default 80).  Prints one JSON line, HIP events on the context's stream,
one warm-up handle, the median, minimum and maximum over N rounds (default 5, a fresh handle each):
  * ms of the fused path's first run on a fresh handle (its allocations and its setup included) and of its repeat run;
  * the repeat run's setup and walk apart, from one more run with mgx_rw_set_timing, and M steps / s of the walk;
  * tries per step, fallbacks, dead ends, restarts, launches and host waits, the rows per body of the setup;
  * with --operator the operator path's first and repeat run on the same input in the same process (ONE round), checked against
    the fused path's ends and lengths;
  * one full-frontier neighbour-reduce call (mgx_segreduce_f32_plus) on the same graph for scale: it gathers every entry once.
The switches MGX_RW_* are read from the environment as every handle reads them (MGX_RW_TILE=1: every path slot stored on its own)."""
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
    ap.add_argument("--length", type=int, default=80)
    ap.add_argument("--walks", type=int, default=1)
    ap.add_argument("--weighted", action="store_true")
    ap.add_argument("--p", type=float, default=1.0)
    ap.add_argument("--q", type=float, default=1.0)
    ap.add_argument("--restart", type=float, default=0.0)
    ap.add_argument("--no-paths", action="store_true")
    ap.add_argument("--visits", action="store_true")
    ap.add_argument("--operator", action="store_true", help="time the operator path as well (one round)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--edgefactor", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rw_bench.py needs a GPU")

    stream = torch.cuda.current_stream()
    ctx = mini_amd.Context(0, stream.cuda_stream)
    if args.graph == "rmat":
        d = rmat.rmat_csr(ctx, args.scale, args.edgefactor, seed=args.scale, weighted=args.weighted)
    elif args.graph == "uniform":
        d = rmat.uniform_csr(ctx, args.scale, args.edgefactor)
    else:
        d = rmat.grid2d_csr(ctx, args.scale)
    n, m = d["n"], d["m"]
    weights = d.get("weights") if args.weighted else None
    g = mini_amd.Graph.from_device(ctx, n, m, d["row_offsets"], d["col_indices"], weights)
    run_args = dict(starts=None, length=args.length, walks_per_start=args.walks, seed=args.scale, weighted=args.weighted, p=args.p, q=args.q,
                    restart=args.restart, paths=not args.no_paths, visits=args.visits)

    def timed(fn, *a, **kw):
        x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        x.record(stream)
        st = fn(*a, **kw)
        y.record(stream)
        y.synchronize()
        return x.elapsed_time(y), st

    def one_handle(method):
        """(ms of the first run, ms of the repeat run, stats of the repeat run, the handle) of a fresh handle"""
        h = mini_amd.RandomWalkProblem(g)
        first, _ = timed(getattr(h, method), **run_args)
        again, st = timed(getattr(h, method), **run_args)
        return first, again, st, h

    one_handle("run")[3].close()                      # warm-up: code objects, allocator
    firsts, repeats = [], []
    for i in range(args.rounds):
        f, r, st, rp = one_handle("run")
        firsts.append(f)
        repeats.append(r)
        if i < args.rounds - 1:
            rp.close()
    out = {"tool": "rw_bench", "graph": args.graph, "scale": args.scale, "n": n, "m": m, "rounds_timed": args.rounds}
    out.update({k: run_args[k] for k in ("length", "walks_per_start", "weighted", "p", "q", "restart", "paths", "visits")})
    out.update({"fused_first_ms": spread(firsts), "fused_repeat_ms": spread(repeats)})
    out.update({k: st[k] for k in ("walkers", "steps", "dead_ends", "restarts", "tries", "fallbacks", "sorted_copy", "launches", "host_waits")})
    out["tries_per_step"] = round(st["tries"] / max(st["steps"] - st["restarts"], 1), 4)
    out["bins"] = rp.bins()
    rp.set_timing(True)
    walks = []
    for _ in range(args.rounds):
        rp.run(**run_args)
        walks.append(rp.phase_ms()["walk"])
    out["fused_walk_ms"] = spread(walks)
    out["fused_msteps_per_s"] = round(st["steps"] / statistics.median(walks) / 1e3, 1)
    rp.set_timing(False)
    fresh = mini_amd.RandomWalkProblem(g)
    fresh.set_timing(True)
    fresh.run(**run_args)
    out["fused_first_phase_ms"] = {k: round(v, 4) for k, v in fresh.phase_ms().items()}
    fresh.close()
    ends, lengths = rp.ends(), rp.lengths()
    rp.close()

    fr = mini_amd.Frontier(ctx, n).fill_iota(n)
    vals = torch.rand(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(args.scale))
    red = torch.empty(n, device="cuda")
    mini_amd.segreduce(g, fr, vals, 0.0, red, "f32_plus")
    out["segreduce_ms"] = spread([timed(mini_amd.segreduce, g, fr, vals, 0.0, red, "f32_plus")[0] for _ in range(args.rounds)])

    if args.operator:
        f, r, sto, ro = one_handle("enact")
        same = np.array_equal(ro.ends(), ends) and np.array_equal(ro.lengths(), lengths)
        ro.close()
        if not same:
            sys.exit("fused and operator path differ")
        out.update({"operator_first_ms": round(f, 4), "operator_repeat_ms": round(r, 4), "host_waits_operator": sto["host_waits"],
                    "operator_over_fused": round(r / out["fused_repeat_ms"]["median"], 2)})
    print(json.dumps(out), flush=True)
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
