#!/usr/bin/env python3
"""Bit-parallel multi-source BFS, fused path (mgx_msbfs_run), against one batched BFS of the same sources (mgx_bfs_run_many) and,
optionally, against the operator path (mgx_msbfs_enact).
usage: msbfs_bench.py SCALE [--graph rmat|uniform|grid2d] [--directed [--csc]] [--sources K] [--operator] [--depths]
                            [--edgefactor EF] [--rounds R]

The graph is symmetric (R-MAT with the swapped copies, edge factor 16; the uniform and grid generators' graphs as they are) and the
run is told so; with --directed the R-MAT pairs are kept as they are and the run is told symmetric = 0: with --csc the genuine CSC
is built first (not timed) and dense levels pull over it, without it every level pushes.  K sources of degree > 0 (default 64).
Prints one JSON line, HIP events on the context's stream, one warm-up handle, the median, minimum and maximum over R rounds (a
fresh handle each):
  * ms of the fused path's first run on a fresh handle (its allocations included) and of its repeat run, and the repeat run's
    ms per 64 sources;
  * the repeat run's phases (PUSH, PULL, LONG, FINALIZE launches) from one more run with the device's wall clock
    (mgx_msbfs_set_timing), its PUSH and PULL levels, launches and host waits, the rows per body;
  * mgx_bfs_run_many (push mode, on the hub-first layout bench.py runs on) over the same sources on the same graph in the same
    process: ms and ms per 64 sources;
  * one full-frontier neighbour-reduce call (mgx_segreduce_f32_plus) on the same graph: a PULL level gathers as many entries;
  * with --operator the operator path's first and repeat run (ONE round), checked against the fused path's results.
The switches MGX_MSBFS_* are read from the environment as every handle reads them."""
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
    ap.add_argument("--directed", action="store_true", help="R-MAT without the swapped copies, symmetric = 0")
    ap.add_argument("--csc", action="store_true", help="build the genuine CSC first (dense levels of a --directed run pull over it)")
    ap.add_argument("--sources", type=int, default=64)
    ap.add_argument("--operator", action="store_true", help="time the operator path as well (one round)")
    ap.add_argument("--depths", action="store_true", help="keep the depth matrix (int32[K][n])")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--edgefactor", type=int, default=16)
    args = ap.parse_args()
    if args.directed and args.graph != "rmat":
        sys.exit("--directed is for --graph rmat")
    if not torch.cuda.is_available():
        sys.exit("msbfs_bench.py needs a GPU")

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
    g.build_layout()                                  # (for mgx_bfs_run_many and the neighbour-reduce; mgx_msbfs_run ignores it)
    K = args.sources
    src = np.array(rmat.pick_sources(d["row_offsets"].cpu().numpy(), K, args.scale), dtype=np.int32)
    run_args = dict(sources=src, symmetric=not args.directed, depths=args.depths)

    def timed(fn, *a, **kw):
        x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        x.record(stream)
        st = fn(*a, **kw)
        y.record(stream)
        y.synchronize()
        return x.elapsed_time(y), st

    def one_handle(method):
        """(ms of the first run, ms of the repeat run, stats of the repeat run, the handle) of a fresh handle"""
        h = mini_amd.MsBfsProblem(g)
        first, _ = timed(getattr(h, method), **run_args)
        again, st = timed(getattr(h, method), **run_args)
        return first, again, st, h

    one_handle("run")[3].close()                      # warm-up: code objects, allocator
    firsts, repeats = [], []
    for i in range(args.rounds):
        f, r, st, mp = one_handle("run")
        firsts.append(f)
        repeats.append(r)
        if i < args.rounds - 1:
            mp.close()
    per64 = 64.0 / K
    out = {"tool": "msbfs_bench", "graph": args.graph, "scale": args.scale, "n": n, "m": m, "symmetric": int(not args.directed),
           "csc": int(args.csc), "sources": K, "depths": int(args.depths), "rounds_timed": args.rounds}
    out.update({"fused_first_ms": spread(firsts), "fused_repeat_ms": spread(repeats),
                "fused_ms_per_64_sources": spread([x * per64 for x in repeats])})
    out.update({k: st[k] for k in ("batches", "deepest", "reach", "push_levels", "pull_levels", "launches", "host_waits")})
    out["bins"] = mp.bins()
    mp.set_timing(True)
    mp.run(**run_args)
    out["fused_phase_ms"] = {k: round(v, 4) for k, v in mp.phase_ms().items()}
    mp.set_timing(False)
    reach, far, harm = mp.reach(), mp.farness(), mp.harmonic()
    mp.close()

    bfs = mini_amd.BfsProblem(g, int(src[0]))
    prepared = mini_amd.BfsProblem.prepare_many(src)
    bfs.run_many(src, prepared=prepared)
    torch.cuda.synchronize()
    many = [timed(lambda: bfs.run_many(src, prepared=prepared))[0] for _ in range(args.rounds)]
    out.update({"bfs_run_many_ms": spread(many), "bfs_run_many_ms_per_64_sources": spread([x * per64 for x in many])})
    out["run_many_over_fused"] = round(statistics.median(many) / statistics.median(repeats), 2)

    fr = mini_amd.Frontier(ctx, n).fill_iota(n)
    vals = torch.rand(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(args.scale))
    red = torch.empty(n, device="cuda")
    mini_amd.segreduce(g, fr, vals, 0.0, red, "f32_plus")
    out["segreduce_ms"] = spread([timed(mini_amd.segreduce, g, fr, vals, 0.0, red, "f32_plus")[0] for _ in range(args.rounds)])

    if args.operator:
        f, r, sto, mo = one_handle("enact")
        same = np.array_equal(mo.reach(), reach) and np.array_equal(mo.farness(), far) and np.array_equal(mo.harmonic(), harm)
        mo.close()
        if not same:
            sys.exit("fused and operator path differ")
        out.update({"operator_first_ms": round(f, 4), "operator_repeat_ms": round(r, 4), "host_waits_operator": sto["host_waits"],
                    "operator_over_fused": round(r / out["fused_repeat_ms"]["median"], 2)})
    print(json.dumps(out), flush=True)
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
