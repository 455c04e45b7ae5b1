#!/usr/bin/env python3
"""Fan-out neighbour sampling, fused path (mgx_nsample_run) against the operator path (mgx_nsample_enact) in the same process.
usage: nsample_bench.py SCALE [--graph rmat|uniform|grid2d] [--seeds S] [--fanouts 15,10,5] [--replace] [--operator]
                              [--edgefactor EF] [--rounds N] [--hubs ROWS]

The graph is symmetric (R-MAT with the swapped copies, edge factor 16; the uniform and grid generators' graphs as they are); the
batch is S distinct random seeds (default 1024).  Prints one JSON line; a run ends with its own host wait, so a batch's time is
the host's wall clock round the call.  One warm-up handle, then the median, minimum and maximum over N rounds (default 5):
  * ms of the fused path's first run on a fresh handle (its allocations included) and of its repeat run, sampled entries / s;
  * the repeat run's sampling and deduplication apart, from runs with mgx_nsample_set_timing (device events);
  * the floor: launches x 2.3 us (a launch chain's measured idle launch) + one host wait, measured here as an empty stream's
    synchronize behind one 8-byte copy;
  * with --operator the operator path's first and repeat run on the same batch, checked against the fused path's arrays;
  * one mgx_rw_run of length H from the same seeds for scale.
--hubs ROWS ignores SCALE and --graph: ROWS seed rows of 100 000 entries against ROWS seed rows of 100 at the first fan-out, the
two medians and their ratio (about 1 when a row's cost does not depend on its degree).
The switches MGX_NSAMPLE_* are read from the environment as every handle reads them."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mini_amd  # noqa: E402
from mini_amd import rmat  # noqa: E402

IDLE_LAUNCH_US = 2.3


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def timed(fn, *a, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = fn(*a, **kw)
    return (time.perf_counter() - t0) * 1e3, st


def fan_graph(ctx, rows, degree, pool=1 << 20):
    """`rows` vertices with `degree` random entries each into a pool of further vertices without entries"""
    gen = torch.Generator(device="cuda").manual_seed(degree)
    n, m = rows + pool, rows * degree
    ro = torch.cat([torch.arange(rows + 1, device="cuda", dtype=torch.int64) * degree, torch.full((pool,), m, device="cuda", dtype=torch.int64)])
    ci = torch.randint(rows, n, (m,), device="cuda", generator=gen, dtype=torch.int32)
    ro = ro.to(torch.int32)
    return mini_amd.Graph.from_device(ctx, n, m, ro, ci, None), (ro, ci)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scale", type=int)
    ap.add_argument("--graph", choices=["rmat", "uniform", "grid2d"], default="rmat")
    ap.add_argument("--seeds", type=int, default=1024)
    ap.add_argument("--fanouts", default="15,10,5")
    ap.add_argument("--replace", action="store_true")
    ap.add_argument("--operator", action="store_true", help="time the operator path as well")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--hubs", type=int, default=0, help="ROWS seed rows of 100 000 entries against ROWS of 100")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("nsample_bench.py needs a GPU")
    fanouts = [int(x) for x in args.fanouts.split(",") if x]
    stream = torch.cuda.current_stream()
    ctx = mini_amd.Context(0, stream.cuda_stream)

    if args.hubs:
        out = {"tool": "nsample_bench", "hubs": args.hubs, "fanout": fanouts[0], "replace": args.replace, "rounds_timed": args.rounds}
        seeds = np.arange(args.hubs)
        for name, degree in (("degree_100000", 100000), ("degree_100", 100)):
            g, keep = fan_graph(ctx, args.hubs, degree)
            sp = mini_amd.NeighborSampleProblem(g)
            sp.run(seeds, fanouts[:1], args.replace, seed=1)
            ms = [timed(sp.run, seeds, fanouts[:1], args.replace, seed=1) for _ in range(args.rounds)]
            out[name + "_ms"] = spread([x[0] for x in ms])
            out[name + "_edges"] = ms[0][1]["edges"]
            sp.set_timing(True)
            ph = []
            for _ in range(args.rounds):
                sp.run(seeds, fanouts[:1], args.replace, seed=1)
                ph.append(sp.phase_ms()["sample"])
            out[name + "_sample_ms"] = spread(ph)
            sp.close()
            g.close()
            del keep
        out["hub_over_flat"] = round(out["degree_100000_ms"]["median"] / out["degree_100_ms"]["median"], 3)
        out["hub_over_flat_sample"] = round(out["degree_100000_sample_ms"]["median"] / out["degree_100_sample_ms"]["median"], 3)
        print(json.dumps(out), flush=True)
        ctx.close()
        return

    if args.graph == "rmat":
        d = rmat.rmat_csr(ctx, args.scale, args.edgefactor, seed=args.scale, weighted=False)
    elif args.graph == "uniform":
        d = rmat.uniform_csr(ctx, args.scale, args.edgefactor)
    else:
        d = rmat.grid2d_csr(ctx, args.scale)
    n, m = d["n"], d["m"]
    g = mini_amd.Graph.from_device(ctx, n, m, d["row_offsets"], d["col_indices"], None)
    seeds = np.random.default_rng(args.scale).choice(n, min(args.seeds, n), replace=False).astype(np.int32)
    run_args = dict(seeds=seeds, fanouts=fanouts, replace=args.replace, seed=args.scale)

    def one_handle(method):
        """(ms of the first run, ms of the repeat run, stats of the repeat run, the handle) of a fresh handle"""
        h = mini_amd.NeighborSampleProblem(g)
        first, _ = timed(getattr(h, method), **run_args)
        again, st = timed(getattr(h, method), **run_args)
        return first, again, st, h

    one_handle("run")[3].close()                      # warm-up: code objects, allocator
    firsts, repeats = [], []
    for i in range(args.rounds):
        f, r, st, sp = one_handle("run")
        firsts.append(f)
        repeats.append(r)
        if i < args.rounds - 1:
            sp.close()
    out = {"tool": "nsample_bench", "graph": args.graph, "scale": args.scale, "n": n, "m": m, "rounds_timed": args.rounds,
           "seeds": len(seeds), "fanouts": fanouts, "replace": args.replace}
    out.update({"fused_first_ms": spread(firsts), "fused_repeat_ms": spread(repeats)})
    out.update({k: st[k] for k in mini_amd.NeighborSampleProblem.KEYS[1:]})
    out["fused_mentries_per_s"] = round(st["edges"] / statistics.median(repeats) / 1e3, 2)
    sp.set_timing(True)
    sample, dedup = [], []
    for _ in range(args.rounds):
        sp.run(**run_args)
        ms = sp.phase_ms()
        sample.append(ms["sample"])
        dedup.append(ms["dedup"])
    sp.set_timing(False)
    out.update({"fused_sample_ms": spread(sample), "fused_dedup_ms": spread(dedup)})
    word = torch.zeros(1, dtype=torch.int64, device="cuda")
    host = torch.zeros(1, dtype=torch.int64).pin_memory()
    waits = []
    for _ in range(args.rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host.copy_(word, non_blocking=True)
        stream.synchronize()
        waits.append((time.perf_counter() - t0) * 1e3)
    out["host_wait_ms"] = spread(waits[1:])
    out["floor_ms"] = round(st["launches"] * IDLE_LAUNCH_US / 1e3 + st["host_waits"] * statistics.median(waits[1:]), 4)
    arrays = [getattr(sp, k)() for k in ("vertices", "hop_offsets", "row_offsets", "cols", "entry_pos", "seed_local")]
    sp.close()

    rw = mini_amd.RandomWalkProblem(g)
    rw.run(seeds, length=len(fanouts), seed=args.scale)
    out["rw_run_ms"] = spread([timed(rw.run, seeds, length=len(fanouts), seed=args.scale)[0] for _ in range(args.rounds)])
    rw.close()

    if args.operator:
        one_handle("enact")[3].close()
        of, orr = [], []
        for i in range(args.rounds):
            f, r, sto, op = one_handle("enact")
            of.append(f)
            orr.append(r)
            if i < args.rounds - 1:
                op.close()
        same = all(np.array_equal(getattr(op, k)(), a) for k, a in zip(("vertices", "hop_offsets", "row_offsets", "cols", "entry_pos", "seed_local"), arrays))
        op.close()
        if not same:
            sys.exit("fused and operator path differ")
        out.update({"operator_first_ms": spread(of), "operator_repeat_ms": spread(orr), "host_waits_operator": sto["host_waits"],
                    "operator_calls": sto["launches"], "operator_over_fused": round(statistics.median(orr) / out["fused_repeat_ms"]["median"], 2)})
    print(json.dumps(out), flush=True)
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
