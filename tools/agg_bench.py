#!/usr/bin/env python3
"""Neighbour feature aggregation, fused path (mgx_agg_run) against the operator path (mgx_agg_enact), one neighbour-reduce call and
torch.sparse.mm in the same process.
usage: agg_bench.py [SCALE] [--graph rmat|uniform|grid2d] [--feats F] [--op sum|mean|max|min] [--weighted] [--in-rows]
                    [--block SEEDS:15,10,5] [--operator] [--torch] [--sweep] [--rounds N] [--edgefactor EF]

The graph is symmetric (R-MAT with the swapped copies, edge factor 16; the uniform and grid generators' graphs as they are), SCALE
defaults to 20; X is random float32, n x F (a block's: vertices x F).  A run only enqueues, so a run's time is the host's wall
clock round the call and a wait for the stream.  Prints one JSON line: one warm-up handle, then the median, minimum and maximum
over N rounds (default 5) of
  * ms of the first run on a fresh handle (the plan's two launches and wait, the allocations) and of the repeat run;
  * the repeat run's rows, items and fold launches apart, from runs with mgx_agg_set_timing (device events);
  * gathered GB/s = (E F 4 + R F 4 + E 4 [+ E 4 weights]) / t, beside the 8 TB/s roof and the per-residency gather rates of whole
    rows into registers or LDS that the X array's size selects (L2 < 4 MiB per XCD, Infinity Cache < 256 MiB, else HBM);
  * with --operator the operator path's repeat run, its bits checked against the fused path's;
  * one neighbour-reduce call (f32 plus over the full frontier) on the same graph: the F = 1 cousin;
  * with --torch torch.sparse.mm on the same CSR (another summation order: compare times only);
  * with --sweep the repeat run under MGX_AGG_SEG = 64, 256 and 1024 (a fresh handle each: the switch is read per handle).
--block SEEDS:FANOUTS aggregates over all rows of one sampling run instead of the graph's rows."""
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

ROOF_TBS = 8.0
# whole rows gathered by index, chip-wide TB/s by where the table sits (measured with 1 152-byte rows)
GATHER_TBS = (("l2", 4 << 20, "16.8-18.8"), ("infinity_cache", 256 << 20, "7.4-8.6"), ("hbm", None, "5.5-6.1"))


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def timed(fn, *a, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = fn(*a, **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scale", type=int, nargs="?", default=20)
    ap.add_argument("--graph", choices=["rmat", "uniform", "grid2d"], default="rmat")
    ap.add_argument("--feats", type=int, default=64)
    ap.add_argument("--op", choices=list(mini_amd.AggregateProblem.OPS), default="sum")
    ap.add_argument("--weighted", action="store_true")
    ap.add_argument("--in-rows", action="store_true", help="the in-entries (builds the CSC)")
    ap.add_argument("--block", default="", help="SEEDS:FANOUTS, e.g. 1024:15,10,5")
    ap.add_argument("--operator", action="store_true", help="time the operator path as well")
    ap.add_argument("--torch", action="store_true", help="time torch.sparse.mm on the same CSR as well")
    ap.add_argument("--sweep", action="store_true", help="the repeat run under MGX_AGG_SEG = 64, 256, 1024")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--edgefactor", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("agg_bench.py needs a GPU")
    stream = torch.cuda.current_stream()
    ctx = mini_amd.Context(0, stream.cuda_stream)
    if args.graph == "rmat":
        d = rmat.rmat_csr(ctx, args.scale, args.edgefactor, seed=args.scale, weighted=args.weighted)
    elif args.graph == "uniform":
        d = rmat.uniform_csr(ctx, args.scale, args.edgefactor)
    else:
        d = rmat.grid2d_csr(ctx, args.scale)
    n, m = d["n"], d["m"]
    w = d.get("weights")
    if args.weighted and w is None:
        w = torch.rand(m, device="cuda", dtype=torch.float32) + 0.5
    g = mini_amd.Graph.from_device(ctx, n, m, d["row_offsets"], d["col_indices"], w if args.weighted else None)
    if args.in_rows:
        g.build_csc()
    how = dict(op=args.op, weighted=args.weighted, rows="in" if args.in_rows else "out")
    sp = None
    if args.block:
        count, _, fo = args.block.partition(":")
        fanouts = [int(x) for x in (fo or "15,10,5").split(",") if x]
        seeds = np.random.default_rng(args.scale).choice(n, min(int(count), n), replace=False).astype(np.int32)
        sp = mini_amd.NeighborSampleProblem(g)
        st = sp.run(seeds, fanouts, seed=args.scale)
        x_rows, R, E = st["vertices"], st["rows"], st["edges"]
        how.update(block=sp, rows="out")
    else:
        x_rows, R, E = n, n, m
    F = args.feats
    gen = torch.Generator(device="cuda").manual_seed(args.scale)
    x = torch.randn((x_rows, F), device="cuda", dtype=torch.float32, generator=gen)
    y = torch.empty((max(R, 1), F), device="cuda", dtype=torch.float32)
    run_args = dict(x=x, out=y, ldx=F, ldy=F, x_rows=x_rows, feats=F, **how)

    def one_handle(method, rounds=1):
        """(ms of the first run, ms of the repeat runs, stats of the last, the handle) of a fresh handle"""
        h = mini_amd.AggregateProblem(g)
        first, _ = timed(getattr(h, method), **run_args)
        again = [timed(getattr(h, method), **run_args) for _ in range(rounds)]
        return first, [a[0] for a in again], again[-1][1], h

    one_handle("run")[3].close()                      # warm-up: code objects, allocator
    firsts, repeats = [], []
    for i in range(args.rounds):
        f, r, st, h = one_handle("run")
        firsts.append(f)
        repeats += r
        if i < args.rounds - 1:
            h.close()
    bytes_moved = E * F * 4 + R * F * 4 + E * 4 + (E * 4 if args.weighted else 0)
    t = statistics.median(repeats)
    table = x_rows * F * 4
    where = next(name for name, cap, _ in GATHER_TBS if cap is None or table <= cap)
    out = {"tool": "agg_bench", "graph": args.graph, "scale": args.scale, "n": n, "m": m, "rounds_timed": args.rounds, "block": args.block or None,
           "x_rows": x_rows, "x_mbytes": round(table / 1e6, 1)}
    out.update({k: v for k, v in how.items() if k != "block"})
    out.update(st)
    out.update({"fused_first_ms": spread(firsts), "fused_repeat_ms": spread(repeats), "bytes": bytes_moved,
                "fused_gbytes_per_s": round(bytes_moved / t / 1e6, 1), "roof_tbytes_per_s": ROOF_TBS,
                "fraction_of_roof": round(bytes_moved / t / 1e6 / (ROOF_TBS * 1e3), 3),
                "x_resides_in": where, "guide_gather_tbytes_per_s": dict((name, rate) for name, _, rate in GATHER_TBS)})
    out["bins"] = h.bins()
    h.set_timing(True)
    phases = {k: [] for k in h.PHASES}
    for _ in range(args.rounds):
        h.run(**run_args)
        for k, v in h.phase_ms().items():
            phases[k].append(v)
    h.set_timing(False)
    out["fused_phase_ms"] = {k: spread(v) for k, v in phases.items()}
    fused_bits = y[:R].clone()
    h.close()

    if args.operator:
        f, r, sto, op = one_handle("enact", args.rounds)
        same = torch.equal(fused_bits.view(torch.int32), y[:R].view(torch.int32))
        op.close()
        if not same:
            sys.exit("fused and operator path differ")
        out.update({"operator_repeat_ms": spread(r), "operator_over_fused": round(statistics.median(r) / t, 2)})

    if not args.block:
        # the F = 1 cousin: one neighbour-reduce (f32 plus) over the full frontier
        fr = mini_amd.Frontier(ctx, n).fill_iota(n)
        val = torch.rand(n, device="cuda", dtype=torch.float32)
        red = torch.empty(n, device="cuda", dtype=torch.float32)
        mini_amd.segreduce(g, fr, val, 0.0, red)
        out["neighbour_reduce_ms"] = spread([timed(mini_amd.segreduce, g, fr, val, 0.0, red)[0] for _ in range(args.rounds)])
        fr.close()

    if args.torch and not args.block:
        ro, ci = (d["row_offsets"], d["col_indices"])
        if args.in_rows:
            co, ri, rv = g.csc_arrays()
            ro, ci = torch.from_numpy(co).cuda(), torch.from_numpy(ri).cuda()
            vals = torch.from_numpy(rv).cuda() if args.weighted else torch.ones(m, device="cuda")
        else:
            vals = w if args.weighted else torch.ones(m, device="cuda", dtype=torch.float32)
        a = torch.sparse_csr_tensor(ro.to(torch.int64), ci.to(torch.int64), vals, size=(n, n))
        ref = torch.sparse.mm(a, x)
        out["torch_sparse_mm_ms"] = spread([timed(torch.sparse.mm, a, x)[0] for _ in range(args.rounds)])
        out["torch_over_fused"] = round(out["torch_sparse_mm_ms"]["median"] / t, 2)
        if args.op == "sum":
            out["max_abs_diff_to_torch"] = float((ref - fused_bits).abs().max())

    if args.sweep:
        sweep = {}
        for seg in (64, 256, 1024):
            os.environ["MGX_AGG_SEG"] = str(seg)
            f, r, sts, hs = one_handle("run", args.rounds)
            hs.close()
            sweep[str(seg)] = dict(spread(r), launches=sts["launches"])
        os.environ.pop("MGX_AGG_SEG", None)
        out["seg_sweep_ms"] = sweep
    print(json.dumps(out), flush=True)
    if sp:
        sp.close()
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
