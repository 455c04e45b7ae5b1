#!/usr/bin/env python3
"""The backward of the neighbour feature aggregation, fused path (mgx_aggbwd_run), beside the forward on the same graph in the same
process: mgx_agg_run over the out-rows, mgx_agg_run over the in-rows with a CSC (the same gather as the backward's, without t_pos),
and with --torch the backward of torch.sparse.mm on the same CSR.
usage: aggbwd_bench.py [SCALE] [--graph rmat|uniform|grid2d] [--feats F] [--op sum|mean|max|min] [--weighted]
                       [--block SEEDS:15,10,5] [--operator] [--torch] [--rounds N] [--edgefactor EF]

The graph is rmat.py's (R-MAT with the swapped copies, edge factor 16; the uniform and grid generators' graphs as they are), SCALE
defaults to 20; GY and X are random float32.  A repeat run only enqueues, so a run's time is the host's wall clock round the call
and a wait for the stream.  Prints one JSON line: one warm-up handle, then the median, minimum and maximum over N rounds (default
5) of
  * ms of the first run on a fresh handle (the transpose's and the plan's launches and waits, the allocations) and of the repeat run;
  * the repeat run's phases apart (transpose, winners or the mean's g, rows, items, fold), from runs with mgx_aggbwd_set_timing; for
    a block every run builds, so its transpose phase is the build;
  * the forward mgx_agg_run's repeat run with the same op, and (not for a block) the forward over rows="in" after build_csc();
  * with --operator the operator path's repeat run, its bits checked against the fused path's;
  * with --torch (sum, no block) the backward of torch.sparse.mm on the same CSR: (A x).backward(gy), another summation order."""
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
    ap.add_argument("--block", default="", help="SEEDS:FANOUTS, e.g. 1024:15,10,5")
    ap.add_argument("--operator", action="store_true", help="time the operator path as well")
    ap.add_argument("--torch", action="store_true", help="time the backward of torch.sparse.mm on the same CSR as well")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--edgefactor", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("aggbwd_bench.py needs a GPU")
    ctx = mini_amd.Context(0, torch.cuda.current_stream().cuda_stream)
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
    how = dict(op=args.op, weighted=args.weighted)
    sp = None
    if args.block:
        count, _, fo = args.block.partition(":")
        fanouts = [int(x) for x in (fo or "15,10,5").split(",") if x]
        seeds = np.random.default_rng(args.scale).choice(n, min(int(count), n), replace=False).astype(np.int32)
        sp = mini_amd.NeighborSampleProblem(g)
        st = sp.run(seeds, fanouts, seed=args.scale)
        x_rows, R, E = st["vertices"], st["rows"], st["edges"]
        how.update(block=sp)
    else:
        x_rows, R, E = n, n, m
    F = args.feats
    gen = torch.Generator(device="cuda").manual_seed(args.scale)
    x = torch.randn((x_rows, F), device="cuda", dtype=torch.float32, generator=gen)
    gy = torch.randn((max(R, 1), F), device="cuda", dtype=torch.float32, generator=gen)
    gx = torch.empty((max(x_rows, 1), F), device="cuda", dtype=torch.float32)
    y = torch.empty((max(R, 1), F), device="cuda", dtype=torch.float32)
    bwd_args = dict(gy=gy, x=x, out=gx, ldgy=F, ldx=F, ldgx=F, x_rows=x_rows, feats=F, **how)
    fwd_args = dict(x=x, out=y, ldx=F, ldy=F, x_rows=x_rows, feats=F, **how)

    def one_handle(cls, method, run_args, rounds=1):
        """(ms of the first run, ms of the repeat runs, stats of the last, the handle) of a fresh handle"""
        h = cls(g)
        first, _ = timed(getattr(h, method), **run_args)
        again = [timed(getattr(h, method), **run_args) for _ in range(rounds)]
        return first, [a[0] for a in again], again[-1][1], h

    one_handle(mini_amd.AggregateGradProblem, "run", bwd_args)[3].close()          # warm-up: code objects, allocator
    firsts, repeats = [], []
    for i in range(args.rounds):
        f, r, st, h = one_handle(mini_amd.AggregateGradProblem, "run", bwd_args)
        firsts.append(f)
        repeats += r
        if i < args.rounds - 1:
            h.close()
    t = statistics.median(repeats)
    out = {"tool": "aggbwd_bench", "graph": args.graph, "scale": args.scale, "n": n, "m": m, "rounds_timed": args.rounds, "block": args.block or None,
           "x_rows": x_rows, "fwd_rows": R, "op": args.op, "weighted": args.weighted}
    out.update(st)
    out.update({"backward_first_ms": spread(firsts), "backward_repeat_ms": spread(repeats), "bins": h.bins()})
    h.set_timing(True)
    phases = {k: [] for k in h.PHASES}
    for _ in range(args.rounds):
        h.run(**bwd_args)
        for k, v in h.phase_ms().items():
            phases[k].append(v)
    h.set_timing(False)
    out["backward_phase_ms"] = {k: spread(v) for k, v in phases.items()}
    fused_bits = gx[:x_rows].clone()
    h.close()

    # the comparison points: the forward on the same graph, in the same process
    one_handle(mini_amd.AggregateProblem, "run", fwd_args)[3].close()
    f, r, stf, hf = one_handle(mini_amd.AggregateProblem, "run", fwd_args, args.rounds)
    hf.close()
    out.update({"forward_repeat_ms": spread(r), "backward_over_forward": round(t / statistics.median(r), 2)})
    if not args.block:
        g.build_csc()
        f, r, stf, hf = one_handle(mini_amd.AggregateProblem, "run", dict(fwd_args, rows="in"), args.rounds)
        hf.close()
        out.update({"forward_in_rows_repeat_ms": spread(r), "backward_over_forward_in_rows": round(t / statistics.median(r), 2)})

    if args.operator:
        f, r, sto, op = one_handle(mini_amd.AggregateGradProblem, "enact", bwd_args, args.rounds)
        same = torch.equal(fused_bits.view(torch.int32), gx[:x_rows].view(torch.int32))
        op.close()
        if not same:
            sys.exit("fused and operator path differ")
        out.update({"operator_repeat_ms": spread(r), "operator_over_fused": round(statistics.median(r) / t, 2)})

    if args.torch and not args.block and args.op == "sum":
        vals = w if args.weighted else torch.ones(m, device="cuda", dtype=torch.float32)
        a = torch.sparse_csr_tensor(d["row_offsets"].to(torch.int64), d["col_indices"].to(torch.int64), vals, size=(n, n))
        xt = x.clone().requires_grad_(True)

        def torch_backward():
            xt.grad = None
            yt = torch.sparse.mm(a, xt)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            yt.backward(gy[:n])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        try:
            torch_backward()
            ts = [torch_backward() for _ in range(args.rounds)]
            out.update({"torch_sparse_mm_backward_ms": spread(ts), "torch_over_fused": round(statistics.median(ts) / t, 2),
                        "max_abs_diff_to_torch": float((xt.grad - fused_bits).abs().max())})
        except RuntimeError as e:                                # (a torch build without this backward: say so, keep the rest)
            out["torch_sparse_mm_backward_ms"] = "not available: " + str(e).splitlines()[0][:120]
    print(json.dumps(out), flush=True)
    if sp:
        sp.close()
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
