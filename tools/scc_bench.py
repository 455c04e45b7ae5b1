#!/usr/bin/env python3
"""Strongly connected components, fused path (mgx_scc_run), optionally against the operator path (mgx_scc_enact).
usage: scc_bench.py SCALE [--graph rmat|uniform|grid2d] [--operator] [--rounds K] [--edgefactor EF]

The graph is directed: R-MAT without the swapped copies (edge factor 16), or the uniform / grid generators' graphs as they are; the
genuine CSC is built on the device first and is not timed.  Prints one JSON line, HIP events on the context's stream, one warm-up
handle, the median, minimum and maximum over K rounds (a fresh handle each):
  * ms of the fused path's first run on a fresh handle (its allocations included) and of its repeat run;
  * the repeat run's phases (degree init, trims, pivot phase, rounds) from one more run with the device's wall clock
    (mgx_scc_set_timing), and its launches and host waits;
  * mgx_cc_run's repeat run with the CSC on the same graph: the weakly connected components, the one other labelling of it;
  * the stats;
  * with --operator the operator path's first and repeat run (ONE round: it waits once per operator call), and repeat / repeat."""
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

STATS = ("components", "largest", "largest_label", "trimmed", "pivot_size", "rounds")


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scale", type=int)
    ap.add_argument("--graph", choices=["rmat", "uniform", "grid2d"], default="rmat")
    ap.add_argument("--operator", action="store_true", help="time the operator path as well (one round)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--edgefactor", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scc_bench.py needs a GPU")

    stream = torch.cuda.current_stream()
    ctx = mini_amd.Context(0, stream.cuda_stream)
    if args.graph == "rmat":
        d = rmat.rmat_csr(ctx, args.scale, args.edgefactor, seed=args.scale, undirected=False)
    elif args.graph == "uniform":
        d = rmat.uniform_csr(ctx, args.scale, args.edgefactor)
    else:
        d = rmat.grid2d_csr(ctx, args.scale)
    g = mini_amd.Graph.from_device(ctx, d["n"], d["m"], d["row_offsets"], d["col_indices"])
    g.build_csc()

    def timed(fn, *a):
        x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        x.record(stream)
        st = fn(*a)
        y.record(stream)
        y.synchronize()
        return x.elapsed_time(y), st

    def one_handle(cls, method, *a):
        """(ms of the first run, ms of the repeat run, stats of the repeat run, the handle) of a fresh handle"""
        h = cls(g)
        first, _ = timed(getattr(h, method), *a)
        again, st = timed(getattr(h, method), *a)
        return first, again, st, h

    def rounds_of(cls, method, rounds, *a):
        one_handle(cls, method, *a)[3].close()          # warm-up: code objects, allocator
        firsts, repeats = [], []
        for i in range(rounds):
            f, r, st, h = one_handle(cls, method, *a)
            firsts.append(f)
            repeats.append(r)
            if i < rounds - 1:
                h.close()
        return firsts, repeats, st, h

    out = {"tool": "scc_bench", "graph": args.graph, "scale": args.scale, "n": d["n"], "m": d["m"], "rounds_timed": args.rounds}
    firsts, repeats, st, sp = rounds_of(mini_amd.SccProblem, "run", args.rounds)
    out.update({"fused_first_ms": spread(firsts), "fused_repeat_ms": spread(repeats)})
    out.update({k: st[k] for k in STATS})
    out.update({"launches_repeat": st["launches"], "host_waits_repeat": st["host_waits"]})
    kinds = sp.step_kinds()
    out["launches_by_kind"] = {name: int((kinds == code).sum()) for code, name in mini_amd.SccProblem.STEP_KINDS.items()}
    sp.set_timing(True)
    sp.run()
    out["fused_phase_ms"] = {k: round(v, 4) for k, v in sp.phase_ms().items()}
    sp.set_timing(False)
    labels = sp.labels()
    sp.close()
    _, cc_repeats, cst, cp = rounds_of(mini_amd.CcProblem, "run", args.rounds, False)
    cp.close()
    out["cc_repeat_ms"] = spread(cc_repeats)
    out["cc_components"] = cst["components"]
    if args.operator:
        f, r, sto, so = one_handle(mini_amd.SccProblem, "enact")
        same = np.array_equal(so.labels(), labels) and all(sto[k] == st[k] for k in STATS)
        so.close()
        if not same:
            sys.exit("fused and operator path differ")
        out.update({"operator_first_ms": round(f, 4), "operator_repeat_ms": round(r, 4), "host_waits_operator": sto["host_waits"],
                    "repeat_speedup": round(r / out["fused_repeat_ms"]["median"], 2)})
    print(json.dumps(out), flush=True)
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
