#!/usr/bin/env python3
"""Minimum spanning forest: the fused path's first run (setup + rounds) and repeat run (rounds only), the operator path, and
beside them, on the same graph, what a forest cannot be cheaper than: its components (mgx_cc_run) and one segmented sort of the
incident entries.
usage: mst_bench.py SCALE [--graph rmat|uniform|grid2d|star] [--directed --csc] [--operator] [--repeats K] [--edgefactor EF]

Prints one JSON line: ms of each (HIP events on the context's stream; the first run once, the others the median of K after a
warm-up), the run's stats and info.  rmat carries the generator's % 64 weights, uniform and grid2d none (all 1.0: every choice
is a tie); star is vertex 0 joined to 2^SCALE leaves, random weights 0 .. 63: one row for the wave path and its windows.  --directed generates unsymmetrised R-MAT entries and needs --csc (the library builds the CSC; symmetric = 0).  The
operator path is run only with --operator (it rescans every entry every round).  The sort yardstick is the library's
mgx_segmented_sort_i32 within the CSR's rows, int32 views of the weights as keys and the neighbours as values: as many bytes an
entry as the setup sorts as one 64-bit key, but not the setup's sort -- another instantiation of the kernels, self-loops included,
the in-entries of a --directed run not, and the library sort's own host wait, which the setup avoids, in the time.  MGX_MST_LONG_MIN and MGX_MST_SEG are read by the library per run."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mini_amd  # noqa: E402
from mini_amd import rmat  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scale", type=int)
    ap.add_argument("--graph", choices=["rmat", "uniform", "grid2d", "star"], default="rmat")
    ap.add_argument("--directed", action="store_true")
    ap.add_argument("--csc", action="store_true")
    ap.add_argument("--operator", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--edgefactor", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mst_bench.py needs a GPU")
    if args.directed and (args.graph != "rmat" or not args.csc):
        sys.exit("--directed is for --graph rmat and needs --csc")

    stream = torch.cuda.current_stream()
    ctx = mini_amd.Context(0, stream.cuda_stream)
    if args.graph == "rmat":
        d = rmat.rmat_csr(ctx, args.scale, args.edgefactor, seed=args.scale, weighted=True, undirected=not args.directed)
    elif args.graph == "uniform":
        d = rmat.uniform_csr(ctx, args.scale, args.edgefactor)
    elif args.graph == "star":
        leaves = 1 << args.scale
        dev = torch.device("cuda", 0)
        tail = torch.arange(leaves, 2 * leaves + 1, dtype=torch.int32, device=dev)
        wl = torch.randint(0, 64, (leaves,), generator=torch.Generator(device=dev).manual_seed(args.scale), device=dev).float()
        d = {"n": leaves + 1, "m": 2 * leaves,
             "row_offsets": torch.cat([torch.zeros(1, dtype=torch.int32, device=dev), tail]),
             "col_indices": torch.cat([torch.arange(1, leaves + 1, dtype=torch.int32, device=dev),
                                       torch.zeros(leaves, dtype=torch.int32, device=dev)]),
             "weights": torch.cat([wl, wl])}
    else:
        d = rmat.grid2d_csr(ctx, args.scale)
    weights = d.get("weights")
    g = mini_amd.Graph.from_device(ctx, d["n"], d["m"], d["row_offsets"], d["col_indices"], weights)
    if args.csc:
        g.build_csc()
    symmetric = not args.directed

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        out = fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), out

    def median(fn):
        runs = [timed(fn) for _ in range(args.repeats)]
        return statistics.median(r[0] for r in runs), runs[-1][1]

    warm = mini_amd.MstProblem(g)                       # code objects, the context's scratch arena
    warm.run(symmetric)
    warm.close()
    torch.cuda.synchronize()
    mp = mini_amd.MstProblem(g)
    first_ms, first = timed(lambda: mp.run(symmetric))
    info_first = mp.info()
    repeat_ms, st = median(lambda: mp.run(symmetric))
    info = mp.info()
    total = mp.weight()
    out = {
        "tool": "mst_bench", "graph": args.graph, "scale": args.scale, "n": d["n"], "m": d["m"], "directed": args.directed,
        "csc": args.csc, "repeats": args.repeats,
        "fused_first_ms": round(first_ms, 4), "fused_repeat_ms": round(repeat_ms, 4), "setup_ms": round(first_ms - repeat_ms, 4),
        "stats": st, "info": info, "setup_reused_first": info_first["setup_reused"], "total_weight": total,
        "cursor_bound": st["entries"] + st["rounds"] * d["n"],
    }
    if args.operator:
        mp.enact(symmetric)
        op_ms, so = median(lambda: mp.enact(symmetric))
        same = ("edges", "components", "largest", "largest_label", "rounds", "entries")
        if {k: so[k] for k in same} != {k: st[k] for k in same} or mp.weight() != total:
            sys.exit("fused and operator path differ: %r / %r" % (st, so))
        out.update({"operator_ms": round(op_ms, 4), "operator_host_waits": so["host_waits"], "speedup_repeat": round(op_ms / repeat_ms, 2),
                    "speedup_first": round(op_ms / first_ms, 2)})
    mp.close()
    cp = mini_amd.CcProblem(g)
    cp.run(symmetric)
    cc_ms, cs = median(lambda: cp.run(symmetric))
    cp.close()
    out["cc_run_ms"] = round(cc_ms, 4)
    if cs["components"] != st["components"]:
        sys.exit("components differ: %r / %r" % (cs, st))
    if d["m"] > 0:
        heads = d["row_offsets"][1:-1].contiguous()
        src_k = (weights.view(torch.int32) if weights is not None else torch.ones(d["m"], dtype=torch.int32, device=heads.device))
        src_v = d["col_indices"]

        def sort_once():
            mini_amd.segmented_sort(ctx, keys, heads, vals)
        sorts = []
        for _ in range(args.repeats + 1):
            keys, vals = src_k.clone(), src_v.clone()
            torch.cuda.synchronize()
            sorts.append(timed(sort_once)[0])
        out["segmented_sort_ms"] = round(statistics.median(sorts[1:]), 4)
    print(json.dumps(out), flush=True)
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
