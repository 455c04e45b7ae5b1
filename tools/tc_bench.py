#!/usr/bin/env python3
"""Triangle counting, fused path (mgx_tc_run) against the operator path (mgx_tc_enact).
usage: tc_bench.py SCALE [--graph rmat|uniform|grid2d] [--directed] [--operator] [--rounds K] [--edgefactor EF]
                         [--ab SHORT/WAVE/STAGE,SHORT/WAVE/STAGE,...]

Prints one JSON line: ms of the fused path's first run on a fresh handle (build of the oriented graph + count) and of its repeat
run (count only), HIP events on the context's stream, one warm-up handle, the median, minimum and maximum over K rounds (a fresh
handle each); with --operator the same two figures for the operator path; the triangles, wedges and the longest oriented row; and
a byte floor of the count phase: every DAG entry (a, b) streams row b once (4 B x sum over b of indeg(b) d+(b)), every row is
staged once (4 B x m_dag), and every vertex's count is cleared and added to (16 B x n).
--directed builds the R-MAT graph without the swapped copies and runs both paths with symmetric = 0.
--ab measures the repeat run under each setting of MGX_TC_SHORT_MAX / MGX_TC_WAVE_MAX / MGX_TC_STAGE (a handle reads them at its
first run), K interleaved rounds in this one process, and prints median / min / max per setting."""
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
    ap.add_argument("--directed", action="store_true", help="R-MAT without the swapped copies; both paths run with symmetric = 0")
    ap.add_argument("--operator", action="store_true", help="time the operator path as well")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--ab", default="", help="SHORT/WAVE/STAGE settings, comma-separated: the repeat run under each")
    args = ap.parse_args()
    if args.directed and args.graph != "rmat":
        sys.exit("--directed needs --graph rmat")
    if not torch.cuda.is_available():
        sys.exit("tc_bench.py needs a GPU")

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

    def one_handle(method):
        """(ms of the first run, ms of the repeat run, stats of the repeat run, tri) of a fresh handle"""
        tp = mini_amd.TcProblem(g)
        first, _ = timed(getattr(tp, method), symmetric)
        again, st = timed(getattr(tp, method), symmetric)
        tri = tp.triangles()
        tp.close()
        return first, again, st, tri

    out = {"tool": "tc_bench", "graph": args.graph, "scale": args.scale, "n": d["n"], "m": d["m"], "directed": args.directed,
           "rounds": args.rounds}
    if args.ab:
        settings = [tuple(int(x) for x in s.split("/")) for s in args.ab.split(",")]
        handles = []
        for short, wave, stage in settings:
            os.environ["MGX_TC_SHORT_MAX"], os.environ["MGX_TC_WAVE_MAX"], os.environ["MGX_TC_STAGE"] = str(short), str(wave), str(stage)
            tp = mini_amd.TcProblem(g)
            tp.run(symmetric)                       # builds, reads the switches; also the warm-up
            handles.append(tp)
        ms = [[] for _ in settings]
        for _ in range(args.rounds):
            for k, tp in enumerate(handles):
                t, st = timed(tp.run, symmetric)
                ms[k].append(t)
        out["ab_repeat_ms"] = {"%d/%d/%d" % s: spread(ms[k]) for k, s in enumerate(settings)}
        out["triangles"] = st["triangles"]
        for tp in handles:
            tp.close()
        print(json.dumps(out), flush=True)
        g.close()
        ctx.close()
        return

    one_handle("run")                               # warm-up: code objects, allocator
    firsts, repeats = [], []
    for _ in range(args.rounds):
        f, r, st, tri = one_handle("run")
        firsts.append(f)
        repeats.append(r)
    out.update({"fused_first_ms": spread(firsts), "fused_repeat_ms": spread(repeats), "triangles": st["triangles"],
                "edges": st["edges"], "wedges": st["wedges"], "max_row": st["max_row"], "rows_sorted": st["rows_sorted"],
                "host_waits_fused": st["host_waits"], "launches_repeat": st["launches"]})
    if args.operator:
        one_handle("enact")
        firsts, repeats = [], []
        for _ in range(args.rounds):
            f, r, sto, tri_o = one_handle("enact")
            firsts.append(f)
            repeats.append(r)
        if not np.array_equal(tri_o, tri) or sto["triangles"] != st["triangles"]:
            sys.exit("fused and operator path differ")
        out.update({"operator_first_ms": spread(firsts), "operator_repeat_ms": spread(repeats),
                    "host_waits_operator": sto["host_waits"],
                    "repeat_speedup": round(statistics.median(repeats) / out["fused_repeat_ms"]["median"], 2)})
    tp = mini_amd.TcProblem(g)
    tp.run(symmetric)
    dro, dci = tp.dag()
    tp.close()
    dplus = np.diff(dro.astype(np.int64))
    indeg = np.bincount(dci, minlength=d["n"]).astype(np.int64)
    streamed = int((indeg * dplus).sum())
    floor = 4 * streamed + 4 * int(len(dci)) + 16 * d["n"]
    out.update({"entries_streamed": streamed, "byte_floor": floor,
                "byte_floor_note": "4 B x sum indeg(b) d+(b) streamed, 4 B x m_dag staged, 16 B a vertex of counts",
                "floor_GBps_at_fused_repeat": round(floor / (out["fused_repeat_ms"]["median"] * 1e-3) / 1e9, 2)})
    print(json.dumps(out), flush=True)
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
