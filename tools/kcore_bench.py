#!/usr/bin/env python3
"""k-core decomposition, fused path (mgx_kcore_run) against the operator path (mgx_kcore_enact: the reference's peeling loop on
filter / advance<has_output=false> / filter).
usage: kcore_bench.py [SCALE] [--graph rmat|uniform|grid2d] [--edgefactor EF] [--runs K] [--no-oracle]

Prints one JSON line: ms per run of both paths in one process (HIP events on the context's stream, one warm-up run each, the
median over K runs, the hub-first layout built as bench.py has it -- the k-core paths read the plain CSR), the stats of both,
and whether core numbers, working degrees and largest k-core of the two paths are equal.  Up to scale 20 both are also checked
against the oracle's restatement of kcore_enactor_t::enact."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scale", type=int, nargs="?", default=18)
    ap.add_argument("--graph", choices=["rmat", "uniform", "grid2d"], default="rmat")
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-oracle", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kcore_bench.py needs a GPU")

    stream = torch.cuda.current_stream()
    ctx = mini_amd.Context(0, stream.cuda_stream)
    if args.graph == "rmat":
        d = rmat.rmat_csr(ctx, args.scale, args.edgefactor, seed=args.scale)
    elif args.graph == "uniform":
        d = rmat.uniform_csr(ctx, args.scale, args.edgefactor)
    else:
        d = rmat.grid2d_csr(ctx, args.scale)
    g = mini_amd.Graph.from_device(ctx, d["n"], d["m"], d["row_offsets"], d["col_indices"])
    g.build_layout()
    kc = mini_amd.KcoreProblem(g)

    def timed(fn):
        x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        x.record(stream)
        out = fn()
        y.record(stream)
        y.synchronize()
        return x.elapsed_time(y), out

    kc.run()                                    # warm-up: code objects, the handle's scratch
    kc.reset()
    kc.enact()
    torch.cuda.synchronize()
    fused, oper = [], []
    equal = True
    for _ in range(args.runs):
        ms, (largest, st) = timed(kc.run)
        fused.append(ms)
        cores, deg = kc.num_cores(), kc.degrees()
        kc.reset()
        torch.cuda.synchronize()
        ms, (elargest, est) = timed(kc.enact)
        oper.append(ms)
        equal = equal and largest == elargest and np.array_equal(cores, kc.num_cores()) and np.array_equal(deg, kc.degrees())
    oracle_equal = None
    if not args.no_oracle and args.scale <= 20:
        from tests.oracle_binding import Oracle
        want, wl, _ = Oracle().kcore_enact(d["row_offsets"].cpu().numpy(), d["col_indices"].cpu().numpy())
        oracle_equal = bool(wl == largest and np.array_equal(cores, want) and np.array_equal(kc.num_cores(), want))
    f_ms, o_ms = statistics.median(fused), statistics.median(oper)
    out = {
        "tool": "kcore_bench", "graph": args.graph, "scale": args.scale, "n": d["n"], "m": d["m"],
        "fused_ms": round(f_ms, 4), "operator_ms": round(o_ms, 4), "speedup": round(o_ms / f_ms, 2),
        "fused_ms_all": [round(x, 4) for x in fused], "operator_ms_all": [round(x, 4) for x in oper],
        "ranges_apart": max(fused) < min(oper),
        "largest_k_core": largest, "levels": st["levels"], "passes": st["passes"], "expanded": st["expanded"],
        "removed": st["removed"], "stranded": st["stranded"], "host_waits_fused": st["host_waits"],
        "operator_k_values": est["rounds"], "operator_passes": est["passes"],
        "fused_M_entries_per_s": round(st["expanded"] / (f_ms * 1e-3) / 1e6, 1),
        "paths_equal": bool(equal), "oracle_equal": oracle_equal,
    }
    print(json.dumps(out), flush=True)
    kc.close()
    g.close()
    ctx.close()
    if not equal or oracle_equal is False:
        sys.exit("k-core: the paths (or the oracle) disagree")


if __name__ == "__main__":
    main()
