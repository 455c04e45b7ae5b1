#!/usr/bin/env python3
"""Vertex similarity, fused path (mgx_sim_run) against the operator path (mgx_sim_enact) in the same process.
usage: sim_bench.py SCALE [--graph uniform|grid2d|rmat] [--pairs P] [--mode random|edges|twohop|hub|sweep] [--measure M] [--operator]
                          [--edgefactor EF] [--rounds N]

The graph is symmetric (the generators' graphs as they are, edge factor 16).  The pairs: `random` P pairs of uniformly random
vertices (default 2^20); `edges` every edge of the simple graph (edges mode); `twohop` P pairs (u, a random neighbour of a random
neighbour of u); `hub` ignores SCALE and --graph: 1 024 pairs of a row of 16 - 20 entries against rows of 100 000, and the same
rows against rows of 100; `sweep` ignores them too: 4 096 pairs (la = 256, lb = 256 r) for r = 1 .. 64 with MGX_SIM_PROBE_RATIO
forced to 1 (every pair a group's: PROBE) and to 2^30 (every pair a wave's), the pair kernels' device time of each: where the two
cross is the default ratio.
Prints one JSON line.  A run ends with its own host wait, so a run's time is the host's wall clock round the call.  One warm-up
handle, then the median, minimum and maximum over N rounds (default 5) of
  * the first run on a fresh handle (the adjacency's build and the allocations included), the build apart (device events), and the
    repeat run; M pairs / s of the repeat run;
  * the repeat run's classifying launch and pair kernels apart (device events), and entries_read x 4 B over the pair kernels' time
    as a share of the 8.0 TB/s the memory is specified for -- the adjacency bytes the kernels asked for, not what reached HBM;
  * with --operator the operator path's repeat run on the same pairs, checked against the fused path's common();
  * one neighbour-reduce call over every row of the graph for scale, and for `edges` k-truss's support phase on the same graph.
The switches MGX_SIM_* are read from the environment as every handle reads them."""
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


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def timed(fn, *a, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = fn(*a, **kw)
    return (time.perf_counter() - t0) * 1e3, st


def rows_graph(ctx, rows, pool):
    """row vertex i is adjacent to the pool vertices rows[i] (indices into the pool, which follows the row vertices) -> Graph"""
    R = len(rows)
    a = np.concatenate([np.full(len(r), i, dtype=np.int64) for i, r in enumerate(rows)])
    b = np.concatenate(rows).astype(np.int64) + R
    src, dst = np.concatenate([a, b]), np.concatenate([b, a])
    order = np.lexsort((dst, src))
    n = R + pool
    ro = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=ro[1:])
    return mini_amd.Graph.from_host(ctx, ro.astype(np.int32), dst[order].astype(np.int32), None)


def measure_pairs(g, pairs, measure, rounds, weights=None):
    """repeat runs of one handle: wall clock, the phases, the bins"""
    sp = mini_amd.SimilarityProblem(g)
    args = dict(pairs=pairs, measure=measure, weights=weights)
    sp.run(**args)
    ms = [timed(sp.run, **args) for _ in range(rounds)]
    sp.set_timing(True)
    ph = []
    for _ in range(rounds):
        sp.run(**args)
        ph.append(sp.phase_ms())
    b = sp.bins()
    out = {"repeat_ms": spread([x[0] for x in ms]), "classify_ms": spread([p["classify"] for p in ph]), "pairs_ms": spread([p["pairs"] for p in ph]),
           "bins": {k: b[k] for k in ("none", "lane", "probe", "wave", "block")}, "entries_read": b["entries_read"], "stats": ms[0][1]}
    pairs_s = statistics.median([p["pairs"] for p in ph]) / 1e3
    out["roof_share"] = round(b["entries_read"] * 4 / pairs_s / (ROOF_TBS * 1e12), 5) if pairs_s > 0 else None
    return out, sp


def hub_mode(ctx, args):
    rng = np.random.default_rng(5)
    pool = 125000
    hubs = [np.sort(rng.permutation(pool)[:100000]) for _ in range(4)]
    plain = [np.sort(rng.permutation(pool)[:100]) for _ in range(4)]
    small = [np.sort(rng.choice(np.unique(rng.integers(0, pool, 64)), 16 + i % 5, replace=False)) for i in range(1024)]
    g = rows_graph(ctx, hubs + plain + small, pool)
    out = {"tool": "sim_bench", "mode": "hub", "pairs": 1024, "measure": args.measure, "rounds_timed": args.rounds}
    for name, first in (("rows_100000", 0), ("rows_100", 4)):
        pr = np.array([(8 + i, first + i % 4) for i in range(1024)], dtype=np.int32)
        r, sp = measure_pairs(g, pr, args.measure, args.rounds)
        sp.close()
        out[name] = {k: r[k] for k in ("repeat_ms", "pairs_ms", "bins", "entries_read")}
    out["hub_over_plain"] = round(out["rows_100000"]["repeat_ms"]["median"] / out["rows_100"]["repeat_ms"]["median"], 3)
    out["hub_over_plain_pair_kernels"] = round(out["rows_100000"]["pairs_ms"]["median"] / out["rows_100"]["pairs_ms"]["median"], 3)
    print(json.dumps(out), flush=True)
    g.close()


def sweep_mode(ctx, args):
    rng = np.random.default_rng(9)
    la, P = 256, 4096
    out = {"tool": "sim_bench", "mode": "sweep", "la": la, "pairs": P, "rounds_timed": args.rounds, "ratios": {}}
    for r in (1, 2, 4, 8, 16, 32, 64):
        lb = la * r
        pool = 4 * lb
        rows = [np.sort(rng.permutation(pool)[:la]) for _ in range(64)] + [np.sort(rng.permutation(pool)[:lb]) for _ in range(16)]
        g = rows_graph(ctx, rows, pool)
        pr = np.array([(i % 64, 64 + (i // 64) % 16) for i in range(P)], dtype=np.int32)
        line = {}
        for name, ratio in (("probe", 1), ("wave", 1 << 30)):
            os.environ["MGX_SIM_PROBE_RATIO"] = str(ratio)         # (read by the handle's first run)
            res, sp = measure_pairs(g, pr, "common", args.rounds)
            sp.close()
            assert res["bins"][name] == P, res["bins"]
            line[name + "_pairs_ms"] = res["pairs_ms"]
        del os.environ["MGX_SIM_PROBE_RATIO"]
        line["probe_over_wave"] = round(line["probe_pairs_ms"]["median"] / line["wave_pairs_ms"]["median"], 3)
        out["ratios"][str(r)] = line
        g.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scale", type=int)
    ap.add_argument("--graph", choices=["uniform", "grid2d", "rmat"], default="uniform")
    ap.add_argument("--pairs", type=int, default=1 << 20)
    ap.add_argument("--mode", choices=["random", "edges", "twohop", "hub", "sweep"], default="random")
    ap.add_argument("--measure", choices=list(mini_amd.SimilarityProblem.MEASURES)[:5] + ["adamic_adar", "resource_allocation"], default="jaccard")
    ap.add_argument("--operator", action="store_true", help="time the operator path as well")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--edgefactor", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sim_bench.py needs a GPU")
    ctx = mini_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    weights = args.measure if args.measure in ("adamic_adar", "resource_allocation") else None
    measure = "weighted" if weights else args.measure
    if args.mode == "hub":
        hub_mode(ctx, args)
        ctx.close()
        return
    if args.mode == "sweep":
        sweep_mode(ctx, args)
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
    gen = torch.Generator(device="cuda").manual_seed(args.scale)
    if args.mode == "edges":
        pairs = None
    else:
        u = torch.randint(0, n, (args.pairs,), device="cuda", generator=gen, dtype=torch.int64)
        if args.mode == "random":
            v = torch.randint(0, n, (args.pairs,), device="cuda", generator=gen, dtype=torch.int64)
        else:
            ro, ci = d["row_offsets"].to(torch.int64), d["col_indices"].to(torch.int64)

            def hop(x):
                deg = ro[x + 1] - ro[x]
                pick = torch.randint(0, 1 << 30, x.shape, device="cuda", generator=gen, dtype=torch.int64) % torch.clamp(deg, min=1)
                return torch.where(deg > 0, ci[torch.clamp(ro[x] + pick, max=m - 1)], x)
            v = hop(hop(u))
        pairs = torch.stack([u, v], dim=1).to(torch.int32).cpu().numpy()

    # first runs on fresh handles: the build and the allocations included
    warm = mini_amd.SimilarityProblem(g)                         # warm-up: code objects, allocator
    warm.run(pairs=pairs, measure=measure, weights=weights)
    warm.close()
    firsts, builds = [], []
    for _ in range(max(args.rounds // 2, 1) + 1):
        h = mini_amd.SimilarityProblem(g)
        h.set_timing(True)
        ms, _ = timed(h.run, pairs=pairs, measure=measure, weights=weights)
        firsts.append(ms)
        builds.append(h.phase_ms()["build"])
        h.close()
    res, sp = measure_pairs(g, pairs, measure, args.rounds, weights)
    st = res.pop("stats")
    out = {"tool": "sim_bench", "graph": args.graph, "scale": args.scale, "n": n, "m": m, "mode": args.mode, "measure": args.measure,
           "rounds_timed": args.rounds, "fused_first_ms": spread(firsts), "build_ms": spread(builds)}
    out.update({k: st[k] for k in mini_amd.SimilarityProblem.KEYS})
    out.update({"fused_" + k if k.endswith("_ms") else k: v for k, v in res.items()})
    out["fused_mpairs_per_s"] = round(st["pairs"] / res["repeat_ms"]["median"] / 1e3, 3)
    common = sp.common()

    fr = mini_amd.Frontier(ctx, n).fill_iota(n)
    vals = torch.rand(n, device="cuda", generator=gen)
    red = torch.empty(n, device="cuda")
    mini_amd.segreduce(g, fr, vals, 0.0, red, "f32_plus")
    out["segreduce_ms"] = spread([timed(mini_amd.segreduce, g, fr, vals, 0.0, red, "f32_plus")[0] for _ in range(args.rounds)])
    if args.mode == "edges":
        kt = mini_amd.KtrussProblem(g)
        kt.set_timing(True)
        kt.run()
        sup = []
        for _ in range(max(args.rounds // 2, 1)):
            kt.run()
            sup.append(kt.phase_ms()["support"])
        out["ktruss_support_ms"] = spread(sup)
        kt.close()
    if args.operator:
        oargs = dict(pairs=pairs, measure=measure, weights=weights)
        sp.enact(**oargs)
        oms = [timed(sp.enact, **oargs)[0] for _ in range(args.rounds)]
        if not np.array_equal(sp.common(), common):
            sys.exit("fused and operator path differ")
        out["operator_repeat_ms"] = spread(oms)
        out["operator_over_fused"] = round(statistics.median(oms) / res["repeat_ms"]["median"], 2)
    sp.close()
    print(json.dumps(out), flush=True)
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
