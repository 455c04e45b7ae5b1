"""bench_dist.py -- bench.py's body for N > 1 (one process per GPU, launched by torch.distributed.run; RCCL over xGMI).

Part of the benchmark, not of the product: it drives mini_amd.dist_bfs (the partitioned traversal) and -- as bench.py
does at N = 1 -- checks the first timed source against the CPU oracle before it prints the line (bench.py --full).
"""
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

from mini_amd.dist_bfs import (DistBfs, DistBfs2, HipRankEngine, HipRankEngine2, pick_sources_dist, rmat_cyclic_shard,
                               rmat_shard_csr)


def _tree_check_local(labels_new, ro_local, col, ranks, rank, src_new):
    """BFS-tree properties of a gathered label array (hub-first global ids, device tensor) over the rows THIS rank owns
    (vertex v = local row * ranks + rank; the graph is symmetric, so a vertex's row lists all its neighbours): every edge
    spans at most one level and stays inside the reached set; every reached vertex other than the source has a neighbour
    one level up.  Returns a bool."""
    lab = labels_new.to(torch.int64)
    nl = ro_local.numel() - 1
    deg = (ro_local[1:] - ro_local[:-1]).to(torch.int64)
    rows_local = torch.repeat_interleave(torch.arange(nl, device=lab.device), deg)
    lu = lab[rows_local * ranks + rank]
    lv = lab[col.to(torch.int64)]
    reached = lu >= 0
    ok = bool(((lv[reached] >= 0) & ((lv[reached] - lu[reached]).abs() <= 1)).all())
    ok = ok and bool((lv[~reached] < 0).all())
    big = torch.iinfo(torch.int64).max
    best = torch.full((nl,), big, dtype=torch.int64, device=lab.device)
    best.scatter_reduce_(0, rows_local, torch.where(lv >= 0, lv, torch.full_like(lv, big)), reduce="amin", include_self=True)
    mine = lab[torch.arange(nl, device=lab.device) * ranks + rank]
    need = (mine > 0)
    ok = ok and bool((best[need] == mine[need] - 1).all())
    if src_new % ranks == rank:
        ok = ok and int(mine[src_new // ranks]) == 0
    return ok


def _measure(args, rank, world, local_rank, ctx, device, gscale, steps, warmup, weak):
    """build this rank's shard of RMAT-<gscale>, run warmup + steps traversals between barriers, verify the first timed
    source; returns the fields of the JSON line (rank 0 uses them) -- collectives inside: every rank calls it alike"""
    import mini_amd
    seed = gscale if args.seed is None else args.seed
    n = 1 << gscale
    t_build = time.time()
    verbose = os.environ.get("MGX_BENCH_VERBOSE") == "1"

    def say(what):
        if verbose:
            print("[rank %d %.1f s] %s" % (rank, time.time() - t_build0, what), file=sys.stderr, flush=True)

    t_build0 = t_build
    gen = int(os.environ.get("MGX_DIST_GEN", "2"))
    comm_dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
    if gen == 2:
        ro, col, new_of_old, old_of_new, deg_new = rmat_cyclic_shard(ctx, gscale, args.edgefactor, seed, world, rank, device)
        torch.cuda.synchronize()
        t_build = time.time() - t_build
        say("shard built: %d rows %d edges" % (ro.numel() - 1, col.numel()))
        eng = HipRankEngine2(ctx, n, world, rank, ro, col)
        bfs = DistBfs2(eng, rank, world, comm_dev)
        from mini_amd.rmat import _mix64_py
        cand = [int(_mix64_py(seed + k) % n) for k in range(8 * (steps + warmup) + 64)]
        cand_new = new_of_old[torch.tensor(cand, device=device)].cpu().tolist()
        cand_deg = deg_new[torch.tensor(cand_new, device=device)].cpu().tolist()
        sources = [v for v, dg in zip(cand_new, cand_deg) if dg > 0][: steps + warmup]
    else:
        ro, col = rmat_shard_csr(ctx, gscale, args.edgefactor, seed, world, rank, device)
        torch.cuda.synchronize()
        t_build = time.time() - t_build
        eng = HipRankEngine(ctx, n, world, rank, ro, col)
        bfs = DistBfs(eng, rank, world, comm_dev)
        ro_host = ro.cpu().numpy()
        sources = pick_sources_dist(ro_host, eng.lo, eng.hi, n, steps + warmup, seed, device)
        new_of_old = old_of_new = None
    say("sources picked")
    for s in sources[: warmup]:
        st = bfs.run(s)
        say("warmup traversal done: %s" % (st,))
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    edges_local, levels = 0, 0
    for s in sources[warmup:]:
        st = bfs.run(s)
        say("traversal done: %s" % (st,))
        edges_local += st["edges_local"]
        levels += st["levels"]
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    t = torch.tensor([elapsed], dtype=torch.float64, device=device if comm_dev == "cuda" else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())
    e = torch.tensor([edges_local], dtype=torch.int64, device=device if comm_dev == "cuda" else "cpu")
    dist.all_reduce(e)
    m_t = int(e.item())
    # how many ranks really took part in the collectives (a launcher that started fewer processes than --gpus must not
    # pass for an N-GPU run): every rank adds one
    ones = torch.tensor([1], dtype=torch.int64, device=device if comm_dev == "cuda" else "cpu")
    dist.all_reduce(ones)
    ranks_seen = int(ones.item())

    # ---- parity of the first timed source (untimed) ---------------------------------------------------------------
    parity, parity_how, cpu = None, None, None
    if not args.no_check and steps > 0:
        src = sources[warmup]
        bfs.run(src)
        labels = bfs.gather_labels()                       # every rank: global labels (generation 2: hub-first ids)
        if gscale <= 23 and os.environ.get("MGX_BENCH_TREE_CHECK") != "1":     # (the switch: pre-flight of the other branch)
            ok = 1
            if rank == 0:
                from mini_amd import rmat as rmat_mod
                from tests.oracle_binding import Oracle
                orc = Oracle()
                g = rmat_mod.rmat_csr(ctx, gscale, args.edgefactor, seed=seed, weighted=False)
                ro_h, ci_h = g["row_offsets"].cpu().numpy(), g["col_indices"].cpu().numpy()
                del g
                if gen == 2:
                    o2n = old_of_new.cpu().numpy()
                    src_old = int(o2n[src])
                else:
                    o2n, src_old = None, src
                tc = time.perf_counter()
                want = orc.bfs_cpu(ro_h, ci_h, src_old)
                cpu_time = time.perf_counter() - tc
                deg_h = np.diff(ro_h)
                cpu_edges, used = int(deg_h[want >= 0].sum()), 1
                ok = int(np.array_equal(labels, want[o2n] if o2n is not None else want))
                if not args.no_cpu_baseline:
                    for s2 in sources[warmup + 1:]:
                        if cpu_time > args.cpu_seconds:
                            break
                        s2_old = int(o2n[s2]) if o2n is not None else s2
                        tc = time.perf_counter()
                        w2 = orc.bfs_cpu(ro_h, ci_h, s2_old)
                        cpu_time += time.perf_counter() - tc
                        cpu_edges += int(deg_h[w2 >= 0].sum()); used += 1
                    cpu = {"value": round(cpu_edges / max(cpu_time, 1e-9) / 1e6, 2), "unit": "MTEPS", "cores": 1, "kind": "port",
                           "host_cpus": os.cpu_count(),
                           "sample": "oracle orc_bfs_cpu (restated bfs_problem_t::cpu) on %d of the %d timed sources, the whole "
                                     "graph rebuilt on rank 0, 1 thread, %.1f s" % (used, steps, cpu_time)}
            flag = torch.tensor([ok], dtype=torch.int64, device=device if comm_dev == "cuda" else "cpu")
            dist.broadcast(flag, 0)
            parity, parity_how = bool(flag.item()), "labels of the first timed source == oracle (rank 0, whole graph)"
        elif gen == 2:
            lab_dev = torch.from_numpy(labels).to(device)
            ok = int(_tree_check_local(lab_dev, ro, col, world, rank, src))
            flag = torch.tensor([ok], dtype=torch.int64, device=device if comm_dev == "cuda" else "cpu")
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            parity, parity_how = bool(flag.item()), "BFS-tree properties of the first timed source's labels over every rank's rows"
    exch = ("one RCCL all-gather per level" if getattr(bfs, "exchange", "gather") == "gather"
            else "RCCL all-to-all of slices + all-gather of the merged slices per level")
    res = {"gscale": gscale, "seed": seed, "m_t": m_t, "elapsed": elapsed, "levels": levels, "t_build": t_build, "ranks_seen": ranks_seen,
           "parity": parity, "parity_how": parity_how, "cpu": cpu, "exch": exch, "steps": steps, "warmup": warmup,
           "native": bool(getattr(bfs, "native", False)), "native_error": getattr(bfs, "native_error", None),
           "rccl": getattr(getattr(bfs, "comm", None), "library", None),
           "sparse_levels": getattr(bfs, "sparse_levels", None), "dense_levels": getattr(bfs, "dense_levels", None)}
    # which paths of the rank engine the LAST traversal took on this rank: a first run on real GPUs should
    # say more than a number
    e = getattr(bfs, "e", None)
    if e is not None and hasattr(e, "path_levels"):
        try:
            p = e.path_levels()
            res["rank_paths"] = {"levels_appended_by_the_push": p[0], "levels_short_rows_vertex_by_vertex": p[1], "a_list_declared_overflowed": bool(p[2]),
                                 "cold_edge_slices_packed": p[3], "levels_from_unit_blocks": e.dense_levels(), "levels_with_cold_edge_pass": e.cold_levels()[0]}
        except Exception as ex:                      # (diagnostics only)
            res["rank_paths"] = {"error": repr(ex)}
    return res


def bench_single_sharded(args, ctx, shards):
    """ONE GPU, a graph whose CSR does not fit int32 row offsets (RMAT-26 ef 16: 2^31 entries; SURVEY F12,
    /root/reference/gunrock/src/graph.hxx:19-26): the graph is cut into `shards` cyclic vertex shards of < 2^31 entries each,
    every shard gets a rank engine on THIS device, and a traversal runs the engines in turn (mgx_dbfs2_run_group: the C++
    loop of the partitioned traversal, its level plan, the "collectives" as device copies into one shared buffer).  All the
    work of the traversal is done by the one GPU: this is the 1-GPU figure for RMAT-26 -- the denominator of the north
    star's ">= 5x at 8 GPUs over 1 GPU on RMAT-26"."""
    import json
    device = torch.device("cuda", 0)
    scale, ef = args.scale, args.edgefactor
    seed = scale if args.seed is None else args.seed
    n = 1 << scale
    t0 = time.time()
    engs, rows = [], []
    for r in range(shards):
        ro, col, new_of_old, old_of_new, deg_new = rmat_cyclic_shard(ctx, scale, ef, seed, shards, r, device)
        engs.append(HipRankEngine2(ctx, n, shards, r, ro, col))
        rows.append((ro, col))
    torch.cuda.synchronize()
    t_build = time.time() - t0
    from mini_amd.rmat import _mix64_py
    steps, warmup = args.steps, max(args.warmup, 1)          # (the first traversal of an engine leaves the level plan)
    cand = [int(_mix64_py(seed + k) % n) for k in range(8 * (steps + warmup) + 64)]
    cand_new = new_of_old[torch.tensor(cand, device=device)].cpu().tolist()
    cand_deg = deg_new[torch.tensor(cand_new, device=device)].cpu().tolist()
    sources = [v for v, dg in zip(cand_new, cand_deg) if dg > 0][: steps + warmup]
    for s in sources[:warmup]:
        HipRankEngine2.run_group(engs, s)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m_t = levels = 0
    for s in sources[warmup:]:
        sts = HipRankEngine2.run_group(engs, s)
        m_t += sum(st["edges_local"] for st in sts)
        levels += sts[0]["levels"]
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs:
        # the last timed traversal's labels, hub-first ids, every shard's rows in place
        from bench import dump_outputs
        lab = np.empty(n, dtype=np.int32)
        for r, e in enumerate(engs):
            lab[r::shards] = e.labels()
        dump_outputs(args.dump_outputs, {"labels": lab})
        del lab
    parity = None
    if not args.no_check and steps > 0:
        src = sources[warmup]
        HipRankEngine2.run_group(engs, src)
        lab = torch.empty(n, dtype=torch.int32, device=device)
        for r, e in enumerate(engs):
            lab[r::shards] = torch.from_numpy(e.labels()).to(device)
        parity = all(_tree_check_local(lab, ro, col, shards, r, src) for r, (ro, col) in enumerate(rows))
    value = m_t / elapsed / 1e6
    out = {"metric": "MTEPS (million traversed edges/sec) BFS advance+filter, RMAT-%d" % scale,
           "value": round(value, 2), "unit": "MTEPS", "n_gpus": 1, "steps": steps, "warmup": warmup,
           "ms_per_step": round(elapsed * 1e3 / max(steps, 1), 4), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
           "dtype": "int32", "data": "synthetic",
           "config": {"workload": "BFS push on RMAT scale %d ef %d, symmetrised (n=%d, %d CSR entries: more than int32 row offsets hold), on ONE "
                                  "GPU as %d cyclic vertex shards of < 2^31 entries, a rank engine each, run in turn by the partitioned "
                                  "traversal's C++ loop (mgx_dbfs2_run_group; the exchanges are device copies), %d seeded sources"
                                  % (scale, ef, n, 2 * ef * n, shards, steps),
                      "scale": scale, "edgefactor": ef, "seed": seed, "parallelism": "1 GPU, %d shards in turn" % shards,
                      "level_plan": dict(zip(("planned_ahead", "frozen", "longer_than_planned", "levels", "lists_mask"), engs[0].spec_stats()))},
           "roofline": {"bound": "hbm", "kernel": "k_bfs_push_level (all shards)", "achieved": round(8.0 * m_t / elapsed / 1e9, 2), "peak": 8000.0,
                        "unit": "GB/s", "frac": round(8.0 * m_t / elapsed / 1e9 / 8000.0, 5), "traffic": None,
                        "note": "algorithmic bytes (8 B/edge) over the whole traversal loop of all shards"},
           "cpu_baseline": None, "parity_vs_oracle": parity,
           "parity_check": "BFS-tree properties of the first timed source's labels over every shard's rows (the oracle needs the whole CSR in int32)",
           "avg_levels": round(levels / max(steps, 1), 2), "graph_build_s": round(t_build, 2)}
    print(json.dumps(out), flush=True)
    for e in engs:
        e.close()
    if parity is False:
        print("bench.py: the sharded traversal's labels failed the check -- the line above is NOT a valid measurement", file=sys.stderr)
        sys.exit(1)


def _measure_replicas(args, rank, world, ctx, device, stream):
    """The other way to use N GPUs for a graph that fits ONE (RMAT-22: 2 GB with its layout): every rank holds the whole graph and
    takes its share of the K sources -- no data-path collective at all ("replicas").  Not what the line's `value` measures (that is
    ONE traversal at a time over the partitioned graph, the north star's shape); reported beside it so that a scaling run shows
    both.  Collective-safe: whatever happens locally, every rank reaches the same two reductions."""
    import mini_amd
    from mini_amd import rmat
    ok, elapsed, m_t, parity = 1, 0.0, 0, 1
    try:
        seed = args.scale if args.seed is None else args.seed
        g = rmat.rmat_csr(ctx, args.scale, args.edgefactor, seed=seed, weighted=False)
        graph = mini_amd.Graph.from_device(ctx, g["n"], g["m"], g["row_offsets"], g["col_indices"])
        graph.build_layout()
        ro_host = g["row_offsets"].cpu().numpy()
        sources = rmat.pick_sources(ro_host, args.steps + args.warmup, seed)
        mine = [int(s) for s in sources[args.warmup:][rank::world]]
        bfs = mini_amd.BfsProblem(graph, sources[0])
        for s in sources[:max(args.warmup, 1)]:
            bfs.run(int(s))
        if mine:
            bfs.run_many(mine[:2])
        torch.cuda.synchronize()
    except Exception as ex:                                   # noqa: BLE001 -- reported through the reduction below
        print("[rank %d] replicas: %r" % (rank, ex), file=sys.stderr, flush=True)
        ok = 0
    flag = torch.tensor([ok], dtype=torch.int64, device=device)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if int(flag.item()) != 1:
        return None
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        if mine:
            sts, _ = bfs.run_many(mine)
            m_t = sum(st["m_t"] for st in sts)
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        if rank == 0 and mine and not args.no_check:
            from tests.oracle_binding import Oracle
            want = Oracle().bfs_cpu(ro_host, g["col_indices"].cpu().numpy(), mine[-1])
            parity = int(np.array_equal(bfs.labels(), want))
    except Exception as ex:                                   # noqa: BLE001
        print("[rank %d] replicas: %r" % (rank, ex), file=sys.stderr, flush=True)
        ok = 0
    t = torch.tensor([elapsed if ok else 1e30, float(m_t), float(parity if ok else 0)], dtype=torch.float64, device=device)
    tmax = t.clone(); dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    tsum = t.clone(); dist.all_reduce(tsum, op=dist.ReduceOp.SUM)
    tmin = t.clone(); dist.all_reduce(tmin, op=dist.ReduceOp.MIN)
    if float(tmax[0]) >= 1e29:
        return None
    return {"workload": "the same %d seeded sources dealt round-robin to the %d ranks, every rank traverses ITS sources on its own copy of the "
                        "whole RMAT-%d graph (fused single-GPU engine, one batch per rank); no data-path collective" % (args.steps, world, args.scale),
            "value": round(float(tsum[1]) / float(tmax[0]) / 1e6, 2), "unit": "MTEPS", "ms_per_step": round(float(tmax[0]) * 1e3 / max(args.steps, 1), 4),
            "scaling": "weak in sources per GPU, none in graph size", "parity_vs_oracle": bool(int(tmin[2]) == 1) if not args.no_check else None}


def bench_main(args, rank, world, local_rank):
    """bench.py body for N > 1 (one process per GPU, RCCL).  --scaling strong (default): the SAME RMAT-<scale> graph
    partitioned over the N GPUs (the metric's "RMAT-22 @1/2/4/8"; --scale 26 at N = 8 is BASELINE config 5);
    --scaling weak: RMAT-(scale + log2 N), a fixed share per GPU.  With --full the first timed source is verified before the line
    is printed: against the oracle (rank 0 rebuilds the whole graph; scales <= 23) or, above that, by the BFS-tree
    properties over every rank's own rows.  With --full at N = 8 and the default workload (strong RMAT-22) the line also carries
    `config5`: the same measurement on RMAT-26 -- BASELINE config 5, the graph the north star's ">= 5x at 8 GPUs" is
    quoted on -- with fewer sources (MGX_BENCH_CONFIG5=0 switches it off)."""
    import json
    import mini_amd
    device = torch.device("cuda", local_rank)
    stream = torch.cuda.current_stream()
    ctx = mini_amd.Context(local_rank, stream.cuda_stream)
    weak = getattr(args, "scaling", "strong") == "weak"
    gscale = args.scale + (int(np.log2(world)) if weak else 0)
    r = _measure(args, rank, world, local_rank, ctx, device, gscale, args.steps, args.warmup, weak)
    c5 = None
    want5 = os.environ.get("MGX_BENCH_CONFIG5", "auto")
    if args.full and (want5 == "1" or (want5 == "auto" and world == 8 and gscale == 22)) and not weak and r["parity"] is not False:
        c5_scale = int(os.environ.get("MGX_BENCH_CONFIG5_SCALE", "26"))
        c5 = _measure(args, rank, world, local_rank, ctx, device, c5_scale, min(args.steps, 16), 1, False)
    rep = None
    if args.full and os.environ.get("MGX_BENCH_REPLICAS", "auto") != "0" and not weak and dist.get_backend() == "nccl" and gscale <= 24:
        rep = _measure_replicas(args, rank, world, ctx, device, stream)
    m_t, elapsed, levels, parity, ranks_seen = r["m_t"], r["elapsed"], r["levels"], r["parity"], r["ranks_seen"]
    if c5 is not None and c5["parity"] is False:
        parity = False
    if rank == 0:
        value = m_t / elapsed / 1e6
        out = {"metric": "MTEPS (million traversed edges/sec) BFS advance+filter, RMAT-%d" % gscale,
               "value": round(value, 2), "unit": "MTEPS", "n_gpus": world, "steps": args.steps,
               "warmup": args.warmup, "ms_per_step": round(elapsed * 1e3 / max(args.steps, 1), 4),
               "higher_is_better": True, "scaling": "weak" if weak else "strong", "vs_baseline": None, "dtype": "int32",
               "data": "synthetic",
               "config": {"workload": "BFS push on RMAT scale %d ef %d, symmetrised (%s), hub-first ids, cyclic vertex partition "
                                      "over %d GPUs, fused level kernels per rank, new-visited bitmaps OR-ed across ranks (%s), "
                                      "%d seeded sources" % (gscale, args.edgefactor,
                                                             "weak scaling: scale %d per GPU + log2 N" % args.scale if weak else
                                                             "strong scaling: the same graph for every N" + ("; BASELINE config 5" if gscale == 26 and world == 8 else ""),
                                                             world, r["exch"], args.steps),
                          "scale": gscale, "edgefactor": args.edgefactor, "seed": r["seed"],
                          "parallelism": "vertex-cyclic x%d" % world,
                          "native_loop": r["native"], "native_error": r["native_error"], "rccl": r["rccl"],
                          "rank0_paths_last_traversal": r.get("rank_paths")},
               "roofline": {"bound": "hbm", "kernel": "k_bfs_push_level (per rank)",
                            "achieved": round(8.0 * m_t / world / elapsed / 1e9, 2), "peak": 8000.0, "unit": "GB/s",
                            "frac": round(8.0 * m_t / world / elapsed / 1e9 / 8000.0, 5), "traffic": None,
                            "note": "per-GPU algorithmic bytes (8 B/edge) over the whole superstep loop incl. exchange"},
               "cpu_baseline": r["cpu"], "parity_vs_oracle": parity, "parity_check": r["parity_how"],
               "rccl_ranks": ranks_seen, "collective_backend": dist.get_backend(),
               "avg_levels": round(levels / max(args.steps, 1), 2),
               "graph_build_s": round(r["t_build"], 2)}
        if rep is not None:
            out["replicas"] = rep
        if c5 is not None:
            v5 = c5["m_t"] / c5["elapsed"] / 1e6
            out["config5"] = {"workload": "BASELINE config 5: BFS on RMAT scale %d ef %d, cyclic vertex partition over %d GPUs (%s), %d seeded "
                                          "sources after 1 warm-up, same engine and loop as the line's value" % (c5["gscale"], args.edgefactor, world, c5["exch"], c5["steps"]),
                              "value": round(v5, 2), "unit": "MTEPS", "ms_per_step": round(c5["elapsed"] * 1e3 / max(c5["steps"], 1), 4),
                              "steps": c5["steps"], "avg_levels": round(c5["levels"] / max(c5["steps"], 1), 2),
                              "parity": c5["parity"], "parity_check": c5["parity_how"], "shard_build_s": round(c5["t_build"], 2),
                              "per_gpu_alg_GBps": round(8.0 * c5["m_t"] / world / c5["elapsed"] / 1e9, 2),
                              "rank0_paths_last_traversal": c5.get("rank_paths"),
                              "note": "vs_1gpu_rmat26: this value / the one-GPU RMAT-26 figure of profiles/rmat26_1gpu.json (bench.py --scale 26 "
                                      "--gpus 1: the graph as two shards in turn on one MI355X, round 5) -- the ratio the north star's >= 5x names"}
            try:
                one = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "rmat26_1gpu.json")))
                if c5["gscale"] == 26:
                    out["config5"]["vs_1gpu_rmat26"] = round(v5 / float(one["value"]), 3)
                    out["config5"]["one_gpu_rmat26_MTEPS"] = one["value"]
                    # the denominator is a COMMITTED measurement of another run: say which sources and round it was taken on, and whether
                    # the kernels have changed since -- a stale denominator is visible on the line, not silent
                    from bench import source_sha
                    out["config5"]["one_gpu_rmat26_from"] = {"file": "profiles/rmat26_1gpu.json", "round": one.get("round"), "steps": one.get("steps"),
                                                             "source_sha": one.get("source_sha"), "current_source_sha": source_sha(),
                                                             "stale": one.get("source_sha") != source_sha()}
            except Exception:                    # (the file is a committed measurement: without it the ratio is simply not quoted)
                pass
        print(json.dumps(out), flush=True)
        if parity is False:
            print("bench.py: the partitioned traversal's labels failed the check -- the line above is NOT a valid measurement", file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()
    if parity is False:
        sys.exit(1)
    if ranks_seen != args.gpus:
        print("bench.py: %d ranks took part, --gpus says %d" % (ranks_seen, args.gpus), file=sys.stderr)
        sys.exit(1)
