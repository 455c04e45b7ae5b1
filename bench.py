#!/usr/bin/env python3
"""bench.py -- BFS advance+filter MTEPS on synthetic R-MAT (BASELINE.json metric).

  python bench.py [--gpus 1] [--steps K] [--warmup W]           config 2: RMAT-22 ef 16 on one MI355X
  python -m torch.distributed.run ... bench.py --gpus N ...     RMAT-22 over N GPUs (strong scaling, the metric's
                                                                "RMAT-22 @1/2/4/8"); --scale 26 at N = 8 is config 5;
                                                                --scaling weak: RMAT-(scale + log2 N)
  python bench.py --file g.mtx [--undirected] --src S --validate the reference's own driver flags (tests/bfs/test_bfs.cu:14-31)

A "step" is one whole BFS traversal (label reset + every advance+filter level) from one seeded source, inputs resident
in HBM.  value = sum over steps of m_t (CSR entries of reached vertices) / wall time of the K steps / 1e6,
max over ranks.  With --full the line is only printed with exit status 0 when the first timed source's labels equal the
oracle's (or, at RMAT-26, pass the BFS-tree property check): a wrong traversal that ends early would report a HIGHER rate.

A plain run sets up, warms up, times the K steps and prints the line (--dump-outputs DIR: and writes the last timed step's
outputs as DIR/<name>.npy).  Everything else -- the oracle check, the CPU baseline, the per-call, roofline and per-level
passes, at N > 1 the config5 and replicas measurements -- runs only with --full (--validate turns the oracle check on by
itself); without it those objects are null.

Extra objects on the JSON line (--full):
  roofline     the product kernel k_bfs_push (one launch per slot: long rows + short rows, or a chain of small levels):
               algorithmic bytes (8 B/edge + 20 B/frontier vertex) per launch / average launch duration (HIP
               events around every launch, on the launch stream, in a second pass over the same sources), vs 8 TB/s.
               traffic: HBM bytes per launch from the committed PMC passes (profiles/pmc_traffic.json: 2 x FETCH_SIZE +
               WRITE_SIZE, gfx950 correction) -- only when that file was measured on exactly these sources (source hash).
  cpu_baseline the CPU oracle's restatement of bfs_problem_t::cpu (bfs_problem.hxx:52-72), one host thread, on a bounded
               sample of the same sources ("port": the reference itself cannot be built here).
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0      # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s spec, ~6.3 achievable)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--scaling", choices=["strong", "weak"], default="strong",
                    help="N > 1: strong = the SAME RMAT-<scale> over N GPUs (the metric's RMAT-22 @1/2/4/8; --scale 26 "
                         "--gpus 8 is config 5); weak = RMAT-(scale + log2 N)")
    ap.add_argument("--dist-timeout", type=float, default=900.0,
                    help="N > 1: seconds the whole multi-rank run may take.  The self-launcher kills its child process group when "
                         "they are up and exits 124 with a one-line reason; every rank also arms a watchdog of its own (a launch by "
                         "torch.distributed.run has no parent of ours): a collective that never returns must not eat the caller's clock")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="budget of the cpu_baseline sample")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--mode", choices=["push", "do", "sssp", "pr"], default="push",
                    help="push = BASELINE config 2 (headline); do = direction-optimising (config 4); sssp = config 3 (fused "
                         "frontier Bellman-Ford on weighted RMAT, value = edge relaxations/s); pr = the segmented "
                         "neighbour-reduce over the full frontier (value = reduced edges/s)")
    ap.add_argument("--per-call", action="store_true",
                    help="BFS: time one library call per source instead of submitting the K sources as one batch "
                         "(mgx_bfs_run_many); the per-call figure is on the line either way (per_call)")
    ap.add_argument("--alpha", type=float, default=4.0, help="bottom-up switch: unvisited < frontier*alpha")
    ap.add_argument("--no-layout", action="store_true", help="keep generator vertex ids (no hub-first relabelling)")
    ap.add_argument("--pmc-json", default=os.path.join(ROOT, "profiles", "pmc_traffic.json"))
    # the reference's driver flags (tests/bfs/test_bfs.cu:14-31)
    ap.add_argument("--graph", choices=["rmat", "uniform", "grid2d"], default="rmat",
                    help="synthetic input: rmat (BASELINE's), uniform = edgefactor * 2^scale uniformly random pairs, symmetrised (no hubs), "
                         "grid2d = a 2^(scale/2) x 2^(scale/2) 4-neighbour grid (thousands of levels); built on the device, seeded")
    ap.add_argument("--shards", type=int, default=0,
                    help="push, 1 GPU: run the graph as this many cyclic vertex shards in turn (the RMAT-26 path) whatever its size")
    ap.add_argument("--file", default=None, help="MatrixMarket file instead of the synthetic R-MAT")
    ap.add_argument("--undirected", action="store_true", help="--file: append the swapped copy of every entry")
    ap.add_argument("--src", type=int, default=None, help="source vertex (default: seeded sources; --file: 0)")
    ap.add_argument("--validate", action="store_true", help="compare EVERY timed source with the oracle (default, with --full: the first)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: the oracle check, the CPU baseline, the per-call / roofline / per-level passes and, at "
                         "N > 1, config5 and replicas (a plain run only sets up, warms up and times the steps)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last one computed (labels / distances / reduced values, one GPU) "
                         "as DIR/<name>.npy in float32 or float64, at most 64 MB in all (a fixed seeded sample of a larger output)")
    args = ap.parse_args()
    if args.dump_outputs and args.gpus > 1:
        ap.error("--dump-outputs: one GPU only")
    if not args.full:
        args.no_cpu_baseline = True
        args.no_check = args.no_check or not args.validate
    return args


DUMP_BYTES = 60 * 1000 * 1000          # --dump-outputs: everything written, headers aside, stays under 64 MB


def dump_outputs(d, arrays):
    """--dump-outputs: {name: array} of the last timed step -> d/<name>.npy.  float32 outputs, and integer ones whose values
    float32 holds exactly, as float32; other integers as float64.  The arrays share DUMP_BYTES, the smallest served first;
    one over its share is written as a fixed sample of its entries (seeded: the same positions for every run of the same
    arguments), the sampled positions beside it as <name>_index.npy."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    arrays = {k: np.asarray(v).ravel() for k, v in arrays.items()}
    left = DUMP_BYTES
    for i, (name, a) in enumerate(sorted(arrays.items(), key=lambda kv: kv[1].size)):
        exact32 = a.dtype == np.float32 or (a.dtype.kind in "iu" and (a.size == 0 or int(np.abs(a.astype(np.int64)).max()) < (1 << 24)))
        a = a.astype(np.float32 if exact32 else np.float64)
        share = left // (len(arrays) - i)
        if a.nbytes > share:
            k = share // (a.itemsize + 8)
            idx = np.sort(np.random.default_rng(12345).choice(a.size, size=k, replace=False))
            np.save(os.path.join(d, name + "_index.npy"), idx.astype(np.float64))
            a = a[idx]
            left -= 8 * k
        left -= a.nbytes
        np.save(os.path.join(d, name + ".npy"), a)


def source_sha():
    """hash of the product sources (kernels + C-ABI): ties a committed PMC measurement to the code it was taken on"""
    h = hashlib.sha256()
    for base in ("include", os.path.join("mini_amd", "csrc")):
        for d, _, files in sorted(os.walk(os.path.join(ROOT, base))):
            for f in sorted(files):
                if f.endswith((".hpp", ".hxx", ".h", ".hip")):
                    h.update(f.encode())
                    h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def self_launch(args):
    """`python bench.py --gpus N` (N > 1) WITHOUT a launcher: start the N ranks as fresh child processes -- before this
    process has imported torch or touched the GPU -- through torch.distributed.run on 127.0.0.1, relay their output (rank
    0 prints the one JSON line) and return the launcher's exit code.  Never falls through to the 1-GPU body."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    # fresh children in a process group (session) of their own: on expiry the GROUP is ended -- launcher and ranks --
    # and nothing that has touched the GPU is ever re-executed
    import signal
    child = subprocess.Popen(cmd, env=env, start_new_session=True)
    try:
        return child.wait(timeout=args.dist_timeout if args.dist_timeout > 0 else None)
    except subprocess.TimeoutExpired:
        print("bench.py: the %d-rank run did not finish within --dist-timeout %.0f s (a collective or a rank hangs): "
              "ending the child process group" % (args.gpus, args.dist_timeout), file=sys.stderr, flush=True)
        for sig, grace in ((signal.SIGTERM, 10.0), (signal.SIGKILL, 10.0)):
            try:
                os.killpg(child.pid, sig)
            except ProcessLookupError:
                break
            try:
                child.wait(timeout=grace)
                break
            except subprocess.TimeoutExpired:
                continue
        return 124
    except KeyboardInterrupt:
        try:
            os.killpg(child.pid, signal.SIGTERM)
        except ProcessLookupError:
            pass
        raise


def arm_watchdog(seconds, what):
    """a rank's own deadline (daemon timer thread; library calls release the GIL): one line on stderr, then the process
    ends with status 124 -- it does not try to unwind a collective that never returns"""
    import threading

    def expire():
        print("bench.py: %s did not finish within %.0f s (--dist-timeout): exiting 124" % (what, seconds), file=sys.stderr, flush=True)
        os._exit(124)
    if seconds and seconds > 0:
        t = threading.Timer(seconds, expire)
        t.daemon = True
        t.start()
        return t
    return None


def main():
    args = parse()
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(self_launch(args))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and os.environ.get("MGX_BENCH_WATCHDOG_OFF") != "1":
        # (a little under the self-launcher's limit, so that a rank's own one-line reason is what the caller reads)
        arm_watchdog(max(args.dist_timeout - 15.0, 0.9 * args.dist_timeout), "rank %d of %d" % (rank, world))
    launch_only = os.environ.get("MGX_BENCH_LAUNCH_ONLY")
    if launch_only:      # (CPU tests of the launch contract: who was started, nothing else; "hang": a rank that never returns)
        print("launched rank %s of %s (--gpus %d)" % (os.environ.get("RANK"), os.environ.get("WORLD_SIZE"), args.gpus), flush=True)
        if launch_only == "hang" and (rank == 1 or os.environ.get("MGX_BENCH_HANG_ALL") == "1"):
            while True:
                time.sleep(3600)
        return
    import numpy as np
    import torch
    import torch.distributed as dist

    if world != args.gpus and world > 1:
        args.gpus = world
    # Pre-flight switches for a one-GPU box (never a reported number): MGX_BENCH_ALL_ON_GPU0=1 puts every rank on
    # cuda:0, MGX_BENCH_DIST_BACKEND=gloo replaces RCCL (which refuses two ranks on one device)
    if os.environ.get("MGX_BENCH_ALL_ON_GPU0") == "1":
        local_rank = 0
    backend = os.environ.get("MGX_BENCH_DIST_BACKEND", "nccl")
    torch.cuda.set_device(local_rank)
    # MGX_BENCH_FORCE_DIST=1 under a one-rank torchrun: run the N>1 code path (RCCL group of one) -- a
    # pre-flight for the multi-GPU bench on a one-GPU box, never a reported number
    force_dist = os.environ.get("MGX_BENCH_FORCE_DIST") == "1" and "RANK" in os.environ
    if world > 1 or force_dist:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)

    import __graft_entry__ as ge
    if rank == 0 and not os.path.exists(ge.LIB_OUT):
        ge.build()
    if world > 1:
        dist.barrier()
    import mini_amd
    from mini_amd import rmat

    if world > 1 or force_dist:
        if args.dump_outputs:
            sys.exit("bench.py: --dump-outputs: one GPU only")
        import bench_dist
        return bench_dist.bench_main(args, rank, world, local_rank)

    stream = torch.cuda.current_stream()
    ctx = mini_amd.Context(local_rank, stream.cuda_stream)
    if args.mode == "push" and not args.file and args.graph == "rmat" and ((2 * args.edgefactor << args.scale) >= (1 << 31) or args.shards > 1):
        # more CSR entries than int32 row offsets hold (RMAT-26): the graph as shards of < 2^31 entries, in turn on this GPU
        import bench_dist
        shards = max(2, args.shards)
        while (2 * args.edgefactor << args.scale) // shards >= (1 << 31):
            shards *= 2
        return bench_dist.bench_single_sharded(args, ctx, shards)
    if args.mode == "sssp":
        return bench_sssp(args, ctx, stream)
    if args.mode == "pr":
        return bench_pr(args, ctx, stream)
    return bench_bfs(args, ctx, stream)


def _pmc_traffic(args, kname, sha):
    """roofline.traffic from the committed PMC passes -- only when they were taken on exactly these sources"""
    traffic, note = None, "no PMC measurement for these sources (profiles/pmc_traffic.json)"
    if os.path.exists(args.pmc_json) and not args.file and getattr(args, "graph", "rmat") == "rmat":
        try:
            pj = json.load(open(args.pmc_json))
            entries = pj.get("entries", [pj])
            for e in entries:
                if e.get("scale") == args.scale and e.get("kernel") == kname and e.get("source_sha") == sha and e.get("mode") == args.mode:
                    return e.get("hbm_bytes_per_launch"), ("2 x FETCH_SIZE + WRITE_SIZE per dispatch of this kernel, separate --pmc "
                                                           "passes of this command (profiles/)")
            note = "profiles/pmc_traffic.json was measured on other sources/kernels (%s vs %s): not reported" % (
                entries[0].get("source_sha") if entries else None, sha)
        except Exception:
            pass
    return traffic, note


def bench_bfs(args, ctx, stream):
    import numpy as np
    import torch
    import mini_amd
    from mini_amd import rmat
    seed = args.scale if args.seed is None else args.seed
    t_build = time.time()
    if args.file:
        # a MatrixMarket file is parsed and sorted once; its binary CSR cache (mgx_graph_save_csr) is used from then on
        cache = args.file if args.file.endswith(".mgxcsr") else args.file + (".undir" if args.undirected else "") + ".mgxcsr"
        loaded = None
        # the cache is used only while it is at least as new as the text file; a truncated or corrupt one (an interrupted
        # run) is re-made from the text instead of ending the run
        if os.path.exists(cache) and (cache == args.file or os.path.getmtime(cache) >= os.path.getmtime(args.file)):
            try:
                loaded = mini_amd.load_csr_cache(cache)
            except mini_amd.MgxError:
                if cache == args.file:
                    raise
        if loaded is not None:
            n, ro_host, ci_host, w_host = loaded["n"], loaded["row_offsets"], loaded["col_indices"], loaded["weights"]
        else:
            n, ro_host, ci_host, w_host = mini_amd.load_mtx(args.file, undir=args.undirected)
            try:
                tmp = "%s.tmp.%d" % (cache, os.getpid())
                mini_amd.save_csr_cache(tmp, ro_host, ci_host, w_host, undirected=args.undirected)
                os.replace(tmp, cache)              # (never a half-written cache under the final name)
            except (mini_amd.MgxError, OSError):
                pass                    # (a read-only directory: no cache, nothing else changes)
        graph = mini_amd.Graph.from_host(ctx, ro_host, ci_host, w_host)
        if args.mode == "do" and not args.undirected:
            graph.build_csc()
        m = len(ci_host)
        what = "%s%s" % (os.path.basename(args.file), " (undirected)" if args.undirected else "")
    else:
        if args.graph == "uniform":
            g = rmat.uniform_csr(ctx, args.scale, args.edgefactor, seed=seed)
            what = "uniform random graph, scale %d ef %d (2^%d vertices, %d x 2^%d random pairs), symmetrised" % (args.scale, args.edgefactor, args.scale, args.edgefactor, args.scale)
        elif args.graph == "grid2d":
            g = rmat.grid2d_csr(ctx, args.scale)
            what = "2-d grid %d x %d, 4 neighbours" % (1 << (args.scale // 2), 1 << (args.scale - args.scale // 2))
        else:
            g = rmat.rmat_csr(ctx, args.scale, args.edgefactor, seed=seed, weighted=False)
            what = "RMAT scale %d ef %d, symmetrised" % (args.scale, args.edgefactor)
        graph = mini_amd.Graph.from_device(ctx, g["n"], g["m"], g["row_offsets"], g["col_indices"])
        ro_host = g["row_offsets"].cpu().numpy()
        ci_host = None
        n, m = g["n"], g["m"]
    t_build = time.time() - t_build
    t_layout = time.time()
    use_layout = not args.no_layout and not (args.mode == "do" and args.file and not args.undirected)
    if use_layout:
        # hub-first layout (vertex ids by descending degree) + unit blocks of its long rows: part of graph construction
        # like the CSR build, not of the timed traversal; labels stay in original ids
        graph.build_layout()          # mgx_graph_build_layout: device-side, inside the library
        torch.cuda.synchronize()
    t_layout = time.time() - t_layout
    if args.src is not None or args.file:
        sources = [args.src or 0] * (args.steps + args.warmup)
    else:
        sources = rmat.pick_sources(ro_host, args.steps + args.warmup, seed)
    bfs = mini_amd.BfsProblem(graph, sources[0])

    mode = mini_amd.MGX_BFS_DIRECTION_OPT if args.mode == "do" else mini_amd.MGX_BFS_PUSH
    timed = [int(s) for s in sources[args.warmup:]]
    alpha_f = float(args.alpha)
    # warm-up: the W warm-up sources one call each, then (batched submission) the timed batch shape once, so that the
    # slot hint the batch is sized by has seen this graph's level structure
    for s in sources[:args.warmup]:
        bfs.run(s, mode, args.alpha)
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reruns = 0
    if args.per_call:
        # K whole traversals, one library call each (each call returns when its labels are complete); the counters go into
        # buffers made beforehand, nothing is converted or allocated between two traversals
        bufs = [bfs.new_stats() for _ in timed]
        run_into = bfs.run_into
        t0 = time.perf_counter()
        ev0.record(stream)
        for s, st in zip(timed, bufs):
            run_into(s, mode, alpha_f, st)
        ev1.record(stream)
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        stats = [bfs.stats_dict(st) for st in bufs]
    else:
        # the timed region: the K traversals handed to the library as ONE batch (mgx_bfs_run_many): each traversal is
        # complete (labels re-initialised, every level run, counters taken) before the next one starts on the device, but
        # the host waits once, at the end -- no host round trip between two traversals
        prepared = bfs.prepare_many(timed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev0.record(stream)
        raw, reruns = bfs.run_many(timed, mode, alpha_f, prepared=prepared)
        ev1.record(stream)
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        L = bfs.STATS_LEN
        stats = [bfs.stats_dict(raw[i * L:(i + 1) * L]) for i in range(len(timed))]
    dev_ms = ev0.elapsed_time(ev1)
    if args.dump_outputs:
        # the labels the timed call leaves are its last source's (batch or per call); m_t / reached / levels of that traversal
        last = stats[-1] if stats else {"levels": 0, "reached": 0, "m_t": 0}
        dump_outputs(args.dump_outputs, {"labels": bfs.labels(), "counts": [last["levels"], last["reached"], last["m_t"]]})
    # Per-call pass (--full): the same K sources, one call each, each timed on the host -> the per-call mean beside the
    # batched figure, and the per-source median SURVEY 8d asks for
    per_src_s = []
    for s in (timed if args.full else []):
        st1 = bfs.new_stats()
        torch.cuda.synchronize()
        tc = time.perf_counter()
        bfs.run_into(s, mode, alpha_f, st1)
        per_src_s.append(time.perf_counter() - tc)
    per_src_mt = [st["m_t"] for st in stats]
    slots_hist = {}
    # Roofline pass: the SAME K sources again, now with HIP events around every launch of the product kernel k_bfs_push
    # and of the queue build behind it (on the launch stream).  A pass of its own because every event record between two
    # kernels leaves a ~6 us gap on the stream (rocprofv3 kernel trace, profiles/): inside the timed region they would cost
    # several % of `value`.
    passes = timed if args.full else []
    bfs.set_kernel_timing(2)
    stats_timed, kernel_times = [], []
    build_launches, build_ns = 0, 0
    for s in passes:
        stats_timed.append(bfs.run(s, mode, args.alpha))
        slots_hist[stats_timed[-1]["slots"]] = slots_hist.get(stats_timed[-1]["slots"], 0) + 1
        kt = bfs.kernel_times()
        kernel_times.append(kt["stream"])
        build_launches += kt["wave"]["launches"]
        build_ns += kt["wave"]["ns"]
    # ... and once more with the launch split into its parts (long rows / short rows), for the breakdown only
    bfs.set_kernel_timing(1)
    parts = {"stream": {"launches": 0, "ns": 0, "edges": 0, "vertices": 0}, "wave": {"launches": 0, "ns": 0, "edges": 0, "vertices": 0}}
    for s in passes:
        bfs.run(s, mode, args.alpha)
        k = bfs.kernel_times()
        for name in parts:
            for f in parts[name]:
                parts[name][f] += k[name][f]
    bfs.set_kernel_timing(0)
    # ... and the levels of the PRODUCT launches (merged push, no events on the stream) from the stamps a level's opener takes on the device:
    # a level's time runs from its opener to the next one's (push + queue build + whatever sits between them); levels are lined up by their
    # distance from the traversal's biggest one
    by_rel = {}
    if mode == mini_amd.MGX_BFS_PUSH:
        for s in passes[:32]:
            bfs.run(s, mode, args.alpha)
            tms, tr = bfs.level_times_ms(), bfs.level_trace()
            L = min(len(tms), len(tr))
            if L == 0:
                continue
            peak = max(range(L), key=lambda i: tr[i][1])
            for i in range(L):
                rel = max(-3, min(3, i - peak))
                a = by_rel.setdefault(rel, [0, 0.0, 0, 0])
                a[0] += 1; a[1] += tms[i] * 1e3; a[2] += tr[i][1]; a[3] += tr[i][0]
    levels = [{"rel_to_peak": ("<=-3" if r == -3 else ">=3" if r == 3 else r), "levels": c, "us": round(us / c, 2), "edges": int(e / c), "vertices": int(v / c),
               "frac": round((8.0 * e + 20.0 * v) / max(us * 1e-6, 1e-12) / 1e9 / HBM_PEAK_GBPS, 4)} for r, (c, us, e, v) in sorted(by_rel.items())]

    m_t = sum(st["m_t"] for st in stats)
    reached = sum(st["reached"] for st in stats)
    launches = sum(st["kernel_launches"] for st in stats_timed)      # (batch events only exist in the second pass)
    kernel_ns = sum(st["kernel_ns"] for st in stats_timed)
    nf_total = sum(st["frontier_vertices"] for st in stats)   # vertices expanded (degree >= 1)
    # algorithmic bytes: top-down levels 8 B/edge expanded, bottom-up levels 4.125 B per inspected in-edge
    # (SURVEY 8d), 20 B per frontier vertex either way
    push_edges = sum(st["push_edges"] for st in stats)
    pull_edges = sum(st["pull_edges"] for st in stats)
    alg_bytes = 8.0 * push_edges + 4.125 * pull_edges + 20.0 * nf_total
    value = m_t / elapsed / 1e6

    # Dominant kernel: k_bfs_push, ONE launch per slot.  achieved = algorithmic bytes of what the kernel itself moves --
    # 8 B per edge (column index + visited probe) + 12 B per frontier vertex (id, two row offsets); the other 8 B per
    # vertex of SURVEY 8d's 20 (label write, next-frontier write) are moved by the queue build and credited to the slot
    # (push + build) below -- / device time of ALL its launches (the ones that run a chain of small levels or find nothing
    # to do included, as rocprofv3 --stats averages over them too).
    dom = {f: sum(k[f] for k in kernel_times) for f in ("launches", "ns", "edges", "vertices")}
    kname = "k_bfs_push<false, 0>"
    slot_frac = None
    if dom["launches"] and dom["ns"] and dom["edges"]:
        dom_bytes = 8.0 * dom["edges"] + 12.0 * dom["vertices"]
        avg_launch_s = (dom["ns"] / 1e9) / dom["launches"]
        bytes_per_launch = dom_bytes / dom["launches"]
        if build_ns:
            slot_frac = (8.0 * dom["edges"] + 20.0 * dom["vertices"]) / ((dom["ns"] + build_ns) / 1e9) / 1e9 / HBM_PEAK_GBPS
    else:
        avg_launch_s = (kernel_ns / 1e9) / max(launches, 1)
        bytes_per_launch = alg_bytes / max(launches, 1)
        kname = "bfs level kernels (all)"
    achieved = bytes_per_launch / avg_launch_s / 1e9 if avg_launch_s > 0 else 0.0
    sha = source_sha()
    traffic, traffic_note = _pmc_traffic(args, kname, sha)
    long_ns, short_ns = parts["stream"]["ns"], parts["wave"]["ns"]
    K = max(len(stats), 1)
    roofline = {"bound": "hbm", "kernel": kname, "achieved": round(achieved, 2),
                "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBPS, 5),
                "traffic": traffic, "traffic_note": traffic_note, "launches": dom["launches"] if dom["launches"] else launches,
                "alg_bytes": "8 B per traversed edge + 12 B per frontier vertex (this kernel's share of SURVEY 8d's 8 + 20; the "
                             "label and next-frontier writes, 8 B per vertex, belong to the queue build: slot_frac)",
                "timing": "HIP events around every launch of this kernel on the launch stream, second pass over the same %d "
                          "sources (events kept out of the timed region: each leaves a ~6 us gap on the stream)" % len(stats),
                "avg_launch_us": round(avg_launch_s * 1e6, 3),
                "alg_bytes_per_launch": round(bytes_per_launch, 1),
                "share_of_edges": round(dom["edges"] / max(m_t, 1), 4) if dom["launches"] else 1.0,
                "slot_frac": round(slot_frac, 5) if slot_frac is not None else None,
                "slot_note": "advance + filter: (8 B/edge + 20 B/vertex) / (device time of k_bfs_push + k_bfs_build2 of every slot) / peak",
                "build_us_per_traversal": round(build_ns / 1e3 / K, 2), "build_launches_per_traversal": round(build_launches / K, 2),
                "push_us_per_traversal": round(dom["ns"] / 1e3 / K, 2),
                "parts": {"long_rows": {"alg_GBps": round((8.0 * parts["stream"]["edges"] + 12.0 * parts["stream"]["vertices"]) / max(long_ns, 1), 2),
                                        "us_per_traversal": round(long_ns / 1e3 / K, 2), "edges_share": round(parts["stream"]["edges"] / max(m_t, 1), 4)},
                          "short_rows": {"alg_GBps": round((8.0 * parts["wave"]["edges"] + 12.0 * parts["wave"]["vertices"]) / max(short_ns, 1), 2),
                                         "us_per_traversal": round(short_ns / 1e3 / K, 2), "edges_share": round(parts["wave"]["edges"] / max(m_t, 1), 4)},
                          "note": "third pass, the launch split into its parts (k_bfs_push<false, 2> / <false, 3>) with events around each"},
                "levels": levels or None,
                "levels_note": "fourth pass (up to 32 of the same sources, one call each, the product's merged launches): mean time from a level's opener to "
                               "the next one's by distance from the traversal's biggest level, (8 B/edge + 20 B/vertex) / that time / peak",
                "all_level_kernels_alg_GBps": round(alg_bytes / max(kernel_ns / 1e9, 1e-12) / 1e9, 2),
                "whole_bfs_alg_GBps": round(alg_bytes / (dev_ms / 1e3) / 1e9, 2),
                "whole_bfs_frac": round(alg_bytes / (dev_ms / 1e3) / 1e9 / HBM_PEAK_GBPS, 5)}

    cpu = None
    parity = None
    if not args.no_cpu_baseline or not args.no_check:
        from tests.oracle_binding import Oracle
        orc = Oracle()
        if ci_host is None:
            ci_host = g["col_indices"].cpu().numpy()
        deg = np.diff(ro_host)
        cpu_edges, cpu_time, used = 0, 0.0, 0
        for s in timed:
            tc = time.perf_counter()
            want = orc.bfs_cpu(ro_host, ci_host, s)
            cpu_time += time.perf_counter() - tc
            cpu_edges += int(deg[want >= 0].sum())
            used += 1
            if (used == 1 or args.validate) and not args.no_check:
                bfs.run(s, mode, args.alpha)
                ok = bool(np.array_equal(bfs.labels(), want))
                if used == 1 and not args.per_call:
                    # ... and the batched call itself: the labels it leaves are the LAST source's -- run [first, this] as a batch
                    bfs.run_many([timed[-1], s], mode, alpha_f)
                    ok = ok and bool(np.array_equal(bfs.labels(), want))
                parity = ok if parity is None else (parity and ok)
            if (cpu_time > args.cpu_seconds or args.no_cpu_baseline) and not args.validate:
                break
        if not args.no_cpu_baseline:
            cpu = {"value": round(cpu_edges / max(cpu_time, 1e-9) / 1e6, 2), "unit": "MTEPS", "cores": 1, "kind": "port",
                   "host_cpus": os.cpu_count(),
                   "sample": "oracle orc_bfs_cpu (restated bfs_problem_t::cpu) on %d of the %d timed sources, "
                             "same in-memory CSR, 1 thread, %.1f s" % (used, len(stats), cpu_time)}

    per_call_ms = sorted(x * 1e3 for x in per_src_s)
    med = per_call_ms[len(per_call_ms) // 2] if per_call_ms else 0.0
    per_src_rate = sorted(mt / max(t, 1e-12) / 1e6 for mt, t in zip(per_src_mt, per_src_s))
    submission = "one library call per source" if args.per_call else \
        ("the %d sources submitted as ONE batch (mgx_bfs_run_many: the traversals one after the other on the device, each complete before the "
         "next one's init kernel resets the state; the host waits once, at the end)" % len(timed))
    gname = {"rmat": "RMAT-%d", "uniform": "uniform-%d", "grid2d": "grid2d-%d"}[args.graph] % args.scale
    out = {"metric": "MTEPS (million traversed edges/sec) BFS advance+filter, %s" % (gname if not args.file else os.path.basename(args.file)),
           "value": round(value, 2), "unit": "MTEPS", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(elapsed * 1e3 / max(args.steps, 1), 4), "higher_is_better": True,
           "scaling": "strong", "vs_baseline": None, "dtype": "int32", "data": "synthetic" if not args.file else "file",
           "config": {"workload": "BFS %s (fused LB advance + idempotent-visited filter) on %s, n=%d m=%d, %d %s, %s; "
                                  "untimed one-time preprocessing per graph: hub-first copy + unit blocks (layout_build_s)"
                                  % ("push" if args.mode == "push" else "direction-optimising alpha=%g" % args.alpha,
                                     what, n, m, args.steps, "seeded sources" if args.src is None and not args.file else "runs from source %d" % sources[0],
                                     submission),
                      "scale": args.scale if not args.file else None, "edgefactor": args.edgefactor if not args.file else None,
                      "graph": args.graph if not args.file else "file",
                      "seed": seed, "parallelism": "1 GPU", "submission": "per_call" if args.per_call else "batch",
                      "layout": "hub-first (degree-sorted) copy + unit blocks for the fused kernel" if use_layout else "generator ids"},
           "roofline": roofline if args.full else None, "cpu_baseline": cpu, "parity_vs_oracle": parity,
           "per_call": None if not args.full else {"ms_per_step": round(sum(per_src_s) * 1e3 / K, 4), "value": round(m_t / max(sum(per_src_s), 1e-12) / 1e6, 2),
                        "ms_per_step_median": round(med, 4),
                        "value_median_source": round(per_src_rate[len(per_src_rate) // 2], 2) if per_src_rate else None,
                        "note": "the same %d sources, one mgx_bfs_run call each, each timed on the host (call to return); the median is "
                                "over sources (SURVEY 8d)" % len(timed)},
           "graph500_MTEPS": round(m_t / 2.0 / elapsed / 1e6, 2),
           "graph500_note": "Graph500 convention: undirected input edges inside the reached component / time = m_t / 2 on the symmetrised CSR (SURVEY 8d)",
           "batch_reruns": reruns, "slots_needed_hist": {str(k): v for k, v in sorted(slots_hist.items())} if args.full else None,
           "device_ms_per_step": round(dev_ms / max(args.steps, 1), 4),
           "avg_levels": round(sum(st["levels"] for st in stats) / K, 2),
           "avg_slots": round(sum(st["slots"] for st in stats) / K, 2),
           "avg_reached": reached // K, "graph_build_s": round(t_build, 2), "layout_build_s": round(t_layout, 2),
           "layout": (dict(graph.layout_info(), csr_bytes=4 * (n + 1) + 4 * m,
                           note="what the fast path keeps beside the CSR (mgx_graph_layout_info): hub-first copy, id maps, unit blocks and their "
                                "24-bit copy, cold-edge lists, the unit blocks without the lists' entries; device_bytes sums them")
                      if use_layout else None),
           "source_sha": sha}
    print(json.dumps(out), flush=True)
    if parity is False:
        print("bench.py: labels differ from the oracle's -- the line above is NOT a valid measurement", file=sys.stderr)
        sys.exit(1)



def bench_sssp(args, ctx, stream):
    """BASELINE config 3: SSSP on the weighted RMAT (integer weights in [0, 63]).  step = one whole run from a seeded source
    (mgx_sssp_run: the fused frontier Bellman-Ford of sssp_enactor.hxx:40-72, advance = relax every edge of the frontier,
    filter = one entry per improved vertex); value = edge relaxations / s."""
    import numpy as np
    import torch
    import mini_amd
    from mini_amd import rmat
    seed = args.scale if args.seed is None else args.seed
    t_build = time.time()
    g = rmat.rmat_csr(ctx, args.scale, args.edgefactor, seed=seed, weighted=True)
    graph = mini_amd.Graph.from_device(ctx, g["n"], g["m"], g["row_offsets"], g["col_indices"], g["weights"])
    ro_host = g["row_offsets"].cpu().numpy()
    n, m = g["n"], g["m"]
    t_build = time.time() - t_build
    t_layout = time.time()
    if not args.no_layout:
        graph.build_layout(weights=True)
        torch.cuda.synchronize()
    t_layout = time.time() - t_layout
    sources = [args.src] * (args.steps + args.warmup) if args.src is not None else rmat.pick_sources(ro_host, args.steps + args.warmup, seed)
    sssp = mini_amd.SsspProblem(graph, sources[0])
    for s in sources[:args.warmup]:
        sssp.run(s)
    timed = [int(s) for s in sources[args.warmup:]]
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stats = []
    t0 = time.perf_counter()
    ev0.record(stream)
    for s in timed:
        stats.append(sssp.run(s))
    ev1.record(stream)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    dev_ms = ev0.elapsed_time(ev1)
    relax = sum(st["relaxations"] for st in stats)
    ftot = sum(st["frontier_total"] for st in stats)
    iters = sum(st["iterations"] for st in stats)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"distances": sssp.distances()})
    passes = timed if args.full else []
    # roofline pass (--full): the same sources with HIP events around every k_sssp_relax launch (on the launch stream)
    sssp.set_kernel_timing(True)
    k_launch, k_ns, relax2, ftot2 = 0, 0, 0, 0
    for s in passes:
        st = sssp.run(s)
        kt = sssp.kernel_times()
        k_launch += kt["launches"]; k_ns += kt["ns"]
        relax2 += st["relaxations"]; ftot2 += st["frontier_total"]
    sssp.set_kernel_timing(False)
    # ... and the iterations of the product's launches from the device-side stamps (no events on the stream), lined up by their distance from
    # the run's heaviest one: time from an iteration's opener to the next one's (relax + sweep + queue build)
    by_rel = {}
    for s in passes[:32]:
        sssp.run(s)
        tr = sssp.iteration_trace()
        if not tr:
            continue
        peak = max(range(len(tr)), key=lambda i: tr[i][1])
        for i, (nf_i, ne_i, ms_i) in enumerate(tr):
            if ms_i <= 0:
                continue
            rel = max(-3, min(3, i - peak))
            a = by_rel.setdefault(rel, [0, 0.0, 0, 0])
            a[0] += 1; a[1] += ms_i * 1e3; a[2] += ne_i; a[3] += nf_i
    iterations = [{"rel_to_heaviest": ("<=-3" if r == -3 else ">=3" if r == 3 else r), "iterations": c, "us": round(us / c, 2), "edges": int(e / c), "vertices": int(v / c),
                   "G_relax_per_s": round(e / max(us, 1e-9) / 1e3, 1), "frac": round((12.0 * e + 24.0 * v) / max(us * 1e-6, 1e-12) / 1e9 / HBM_PEAK_GBPS, 4)}
                  for r, (c, us, e, v) in sorted(by_rel.items())]
    # algorithmic bytes: 12 B per relaxation (column index, weight, dist[dst]) + 24 B per frontier vertex
    # (id, two offsets, dist[src], next-frontier entry, mark); the relax kernel's share: 12 B + 16 B
    alg_bytes = 12.0 * relax + 24.0 * ftot
    k_bytes = 12.0 * relax2 + 16.0 * ftot2
    avg_launch_s = (k_ns / 1e9) / max(k_launch, 1)
    achieved = (k_bytes / max(k_launch, 1)) / max(avg_launch_s, 1e-12) / 1e9
    sha = source_sha()
    traffic, traffic_note = _pmc_traffic(args, "k_sssp_relax<1024> (+ k_sssp_relax_dense<1024> on heavy iterations)", sha)
    K = max(len(timed), 1)
    roofline = {"bound": "hbm", "kernel": "k_sssp_relax<1024> (+ k_sssp_relax_dense<1024> on heavy iterations)", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBPS, 5), "traffic": traffic, "traffic_note": traffic_note,
                "launches": k_launch, "avg_launch_us": round(avg_launch_s * 1e6, 3),
                "alg_bytes_per_launch": round(k_bytes / max(k_launch, 1), 1),
                "alg_bytes": "12 B per edge relaxation + 16 B per frontier vertex (this kernel's share of SURVEY 8d's 12 + 24; the "
                             "queue build moves the other 8 B per vertex)",
                "timing": "HIP events around every launch of this kernel on the launch stream, second pass over the same %d sources" % len(timed),
                "iterations": iterations or None,
                "iterations_note": "third pass (up to 32 of the same sources): mean time from an iteration's opener to the next one's by distance from the "
                                   "run's heaviest iteration, (12 B/relaxation + 24 B/vertex) / that time / peak",
                "whole_run_alg_GBps": round(alg_bytes / (dev_ms / 1e3) / 1e9, 2),
                "whole_run_frac": round(alg_bytes / (dev_ms / 1e3) / 1e9 / HBM_PEAK_GBPS, 5)}
    cpu, parity = None, None
    if not args.no_cpu_baseline or not args.no_check:
        from tests.oracle_binding import Oracle
        orc = Oracle()
        ci_host, w_host = g["col_indices"].cpu().numpy(), g["weights"].cpu().numpy()
        deg = np.diff(ro_host)
        if not args.no_check:
            s = timed[0]
            want = orc.sssp_dijkstra_f32(ro_host, ci_host, w_host, s)       # float32 Dijkstra: the unique min-plus fixed point
            sssp.run(s)
            parity = bool(np.array_equal(sssp.distances(), want))
        if not args.no_cpu_baseline:
            cpu_time, cpu_edges, used = 0.0, 0, 0
            for s in timed:
                tc = time.perf_counter()
                _, idist = orc.sssp_cpu(ro_host, ci_host, w_host, s)        # restated sssp_problem_t::cpu (sssp_problem.hxx:59-88)
                cpu_time += time.perf_counter() - tc
                cpu_edges += int(deg[idist < np.iinfo(np.int32).max].sum())
                used += 1
                if cpu_time > args.cpu_seconds:
                    break
            cpu = {"value": round(cpu_edges / max(cpu_time, 1e-9) / 1e6, 2), "unit": "MTEPS (out-edges of reached vertices / s)", "cores": 1,
                   "kind": "port", "host_cpus": os.cpu_count(), "seconds_per_source": round(cpu_time / max(used, 1), 3),
                   "sample": "oracle orc_sssp_cpu (restated sssp_problem_t::cpu: label-correcting, priority queue) on %d of the %d timed "
                             "sources, same in-memory CSR, 1 thread, %.1f s; it scans an edge once per improvement of its source, "
                             "so its rate is quoted on the traversed edges m_t, next to traversed_MTEPS of the GPU run" % (used, len(timed), cpu_time)}
    out = {"metric": "MTEPS (million edge relaxations/sec) SSSP advance+filter, RMAT-%d weighted" % args.scale,
           "value": round(relax / elapsed / 1e6, 2), "unit": "MTEPS", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(elapsed * 1e3 / max(args.steps, 1), 4), "higher_is_better": True, "scaling": "strong",
           "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": "SSSP (fused frontier Bellman-Ford: relax every edge of the frontier with atomicMin, one queue entry per "
                                  "improved vertex) on RMAT scale %d ef %d symmetrised, integer weights in [0, 63] as float32, n=%d m=%d, "
                                  "%d seeded sources, one library call per source; untimed one-time preprocessing per graph: hub-first "
                                  "copy with weights (layout_build_s)" % (args.scale, args.edgefactor, n, m, args.steps),
                      "scale": args.scale, "edgefactor": args.edgefactor, "seed": seed, "parallelism": "1 GPU",
                      "layout": "generator ids" if args.no_layout else "hub-first (degree-sorted) copy with weights"},
           "roofline": roofline if args.full else None, "cpu_baseline": cpu, "parity_vs_oracle": parity,
           "traversed_MTEPS": None,
           "relaxations_per_source": relax // K, "frontier_total_per_source": ftot // K, "iterations_per_source": round(iters / K, 2),
           "device_ms_per_step": round(dev_ms / max(args.steps, 1), 4), "graph_build_s": round(t_build, 2), "layout_build_s": round(t_layout, 2),
           "source_sha": sha}
    # traversed edges of the reached component (Gunrock's m_t), for the comparison with the CPU validator's rate
    if cpu is not None or parity is not None:
        reached_deg = None
        try:
            d0 = sssp.distances()
            reached_deg = int(np.diff(ro_host)[d0 < np.finfo(np.float32).max].sum())
        except Exception:
            pass
        if reached_deg is not None:
            out["traversed_MTEPS"] = round(reached_deg / (elapsed / K) / 1e6, 2)
    print(json.dumps(out), flush=True)
    if parity is False:
        print("bench.py: distances differ from the oracle's -- the line above is NOT a valid measurement", file=sys.stderr)
        sys.exit(1)


def bench_pr(args, ctx, stream):
    """The segmented neighbour-reduce (neighborhood.hxx:12-70, the operator PR is built on): step = one reduce over the full
    frontier (every vertex), reduced[v] = sum of value[u] over the row of v; value = reduced edges / s."""
    import numpy as np
    import torch
    import mini_amd
    from mini_amd import rmat
    seed = args.scale if args.seed is None else args.seed
    t_build = time.time()
    g = rmat.rmat_csr(ctx, args.scale, args.edgefactor, seed=seed, weighted=False)
    graph = mini_amd.Graph.from_device(ctx, g["n"], g["m"], g["row_offsets"], g["col_indices"])
    n, m = g["n"], g["m"]
    t_build = time.time() - t_build
    t_layout = time.time()
    if not args.no_layout:
        graph.build_layout()          # the operator's full-frontier path reads the graph's hub-first copy (mgx/nreduce.hpp)
        torch.cuda.synchronize()
    t_layout = time.time() - t_layout
    f = mini_amd.Frontier(ctx, n).fill_iota(n)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    vals = torch.rand(n, device="cuda", generator=gen)
    red = torch.empty(n, device="cuda")
    t_slices = time.time()
    mini_amd.segreduce(graph, f, vals, 0.0, red, "f32_plus")     # (the graph's first full-frontier reduce: the library regroups the long rows by slice of their destinations, untimed one-time preprocessing)
    torch.cuda.synchronize()
    t_slices = time.time() - t_slices
    for _ in range(max(args.warmup, 1)):
        mini_amd.segreduce(graph, f, vals, 0.0, red, "f32_plus")
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record(stream)
    nz = 0
    for _ in range(args.steps):
        nz = mini_amd.segreduce(graph, f, vals, 0.0, red, "f32_plus")
    ev1.record(stream)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    dev_ms = ev0.elapsed_time(ev1)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"reduced": red.cpu().numpy()})
    # roofline pass (--full): events around each operator call (all its kernels run on this stream; the count read-back included)
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps if args.full else 0)]
    for a, b in evs:
        a.record(stream)
        mini_amd.segreduce(graph, f, vals, 0.0, red, "f32_plus")
        b.record(stream)
    torch.cuda.synchronize()
    op_ms = sum(a.elapsed_time(b) for a, b in evs) / max(len(evs), 1)
    alg = 8.0 * nz + 16.0 * n
    achieved = alg / (op_ms / 1e3) / 1e9 if op_ms > 0 else 0.0
    sha = source_sha()
    traffic, traffic_note = _pmc_traffic(args, "neighbour-reduce operator", sha)
    roofline = {"bound": "hbm", "kernel": "neighbour-reduce operator (every kernel of one mgx_segreduce_f32_plus call over the full frontier: "
                                          "k_nr_values (with the frontier check), k_nrs_edges -- the long rows by slice of their destinations + the short rows, the dominant one --, k_nrs_fold; k_nr_edges / k_nr_fold under MGX_NR_SLICED=0)", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBPS, 5), "traffic": traffic, "traffic_note": traffic_note, "launches": len(evs),
                "avg_launch_us": round(op_ms * 1e3, 3), "alg_bytes_per_launch": alg,
                "alg_bytes": "8 B per edge (column index + value gather) + 16 B per frontier vertex (SURVEY 8d)",
                "timing": "HIP events around every operator call on the launch stream, second pass"}
    cpu, parity = None, None
    if not args.no_cpu_baseline or not args.no_check:
        from tests.oracle_binding import Oracle
        orc = Oracle()
        ro_h, ci_h = g["row_offsets"].cpu().numpy(), g["col_indices"].cpu().numpy()
        fin = np.arange(n, dtype=np.int32)
        v_h = vals.cpu().numpy()
        tc = time.perf_counter()
        want, onz = orc.neighbor_reduce_f32_plus(ro_h, ci_h, fin, v_h, 0.0)
        cpu_time = time.perf_counter() - tc
        if not args.no_check:
            got = red.cpu().numpy()
            # float sum order differs (the reference's own order is moderngpu's, unpinned): 2e-5 relative to the oracle, as tests/ do.
            # The oracle accumulates serially in float32 like the reference's reduce: on a row of several hundred thousand entries
            # ITS rounding error passes that (RMAT-24, 739 757 entries: 4.2e-5 off the float64 sum; the library's folds 2e-7) -- so a
            # mismatch is settled against the float64 sum of the same float32 values: the library within 2e-6 of it, the oracle
            # within 1e-3.
            parity = bool(onz == nz and np.allclose(got, want, rtol=2e-5, atol=1e-6))
            if not parity and onz == nz:
                rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ro_h))
                want64 = np.bincount(rows, weights=v_h.astype(np.float64)[ci_h], minlength=n)
                parity = bool(np.allclose(got, want64, rtol=2e-6, atol=1e-6) and np.allclose(want, want64, rtol=1e-3, atol=1e-6))
        if not args.no_cpu_baseline:
            cpu = {"value": round(onz / max(cpu_time, 1e-9) / 1e6, 2), "unit": "MTEPS", "cores": 1, "kind": "port", "host_cpus": os.cpu_count(),
                   "sample": "oracle orc_neighbor_reduce_f32_plus (serial restatement of neighborhood.hxx:12-70) once over the same "
                             "%d edges, 1 thread, %.1f s" % (onz, cpu_time)}
    out = {"metric": "MTEPS (million reduced edges/sec) segmented neighbour-reduce, RMAT-%d" % args.scale,
           "value": round(nz * args.steps / elapsed / 1e6, 2), "unit": "MTEPS", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(elapsed * 1e3 / max(args.steps, 1), 4), "higher_is_better": True, "scaling": "strong",
           "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": "neighbour-reduce (float plus) over the full frontier of RMAT scale %d ef %d symmetrised, n=%d m=%d: "
                                  "one operator call per step" % (args.scale, args.edgefactor, n, m),
                      "scale": args.scale, "edgefactor": args.edgefactor, "seed": seed, "parallelism": "1 GPU",
                      "layout": "generator ids" if args.no_layout else "the operator is called with generator ids; for a full frontier the library reads "
                                "the graph's hub-first copy (the long rows regrouped by slice of their destinations -- nr_slices --, degree classes "
                                "for the short rows; untimed one-time preprocessing: layout_build_s + nr_slices_build_s)"},
           "roofline": roofline if args.full else None, "cpu_baseline": cpu, "parity_vs_oracle": parity, "parity_tolerance": "rtol 2e-5 against the serial float32 oracle (float sum order); where the oracle's own rounding exceeds that (rows of several 10^5 entries): rtol 2e-6 against the float64 sum of the same values, the oracle within 1e-3 of it",
           "device_ms_per_step": round(dev_ms / max(args.steps, 1), 4), "graph_build_s": round(t_build, 2), "layout_build_s": round(t_layout, 2),
           "nr_slices_build_s": round(t_slices, 2), "nr_slices": None if args.no_layout else graph.nr_slices_info(),
           "source_sha": sha}
    print(json.dumps(out), flush=True)
    if parity is False:
        print("bench.py: reduced values differ from the oracle's -- the line above is NOT a valid measurement", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
