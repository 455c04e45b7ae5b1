#!/usr/bin/env python3
"""Where a fused k-core run's time goes, by kind of step: a rocprofv3 kernel trace joined with the run's own record of what
each launch was (mgx_kcore_step_kinds).

    rocprofv3 --kernel-trace --stats -d DIR -o kc --output-format csv -- python tools/kcore_trace_split.py run KINDS.json [SCALE] [--graph G]
    python tools/kcore_trace_split.py split DIR KINDS.json

`run` does one warm-up and one recorded run and writes the kinds; `split` takes the last run's launches from the trace (as many
k_kcore_step dispatches as the run enqueued) and prints, per kind: launches, busy time, the longest; then the idle time
between launches and the launches behind the run's end."""
import argparse
import collections
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(args):
    import torch
    import mini_amd
    from mini_amd import rmat
    stream = torch.cuda.current_stream()
    ctx = mini_amd.Context(0, stream.cuda_stream)
    if args.graph == "rmat":
        d = rmat.rmat_csr(ctx, args.scale, 16, seed=args.scale)
    elif args.graph == "uniform":
        d = rmat.uniform_csr(ctx, args.scale, 16)
    else:
        d = rmat.grid2d_csr(ctx, args.scale)
    g = mini_amd.Graph.from_device(ctx, d["n"], d["m"], d["row_offsets"], d["col_indices"])
    kc = mini_amd.KcoreProblem(g)
    kc.run()
    torch.cuda.synchronize()
    x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    x.record(stream)
    largest, st = kc.run()
    y.record(stream)
    y.synchronize()
    kinds = kc.step_kinds()
    json.dump({"graph": args.graph, "scale": args.scale, "ms": x.elapsed_time(y), "largest": largest, "stats": st,
               "kinds": kinds.tolist()}, open(args.kinds, "w"))
    kc.close()
    g.close()
    ctx.close()


def split(args):
    rec = json.load(open(args.kinds))
    kinds = rec["kinds"]
    names = {1: "min", 2: "list", 3: "expand", 4: "filter", 5: "idle (behind the end)", 6: "mini"}
    f = glob.glob(args.dir + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    ks = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows if "k_kcore_step" in r["Kernel_Name"]]
    assert len(ks) >= len(kinds), (len(ks), len(kinds))
    seg = ks[-len(kinds):]
    live = [i for i, k in enumerate(kinds) if k != 5]
    end = live[-1] if live else 0
    span = (seg[end][1] - seg[0][0]) / 1e3
    tot = collections.defaultdict(lambda: [0, 0.0, 0.0])
    busy = 0.0
    for (s, e), k in zip(seg, kinds):
        du = (e - s) / 1e3
        t = tot[k]
        t[0] += 1
        t[1] += du
        t[2] = max(t[2], du)
        if k != 5:
            busy += du
    print("%s-%d: %.3f ms by the events; %d launches, %d of them steps; first to last step %.1f us: busy %.1f, idle between launches %.1f"
          % (rec["graph"], rec["scale"], rec["ms"], len(kinds), len(live), span, busy, span - busy))
    print("stats", rec["stats"])
    for k in (1, 2, 3, 4, 6, 5):
        c, u, mx = tot[k]
        if c:
            print("  %-22s %5d launches  %9.1f us  (avg %6.2f, longest %7.1f)" % (names[k], c, u, u / c, mx))
    if args.show:
        print("us of every %s step, in order:" % names[args.show],
              " ".join("%.1f" % ((e - s) / 1e3) for (s, e), k in zip(seg, kinds) if k == args.show))
    level = tot[1][1] + tot[2][1]
    passes = tot[3][1] + tot[4][1] + tot[6][1]
    print("level steps (min + list) %.1f us, pass steps (expand + filter + mini) %.1f us, idle %.1f us, behind the end %.1f us"
          % (level, passes, span - busy, (seg[-1][1] - seg[end][1]) / 1e3))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("kinds")
    r.add_argument("scale", type=int, nargs="?", default=20)
    r.add_argument("--graph", choices=["rmat", "uniform", "grid2d"], default="rmat")
    s = sub.add_parser("split")
    s.add_argument("dir")
    s.add_argument("kinds")
    s.add_argument("--show", type=int, default=0, help="print the duration of every step of this kind (1 min, 2 list, 3 expand, 4 filter, 6 mini)")
    args = ap.parse_args()
    run(args) if args.cmd == "run" else split(args)


if __name__ == "__main__":
    main()
