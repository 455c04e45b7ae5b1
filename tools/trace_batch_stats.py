#!/usr/bin/env python3
"""Per-traversal accounting of a rocprofv3 kernel trace of `bench.py` (batched submission): the timed batch's traversals
(delimited by the launch that holds a traversal's init: k_bfs_fused_init, or a seam launch k_bfs_seam_*_init of a batch with two
states), per kernel type: launches and us per traversal; push / build launches by duration class; the SEAM between two
traversals (everything between the last k_bfs_build2 of one and the first k_bfs_push of the next); with --timeline K the
launches of traversals K and K + 1 of the timed batch one by one.
   python tools/trace_batch_stats.py <trace dir> [steps] [--timeline K]"""
import collections, csv, glob, sys
args = [a for a in sys.argv[1:] if not a.startswith("--")]
d = args[0]
steps = int(args[1]) if len(args) > 1 else 64
timeline = int(sys.argv[sys.argv.index("--timeline") + 1]) if "--timeline" in sys.argv else None
f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r['Start_Timestamp']))
def short(n):
    n = n.replace('void mgx::', '').replace('mgx::', '')
    return n.split('(')[0][:40]
def is_init(r):
    n = r['Kernel_Name']
    return 'k_bfs_fused_init' in n or 'k_bfs_seam_mini_init' in n or 'k_bfs_seam_chain_init' in n
def dur(r):
    return (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
inits = [i for i, r in enumerate(rows) if is_init(r)]
# the timed batch: the longest run of `steps` consecutive inits whose gaps are small (no host work between them)
best = None
for k in range(len(inits) - steps + 1):
    span = int(rows[inits[k + steps - 1]]['Start_Timestamp']) - int(rows[inits[k]]['Start_Timestamp'])
    if best is None or span < best[0]:
        best = (span, k)
k0 = best[1]
i0, i1 = inits[k0], (inits[k0 + steps] if k0 + steps < len(inits) else len(rows))
seg = rows[i0:i1]
# cut at the publish kernel behind the last traversal
for j, r in enumerate(seg):
    if 'k_bfs_publish' in r['Kernel_Name'] and j > len(seg) - 40:
        seg = seg[:j + 1]; break
t0, t1 = int(seg[0]['Start_Timestamp']), int(seg[-1]['End_Timestamp'])
print("timed batch: %d launches, %.1f us per traversal (span / %d)" % (len(seg), (t1 - t0) / 1e3 / steps, steps))
tot = collections.defaultdict(lambda: [0, 0.0])
classes = {"k_bfs_push": collections.defaultdict(lambda: [0, 0.0]), "k_bfs_build2": collections.defaultdict(lambda: [0, 0.0])}
busy = 0.0
for r in seg:
    du = dur(r)
    n = short(r['Kernel_Name'])
    tot[n][0] += 1; tot[n][1] += du; busy += du
    for key in classes:
        if n.startswith(key):
            b = 4 if du < 4 else 8 if du < 8 else 16 if du < 16 else 32 if du < 32 else 64 if du < 64 else 999
            classes[key][b][0] += 1; classes[key][b][1] += du
print("busy %.1f us per traversal, gaps %.1f" % (busy / steps, ((t1 - t0) / 1e3 - busy) / steps))
for n, (c, u) in sorted(tot.items(), key=lambda kv: -kv[1][1]):
    print("  %-42s %6.2f launches  %7.1f us per traversal  (avg %6.1f us)" % (n, c / steps, u / steps, u / c))
for key, cl in classes.items():
    print("  %s by duration:" % key)
    for b in sorted(cl):
        c, u = cl[b]
        print("      < %3s us: %6.2f launches  %7.1f us per traversal" % (b if b < 999 else "inf", c / steps, u / steps))
# the device-wide launches by their position in the traversal (the k-th push / build behind an init launch)
for key in classes:
    pos = collections.defaultdict(lambda: [0, 0.0])
    k = 0
    for r in seg:
        if is_init(r):
            k = 0
        elif short(r['Kernel_Name']).startswith(key):
            pos[k][0] += 1; pos[k][1] += dur(r); k += 1
    print("  %s by position: %s" % (key, "  ".join("#%d %.1f us x %d" % (k, u / c, c) for k, (c, u) in sorted(pos.items()))))
# the seams: from the end of the last k_bfs_build2 in front of an init launch to the start of the first k_bfs_push behind it
seams = []
for k in range(k0 + 1, k0 + steps):
    i = inits[k]
    a = i
    while a > i0 and 'k_bfs_build2' not in rows[a - 1]['Kernel_Name']:
        a -= 1
    b = i
    while b < len(rows) - 1 and 'k_bfs_push' not in rows[b]['Kernel_Name']:
        b += 1
    if a == i0 or b >= len(rows) - 1:
        continue
    seams.append(((int(rows[b]['Start_Timestamp']) - int(rows[a - 1]['End_Timestamp'])) / 1e3, b - a))
if seams:
    s = sorted(x[0] for x in seams)
    print("seam (last build of a traversal -> first push of the next): %d seams, %.1f us on average, median %.1f, %.2f launches" % (
        len(seams), sum(s) / len(s), s[len(s) // 2], sum(x[1] for x in seams) / len(seams)))
if timeline is not None and k0 + timeline + 2 <= len(inits):
    a, b = inits[k0 + timeline], (inits[k0 + timeline + 2] if k0 + timeline + 2 < len(inits) else len(rows))
    # (from the last build in front of the first of the two inits, to show the seam it belongs to)
    while a > i0 and 'k_bfs_build2' not in rows[a - 1]['Kernel_Name']:
        a -= 1
    print("--- traversals %d and %d of the timed batch" % (timeline, timeline + 1))
    base, prev_end = int(rows[a]['Start_Timestamp']), None
    for r in rows[a:b + 1]:
        st = int(r['Start_Timestamp'])
        print("  %9.1f us  %-74s dur %8.1f us  gap %7.1f us" % ((st - base) / 1e3, r['Kernel_Name'].replace('void mgx::', '').replace('mgx::', '')[:74],
                                                                 dur(r), 0.0 if prev_end is None else (st - prev_end) / 1e3))
        prev_end = int(r['End_Timestamp'])
