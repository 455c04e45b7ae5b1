"""The definition of the Louvain community detection in numpy: what mgx_louvain_run computes, bit for bit.
Everything is integer arithmetic (int64), so no result depends on an order of additions.

Level 0 graph.  Votes as in tests/lpa_model.py: symmetric: every CSR entry (v, u), u != v, is weight 1 from v to u; else every
entry gives weight 1 to both ends.  Self-loops are dropped, duplicates add.  k_v = the sum of v's weights, W = the sum of all k_v.
Iteration t of a level (labels start as lab[v] = v).  Sigma_c = the k of the vertices labelled c; k_{v,c} = the weight from v to
vertices labelled c, v's own self entry excluded.  s(c) = k_{v,c} W - (Sigma_c - [c == lab[v]] k_v) k_v over the candidates
lab[v] and the labels of v's neighbours; key(c) = fmix32(c ^ seed).  best(v): the greatest score; on equal scores the current label
wins, otherwise the smaller key.  v moves iff best(v) != lab[v] and key(best) < key(lab[v]) (t even) or > (t odd).  All moves of an
iteration read lab_t and Sigma_t.
Acceptance.  Qnum(lab) = S_in W - S_sq (self entries of coarse levels count in S_in).  The moved labelling is accepted iff a vertex
moved and Qnum(new) - Qnum(old) > thr, thr = min(ceil(tol * float(W) * float(W)), 2^62).  A level ends after two consecutive rejected
iterations or at max_iter.
Aggregation.  A level that accepted no iteration ends the run, and so does level == max_levels.  Otherwise the communities get dense
ids in ascending order of their label (that map is a level of the dendrogram), and, unless max_levels is reached, the coarse graph
is built: one row per community, columns ascending and unique, weights summed, the self entry (a, a) holding the internal weight
(both directions), so that a coarse k_a is the sum of its members' k and W is the same on every level."""
import math

import numpy as np

from tests import coloring_model, lpa_model, row_bodies

SEED = 0x9E3779B9
STAT_KEYS = ("communities", "largest", "largest_id", "levels", "s_in", "s_sq", "w")
# the defaults of MGX_LOUVAIN_SHORT_MAX, MGX_LOUVAIN_WAVE_MAX and MGX_LOUVAIN_SEG (include/mgx/louvain_fused.hpp)
SHORT_MAX, WAVE_MAX, SEG = 16, 256, 256
# the kinds of the fused path's launches
SETUP, EVAL, LONG_FILL, LONG_SCAN, APPLY, QNUM, DONE = range(1, 8)
THR_MAX = 1 << 62


def keys(c, seed):
    return coloring_model.fmix32(np.asarray(c, dtype=np.int64).astype(np.uint32) ^ np.uint32(seed & 0xFFFFFFFF)).astype(np.int64)


def threshold(tol, w):
    x = tol * float(w) * float(w)
    return THR_MAX if x >= float(THR_MAX) else min(int(math.ceil(x)), THR_MAX)


def level0(ro, ci, symmetric):
    """-> (n, rcv, snd, weight, row entries) of level 0: int64 arrays, one item per vote"""
    n = len(ro) - 1
    rcv, snd = lpa_model.votes(ro, ci, symmetric)
    return n, rcv, snd, np.ones(len(rcv), dtype=np.int64), lpa_model.row_entries(ro, ci, symmetric)


def degrees(n, rcv, wt):
    return np.bincount(rcv, weights=None if len(rcv) == 0 else wt, minlength=n).astype(np.int64) if n else np.zeros(0, np.int64)


def qnum(n, rcv, snd, wt, k, lab):
    """(Qnum, S_in, S_sq) of lab in Python integers"""
    w = int(k.sum())
    s_in = int(wt[lab[rcv] == lab[snd]].sum())
    tot = np.bincount(lab, weights=k, minlength=max(n, 1)).astype(np.int64)
    s_sq = sum(int(x) * int(x) for x in tot[tot > 0])
    return s_in * w - s_sq, s_in, s_sq


def best_labels(n, rcv, snd, wt, k, w, lab, seed):
    """best(v) of every vertex under lab"""
    sigma = np.bincount(lab, weights=k, minlength=n).astype(np.int64)
    m = rcv != snd
    v = np.concatenate([rcv[m], np.arange(n, dtype=np.int64)])              # (the current label is a candidate of weight 0)
    c = np.concatenate([lab[snd[m]], lab])
    x = np.concatenate([wt[m], np.zeros(n, dtype=np.int64)])
    pair, inv = np.unique(v * n + c, return_inverse=True)
    kvc = np.bincount(inv, weights=x, minlength=len(pair)).astype(np.int64)
    pv, pc = pair // n, pair % n
    cur = (pc == lab[pv]).astype(np.int64)
    score = kvc * w - (sigma[pc] - cur * k[pv]) * k[pv]
    order = np.lexsort((keys(pc, seed), -cur, -score, pv))                 # by vertex: score down, current first, key up
    first = np.ones(len(order), dtype=bool)
    first[1:] = pv[order][1:] != pv[order][:-1]
    best = np.empty(n, dtype=np.int64)
    best[pv[order][first]] = pc[order][first]
    return best


def iterate(n, rcv, snd, wt, k, w, lab, t, seed):
    """-> (labels after iteration t's moves, vertices that moved)"""
    best = best_labels(n, rcv, snd, wt, k, w, lab, seed)
    kb, kc = keys(best, seed), keys(lab, seed)
    moves = (best != lab) & ((kb < kc) if t % 2 == 0 else (kb > kc))
    return np.where(moves, best, lab), int(moves.sum())


def run_level(n, rcv, snd, wt, seed, max_iter, thr):
    """-> (labels, trace [(moved, accepted, Qnum of the moved labelling)], accepted iterations, Qnum, ended by rejections)"""
    k = degrees(n, rcv, wt)
    w = int(k.sum())
    lab = np.arange(n, dtype=np.int64)
    q = qnum(n, rcv, snd, wt, k, lab)[0]
    trace, rejects, accepted, t = [], 0, 0, 0
    while t < max_iter and rejects < 2:
        new, moved = iterate(n, rcv, snd, wt, k, w, lab, t, seed)
        qn = qnum(n, rcv, snd, wt, k, new)[0]
        ok = moved > 0 and qn - q > thr
        trace.append((moved, int(ok), qn))
        if ok:
            lab, q, rejects, accepted = new, qn, 0, accepted + 1
        else:
            rejects += 1
        t += 1
    return lab, trace, accepted, q, rejects >= 2


def aggregate(rcv, snd, wt, dense):
    """the coarse graph of the map `dense`: (communities' rcv, snd, weight), rows and columns ascending, unique"""
    nc = int(dense.max()) + 1
    pair, inv = np.unique(dense[rcv] * nc + dense[snd], return_inverse=True)
    return pair // nc, pair % nc, np.bincount(inv, weights=wt, minlength=len(pair)).astype(np.int64)


def body_bins(lens, short_max, wave_max):
    return list(row_bodies.bodies(lens, short_max, wave_max).values())


def louvain(ro, ci, symmetric=True, seed=SEED, max_iter=100, max_levels=32, tol=0.0, short_max=SHORT_MAX, wave_max=WAVE_MAX,
            seg=SEG):
    """-> dict(labels int32[n], maps [int32 per aggregated level], levels [(vertices, entries, iterations, accepted, communities,
    Qnum)], trace [(moved, accepted, Qnum) over all levels], stats (STAT_KEYS), kinds [the fused path's launches, level by level],
    bins [vertices per body over the levels: none, short, wave, long], items (the long rows' (vertex, segment) items over the
    run), ended [a level ended by two rejections])"""
    n, rcv, snd, wt, lens = level0(ro, ci, symmetric)
    w = int(len(rcv))
    thr = threshold(tol, w)
    out = {"labels": np.arange(n, dtype=np.int32), "maps": [], "levels": [], "trace": [], "kinds": [], "bins": [0, 0, 0, 0],
           "items": 0, "ended": []}
    level, n_l = 0, n
    s = (0, int(w), int(w))                                                # (S_in, S_sq, W of identity labels)
    if w > 0:
        k = degrees(n, rcv, wt)
        s = qnum(n, rcv, snd, wt, k, np.arange(n, dtype=np.int64))[1:] + (w,)
    while w > 0 and level < max_levels:
        lab, trace, accepted, q, ended = run_level(n_l, rcv, snd, wt, seed, max_iter, thr)
        long_items = row_bodies.bodies(lens, short_max, wave_max, seg)["segments"]
        out["kinds"].append(SETUP)
        for _ in trace:
            out["kinds"] += [EVAL] + ([LONG_FILL, LONG_SCAN] if long_items else []) + [APPLY, QNUM]
            out["items"] += long_items
        out["kinds"].append(DONE)
        for b, c in enumerate(body_bins(lens, short_max, wave_max)):
            out["bins"][b] += c
        ids, dense = np.unique(lab, return_inverse=True)
        out["levels"].append((n_l, int(lens.sum()), len(trace), accepted, len(ids), q))
        out["trace"] += trace
        out["ended"].append(ended)
        if accepted == 0:
            break
        dense = dense.astype(np.int64)
        out["maps"].append(dense.astype(np.int32))
        out["labels"] = dense[out["labels"]].astype(np.int32)
        s = qnum(n_l, rcv, snd, wt, degrees(n_l, rcv, wt), lab)[1:] + (w,)
        level += 1
        if level == max_levels:
            break
        rcv, snd, wt = aggregate(rcv, snd, wt, dense)
        n_l = len(ids)
        lens = np.bincount(rcv, minlength=n_l).astype(np.int64)
    ids, sizes = np.unique(out["labels"], return_counts=True) if n else (np.zeros(0), np.zeros(0))
    big = int(np.argmax(sizes)) if n else 0
    out["stats"] = dict(zip(STAT_KEYS, (len(ids), int(sizes[big]) if n else 0, int(ids[big]) if n else 0, len(out["maps"]),
                                        s[0], s[1], s[2])))
    return out


def chains(kinds):
    """K of every level's chain of launches (tests/chain_model.py), from the kinds of a run: a SETUP begins a chain; a run without
    a level (max_levels == 0, W == 0) is one chain of SETUP and DONE"""
    out = []
    for k in kinds:
        if k == SETUP:
            out.append(0)
        out[-1] += 1
    return out or [2]


def modularity(r):
    s = r["stats"]
    return 0.0 if s["w"] == 0 else s["s_in"] / s["w"] - s["s_sq"] / (s["w"] * s["w"])
