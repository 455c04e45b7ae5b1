"""numpy model of the k-truss decomposition (include/mgx/ktruss_fused.hpp): the definition the fused path and the
operator path must both reproduce exactly.

    graph:      the underlying simple undirected graph of tests/tc_model.py; its edges are the entries of that model's DAG: edge e =
                position e of dag_ci, joining row src[e] to dag_ci[e]
    adjacency:  adj_ro[n + 1], adj_ci[2 m], adj_eid[2 m]: row v = the simple neighbours of v ascending, each with its edge's id
    sup0[e]:    the triangles that contain e (int32)
    peel:       loop: no edge alive: stop.  k = 2 + min(sup over alive edges).  front = { alive e : sup[e] <= k - 2 }
                      while the front is not empty (one PASS):
                          every triangle with an edge in the front and none removed: with one edge in the front the other two lose
                          1, with two the third loses 1 ONCE, with three nothing
                          truss[front] = k; the front is removed
                          front = the alive edges whose sup this pass took from > k - 2 to <= k - 2
    vtruss[v]:  the largest trussness of an edge at v, 0 if there is none (int32); hist[k]: the edges of trussness k (int64)
    stats:      [0] the largest trussness (0 without edges), [1] m, [2] triangles, [3] levels, [4] passes

The rule is simultaneous, so the supports after every pass, and with them levels and passes, are unique.  The triangles are
enumerated once, as triples of edge ids, from the DAG's wedges (pairs of entries of one row, closed by a third entry); a triangle is
looked at once more, in the pass in which its first edge leaves.
"""
import numpy as np

from tests import tc_model

STAT_KEYS = ("max_truss", "edges", "triangles", "levels", "passes")


def adjacency(dag_ro, dag_ci):
    """-> (src int32[m], adj_ro int32[n + 1], adj_ci int32[2 m], adj_eid int32[2 m])"""
    ro = np.asarray(dag_ro, dtype=np.int64)
    n, m = len(ro) - 1, len(dag_ci)
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(ro))
    dst = np.asarray(dag_ci, dtype=np.int64)
    rows, cols = np.concatenate([src, dst]), np.concatenate([dst, src])
    eid = np.concatenate([np.arange(m), np.arange(m)])
    perm = np.lexsort((cols, rows))
    adj_ro = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=adj_ro[1:])
    return src.astype(np.int32), adj_ro.astype(np.int32), cols[perm].astype(np.int32), eid[perm].astype(np.int32)


def triangles(dag_ro, dag_ci):
    """-> int64[T, 3]: the edge ids of every triangle, each triangle once"""
    ro = np.asarray(dag_ro, dtype=np.int64)
    ci = np.asarray(dag_ci, dtype=np.int64)
    n, m = len(ro) - 1, len(ci)
    if m == 0:
        return np.zeros((0, 3), dtype=np.int64)
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(ro))
    key = np.minimum(src, ci) * n + np.maximum(src, ci)            # every simple edge once: its id by its pair
    by_key = np.argsort(key)
    sorted_key = key[by_key]
    d = np.diff(ro)
    out = []
    for deg in np.unique(d[d >= 2]):
        rows = np.flatnonzero(d == deg)
        i, j = np.triu_indices(int(deg), 1)
        for lo in range(0, len(rows), max(1, (1 << 22) // len(i))):          # (chunks of about 4 M wedges)
            r = rows[lo:lo + max(1, (1 << 22) // len(i))]
            e1 = (ro[r][:, None] + i[None, :]).ravel()
            e2 = (ro[r][:, None] + j[None, :]).ravel()
            b, c = ci[e1], ci[e2]
            want = np.minimum(b, c) * n + np.maximum(b, c)
            at = np.minimum(np.searchsorted(sorted_key, want), m - 1)
            hit = sorted_key[at] == want
            out.append(np.stack([e1[hit], e2[hit], by_key[at[hit]]], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 3), dtype=np.int64)


def peel(m, tri, sup0):
    """-> (truss int32[m], fronts: the edge ids of every pass's front as a list of arrays, levels, passes)"""
    sup = sup0.astype(np.int64).copy()
    state = np.zeros(m, dtype=np.int8)                              # 0 alive, 1 front, 2 removed
    truss = np.zeros(m, dtype=np.int32)
    T = len(tri)
    flat = tri.ravel()
    inc_t = np.repeat(np.arange(T), 3)[np.argsort(flat, kind="stable")]       # the triangles of edge e: inc_t[inc_ro[e] : inc_ro[e + 1]]
    inc_ro = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(flat, minlength=m), out=inc_ro[1:])
    live = np.ones(T, dtype=bool)                                   # no edge of the triangle has left
    fronts, levels, passes, left = [], 0, 0, m
    while left > 0:
        alive = state == 0
        k = 2 + int(sup[alive].min())
        front = np.flatnonzero(alive & (sup <= k - 2))
        levels += 1
        while len(front):
            passes += 1
            state[front] = 1
            cnt = inc_ro[front + 1] - inc_ro[front]
            at = np.repeat(inc_ro[front] - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt) + np.arange(int(cnt.sum()))
            ts = np.unique(inc_t[at])
            ts = ts[live[ts]]
            tt = tri[ts]
            in_front = state[tt] == 1
            dec = tt[~in_front & (in_front.sum(axis=1) < 3)[:, None]]       # one in the front: the other two; two: the third, once
            np.subtract.at(sup, dec, 1)
            live[ts] = False
            truss[front] = k
            state[front] = 2
            fronts.append(front)
            left -= len(front)
            cand = np.unique(dec)
            front = cand[(state[cand] == 0) & (sup[cand] <= k - 2)]
    return truss, fronts, levels, passes


def decompose(row_offsets, col_indices, symmetric):
    """-> {"dag_ro", "dag_ci", "src", "adj_ro", "adj_ci", "adj_eid", "sup0", "truss", "vtruss", "hist", "fronts", "stats",
           "u", "v", "perm"}: u < v sorted by (u, v) is the canonical edge order, perm takes DAG order to it"""
    dag_ro, dag_ci, _ = tc_model.dag(row_offsets, col_indices, symmetric)
    n, m = len(dag_ro) - 1, len(dag_ci)
    src, adj_ro, adj_ci, adj_eid = adjacency(dag_ro, dag_ci)
    tri = triangles(dag_ro, dag_ci)
    sup0 = np.bincount(tri.ravel(), minlength=m).astype(np.int32)
    truss, fronts, levels, passes = peel(m, tri, sup0)
    vtruss = np.zeros(n, dtype=np.int32)
    np.maximum.at(vtruss, src, truss)
    np.maximum.at(vtruss, dag_ci, truss)
    top = int(truss.max()) if m else 0
    hist = np.bincount(truss, minlength=top + 1).astype(np.int64) if m else np.zeros(1, dtype=np.int64)
    u, v = np.minimum(src, dag_ci), np.maximum(src, dag_ci)
    perm = np.lexsort((v, u))
    stats = {"max_truss": top, "edges": m, "triangles": len(tri), "levels": levels, "passes": passes}
    return {"dag_ro": dag_ro, "dag_ci": dag_ci, "src": src, "adj_ro": adj_ro, "adj_ci": adj_ci, "adj_eid": adj_eid, "sup0": sup0,
            "truss": truss, "vtruss": vtruss, "hist": hist, "fronts": fronts, "stats": stats, "u": u[perm].astype(np.int32),
            "v": v[perm].astype(np.int32), "perm": perm}


MIN, LIST, EXPAND, SEAL, IDLE = 1, 2, 3, 4, 5                      # ktruss_kind_t


def peel_kinds(w):
    """the kinds of the fused peel's launches up to and including the first idle one, from decompose's result: a level (the
    fronts of one trussness) is MIN, LIST, SEAL, then EXPAND, SEAL per pass; behind the last level MIN finds nobody alive"""
    kinds, level = [], None
    for front in w["fronts"]:
        k = int(w["truss"][front[0]])
        if k != level:
            kinds += [MIN, LIST, SEAL]
            level = k
        kinds += [EXPAND, SEAL]
    return kinds + [MIN, IDLE]


def peel_launches(stats):
    """K of the fused peel's chain (tests/chain_model.py), by the kind rule of k_ktruss_step: every level is MIN, LIST and the SEAL
    that makes the listed edges the front, every pass an EXPAND and the SEAL behind it (the level's last one finds no new front,
    and MIN follows); then the MIN that finds nobody alive, and DONE"""
    return 3 * stats["levels"] + 2 * stats["passes"] + 2


def truss_edge_set(r, k):
    """the pairs (u, v), u < v, of the edges of trussness >= k"""
    keep = r["truss"][r["perm"]] >= k
    return set(zip(r["u"][keep].tolist(), r["v"][keep].tolist()))
