"""numpy model of the minimum spanning forest (include/mgx/mst_fused.hpp): the definition the fused path and the
operator path must both reproduce bit for bit.

    entries:   every CSR entry (v, u, w) is the undirected edge {v, u} of float32 weight w; self-loops are ignored, parallel
               entries are parallel edges, a vertex without entries is a tree of its own
    key(w):    the IEEE bits b of w, -0.0 read as +0.0, mapped monotonically to uint32: b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000);
               a NaN weight is an error
    order:     (key(w), min(v, u), max(v, u)); entries with the same triple are the same edge, so the forest is unique
    result:    the triples (a, b, w), a < b (w reported through its key: -0.0 comes back as +0.0), n - components of them;
               their total in double; label[v] = the smallest vertex id of v's component (tests/cc_model.labels)

kruskal() is the definition itself: the entries sorted by the order, then union-find.  boruvka() is the algorithm both GPU paths
run -- every component takes its lightest outgoing edge, a mutual pair once -- with the fused path's sorted incident arrays and
monotone cursors; it reproduces stats[4] (rounds that chose something) and stats[7] (incident entries without self-loops: both
ends' when symmetric is False).
"""
import numpy as np


def key(w):
    """uint32 keys of float32 weights"""
    b = np.ascontiguousarray(w, dtype=np.float32).view(np.uint32).copy()
    b[b == np.uint32(0x80000000)] = 0
    neg = (b >> np.uint32(31)).astype(bool)
    return np.where(neg, b ^ np.uint32(0xFFFFFFFF), b ^ np.uint32(0x80000000)).astype(np.uint32)


def weight_of_key(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    b = np.where((k & np.uint32(0x80000000)).astype(bool), k ^ np.uint32(0x80000000), ~k).astype(np.uint32)
    return b.view(np.float32)


def has_nan(ro, ci, w):
    """a NaN weight on an entry that is no self-loop"""
    ro = np.asarray(ro, dtype=np.int64)
    rows = np.repeat(np.arange(len(ro) - 1, dtype=np.int64), np.diff(ro))
    cols = np.asarray(ci, dtype=np.int64)[ro[0]:ro[-1]]
    return bool(np.isnan(np.asarray(w, dtype=np.float32)[ro[0]:ro[-1]][rows != cols]).any())


def _entries(ro, ci, w, check=True):
    """(v, u, key) of the entries that are no self-loops"""
    ro = np.asarray(ro, dtype=np.int64)
    n = len(ro) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ro))
    cols = np.asarray(ci, dtype=np.int64)[ro[0]:ro[-1]]
    ww = (np.ones(len(cols), np.float32) if w is None else np.asarray(w, dtype=np.float32)[ro[0]:ro[-1]])
    keep = rows != cols
    if check and np.isnan(ww[keep]).any():
        raise ValueError("a NaN edge weight")
    return rows[keep], cols[keep], key(ww[keep])


def canonical(a, b, w):
    """the triples sorted by (key(w), a, b): (a int32, b int32, w float32 through its key)"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    k = key(w)
    order = np.lexsort((b, a, k))
    return a[order].astype(np.int32), b[order].astype(np.int32), weight_of_key(k[order])


def same_triples(x, y):
    """bit for bit"""
    return all(np.array_equal(np.asarray(p).view(np.uint32) if np.asarray(p).dtype == np.float32 else np.asarray(p),
                              np.asarray(q).view(np.uint32) if np.asarray(q).dtype == np.float32 else np.asarray(q))
               for p, q in zip(x, y))


def _settle(lab):
    while True:
        nxt = lab[lab]
        if np.array_equal(nxt, lab):
            return lab
        lab = nxt


def kruskal(ro, ci, w=None):
    """-> ((a, b, w) canonical, total float, labels int32[n]).  The sorted edges are taken in blocks: the edges of a block whose
    ends the blocks before have joined are dropped at once, the others go through a plain union-find one by one."""
    n = len(ro) - 1
    v, u, k = _entries(ro, ci, w)
    a, b = np.minimum(v, u), np.maximum(v, u)
    order = np.lexsort((b, a, k))
    a, b, k = a[order], b[order], k[order]
    parent = list(range(n))
    take = []
    lab = np.arange(n, dtype=np.int64)
    block = max(n, 1024)
    idx = np.arange(len(a), dtype=np.int64)
    while len(idx):
        head, idx = idx[:block], idx[block:]
        for i, x, y in zip(head.tolist(), a[head].tolist(), b[head].tolist()):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            while parent[y] != y:
                parent[y] = parent[parent[y]]
                y = parent[y]
            if x != y:
                if x < y:
                    parent[y] = x
                else:
                    parent[x] = y
                take.append(i)
        lab = _settle(np.array(parent, dtype=np.int64))
        parent = lab.tolist()
        if len(idx):
            idx = idx[lab[a[idx]] != lab[b[idx]]]
        block *= 2
    take = np.array(take, dtype=np.int64)
    wa = weight_of_key(k[take])
    return ((a[take].astype(np.int32), b[take].astype(np.int32), wa), float(np.sum(wa.astype(np.float64))),
            lab.astype(np.int32))


def boruvka(ro, ci, w=None, symmetric=True):
    """-> {"edges": (a, b, w) canonical, "total", "labels", "rounds": stats[4], "entries": stats[7], "left": per round that makes
    a work list (the one that chooses nothing included) every row's entries from its cursor on}.  The incident array of v
    holds its out-entries -- and, symmetric False, its in-entries -- as (key, neighbour) ascending; a cursor per vertex stands
    at its first entry that may still leave its component."""
    n = len(ro) - 1
    v, u, k = _entries(ro, ci, w)
    if not symmetric:
        v, u, k = np.concatenate([v, u]), np.concatenate([u, v]), np.concatenate([k, k])
    order = np.lexsort((u, k, v))
    v, u, k = v[order], u[order], k[order]
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(v, minlength=n), out=off[1:])
    pos = np.arange(len(v), dtype=np.int64)
    cur = off[:-1].copy()
    lab = np.arange(n, dtype=np.int64)
    big = np.int64(len(v))
    chosen = []
    rounds = 0
    rows = np.nonzero(np.diff(off) > 0)[0]
    left = []
    while True:
        left.append(off[1:] - cur)
        leaves = lab[v] != lab[u]
        first = np.full(n, big, dtype=np.int64)
        if len(rows):
            first[rows] = np.minimum.reduceat(np.where(leaves, pos, big), off[rows])
        first = np.where(first < off[1:], first, off[1:])          # (reduceat of the last rows: stay inside the row)
        assert (first >= cur).all(), "an entry behind a cursor left its component"
        cur = first
        live = np.nonzero(cur < off[1:])[0]
        if not len(live):
            break
        p = cur[live]
        r = lab[live]
        cw = np.full(n, np.uint32(0xFFFFFFFF), dtype=np.uint32)
        np.minimum.at(cw, r, k[p])
        light = k[p] == cw[r]
        pair = (np.minimum(live, u[p]).astype(np.uint64) << np.uint64(32)) | np.maximum(live, u[p]).astype(np.uint64)
        cp = np.full(n, np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
        np.minimum.at(cp, r[light], pair[light])
        roots = np.unique(r)
        trip = np.unique(np.stack([cw[roots].astype(np.uint64), cp[roots]], axis=1), axis=0)    # a mutual pair once
        ka = trip[:, 0].astype(np.uint32)
        ea, eb = (trip[:, 1] >> np.uint64(32)).astype(np.int64), (trip[:, 1] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        chosen.append((ea, eb, ka))
        rounds += 1
        while True:                                                # hook the larger label under the smaller, settle, repeat
            la, lb = lab[ea], lab[eb]
            diff = la != lb
            if not diff.any():
                break
            np.minimum.at(lab, np.maximum(la[diff], lb[diff]), np.minimum(la[diff], lb[diff]))
            lab = _settle(lab)
    if chosen:
        ea, eb, ka = (np.concatenate([c[i] for c in chosen]) for i in range(3))
    else:
        ea, eb, ka = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint32)
    edges = canonical(ea, eb, weight_of_key(ka))
    return {"edges": edges, "total": float(np.sum(edges[2].astype(np.float64))), "labels": lab.astype(np.int32), "rounds": rounds,
            "entries": int(len(v)), "left": left}


def total_bound(w):
    """what a double sum of these float weights may differ by from another order's: (edges - 1) * 2^-53 * sum |w|"""
    w = np.asarray(w, dtype=np.float64)
    return max(len(w) - 1, 0) * 2.0 ** -53 * float(np.abs(w).sum())
