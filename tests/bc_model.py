"""The numpy model of the betweenness centrality both GPU paths are compared with: Brandes in the PARITY formulation of
include/mgx/bc_fused.hpp -- no label test per entry.

A CSR entry (u, v) is an edge u -> v; every entry counts once (duplicates are parallel edges, distinct shortest paths); self-loops lie
on no shortest path.  Per source s, with two arrays P[0], P[1] and two arrays Q[0], Q[1], all zero but P[0][s] = 1:
    forward,  d = 1 .. D - 1, v on level d:  P[d & 1][v] = sum over ALL in-entries (u, v) of P[(d - 1) & 1][u]             (= sigma[v])
    the deepest level alone seeds Q[d & 1][v] = 1 / sigma[v]
    backward, d = D - 2 .. 1, v on level d:  delta[v] = sigma[v] * sum over ALL out-entries (v, w) of Q[(d + 1) & 1][w]
                                             Q[d & 1][v] = (1 + delta[v]) / sigma[v];  bc[v] += delta[v]
The sums are sparse matrix-vector products over the level's rows (scipy keeps duplicate entries and adds them)."""
import numpy as np
import scipy.sparse as sp

TWO53 = float(2 ** 53)


def matrices(ro, ci, symmetric):
    """(out-rows, in-rows) as CSR matrices of ones, duplicates kept; the in-rows are the transpose unless `symmetric`"""
    n = len(ro) - 1
    ro, ci = np.asarray(ro, dtype=np.int64), np.asarray(ci, dtype=np.int64)
    out = sp.csr_matrix((np.ones(len(ci), dtype=np.float64), ci, ro), shape=(n, n))
    if symmetric:
        return out, out
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ro))
    order = np.argsort(ci, kind="stable")
    iro = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(ci, minlength=n), out=iro[1:])
    return out, sp.csr_matrix((np.ones(len(ci), dtype=np.float64), rows[order], iro), shape=(n, n))


def bfs(out, s):
    n = out.shape[0]
    label = np.full(n, -1, dtype=np.int32)
    label[s] = 0
    frontier = np.array([s], dtype=np.int64)
    d = 0
    while len(frontier):
        nxt = np.unique(out[frontier].indices)
        nxt = nxt[label[nxt] < 0]
        d += 1
        label[nxt] = d
        frontier = nxt
    return label


def one_source(out, inn, s):
    """labels, sigma, delta of source s"""
    n = out.shape[0]
    label = bfs(out, s)
    D = int(label.max()) + 1
    order = np.argsort(label, kind="stable")
    bounds = np.searchsorted(label[order], np.arange(D + 1))
    level = [order[bounds[d]:bounds[d + 1]] for d in range(D)]
    P = np.zeros((2, n), dtype=np.float64)
    Q = np.zeros((2, n), dtype=np.float64)
    delta = np.zeros(n, dtype=np.float64)
    P[0, s] = 1.0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for d in range(1, D):
            lv = level[d]
            P[d & 1, lv] = inn[lv] @ P[(d - 1) & 1]
            if d == D - 1:
                Q[d & 1, lv] = 1.0 / P[d & 1, lv]
        for d in range(D - 2, 0, -1):
            lv = level[d]
            sig = P[d & 1, lv]
            dl = sig * (out[lv] @ Q[(d + 1) & 1])
            Q[d & 1, lv] = (1.0 + dl) / sig
            delta[lv] = dl
    sigma = np.where(label >= 0, P[label & 1, np.arange(n)], 0.0)
    return label, sigma, delta


def run(ro, ci, sources=None, symmetric=False):
    """-> dict(labels, sigma, delta of the LAST source; bc; stats = [sources, deepest traversal in levels, vertices reached summed,
    inexact, overflow]; longest_in, longest_out; max_sigma over all sources)"""
    n = len(ro) - 1
    out, inn = matrices(ro, ci, symmetric)
    if sources is None:
        sources = np.arange(n)
    bc = np.zeros(n, dtype=np.float64)
    label = np.full(n, -1, dtype=np.int32)
    sigma = np.zeros(n, dtype=np.float64)
    delta = np.zeros(n, dtype=np.float64)
    deepest = reached = inexact = overflow = 0
    max_sigma = 0.0
    for s in sources:
        label, sigma, delta = one_source(out, inn, int(s))
        with np.errstate(invalid="ignore"):
            bc += delta
        deepest = max(deepest, int(label.max()) + 1)
        reached += int((label >= 0).sum())
        finite = np.isfinite(sigma)
        overflow |= int(not finite.all())
        inexact |= int(not finite.all() or (sigma >= TWO53).any())
        max_sigma = max(max_sigma, float(sigma[finite].max()) if finite.any() else 0.0)
    return {"labels": label, "sigma": sigma, "delta": delta, "bc": bc,
            "stats": [len(sources), deepest, reached, inexact, overflow],
            "longest_in": int(np.diff(inn.indptr).max()) if n else 0, "longest_out": int(np.diff(out.indptr).max()) if n else 0,
            "max_sigma": max_sigma}


def dedup(ro, ci):
    """the same graph with every entry once (rows ascending)"""
    n = len(ro) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ro))
    key = np.unique(rows * n + np.asarray(ci, dtype=np.int64))
    r, c = key // n, key % n
    nro = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(r, minlength=n), out=nro[1:])
    return nro, c.astype(np.int32)


def rtol(levels, longest_row, sources):
    """the GPU tests' relative bound on delta and bc between two implementations: every term is non-negative, a level adds at most
    (R + 2) roundings to the relative error, the sum over the sources at most S, two implementations double it"""
    return 2.0 * (levels * (longest_row + 2) + sources) * 2.0 ** -53
