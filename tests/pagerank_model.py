"""numpy model of PageRank (include/mgx/pagerank_fused.hpp), float64: the definition the fused path and the operator
path must both reproduce.

    CSR entry (u, v) is an edge u -> v; duplicates count once each, self-loops count; d(u) = length of row u; n vertices

    r_0[v]     = 1 / n
    D_t        = sum of r_t[u] over the u with d(u) = 0                     (dangling mass)
    S_t[v]     = sum of r_t[u] / d(u) over the entries (u, v)               (in-entries of v, with multiplicity)
    r_{t+1}[v] = (1 - alpha) / n + alpha * (S_t[v] + D_t / n)
    e_{t+1}    = sum over v of | r_{t+1}[v] - r_t[v] |                      (L1 residual)

    stop after the first iteration t + 1 with e_{t+1} <= tol, or after max_iter iterations.

symmetric=True is the caller's word that every entry has its reverse: the in-entries of v are then read from row v of the CSR
(on a graph that is not symmetric this is a different, wrong, matrix -- as in the library).  symmetric=False transposes.
networkx.pagerank without personalisation is the same iteration, stopped at e < n * tol.
"""
import numpy as np


def in_entries(ro, ci, symmetric):
    """(target v, source u) of every in-entry"""
    ro = np.asarray(ro, dtype=np.int64)
    ci = np.asarray(ci, dtype=np.int64)
    n = len(ro) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ro))
    return (rows, ci) if symmetric else (ci, rows)


def step(ro, ci, r, alpha, symmetric):
    """one iteration from the ranks r -> (the next ranks, the residual)"""
    ro = np.asarray(ro, dtype=np.int64)
    n = len(ro) - 1
    d = np.diff(ro)
    r = np.asarray(r, dtype=np.float64)
    tgt, src = in_entries(ro, ci, symmetric)
    contrib = np.zeros(n, dtype=np.float64)
    np.divide(r, d, out=contrib, where=d > 0)
    D = r[d == 0].sum()
    S = np.bincount(tgt, weights=contrib[src], minlength=n)
    nxt = (1.0 - alpha) / n + alpha * (S + D / n)
    return nxt, float(np.abs(nxt - r).sum())


def ranks(ro, ci, alpha=0.85, tol=1e-6, max_iter=100, symmetric=False):
    """-> (r float64[n], residuals e_1 .. e_T float64[T])"""
    n = len(ro) - 1
    r = np.full(n, 1.0 / n, dtype=np.float64) if n else np.zeros(0)
    res = []
    for _ in range(max_iter if n else 0):
        r, e = step(ro, ci, r, alpha, symmetric)
        res.append(e)
        if e <= tol:
            break
    return r, np.array(res, dtype=np.float64)
