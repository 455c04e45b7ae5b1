"""Graphs the random walks' suites share (tests/test_rw_cpu.py, tests/test_gpu_rw.py): the label propagation's and the multi-source
BFS's builders, weights for their entries, and rows in an order other than ascending."""
import numpy as np

from tests.lpa_cases import (clique, directed, empty, grid, path, random_digraph, random_symmetric, star, sym)  # noqa: F401
from tests.msbfs_cases import complete, cuts, fans, with_isolated  # noqa: F401


def weights(ci, seed, zeros=0.0):
    """float32 weights k / 8, k in 1 .. 64, for the entries (exact in float32, so are their products with 2^-k); a share `zeros` of
    them 0.0"""
    rng = np.random.default_rng(seed)
    w = rng.integers(1, 65, len(ci)).astype(np.float32) / np.float32(8)
    if zeros:
        w[rng.random(len(ci)) < zeros] = 0.0
    return w


def descending(ro, ci, w=None):
    """the same graph with every row stored in descending order (and its weights with it)"""
    ro, ci = np.asarray(ro), np.asarray(ci).copy()
    w = None if w is None else np.asarray(w).copy()
    for v in range(len(ro) - 1):
        ci[ro[v]:ro[v + 1]] = ci[ro[v]:ro[v + 1]][::-1]
        if w is not None:
            w[ro[v]:ro[v + 1]] = w[ro[v]:ro[v + 1]][::-1]
    return (ro, ci) if w is None else (ro, ci, w)


def triangle_with_tail():
    """0 - 1 - 2 - 0 and 2 - 3: from prev = 0 at cur = 2 a step returns (0), stays near (1) or moves away (3)"""
    return sym(4, np.array([0, 1, 2, 2]), np.array([1, 2, 0, 3]))


def one_row(weights_of_row):
    """vertex 0 with an entry to each of 1 .. k carrying the given weights, every leaf with an entry back (weight 1)
    -> (ro, ci, w)"""
    k = len(weights_of_row)
    ro = np.concatenate([[0, k], k + 1 + np.arange(k)]).astype(np.int32)
    ci = np.concatenate([1 + np.arange(k), np.zeros(k, dtype=np.int64)]).astype(np.int32)
    w = np.concatenate([np.asarray(weights_of_row, dtype=np.float32), np.ones(k, dtype=np.float32)])
    return ro, ci, w


def prev_rows(lengths, seed=0):
    """for every length r a hub h whose out-row has exactly r distinct entries among a common pool of vertices (and, where r >= 2,
    one of them twice: duplicates), every pool vertex with entries to every hub, to pool vertices below and above every row's range,
    and to itself: a second-order step from (prev = h, cur = pool vertex) asks for candidates that are h itself, absent below,
    absent above, absent between two entries, the row's first and its last entry -> (ro, ci, hubs)"""
    rng = np.random.default_rng(seed)
    pool = 2 * max(lengths) + 8
    hubs = pool + np.arange(len(lengths))
    src, dst = [], []
    for h, r in zip(hubs, lengths):
        row = 2 + 2 * np.sort(rng.choice(max(lengths) + 1, r, replace=False))          # even pool ids in [2, pool - 4]
        src += [np.full(r, h)]
        dst += [row]
        if r >= 2:
            src += [np.array([h])]
            dst += [row[r // 2:r // 2 + 1]]
    pv = np.arange(pool)
    for h in hubs:
        src += [pv]
        dst += [np.full(pool, h)]
    src += [pv, pv, pv, pv]
    dst += [np.zeros(pool, dtype=np.int64), np.full(pool, pool - 1), (pv + 1) % pool, pv]
    ro, ci = directed(pool + len(lengths), np.concatenate(src), np.concatenate(dst))
    return ro, ci, hubs
