"""numpy model of the local sparsification (include/mgx/lspar_fused.hpp): the definition the fused path and the
operator path must both reproduce bit for bit.

    salt_j = fmix32(seed + 0x9E3779B9 * (j + 1)),  h_j(u) = fmix32(u ^ salt_j)     (colouring's keys, uint32)
    mh_j(v) = min of h_j(u) over the entries u of row v (0xFFFFFFFF: empty row)
    sim(p)  = |{ j : mh_j(v) == mh_j(u) }| for entry p of row v, neighbour u
    t(v)    = min(d, floor(pow(d, e) * (1 + 2^-40))), float64
    row v keeps its first t(v) entries in the order (sim descending, position ascending), written in row order.
"""
import numpy as np

from tests.coloring_model import csr, keys, salt  # noqa: F401  (csr: re-exported for the tests)

SEED = 15485863
K = 1
E = 0.5
GUARD = 1.0 + 2.0 ** -40


def keep_count(d, e):
    d = np.asarray(d, dtype=np.int64)
    with np.errstate(over="ignore"):
        p = np.power(d.astype(np.float64), float(e)) * GUARD
    t = np.where(p < d, np.floor(np.where(p < d, p, 0.0)), d)
    return np.where(d <= 0, 0, t).astype(np.int64)


def minhashes(row_offsets, col_indices, seed=SEED, k=K):
    ro = np.asarray(row_offsets, dtype=np.int64)
    ci = np.asarray(col_indices, dtype=np.int64)
    n = len(ro) - 1
    mh = np.full((n, k), 0xFFFFFFFF, dtype=np.uint32)
    rows = np.diff(ro) > 0
    if rows.any():
        starts = ro[:-1][rows] - ro[0]
        for j in range(k):
            h = keys(n, salt(seed, j))
            mh[rows, j] = np.minimum.reduceat(h[ci[ro[0]:ro[-1]]], starts)
    return mh


def sparsify(row_offsets, col_indices, seed=SEED, k=K, e=E):
    """-> (out_ro, out_ci, out_eid, out_sim, minhashes (n, k) uint32)"""
    ro = np.asarray(row_offsets, dtype=np.int64)
    ci = np.asarray(col_indices, dtype=np.int64)
    n, m = len(ro) - 1, int(ro[-1])
    d = np.diff(ro)
    mh = minhashes(ro, ci, seed, k)
    rows = np.repeat(np.arange(n, dtype=np.int64), d)
    sim = (mh[rows] == mh[ci]).sum(axis=1).astype(np.int64) if m else np.zeros(0, np.int64)
    t = keep_count(d, e)
    pos = np.arange(m, dtype=np.int64) - ro[rows]
    order = np.lexsort((pos, -sim, rows))                      # rows ascending, sim descending, position ascending
    rank = np.empty(m, dtype=np.int64)
    rank[order] = np.arange(m, dtype=np.int64) - ro[rows[order]]
    eid = np.nonzero(rank < t[rows])[0]
    out_ro = np.concatenate([[0], np.cumsum(t)]).astype(np.int32)
    return out_ro, ci[eid].astype(np.int32), eid.astype(np.int32), sim[eid].astype(np.int32), mh


def brute_force(row_offsets, col_indices, seed=SEED, k=K, e=E):
    """the definition as a plain Python loop (small graphs only)"""
    import math
    ro = [int(x) for x in row_offsets]
    ci = [int(x) for x in col_indices]
    n = len(ro) - 1

    def fmix(h):
        h &= 0xFFFFFFFF
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        h ^= h >> 16
        return h

    salts = [fmix(seed + 0x9E3779B9 * (j + 1)) for j in range(k)]
    mh = [[min([fmix(u ^ s) for u in ci[ro[v]:ro[v + 1]]], default=0xFFFFFFFF) for s in salts] for v in range(n)]
    out_ro, out_ci, out_eid, out_sim = [0], [], [], []
    for v in range(n):
        dd = ro[v + 1] - ro[v]
        t = 0 if dd == 0 else min(dd, math.floor(math.pow(dd, e) * GUARD))
        ent = [(sum(mh[v][j] == mh[ci[p]][j] for j in range(k)), p) for p in range(ro[v], ro[v + 1])]
        chosen = sorted(sorted(ent, key=lambda x: (-x[0], x[1]))[:t], key=lambda x: x[1])
        for s, p in chosen:
            out_ci.append(ci[p])
            out_eid.append(p)
            out_sim.append(s)
        out_ro.append(out_ro[-1] + t)
    return out_ro, out_ci, out_eid, out_sim, mh
