"""Hand-made graphs of the k-truss tests (tests/test_ktruss_cpu.py, tests/test_gpu_ktruss.py), as CSR from tests/coloring_model.csr,
each with what the decomposition of it is in closed form."""
import numpy as np

from tests import coloring_model as cm


def pairs_of(ids):
    x, y = np.meshgrid(ids, ids, indexing="ij")
    return x[x < y], y[x < y]


def cliques(groups, n):
    """the union of the cliques on the given id arrays (they may share vertices) on n vertices"""
    s, d = zip(*(pairs_of(np.asarray(g)) for g in groups))
    return cm.csr(n, np.concatenate(s), np.concatenate(d))


def clique_chain(lo, hi, seed=None):
    """the disjoint union of K_lo .. K_hi (ids shuffled with a seed): hi - lo + 1 levels (K_2 and K_3 ... each their own), a pass each"""
    sizes = np.arange(lo, hi + 1)
    n = int(sizes.sum())
    ids = np.arange(n) if seed is None else np.random.default_rng(seed).permutation(n)
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    return cliques([ids[cuts[i]:cuts[i + 1]] for i in range(len(sizes))], n)


def two_cliques_sharing_an_edge(p, q, seed=None, extra=0):
    """K_p and K_q with one common edge (ids[0], ids[1]) -> (ro, ci, ids)"""
    n = p + q - 2 + extra
    ids = np.arange(n) if seed is None else np.random.default_rng(seed).permutation(n)
    ro, ci = cliques([ids[:p], np.concatenate([ids[:2], ids[p:p + q - 2]])], n)
    return ro, ci, ids


def disjoint_triangles(t, seed=None, extra=0):
    n = 3 * t + extra
    ids = np.arange(n) if seed is None else np.random.default_rng(seed).permutation(n)
    x, y, z = ids[0:3 * t:3], ids[1:3 * t:3], ids[2:3 * t:3]
    return cm.csr(n, np.concatenate([x, y, z]), np.concatenate([y, z, x]))


def grid(w, h, diagonals):
    """the w x h grid graph; diagonals: plus one diagonal per cell (every edge trussness 3, one level, min(w, h) passes)"""
    v = np.arange(w * h).reshape(h, w)
    s = [v[:, :-1].ravel(), v[:-1, :].ravel()]
    d = [v[:, 1:].ravel(), v[1:, :].ravel()]
    if diagonals:
        s.append(v[:-1, :-1].ravel())
        d.append(v[1:, 1:].ravel())
    return cm.csr(w * h, np.concatenate(s), np.concatenate(d))


def star(leaves, centre):
    n = leaves + 1
    others = np.setdiff1d(np.arange(n), [centre])
    return cm.csr(n, np.full(leaves, centre), others)
