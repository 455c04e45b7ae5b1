"""Graphs the label propagation's suites share (tests/test_lpa_cpu.py, tests/test_gpu_lpa.py): CSR arrays built with
tests/coloring_model.csr (rows and neighbours ascending; `sym`: the swapped copies too, duplicates kept)."""
import numpy as np

from tests import coloring_model as cm


def sym(n, a, b):
    return cm.csr(n, a, b, symmetric=True)


def directed(n, src, dst):
    return cm.csr(n, src, dst, symmetric=False)


def random_pairs(n, m, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n, m), rng.integers(0, n, m)


def random_symmetric(n, m, seed):
    return sym(n, *random_pairs(n, m, seed))


def random_digraph(n, m, seed):
    return directed(n, *random_pairs(n, m, seed))


def empty(n):
    return np.zeros(n + 1, np.int32), np.zeros(0, np.int32)


def clique(k, first=0):
    v = first + np.arange(k)
    a, b = np.meshgrid(v, v, indexing="ij")
    return a[a < b], b[a < b]


def star_pairs(leaves, first=0):
    return np.full(leaves, first, dtype=np.int64), first + 1 + np.arange(leaves)


def star(leaves):
    return sym(leaves + 1, *star_pairs(leaves))


def joined_stars(rows):
    """two stars whose centres are joined: each centre's row has exactly `rows` entries"""
    a, b = star_pairs(rows - 1, first=0)
    a2, b2 = star_pairs(rows - 1, first=rows)
    return sym(2 * rows, np.concatenate([a, a2, [0]]), np.concatenate([b, b2, [rows]]))


def path(n):
    v = np.arange(n - 1)
    return sym(n, v, v + 1)


def grid(w, h):
    v = np.arange(w * h).reshape(h, w)
    return sym(w * h, np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()]), np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()]))


def disjoint(parts):
    """the disjoint union of (vertices, a, b) pair lists, renumbered one behind the other -> symmetric CSR"""
    n, aa, bb = 0, [], []
    for k, a, b in parts:
        aa.append(np.asarray(a) + n)
        bb.append(np.asarray(b) + n)
        n += k
    return sym(n, np.concatenate(aa), np.concatenate(bb))


def cliques_and_stars(votes):
    """for every count c of `votes`: a clique of c + 1 vertices (every vertex has c votes) where that is small, and a star of c
    leaves (its centre has c votes)"""
    parts = []
    for c in votes:
        if c <= 64:
            parts.append((c + 1,) + clique(c + 1))
        parts.append((c + 1,) + star_pairs(c))
    return disjoint(parts)


def multiplicity(dedup=False):
    """vertex 0 has one entry to a = 1 and three to b = 2; 1 and 2 have partners of their own so that nothing else moves first"""
    a = np.array([0, 0, 0, 0])
    b = np.array([1, 2, 2, 2])
    if dedup:
        a, b = a[:2], b[:2]
    return sym(3, a, b)


def tripled_with_loops(ro, ci, every=3):
    n = len(ro) - 1
    src = np.repeat(np.arange(n), np.diff(ro))
    loops = np.arange(0, n, every)
    return directed(n, np.concatenate([src, src, src, loops]), np.concatenate([ci, ci, ci, loops]))


def one_repeated_among_many(distinct=300, repeated=217):
    """vertex 0 with entries to 1 .. distinct, the one to `repeated` twice: under lab_0 its winner has two votes among `distinct`
    labels of one each"""
    b = np.concatenate([1 + np.arange(distinct), [repeated]])
    return sym(distinct + 1, np.zeros(len(b), dtype=np.int64), b)


def planted_blocks(seed, blocks=40, size=50, inside=400, across=300):
    """`blocks` blocks of `size` vertices, `inside` random pairs inside each, `across` random pairs anywhere, ids permuted ->
    (ro, ci, block of every vertex)"""
    rng = np.random.default_rng(seed)
    n = blocks * size
    blk = np.repeat(np.arange(blocks), inside)
    a = blk * size + rng.integers(0, size, len(blk))
    b = blk * size + rng.integers(0, size, len(blk))
    xa, xb = rng.integers(0, n, across), rng.integers(0, n, across)
    ids = rng.permutation(n)
    ro, ci = sym(n, ids[np.concatenate([a, xa])], ids[np.concatenate([b, xb])])
    block = np.empty(n, dtype=np.int64)
    block[ids] = np.arange(n) // size
    return ro, ci, block


def same_partition(labels, block):
    """whether two labellings cut the vertices into the same sets"""
    pairs = np.unique(np.stack([np.asarray(labels, dtype=np.int64), np.asarray(block, dtype=np.int64)]), axis=1)
    return len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))
