"""Graphs the strongly connected components' suites share (tests/test_scc_cpu.py, tests/test_gpu_scc.py): CSR arrays of directed
graphs, built with tests/coloring_model.csr (rows and neighbours ascending, nothing mirrored)."""
import numpy as np

from tests import coloring_model as cm


def directed(n, src, dst):
    return cm.csr(n, src, dst, symmetric=False)


def random_digraph(n, m, seed):
    rng = np.random.default_rng(seed)
    return directed(n, rng.integers(0, n, m), rng.integers(0, n, m))


def planted(nc, maxsz, cross, seed, chords=0):
    """nc rings of random size 2 .. maxsz, `chords` random arcs inside each (they cut the diameter), ids permuted; `cross` random
    arcs, each directed along ONE random order of the components, so none closes a cycle.  -> (ro, ci, the planted labels)"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, maxsz + 1, nc)
    n = int(sizes.sum())
    comp = np.repeat(np.arange(nc), sizes)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    pos = np.arange(n) - first[comp]
    src = [np.arange(n)]
    dst = [first[comp] + (pos + 1) % sizes[comp]]
    if chords:
        c = np.repeat(np.arange(nc), chords)
        src.append(first[c] + rng.integers(0, 1 << 30, len(c)) % sizes[c])
        dst.append(first[c] + rng.integers(0, 1 << 30, len(c)) % sizes[c])
    rank = rng.permutation(nc)                                   # the order the cross arcs follow
    a, b = rng.integers(0, n, cross), rng.integers(0, n, cross)
    keep = comp[a] != comp[b]
    a, b = a[keep], b[keep]
    swap = rank[comp[a]] > rank[comp[b]]
    src.append(np.where(swap, b, a))
    dst.append(np.where(swap, a, b))
    ids = rng.permutation(n)
    s, d = ids[np.concatenate(src)], ids[np.concatenate(dst)]
    lowest = np.full(nc, n, dtype=np.int64)
    np.minimum.at(lowest, comp, ids)
    labels = np.empty(n, dtype=np.int32)
    labels[ids] = lowest[comp]
    ro, ci = directed(n, s, d)
    return ro, ci, labels


def cycle_chain(k, ascending=True):
    """2-cycles {2i, 2i + 1} chained by arcs 2i + 1 -> 2i + 2 (ascending: colour 0 floods everything, a round finds one cycle)
    or 2i + 2 -> 2i + 1 (descending: one round finds them all)"""
    i = np.arange(k)
    j = np.arange(k - 1)
    a, b = (2 * j + 1, 2 * j + 2) if ascending else (2 * j + 2, 2 * j + 1)
    return directed(2 * k, np.concatenate([2 * i, 2 * i + 1, a]), np.concatenate([2 * i + 1, 2 * i, b]))


def fan(k):
    """0 <-> 1, 1 -> a_i, a_i <-> b_i (a_i = 2 + 2i, b_i = 3 + 2i): vertex 1 is the pivot, its sweep lowers all k a_i in one
    launch, and one round takes all k cycles"""
    a = 2 + 2 * np.arange(k)
    one = np.ones(k, dtype=np.int64)
    return directed(2 + 2 * k, np.concatenate([[0, 1], one, a, a + 1]), np.concatenate([[1, 0], a, a + 1, a]))


def layered_trim(k):
    """s -> a_1 .. a_k, every a_i -> c, c <-> d (s = 0, a_i = i, c = k + 1, d = k + 2): the first trim front is s alone, the
    front its expand appends is exactly the k a_i; the 2-cycle stays for the pivot phase"""
    a = 1 + np.arange(k)
    c, d = k + 1, k + 2
    return directed(k + 3, np.concatenate([np.zeros(k, dtype=np.int64), a, [c, d]]), np.concatenate([a, np.full(k, c), [d, c]]))


def ring(n):
    v = np.arange(n)
    return directed(n, v, (v + 1) % n)


def path(n):
    v = np.arange(n - 1)
    return directed(n, v, v + 1)


def star(leaves, out=True, back=True):
    """centre 0; out: 0 -> leaf, back: leaf -> 0"""
    l = 1 + np.arange(leaves)
    z = np.zeros(leaves, dtype=np.int64)
    src = np.concatenate(([z] if out else []) + ([l] if back else []))
    dst = np.concatenate(([l] if out else []) + ([z] if back else []))
    return directed(leaves + 1, src, dst)
