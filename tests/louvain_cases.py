"""Graphs the Louvain suites share (tests/test_louvain_cpu.py, tests/test_gpu_louvain.py), beside those of tests/lpa_cases.py: CSR
arrays built with tests/coloring_model.csr (rows and neighbours ascending; symmetric: the swapped copies too, duplicates kept)."""
import numpy as np

from tests import lpa_cases as lc


def star_of_cliques(cliques, size):
    """`cliques` cliques of `size` vertices, one vertex of each joined to a hub (vertex 0): level 0 merges every clique, so the
    coarse hub row has `cliques` entries and every coarse clique a self entry of weight size (size - 1)"""
    aa, bb = [], []
    for c in range(cliques):
        a, b = lc.clique(size, first=1 + c * size)
        aa += [a, [0]]
        bb += [b, [1 + c * size]]
    return lc.sym(1 + cliques * size, np.concatenate(aa), np.concatenate(bb))


def few_large_blocks(seed, blocks=3, size=400, inside=30000, across=600):
    """few, large, dense blocks: their coarse rows hold many members' entries"""
    return lc.planted_blocks(seed, blocks=blocks, size=size, inside=inside, across=across)


def two_triangles():
    """two triangles joined by one edge (2 - 3): the closed form is two communities, Q = 5 / 14"""
    return lc.sym(6, [0, 0, 1, 3, 3, 4, 2], [1, 2, 2, 4, 5, 5, 3])


def tie_square():
    """a 4-cycle: under identity labels both neighbours of every vertex score the same, the key decides"""
    return lc.sym(4, [0, 1, 2, 3], [1, 2, 3, 0])


def loops_and_duplicates():
    """a triangle whose edge 0 - 1 is there three times, self-loops on every vertex, and a pendant vertex"""
    a = np.array([0, 0, 0, 0, 1, 2, 0, 1, 2, 3])
    b = np.array([1, 1, 1, 2, 2, 3, 0, 1, 2, 3])
    return lc.sym(4, a, b)
