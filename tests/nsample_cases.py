"""Graphs the neighbour sampling's suites share (tests/test_nsample_cpu.py, tests/test_gpu_nsample.py): the label propagation's
builders, rows of given lengths in a random stored order, and the (d, k) pairs the uniformity checks draw."""
import numpy as np

from tests.lpa_cases import directed, empty, grid, path, random_digraph, random_symmetric, star, sym  # noqa: F401

# rows of d entries sampled k at a time whose inclusion counts were measured
UNIFORM_PAIRS = [(2, 1), (3, 2), (7, 3), (11, 10), (17, 16), (33, 32), (65, 64), (130, 64), (100, 10), (1000, 15)]
WIDTHS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64]


def fan_rows(degrees, seed=0, back=0):
    """vertex i of the first len(degrees) has degrees[i] distinct entries into a pool of max(degrees) further vertices, stored in a
    random order (not ascending); back: every pool vertex has that many entries to the first vertices -> (ro, ci)"""
    rng = np.random.default_rng(seed)
    degrees = np.asarray(degrees, dtype=np.int64)
    rows, pool = len(degrees), max(int(degrees.max(initial=0)), 1)
    ci = [rows + rng.permutation(pool)[:d] for d in degrees]
    ci += [rng.integers(0, rows, back) for _ in range(pool)]
    ro = np.concatenate([[0], np.cumsum(np.concatenate([degrees, np.full(pool, back, dtype=np.int64)]))])
    return ro.astype(np.int32), (np.concatenate(ci) if ci else np.zeros(0)).astype(np.int32)


def width_rows(k):
    """seed rows of k - 1, k, k + 1, 2 k + 1, 1 000 and 100 000 entries -> (ro, ci, the seed rows' degrees)"""
    degrees = [k - 1, k, k + 1, 2 * k + 1, 1000, 100000]
    return fan_rows(degrees, seed=k) + (degrees,)


def directed_path(n):
    """0 -> 1 -> ... -> n - 1"""
    return directed(n, np.arange(n - 1), np.arange(1, n))


def loops_and_duplicates(rows=40, d=12, seed=3):
    """every vertex has a self-loop, an entry stored three times and d random ones"""
    rng = np.random.default_rng(seed)
    v = np.arange(rows)
    src = np.concatenate([v, v, v, v, np.repeat(v, d)])
    dst = np.concatenate([v, (v + 1) % rows, (v + 1) % rows, (v + 1) % rows, rng.integers(0, rows, rows * d)])
    return directed(rows, src, dst)


def bitmap_edges(n=200):
    """the words' first and last bits, as seeds and as destinations: vertex 10 has entries to all of them, each of them one to the
    next -> (ro, ci, those vertices)"""
    edge = np.array([0, 63, 64, 65, 127, 128, n - 1])
    src = np.concatenate([np.full(len(edge), 10), edge])
    dst = np.concatenate([edge, np.roll(edge, -1)])
    return directed(n, src, dst) + (edge,)


def reached_twice():
    """0 -> {1, 2}, 1 -> {2, 3}, 2 -> {3}: vertex 2 is reached at hop 0 and again from 1, vertex 3 at hop 1 twice"""
    return directed(5, np.array([0, 0, 1, 1, 2]), np.array([1, 2, 2, 3, 3]))
