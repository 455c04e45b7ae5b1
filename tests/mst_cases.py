"""The hand-made inputs of the minimum spanning forest's GPU suite (tests/test_gpu_mst.py), by name, so that the CPU suite
(tests/test_mst_cpu.py) can hold the two models against each other on the very same graphs.  Every case is
(row_offsets int32, col_indices int32, weights float32, symmetric): symmetric says whether every entry has its reverse with the
same weight (the word the GPU test hands to the library; False runs need the CSC)."""
import numpy as np


def wcsr(n, src, dst, w, symmetric=True):
    """weighted CSR of the entries (row src, neighbour dst, weight w), rows and neighbours ascending (stable); symmetric: the
    swapped copies, with the same weights, too"""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    w = np.broadcast_to(np.asarray(w, dtype=np.float32), src.shape).copy()
    if symmetric:
        src, dst, w = np.concatenate([src, dst]), np.concatenate([dst, src]), np.concatenate([w, w])
    order = np.lexsort((dst, src))
    ro = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=ro[1:])
    return ro.astype(np.int32), dst[order].astype(np.int32), w[order].astype(np.float32)


def no_entries(n):
    return np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), True


def self_loops_only(n=3000):
    v = np.arange(n)
    return wcsr(n, v, v, 3.0, symmetric=False) + (True,)


def ring(n=1000):
    v = np.arange(n)
    return wcsr(n, v, (v + 1) % n, 1.0) + (True,)


def grid(rows=64, cols=64):
    v = np.arange(rows * cols)
    r, c = v // cols, v % cols
    right, down = v[c + 1 < cols], v[r + 1 < rows]
    return wcsr(rows * cols, np.concatenate([right, down]), np.concatenate([right + 1, down + cols]), 1.0) + (True,)


def clique(k=300):
    s, d = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
    m = s < d
    return wcsr(k, s[m], d[m], 1.0) + (True,)


def shuffled_path(n=200000, seed=8):
    p = np.random.default_rng(seed).permutation(n)
    return wcsr(n, p[:-1], p[1:], 1.0) + (True,)


def increasing_path(n=4096, seed=9):
    """weights 1, 2, 3, .. along a path whose ids are shuffled"""
    p = np.random.default_rng(seed).permutation(n)
    return wcsr(n, p[:-1], p[1:], np.arange(1, n, dtype=np.float32)) + (True,)


def star(centre, weights, leaves=100000, seed=6):
    """weights: "equal", or "random" (float32 in [0, 1): the totals are compared within the summation bound)"""
    n = leaves + 1
    lv = np.setdiff1d(np.arange(n), [centre])
    w = 1.0 if weights == "equal" else np.random.default_rng(seed).random(leaves, dtype=np.float32)
    return wcsr(n, np.full(leaves, centre), lv, w) + (True,)


def two_cliques(symmetric, k=300, seed=2):
    """two cliques of k (weights 1 .. 7) on shuffled ids, joined by one entry of weight 1000"""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(2 * k + 50)
    a, b = ids[:k], ids[k:2 * k]
    s, d = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
    m = s < d
    w = rng.integers(1, 8, int(m.sum())).astype(np.float32)
    src = np.concatenate([a[s[m]], b[s[m]]])
    dst = np.concatenate([a[d[m]], b[d[m]]])
    ww = np.concatenate([w, w])
    src, dst, ww = np.concatenate([src, dst]), np.concatenate([dst, src]), np.concatenate([ww, ww])     # the cliques, both ways
    bs, bd, bw = [a[5]], [b[7]], [1000.0]
    if symmetric:
        bs, bd, bw = [a[5], b[7]], [b[7], a[5]], [1000.0, 1000.0]
    return wcsr(len(ids), np.concatenate([src, bs]), np.concatenate([dst, bd]), np.concatenate([ww, bw]), symmetric=False) + (symmetric,)


def parallel_entries():
    """the pair {1, 4} three times with three weights, among a few others"""
    src = [1, 1, 1, 0, 2, 3, 4]
    dst = [4, 4, 4, 1, 3, 4, 5]
    w = [5.0, 2.0, 9.0, 2.0, 2.0, 7.0, 1.0]
    return wcsr(6, src, dst, w) + (True,)


def special_weights():
    """negatives, -0.0 beside +0.0, FLT_MAX and -FLT_MAX, a denormal"""
    fmax = np.finfo(np.float32).max
    src = [0, 1, 2, 3, 4, 5, 0, 2, 6, 7, 1, 8]
    dst = [1, 2, 3, 4, 5, 0, 3, 5, 7, 8, 6, 0]
    w = [-1.5, -0.0, 0.0, fmax, -fmax, 2.0, -0.0, 0.0, 1e-40, -2.5, -1.5, fmax]
    return wcsr(9, src, dst, w) + (True,)


def one_nan():
    ro, ci, w, _ = ring(100)
    w = w.copy()
    w[37] = np.nan
    return ro, ci, w, True                                        # (the reverse entry keeps its 1.0: the run must fail anyway)


def small_components(symmetric, count=10000, seed=10):
    """`count` components of 2 - 5 vertices, a random tree each, weights 0 .. 3"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, 6, count)
    n = int(sizes.sum())
    ids = rng.permutation(n)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    s, d = [], []
    for st, sz in zip(starts, sizes):
        for j in range(1, sz):
            s.append(ids[st + j])
            d.append(ids[st + rng.integers(0, j)])
    w = rng.integers(0, 4, len(s)).astype(np.float32)
    return wcsr(n, s, d, w, symmetric=symmetric) + (symmetric,)


def work_list_edges(seg=2048, seed=12):
    """k_mst_worklist at its edges (include/mgx/mst_fused.hpp; MST_SEG_DEFAULT entries a window, a wave's stage holds 128 rows):
    three rings of 2049 + 2048 + 2048 = 3 * 2048 + 1 vertices, every one a short row in round one (2 - 4 entries), and four hubs
    behind them.  Hubs 0 and 1 have exactly seg entries each and hubs 2 and 3 seg + 1; the heaviest entry of each -- the last of
    its sorted row, for hubs 2 and 3 a window of its own -- is the edge to its partner hub, the only edge between their rings:
    ring 0 (hubs 0 and 2) -- ring 1 (hub 1), ring 0 -- ring 2 (hub 3).  The forest is a tree only if both edges are found."""
    rng = np.random.default_rng(seed)
    sizes = [seg + 1, seg, seg]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    hub = int(starts[-1]) + np.arange(4)
    s, d = [], []
    for k, sz in enumerate(sizes):
        v = starts[k] + np.arange(sz)
        s.append(v)
        d.append(starts[k] + (np.arange(sz) + 1) % sz)
    spokes = [(hub[0], 0, seg - 1), (hub[1], 1, seg - 1), (hub[2], 0, seg), (hub[3], 2, seg)]    # (hub, its ring, spokes)
    for h, k, count in spokes:
        s.append(np.full(count, h))
        d.append(starts[k] + np.arange(count))
    s, d = np.concatenate(s), np.concatenate(d)
    w = rng.permutation(len(s)).astype(np.float32) + 1.0               # distinct integers: the totals are exact
    s = np.concatenate([s, [hub[0], hub[2]]])
    d = np.concatenate([d, [hub[1], hub[3]]])
    w = np.concatenate([w, [1e6, 2e6]]).astype(np.float32)
    return wcsr(int(hub[-1]) + 1, s, d, w) + (True,)


# name -> builder of the cases both suites run (the R-MAT inputs and the fixtures come from the oracle: see the suites)
CASES = {
    "no_entries_1": lambda: no_entries(1),
    "no_entries_1000": lambda: no_entries(1000),
    "self_loops_only": self_loops_only,
    "ring_1000": ring,
    "grid_64x64": grid,
    "clique_300": clique,
    "shuffled_path_200000": shuffled_path,
    "increasing_path_4096": increasing_path,
    "star_0_equal": lambda: star(0, "equal"),
    "star_77777_equal": lambda: star(77777, "equal"),
    "star_0_random": lambda: star(0, "random"),
    "star_77777_random": lambda: star(77777, "random"),
    "two_cliques_directed_bridge": lambda: two_cliques(False),
    "two_cliques_symmetric": lambda: two_cliques(True),
    "parallel_entries": parallel_entries,
    "special_weights": special_weights,
    "small_components_symmetric": lambda: small_components(True),
    "small_components_directed": lambda: small_components(False),
    "work_list_edges": work_list_edges,
}

RMAT_SYMMETRIC = [(10, 1), (11, 2), (12, 4), (13, 8), (14, 16), (15, 1), (16, 16)]
RMAT_DIRECTED = [(10, 2), (12, 4), (14, 8)]
FIXTURES = ["bfs_test.mtx", "kcore_test.mtx", "pr_test.mtx", "sssp_test.mtx", "synthetic_dup.mtx"]
