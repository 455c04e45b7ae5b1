"""Checks shared by the GPU suites of the fused SSSP (tests/test_gpu_parity.py, tests/test_gpu_sssp_paths.py).  numpy only."""
import numpy as np


def check_shortest_path_tree(ro, ci, w, dist, pred, src):
    """pred is a shortest-path tree of dist: pred[src] = pred[unreached] = -1; every other reached v has an edge pred[v] -> v
    with dist[pred[v]] + w == dist[v] (float32, as the loop adds); following preds from any reached vertex ends at src"""
    n = len(ro) - 1
    inf = np.float32(3.402823466e+38)
    reached = dist < inf
    assert pred[src] == -1 and dist[src] == 0
    assert np.all(pred[~reached] == -1)
    rest = reached.copy(); rest[src] = False
    assert np.all(pred[rest] >= 0), "a reached vertex without a predecessor"
    # tight edge pred[v] -> v: among the entries of row pred[v] that point to v, one with the right weight
    srcs = np.repeat(np.arange(n, dtype=np.int64), np.diff(ro))
    key = srcs * n + ci.astype(np.int64)
    tight = (dist[srcs] + w.astype(np.float32)).astype(np.float32) == dist[ci]
    tight &= reached[srcs]
    tkeys = np.unique(key[tight])
    vs = np.nonzero(rest)[0]
    want = pred[vs].astype(np.int64) * n + vs
    assert np.all(np.isin(want, tkeys)), "a predecessor edge that is not tight (or not an edge)"
    # acyclic: pointer doubling -- after ceil(log2 n) + 1 rounds everybody reached stands at the source
    p = pred.astype(np.int64).copy()
    p[src] = src
    p[~reached] = np.arange(n)[~reached]
    for _ in range(int(np.ceil(np.log2(max(n, 2)))) + 1):
        p = p[p]
    assert np.all(p[reached] == src), "the predecessors contain a cycle"
