"""numpy model of the connected components (include/mgx/cc_fused.hpp): the definition the fused path and the operator
path must both reproduce bit for bit.

    components: weakly connected, every CSR entry (v, u) read as the undirected pair {v, u} (self-loops and duplicates change
                nothing; a vertex without entries is a component of its own)
    label[v]:   the smallest vertex id of v's component
    stats:      [0] components, [1] size of the largest, [2] its label (ties: the smallest label)

and of what the fused path's skip counts (stats[3]):
    the partition after the two neighbour rounds: the components of the entries ro[v] + r, r = 0, 1 (rows that long)
    c = the most frequent of its labels over the vertices color_salt(seed, j) % n, j < 1024 (ties: the smaller)
    skipped = vertices with label c that still had entries to link: out-entries from the third on, or (directed, with a
              genuine CSC) in-entries; 0 when the graph is directed and has no CSC
"""
import numpy as np

from tests import coloring_model as cm

SEED = 15485863
SAMPLES = 1024
NEIGHBOR_ROUNDS = 2


def _pair_labels(n, a, b):
    """labels of the undirected pairs (a, b) over n vertices: hook the larger label under the smaller, jump pointers to a fixed
    point, repeat until no pair has labels that differ"""
    lab = np.arange(n, dtype=np.int64)
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    keep = a != b
    a, b = a[keep], b[keep]
    while len(a):
        la, lb = lab[a], lab[b]
        diff = la != lb
        a, b, la, lb = a[diff], b[diff], la[diff], lb[diff]
        if not len(a):
            break
        np.minimum.at(lab, np.maximum(la, lb), np.minimum(la, lb))
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
    return lab


def _entries(ro, ci):
    ro = np.asarray(ro, dtype=np.int64)
    n = len(ro) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ro))
    return n, ro, rows, np.asarray(ci, dtype=np.int64)[ro[0]:ro[-1]]


def labels(ro, ci):
    """int32[n]: the smallest vertex id of every vertex's component"""
    n, _, rows, cols = _entries(ro, ci)
    return _pair_labels(n, rows, cols).astype(np.int32)


def sample_ids(n, seed=SEED):
    j = np.arange(SAMPLES, dtype=np.uint64)
    s = cm.fmix32(((int(seed) + np.uint64(0x9E3779B9) * (j + np.uint64(1))) & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    return (s % np.uint32(n)).astype(np.int64)


def most_frequent(values):
    u, cnt = np.unique(values, return_counts=True)     # u ascending: argmax takes the smaller on a tie
    return int(u[np.argmax(cnt)])


def skip_stats(ro, ci, seed=SEED, symmetric=True, has_csc=False):
    """-> {"partition": labels after the two neighbour rounds, "c": the sampled root, "skipped": the fused path's stats[3]}"""
    ro = np.asarray(ro, dtype=np.int64)
    ci = np.asarray(ci, dtype=np.int64)
    n = len(ro) - 1
    deg = np.diff(ro)
    a, b = [], []
    for r in range(NEIGHBOR_ROUNDS):
        v = np.nonzero(deg > r)[0]
        a.append(v)
        b.append(ci[ro[v] + r])
    part = _pair_labels(n, np.concatenate(a), np.concatenate(b))
    c = most_frequent(part[sample_ids(n, seed)]) if n else -1
    if not symmetric and not has_csc:
        skipped = 0
    else:
        has = deg > NEIGHBOR_ROUNDS
        if not symmetric:
            has |= np.bincount(ci[ro[0]:ro[-1]], minlength=n)[:n] > 0
        skipped = int((has & (part == c)).sum())
    return {"partition": part.astype(np.int32), "c": c, "skipped": skipped}


def stats(lab):
    """{"components", "largest", "largest_label"} of a label array"""
    lab = np.asarray(lab, dtype=np.int64)
    n = len(lab)
    if n == 0:
        return {"components": 0, "largest": 0, "largest_label": 0}
    sizes = np.bincount(lab, minlength=n)
    big = int(np.argmax(sizes))
    return {"components": int((lab == np.arange(n)).sum()), "largest": int(sizes[big]), "largest_label": big}


def transpose(ro, ci):
    """(col_offsets, row_indices) of a CSR: the genuine CSC"""
    n, _, rows, cols = _entries(ro, ci)
    order = np.lexsort((rows, cols))
    co = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=n), out=co[1:])
    return co.astype(np.int32), rows[order].astype(np.int32)
