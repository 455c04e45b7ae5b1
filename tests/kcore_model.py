"""numpy model of the k-core decomposition as worklists (mgx_kcore_run, include/mgx/kcore_fused.hpp).

It restates what kcore_enactor_t::enact computes on ANY CSR (directed, duplicates, self-loops, empty rows):
    deg = row lengths; core = 0; largest = -1
    loop: no deg > 0: stop.   k = 1 + min(deg > 0);  k > n: stop.   front = { deg == k - 1 }
          while front:  core[front] = k - 1; deg[front] = 0; every entry (v, u), v in front: deg[u] -= 1
                        cand  = { u : deg[u] >= k before this pass, < k after it }
                        front = { u in cand : deg[u] > 0 }          (the others are stranded: core 0 for good)
          no deg >= k: largest = k - 1; stop
"""
import numpy as np

STAT_NAMES = ("levels", "passes", "expanded", "removed", "stranded")


def decompose(ro, ci):
    """-> (core numbers, largest_k_core, final working degrees, {"levels", "passes", "expanded", "removed", "stranded"})"""
    ro = np.asarray(ro, dtype=np.int64)
    ci = np.asarray(ci, dtype=np.int64)
    n = len(ro) - 1
    deg = np.diff(ro).astype(np.int64)
    core = np.zeros(n, dtype=np.int32)
    largest = -1
    st = dict.fromkeys(STAT_NAMES, 0)
    while True:
        positive = deg[deg > 0]
        if positive.size == 0:
            break
        k = int(positive.min()) + 1
        if k > n:
            break
        front = np.nonzero(deg == k - 1)[0]
        st["levels"] += 1
        while front.size:
            st["passes"] += 1
            st["removed"] += int(front.size)
            core[front] = k - 1
            deg[front] = 0
            before = deg.copy()
            lens = ro[front + 1] - ro[front]
            total = int(lens.sum())
            st["expanded"] += total
            if total:
                starts = np.repeat(ro[front] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens)
                targets = ci[starts + np.arange(total)]
                deg -= np.bincount(targets, minlength=n)
            cand = np.nonzero((before >= k) & (deg < k))[0]
            front = cand[deg[cand] > 0]
            st["stranded"] += int(cand.size - front.size)
        if not (deg >= k).any():
            largest = k - 1
            break
    return core, largest, deg.astype(np.int32), st


def check_against_enactor(st, est):
    """the relations between the model's (the fused path's) stats and the operator path's [k values, passes, expanded, removed]"""
    return st["passes"] == int(est[1]) - int(est[0]) and st["expanded"] == int(est[2]) and st["removed"] == int(est[3])


# ---- the graphs both suites use ----
def csr(n, src, dst, symmetric=True):
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    if symmetric:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
    order = np.argsort(src, kind="stable")
    ro = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(src, minlength=n), out=ro[1:])
    return ro, dst[order].astype(np.int32)


def path3():
    return csr(3, [0, 1], [1, 2])


def no_entries(n=6):
    return np.zeros(n + 1, dtype=np.int32), np.zeros(0, dtype=np.int32)


def capped_multigraph():
    """6 vertices, every row 8 entries to the next vertex: degrees above n, so no k <= n removes anybody"""
    src = [v for v in range(6) for _ in range(8)]
    dst = [(v + 1) % 6 for v in range(6) for _ in range(8)]
    return csr(6, src, dst, symmetric=False)


def star_forest(stars=50, leaves=7):
    src, dst = [], []
    for s in range(stars):
        hub = s * (leaves + 1)
        for j in range(1 + s % leaves):
            src.append(hub)
            dst.append(hub + 1 + j)
    return csr(stars * (leaves + 1), src, dst)


def tripled_clique(n=40):
    src = [a for a in range(n) for b in range(n) if a != b for _ in range(3)]
    dst = [b for a in range(n) for b in range(n) if a != b for _ in range(3)]
    return csr(n, src, dst, symmetric=False)


def grid(rows, cols):
    v = np.arange(rows * cols).reshape(rows, cols)
    src = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()])
    dst = np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()])
    return csr(rows * cols, src, dst)


def ragged_directed(seed=7, n=500):
    """the directed ragged multigraph of tests/test_gpu_kcore.py (vertices without entries, a self-loop row)"""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 9, size=n)
    deg[rng.integers(0, n, size=min(60, n))] = 0
    ro = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    ci = rng.integers(0, n, size=int(ro[-1])).astype(np.int32)
    if n > 4:
        ci[ro[3]:ro[4]] = 3
    return ro, ci


def sparse_symmetric(seed, n=2000, pairs=1500):
    rng = np.random.default_rng(seed)
    return csr(n, rng.integers(0, n, pairs), rng.integers(0, n, pairs))


def single(loop):
    return (np.array([0, 1], dtype=np.int32), np.zeros(1, dtype=np.int32)) if loop else no_entries(1)
