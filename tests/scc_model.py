"""The strongly connected components of DESIGN 3.14 in numpy, written from the definition: what the fused path (mgx_scc_run) and
the operator path (mgx_scc_enact) are compared against, bit for bit.

The graph is the directed graph of the CSR entries (v -> u).  label[v] = the smallest id of v's strongly connected component.
outdeg / indeg count a vertex's entries to / from ALIVE vertices other than itself (duplicates count, self-loops never).
    alive = all.  TRIM.
    somebody alive (the pivot phase): p = the alive vertex of the largest outdeg * indeg (ties: the smaller id);
        S = (alive reachable from p) & (alive reaching p); label[S] = min(S); S leaves.  TRIM.
    while somebody is alive (a round): col = own id; to the fixpoint col[u] = min(col[u], col[v]) over alive arcs v -> u;
        roots = {col[v] == v}; C = roots, then to the fixpoint every alive v with an arc v -> u, u in C, col[v] == col[u];
        label[C] = col[C]; C leaves.  TRIM.
    TRIM: to the fixpoint, every alive v with outdeg[v] == 0 or indeg[v] == 0: label[v] = v, v leaves.
Every fixpoint is unique, so the alive set after every phase is; how many sweeps one takes is not, and is not reported."""
import numpy as np

STAT_KEYS = ("components", "largest", "largest_label", "trimmed", "pivot_size", "rounds")
NONE = np.iinfo(np.int64).max


def arcs(ro, ci):
    """(src, dst) of the entries that are not self-loops, duplicates kept"""
    ro = np.asarray(ro, dtype=np.int64)
    src = np.repeat(np.arange(len(ro) - 1, dtype=np.int64), np.diff(ro))
    dst = np.asarray(ci, dtype=np.int64)
    keep = src != dst
    return src[keep], dst[keep]


def label_stats(label):
    """(components, largest, its label): the three numbers cc_label_stats_t reports"""
    if len(label) == 0:
        return 0, 0, 0
    ids, sizes = np.unique(label, return_counts=True)
    return len(ids), int(sizes.max()), int(ids[np.argmax(sizes)])          # (argmax: the first, the smaller label)


class _Run:
    def __init__(self, ro, ci):
        self.n = len(ro) - 1
        self.src, self.dst = arcs(ro, ci)
        self.alive = np.ones(self.n, dtype=bool)
        self.label = np.full(self.n, -1, dtype=np.int64)
        self.trimmed = 0

    def alive_arcs(self):
        keep = self.alive[self.src] & self.alive[self.dst]
        return self.src[keep], self.dst[keep]

    def degrees(self):
        s, d = self.alive_arcs()
        return np.bincount(s, minlength=self.n), np.bincount(d, minlength=self.n)

    def trim(self):
        while True:
            outdeg, indeg = self.degrees()
            go = self.alive & ((outdeg == 0) | (indeg == 0))
            if not go.any():
                return
            self.label[go] = np.flatnonzero(go)
            self.alive[go] = False
            self.trimmed += int(go.sum())

    def phase(self, col):
        """col is seeded; forward to the fixpoint, the roots, backward to the fixpoint -> the claimed set"""
        s, d = self.alive_arcs()
        changed = self.alive & (col != NONE)
        while changed.any():
            sel = changed[s]
            before = col.copy()
            np.minimum.at(col, d[sel], before[s[sel]])
            changed = col != before
        claimed = self.alive & (col == np.arange(self.n))
        same = col[s] == col[d]
        s, d = s[same], d[same]
        while True:
            new = np.zeros(self.n, dtype=bool)
            new[s[claimed[d] & ~claimed[s]]] = True
            if not new.any():
                return claimed
            claimed |= new


def decompose(ro, ci):
    """-> {"labels": int32[n], "stats": dict of STAT_KEYS, "phases": [(name, alive bool[n] after it)]}"""
    r = _Run(ro, ci)
    phases = []
    pivot_size = rounds = 0
    r.trim()
    phases.append(("trim", r.alive.copy()))
    if r.alive.any():
        outdeg, indeg = r.degrees()
        prod = np.where(r.alive, outdeg.astype(np.int64) * indeg.astype(np.int64), -1)
        p = int(np.argmax(prod))                                           # (the first of the largest: the smaller id)
        col = np.full(r.n, NONE, dtype=np.int64)
        col[p] = p
        s = r.phase(col)
        r.label[s] = np.flatnonzero(s).min()
        r.alive[s] = False
        pivot_size = int(s.sum())
        r.trim()
        phases.append(("pivot", r.alive.copy()))
    while r.alive.any():
        rounds += 1
        col = np.where(r.alive, np.arange(r.n, dtype=np.int64), NONE)
        c = r.phase(col)
        r.label[c] = col[c]
        r.alive[c] = False
        r.trim()
        phases.append(("round %d" % rounds, r.alive.copy()))
    comps, largest, largest_label = label_stats(r.label)
    stats = dict(zip(STAT_KEYS, (comps, largest, largest_label, r.trimmed, pivot_size, rounds)))
    return {"labels": r.label.astype(np.int32), "stats": stats, "phases": phases}


# ---- the fused path's launches where the graph determines them (the switch in k_scc_step, restated) ----
# A general forward sweep's length depends on what a load sees, so its launches are not a function of the graph.  On a directed
# path nothing sweeps, and on a directed ring every front is one vertex: there the kinds are.
DEGINIT, LIST, EXPAND, PMAX, PPICK, RINIT, FWD, ROOTS, BWD, SEAL, DONE = range(1, 12)      # scc_kind_t


def path_kinds(n):
    """0 -> 1 -> ... -> n - 1, n >= 1: trim only.  LIST takes both ends (indeg 0, outdeg 0), every EXPAND of {j, n - 1 - j} empties
    a counter of j + 1 and of n - 2 - j, which are the next front: ceil(n / 2) fronts, the last one's EXPAND appends nobody (what it
    decrements has left already), and with nobody alive DONE follows"""
    return [DEGINIT, LIST] + [EXPAND] * ((n + 1) // 2) + [DONE]


def ring_kinds(n):
    """v -> (v + 1) % n, n >= 2: nobody is trimmed, every product is 1 and the pivot is vertex 0.  FWD from {0} lowers one vertex
    a launch; the launch whose front is {n - 1} meets vertex 0 and lowers nobody: n launches.  ROOTS claims 0, BWD claims one
    source a launch, the one whose front is {1} meets 0 claimed: n launches.  SEAL removes all n, the EXPAND behind it appends
    nobody, and with nobody alive DONE follows"""
    return [DEGINIT, LIST, PMAX, PPICK, RINIT] + [FWD] * n + [ROOTS] + [BWD] * n + [SEAL, EXPAND, DONE]


def path_launches(n):
    """K of the chain (tests/chain_model.py) on the directed path of n vertices"""
    return (n + 1) // 2 + 3


def ring_launches(n):
    """K of the chain on the directed ring of n >= 2 vertices"""
    return 2 * n + 9


def canonical(n, comp):
    """any component numbering -> the smallest vertex id of each component, int32"""
    comp = np.asarray(comp)
    lowest = np.full(int(comp.max()) + 1 if n else 0, n, dtype=np.int64)
    np.minimum.at(lowest, comp, np.arange(n))
    return lowest[comp].astype(np.int32)


def scipy_labels(ro, ci):
    """scipy's strong components, relabelled to smallest ids"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    n = len(ro) - 1
    m = sp.csr_matrix((np.ones(len(ci), dtype=np.int8), np.asarray(ci), np.asarray(ro)), shape=(n, n))
    _, comp = connected_components(m, directed=True, connection="strong")
    return canonical(n, comp)
