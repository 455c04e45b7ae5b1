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

from tests import chain_model

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


# ---- the launch plan: which kind every launch of mgx_kcore_run is (the switch in k_kcore_step, restated) ----
# The header's thresholds, by name; tests/test_kcore_cpu.py reads their values out of include/mgx/kcore_fused.hpp.
MINI_MAX = 2048          # KCORE_MINI_MAX: entries of a front one workgroup peels on its own
LONG_MIN = 32            # KCORE_LONG_MIN: rows of at least this many entries are long
SEG = 256                # KCORE_SEG: entries of a (vertex, segment) item
BATCH_MIN, BATCH_MAX = chain_model.BATCH_MIN, chain_model.BATCH_MAX     # launches per host wait (launch_chain.hpp)
# the codes of mini_amd.KcoreProblem.STEP_KINDS (kcore_kind_t)
MIN, LIST, EXPAND, FILTER, IDLE, MINI = 1, 2, 3, 4, 5, 6
_INIT = 0
KIND_NAMES = {MIN: "min", LIST: "list", EXPAND: "expand", FILTER: "filter", IDLE: "idle", MINI: "mini"}


class Plan:
    """what launch_plan returns.  kinds: the codes up to and including the first idle launch; fronts: (k, entries, kind that took
    it) per front, a MINI's inner passes included; lists: (short rows, items) of the same fronts, as a step enlists them"""

    def __init__(self):
        self.kinds, self.fronts, self.lists = [], [], []
        self.cores = self.largest = self.degrees = self.stats = None

    def names(self):
        return " ".join(KIND_NAMES[k] for k in self.kinds)


def front_lists(ro, front):
    """(short rows, (vertex, segment) items) a front of these vertices is enlisted as"""
    lens = np.asarray(ro, dtype=np.int64)[np.asarray(front, dtype=np.int64) + 1] - np.asarray(ro, dtype=np.int64)[front]
    long_rows = lens[lens >= LONG_MIN]
    return int((lens < LONG_MIN).sum()), int(((long_rows + SEG - 1) // SEG).sum())


def launch_plan(ro, ci):
    """-> Plan.  The state a launch leaves is (its kind, its k, the front it made, the candidates it found, the smallest positive
    degree it saw); the next launch's kind follows from that alone, as on the device.  Fronts and candidates are sets, so the
    plan is a function of the graph."""
    ro = np.asarray(ro, dtype=np.int64)
    ci = np.asarray(ci, dtype=np.int64)
    n = len(ro) - 1
    deg = np.diff(ro).astype(np.int64)
    core = np.zeros(n, dtype=np.int32)
    st = dict.fromkeys(STAT_NAMES, 0)
    plan = Plan()
    nobody = np.zeros(0, dtype=np.int64)
    largest = -1

    def work_of(front):
        return int((ro[front + 1] - ro[front]).sum())

    def leave(who, number):
        core[who] = number
        deg[who] = 0

    def expand(front, k, kind):
        """one pass: the front's entries take 1 each; -> the vertices that crossed k"""
        lens = ro[front + 1] - ro[front]
        total = int(lens.sum())
        plan.fronts.append((k, total, kind))
        plan.lists.append(front_lists(ro, front))
        st["passes"] += 1
        st["removed"] += int(front.size)
        st["expanded"] += total
        if total == 0:
            return nobody
        starts = np.repeat(ro[front] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens)
        taken = np.bincount(ci[starts + np.arange(total)], minlength=n)
        hit = np.nonzero(taken)[0]
        before = deg[hit]
        deg[hit] = before - taken[hit]
        return hit[(before >= k) & (deg[hit] < k)]

    def filtered(cand, k):
        front = cand[deg[cand] > 0]
        st["stranded"] += int(cand.size - front.size)
        leave(front, k - 1)
        return front

    p_kind, k, front, cand, smallest = _INIT, 0, nobody, nobody, 0
    while True:
        take = MINI if work_of(front) <= MINI_MAX else EXPAND
        new_level = False
        if p_kind == _INIT:
            kind = MIN
        elif p_kind == MIN:
            new_level = True
            if front.size:                       # the MIN listed level k + 1 itself
                k, kind = k + 1, take
            elif smallest == 0:                  # nobody has a positive degree: level k was the last
                kind = IDLE
                if k > 0:
                    largest = k - 1
            else:
                k = smallest + 1
                kind = IDLE if k > n else LIST
        elif p_kind == LIST:
            kind = take
        elif p_kind == EXPAND:
            kind = FILTER if cand.size else MIN
        else:                                    # FILTER, and MINI, which ends where a FILTER ends
            kind = take if front.size else MIN
        plan.kinds.append(kind)
        if new_level and kind != IDLE:
            st["levels"] += 1
        if kind == IDLE:
            break
        if kind == MIN or kind == LIST:
            at = k - 1 if kind == LIST else (k if 1 <= k < n else 0)
            positive = deg[deg > 0]
            smallest = int(positive.min()) if positive.size else 0
            front = np.nonzero(deg == at)[0] if at > 0 else nobody
            leave(front, k if kind == MIN else k - 1)
        elif kind == EXPAND:
            cand = expand(front, k, EXPAND)
            front = nobody
        elif kind == FILTER:
            front = filtered(cand, k)
        else:                                    # MINI: passes of its own until the front is empty or has outgrown it
            while True:
                front = filtered(expand(front, k, MINI), k)
                if front.size == 0 or work_of(front) > MINI_MAX:
                    break
            kind = FILTER
        p_kind = kind
    plan.cores, plan.largest, plan.degrees, plan.stats = core, largest, deg.astype(np.int32), st
    return plan


def host_waits_and_launches(n_kinds):
    """(host waits, launches enqueued) of a run whose first idle launch is launch n_kinds - 1: tests/chain_model.py states the loop"""
    return chain_model.waits_and_launches(n_kinds)


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
