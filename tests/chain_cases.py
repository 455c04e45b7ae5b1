"""Inputs that put each of the six launch chains (include/mgx/launch_chain.hpp) on the edges of its protocol: for every
algorithm one input per K of tests/chain_model.SEAMS -- K: the number of the run's first idle launch plus one -- and the inputs at
and past the log's cap.  They were found with the models and are pinned here by name with their K; tests/test_chain_cases_cpu.py
asserts every K with the model, so a case that drifts off its seam fails there rather than passing beside it, and
tests/test_gpu_launch_chain.py runs them.  numpy only; everything is generated.

Where a model rules a K out, the nearest reachable K on each side stands in, and the case says so:
    Louvain   a level's chain is SETUP, 3 launches an iteration (5 when the level has long rows: one count for the whole level) and
              DONE: K = 3 t + 2 or 5 t + 2.  63, 64, 193 and 448 are neither: 62 and 65, 192 and 194, 447 and 449 stand around them.
"""
from collections import namedtuple
import functools

import numpy as np

from tests import chain_model, kcore_cases, kcore_model, ktruss_cases, ktruss_model, louvain_model, lpa_cases, lpa_model, msbfs_cases
from tests import msbfs_model, scc_cases, scc_model
from tests import coloring_model as cm

# algo: which chain; name: the input; K: the pinned launch count; args: what the algorithm's check is called with
Case = namedtuple("Case", "algo name K args")
ALGOS = ("lpa", "ktruss", "kcore", "msbfs", "scc", "louvain")


# ---- label propagation: synchronous runs that never converge, ended by max_iter ----
def lpa_pair():
    """two vertices that swap labels for ever: SETUP, (EVAL, APPLY) x max_iter, EVAL, IDLE: K = 2 max_iter + 3"""
    return lpa_cases.sym(2, [0], [1])


LPA_EVEN_OPTS = {"wave_max": 40}


def lpa_pair_and_clique():
    """the pair beside a K42, with MGX_LPA_WAVE_MAX = 40 (rows of 41 entries are long).  In iteration 0 every clique vertex moves,
    in iteration 1 vertex 2 moves back, and the clique is still: a MARK in iterations 0 and 1.  Up to iteration 2 somebody of the
    clique is active and the iteration dense, so its rows take a LONG launch; from iteration 3 on the pair alone is listed.  Five
    launches more than the pair's: K = 2 max_iter + 8, max_iter >= 3"""
    return lpa_cases.disjoint([(2, [0], [1]), (42,) + lpa_cases.clique(42)])


def _lpa(name, K, graph, max_iter, opts=None):
    return Case("lpa", name, K, dict(graph=graph, mode=lpa_model.SYNC, max_iter=max_iter, opts=opts or {}))


LPA = [_lpa("pair_i%d" % ((K - 3) // 2), K, lpa_pair, (K - 3) // 2) if K % 2 else
       _lpa("pair_clique_i%d" % ((K - 8) // 2), K, lpa_pair_and_clique, (K - 8) // 2, LPA_EVEN_OPTS) for K in chain_model.SEAMS]
# one launch below the cap, at it and past it: the IDLE is the log's last entry but one, its last, and not in it
LPA_CAP = [_lpa("pair_i32766", 65535, lpa_pair, 32766), _lpa("pair_clique_i32764", 65536, lpa_pair_and_clique, 32764, LPA_EVEN_OPTS),
           _lpa("pair_i32767", 65537, lpa_pair, 32767)]


# ---- k-truss: K = 3 levels + 2 passes + 2 ----
def grid_and_k4(w, h):
    """the triangulated grid and a disjoint K4 behind it: level 3 peels the grid, level 4 is the K4's one pass"""
    ro, ci = ktruss_cases.grid(w, h, True)
    n = len(ro) - 1
    src = np.repeat(np.arange(n), np.diff(ro))
    a, b = ktruss_cases.pairs_of(n + np.arange(4))
    return cm.csr(n + 4, np.concatenate([src[src < ci], a]), np.concatenate([ci[src < ci], b]))


def _ktruss(K):
    if K % 2:                                                   # grid(p + 1, p): one level of p passes, K = 2 p + 5
        p = (K - 5) // 2
        return Case("ktruss", "grid%dx%d" % (p + 1, p), K, dict(graph=functools.partial(ktruss_cases.grid, p + 1, p, True)))
    p = (K - 10) // 2                                           # two levels, p + 1 passes: K = 2 p + 10
    return Case("ktruss", "grid%dx%d_k4" % (p + 1, p), K, dict(graph=functools.partial(grid_and_k4, p + 1, p)))


KTRUSS = [_ktruss(K) for K in chain_model.SEAMS]


# ---- k-core: a MIN and the level's one pass per clique of the stairs, K = 2 hi + 1; a step of two sizes costs a LIST more ----
def stairs_and_a_step(hi):
    """K2 .. K_hi and K_(hi + 2): the last level is two further, so its MIN lists nobody and a LIST follows: K = 2 hi + 4"""
    return kcore_cases.cliques(list(range(2, hi + 1)) + [hi + 2])


def _kcore(K):
    if K % 2:
        return Case("kcore", "stairs2_%d" % ((K - 1) // 2), K, dict(graph=functools.partial(kcore_cases.stairs, 2, (K - 1) // 2)))
    return Case("kcore", "stairs2_%d_step" % ((K - 4) // 2), K, dict(graph=functools.partial(stairs_and_a_step, (K - 4) // 2)))


KCORE = [_kcore(K) for K in chain_model.SEAMS]


# ---- multi-source BFS: K = 2 batches + the levels' (2 + [long rows listed]) + 1 ----
def directed_path_with_a_hub(p, leaves=msbfs_model.WAVE_MAX + 1):
    """0 -> 1 -> ... -> p - 1, and vertex 3 has `leaves` out-entries more, to vertices of their own: no in-entries are given, so
    every level pushes, and the level whose front is vertex 3 lists its row as items: p levels and one LONG, K = 2 p + 4"""
    src = np.concatenate([np.arange(p - 1), np.full(leaves, 3)])
    dst = np.concatenate([np.arange(1, p), p + np.arange(leaves)])
    return msbfs_cases.directed(p + leaves, src, dst)


def _msbfs(K):
    if K % 2:                                                   # the path from its end: n levels, K = 2 n + 3
        n = (K - 3) // 2
        return Case("msbfs", "path%d" % n, K, dict(graph=functools.partial(msbfs_cases.path, n), sources=[0], symmetric=True))
    p = (K - 4) // 2
    return Case("msbfs", "path%d_hub" % p, K, dict(graph=functools.partial(directed_path_with_a_hub, p), sources=[0], symmetric=False))


MSBFS = [_msbfs(K) for K in chain_model.SEAMS]
MSBFS_CAP_LEVELS = (65535, 65536, 65537)                        # the path of that many vertices from vertex 0: as many levels


# ---- SCC: where the graph determines the launches, a directed path (every K) and a directed ring (odd K) ----
def _scc(K):
    n = 2 * (K - 3)                                             # path_launches(n) = ceil(n / 2) + 3
    out = [Case("scc", "path%d" % n, K, dict(graph=functools.partial(scc_cases.path, n), kinds=functools.partial(scc_model.path_kinds, n)))]
    if K % 2:                                                   # ring_launches(n) = 2 n + 9
        n = (K - 9) // 2
        out.append(Case("scc", "ring%d" % n, K, dict(graph=functools.partial(scc_cases.ring, n), kinds=functools.partial(scc_model.ring_kinds, n))))
    return out


SCC = [c for K in chain_model.SEAMS for c in _scc(K)]
SCC_CAP_RING = 32764                                            # the first ring whose launches exceed the log: 2 n + 9 = 65 537


# ---- Louvain: the first level's chain on the seam, ended by max_iter ----
def weighted_path(L=100):
    """a path whose edge i - (i + 1) is there L - i times: the heavy end absorbs the path a vertex or so an iteration, 251
    iterations before two are rejected.  Rows of at most 2 L - 1 entries: a wave's at the defaults"""
    i = np.arange(L - 1)
    a = np.repeat(i, L - i)
    return lpa_cases.sym(L, a, a + 1)


LOUVAIN_ALL_LONG = {"short_max": 0, "wave_max": 0}              # every row goes out as items: 5 launches an iteration


def _louvain(K, per, seam):
    opts = LOUVAIN_ALL_LONG if per == 5 else {}
    t = (K - 2) // per
    return Case("louvain", "weighted_path_i%d%s" % (t, "_long" if per == 5 else ""), K,
                dict(graph=weighted_path, max_iter=t, opts=opts, seam=seam))


# (K, launches an iteration, the seam value it stands at or beside)
LOUVAIN = [_louvain(62, 3, 63), _louvain(65, 3, 65), _louvain(191, 3, 191), _louvain(192, 5, 192), _louvain(194, 3, 193),
           _louvain(447, 5, 447), _louvain(449, 3, 449)]

SEAM_CASES = LPA + KTRUSS + KCORE + MSBFS + SCC + LOUVAIN
CAP_CASES = LPA_CAP


def case_id(c):
    return "%s-%s-K%d" % (c.algo, c.name, c.K)


def by_k(algo, K):
    """the first case of that algorithm with that K"""
    return next(c for c in SEAM_CASES + CAP_CASES if c.algo == algo and c.K == K)


# ---- what the models say ----
_graphs = {}


def graph(c):
    """the case's (ro, ci), built once and read-only"""
    key = (c.algo, c.name)
    if key not in _graphs:
        ro, ci = c.args["graph"]()
        ro.setflags(write=False)
        ci.setflags(write=False)
        _graphs[key] = (ro, ci)
    return _graphs[key]


_wanted = {}


def wanted(c):
    """the model's result for the case, computed once and shared by the tests (read-only by agreement): what the algorithm's
    GPU check takes as `want`"""
    key = (c.algo, c.name)
    if key in _wanted:
        return _wanted[key]
    ro, ci = graph(c)
    a = c.args
    if c.algo == "lpa":
        w = lpa_model.propagate(ro, ci, True, a["mode"], max_iter=a["max_iter"], **a["opts"])
    elif c.algo == "ktruss":
        w = ktruss_model.decompose(ro, ci, True)
    elif c.algo == "kcore":
        w = kcore_model.launch_plan(ro, ci)
    elif c.algo == "msbfs":
        w = msbfs_model.traverse(ro, ci, a["sources"], a["symmetric"], False)
    elif c.algo == "scc":
        w = scc_model.decompose(ro, ci)
    else:
        w = louvain_model.louvain(ro, ci, True, max_iter=a["max_iter"], **a["opts"])
    _wanted[key] = w
    return w


def predicted_k(c):
    """K of the case by its algorithm's model (Louvain: of its first level's chain)"""
    w = wanted(c)
    if c.algo == "lpa":
        return len(w["kinds"])
    if c.algo == "ktruss":
        return ktruss_model.peel_launches(w["stats"])
    if c.algo == "kcore":
        return len(w.kinds)
    if c.algo == "msbfs":
        return w["launches"]
    if c.algo == "scc":
        return len(c.args["kinds"]())
    return louvain_model.chains(w["kinds"])[0]
