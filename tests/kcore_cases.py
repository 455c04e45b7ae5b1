"""Inputs of the fused k-core's path tests, shared by the CPU suite (tests/test_kcore_cpu.py: the launch plan of
tests/kcore_model.py is what each case was built for) and the GPU suite (tests/test_gpu_kcore_paths.py: the device took the
launches the plan predicts).  numpy only; everything is generated.

Builders return (row_offsets, col_indices) as int32, rows sorted by neighbour.  All graphs are symmetric but funnel() and
cap_row().  Each case sits on one of the thresholds of include/mgx/kcore_fused.hpp: a front of 2048 / 2049 entries (one
workgroup or the device), rows of 31 / 32 and 256 / 257 entries (a thread or (vertex, segment) items), the wave stages' flushes
at 128 short and 64 long rows, the scan's last id, k == n, and the host's batches of 64, 128, 256, 256 ... launches."""
import numpy as np

HUB_ROWS = (31, 32, 33, 255, 256, 257, 512, 513, 1024, 1025)


def csr_from_entries(n, src, dst):
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    order = np.lexsort((dst, src))
    ro = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=ro[1:])
    return ro.astype(np.int32), dst[order].astype(np.int32)


def _symmetric(n, a, b):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    return csr_from_entries(n, np.concatenate([a, b]), np.concatenate([b, a]))


def _clique_pairs(first, c):
    s, d = np.meshgrid(np.arange(first, first + c), np.arange(first, first + c), indexing="ij")
    m = s < d
    return s[m], d[m]


def cliques(sizes):
    """disjoint K_c, one per entry of sizes, over contiguous ids in that order"""
    a, b, first = [], [], 0
    for c in sizes:
        s, d = _clique_pairs(first, c)
        a.append(s); b.append(d)
        first += c
    return _symmetric(first, np.concatenate(a), np.concatenate(b))


def clique(c):
    return cliques([c])


def stairs(lo, hi):
    """K_lo, K_(lo + 1) .. K_hi: every level is the next one, so each MIN lists the next front itself"""
    return cliques(list(range(lo, hi + 1)))


def stairs_even(lo, hi):
    """K_lo, K_(lo + 2) .. K_hi: every level is two further, so each needs a LIST"""
    return cliques(list(range(lo, hi + 1, 2)))


def multi_broom(rows=HUB_ROWS):
    """hubs 0 .. len(rows) - 1 whose rows hold exactly rows[i] entries: one K4 vertex (hub i's is K4 vertex i % 4) and leaves of its
    own.  The K4 is the last four ids."""
    h = len(rows)
    n = h + sum(r - 1 for r in rows) + 4
    a, b, nxt = [], [], h
    for i, r in enumerate(rows):
        assert r >= 1
        a.append(np.full(r - 1, i)); b.append(np.arange(nxt, nxt + r - 1))
        nxt += r - 1
        a.append(np.array([i])); b.append(np.array([n - 4 + i % 4]))
    s, d = _clique_pairs(n - 4, 4)
    a.append(s); b.append(d)
    return _symmetric(n, np.concatenate(a), np.concatenate(b))


def broom(leaves):
    """hub 0 with `leaves` leaves and one edge into a K4: its row holds leaves + 1 entries"""
    return multi_broom([leaves + 1])


def star(leaves):
    return _symmetric(leaves + 1, np.zeros(leaves, dtype=np.int64), np.arange(1, leaves + 1))


FUNNEL_SOURCES = 3000


def funnel(sources, t_row):
    """directed: rows 0 .. sources - 1 hold one entry each, vertex t = sources; t's row holds t_row entries, to sinks of their own
    (vertices without rows)"""
    t = sources
    src = np.concatenate([np.arange(sources), np.full(t_row, t)])
    dst = np.concatenate([np.full(sources, t), np.arange(t + 1, t + 1 + t_row)])
    return csr_from_entries(t + 1 + t_row, src, dst)


def tail(n):
    """a K4 on ids 0 .. 3 and vertex n - 1 hung on vertex 0; the ids between have no entries"""
    assert n >= 5
    s, d = _clique_pairs(0, 4)
    return _symmetric(n, np.concatenate([s, [0]]), np.concatenate([d, [n - 1]]))


def cap_row(n=5):
    """directed multigraph, k == n with somebody left AT n: vertex 0 holds n entries and vertex 1 holds n - 1, all to vertex n - 1
    (no row).  Level n takes vertex 1; the MIN behind it must leave vertex 0 alone (a level n + 1 does not exist), so the run ends
    with largest_k_core -1 and vertex 0 at degree n."""
    src = np.concatenate([np.zeros(n, dtype=np.int64), np.ones(n - 1, dtype=np.int64)])
    return csr_from_entries(n, src, np.full(2 * n - 1, n - 1))


TAIL_NS = (5, 255, 256, 257, 1024, 1025, 2049, 4097)

CASES = {
    "broom2047": lambda: broom(2047),
    "broom2048": lambda: broom(2048),
    "broom2049": lambda: broom(2049),
    "multi_broom": lambda: multi_broom(),
    "cliques32x5_33x4": lambda: cliques([32] * 5 + [33] * 4),
    "stairs2_40": lambda: stairs(2, 40),
    "stairs2_100": lambda: stairs(2, 100),
    "stairs_even2_80": lambda: stairs_even(2, 80),
    "stairs_even2_300": lambda: stairs_even(2, 300),
    "star3000": lambda: star(3000),
    "star100": lambda: star(100),
    "funnel1500": lambda: funnel(FUNNEL_SOURCES, 1500),
    "funnel3001": lambda: funnel(FUNNEL_SOURCES, 3001),
    "funnel3002": lambda: funnel(FUNNEL_SOURCES, 3002),
    "clique5": lambda: clique(5),
    "clique2": lambda: clique(2),
    "cap_row5": lambda: cap_row(5),
}
CASES.update({"tail%d" % n: (lambda n=n: tail(n)) for n in TAIL_NS})
DIRECTED = ("funnel1500", "funnel3001", "funnel3002", "cap_row5")

_built = {}


def get(name):
    """the case's (ro, ci), built once and read-only"""
    if name not in _built:
        ro, ci = CASES[name]()
        ro.setflags(write=False)
        ci.setflags(write=False)
        _built[name] = (ro, ci)
    return _built[name]


_plans = {}


def plan(name):
    """the case's launch plan (tests/kcore_model.launch_plan), computed once"""
    if name not in _plans:
        from tests import kcore_model
        _plans[name] = kcore_model.launch_plan(*get(name))
    return _plans[name]
