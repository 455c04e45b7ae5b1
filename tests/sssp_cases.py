"""Inputs of the fused SSSP's path tests, shared by the CPU suite (tests/test_sssp_cases_cpu.py: the oracle is right on them,
and they are what they promise) and the GPU suite (tests/test_gpu_sssp_paths.py).  numpy only; everything is generated.

Graph builders return (row_offsets, col_indices) with every row sorted by neighbour; weights are attached separately by
weights(kind, ro, ci, rng).  Three builders come with weights of their own -- the weights ARE the case: bf_worst, dups_and_loops
and overflow_chain return (ro, ci, w).

The kernels are bit-exact by design, so the inputs are built so that every entry matters: in ladder() under the `distinct`
weights every leaf's distance is a different number, and a dropped, duplicated or mis-owned entry changes exactly one of them."""
import numpy as np

FLT_MAX = np.finfo(np.float32).max

# degrees around the short rows' class cuts (1, 5, 17, long_min), the 64-entry unit, and rows of many units
LADDER_DEGS = (1, 2, 4, 5, 6, 16, 17, 18, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513,
               4095, 4096, 4097, 5000)
# n around the LDS tables of 16-bit bounds: 32768 (queue walk) and 73728 (sweep) entries, and hot_n = n & ~1 for an odd n below them
SIZED_NS = (1, 2, 15, 16, 17, 31, 33, 32767, 32768, 32769, 73727, 73728, 73729)


def csr_from_edges(n, src, dst, w=None):
    """rows sorted by neighbour (stable: parallel entries keep their order); duplicates and self loops are kept"""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    order = np.lexsort((np.arange(len(src)), dst, src))
    ro = np.zeros(n + 1, dtype=np.int64)
    np.add.at(ro, src + 1, 1)
    ro = np.cumsum(ro).astype(np.int32)
    ci = dst[order].astype(np.int32)
    if w is None:
        return ro, ci
    return ro, ci, np.asarray(w, dtype=np.float32)[order]


def _undirected(n, a, b):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    return csr_from_edges(n, np.concatenate([a, b]), np.concatenate([b, a]))


def ladder(degs=LADDER_DEGS):
    """vertex 0 (the source) has one hub per degree in degs: hubs 1 .. len(degs), in that order.  A hub's row holds the source
    and, in every other entry, a leaf of its own (a leaf's row: its hub).  Row lengths of the hubs are exactly degs."""
    h = len(degs)
    a, b = [np.zeros(h, dtype=np.int64)], [np.arange(1, h + 1, dtype=np.int64)]
    nxt = h + 1
    for i, d in enumerate(degs):
        assert d >= 1
        a.append(np.full(d - 1, i + 1, dtype=np.int64))
        b.append(np.arange(nxt, nxt + d - 1, dtype=np.int64))
        nxt += d - 1
    return _undirected(nxt, np.concatenate(a), np.concatenate(b))


def ladder_leaves(ro, degs=LADDER_DEGS):
    return np.arange(len(degs) + 1, len(ro) - 1)


def path(n, shuffled=False, seed=1):
    """an undirected path over n vertices; shuffled: the ids along it are a random permutation (position k holds order[k])"""
    order = np.random.default_rng(seed).permutation(n) if shuffled else np.arange(n)
    ro, ci = _undirected(n, order[:-1], order[1:])
    return ro, ci


def path_order(n, shuffled=False, seed=1):
    return np.random.default_rng(seed).permutation(n) if shuffled else np.arange(n)


def grid(h, w):
    ids = np.arange(h * w).reshape(h, w)
    a = np.concatenate([ids[:, :-1].ravel(), ids[:-1, :].ravel()])
    b = np.concatenate([ids[:, 1:].ravel(), ids[1:, :].ravel()])
    return _undirected(h * w, a, b)


def star(leaves=100000, centre=0):
    """centre: 0 or `leaves` (= n - 1)"""
    n = leaves + 1
    rest = np.setdiff1d(np.arange(n), [centre])
    return _undirected(n, np.full(len(rest), centre), rest)


def bf_worst(n=1500):
    """directed: the path i -> i + 1 at weight 1, and shortcuts u -> u + 2^j (j >= 1) that cost 2^j * (j + 1): the fewer hops a
    route has the more it costs.  A frontier Bellman-Ford reaches a far vertex early over a few expensive hops and then improves it
    again and again (once per cheaper mix of spans) until the all-path route arrives in iteration v.  Integer weights."""
    s, d, w = [], [], []
    for j in range(0, 12):
        span = 1 << j
        if span >= n:
            break
        u = np.arange(0, n - span)
        s.append(u); d.append(u + span); w.append(np.full(len(u), float(span * (j + 1))))
    return csr_from_edges(n, np.concatenate(s), np.concatenate(d), np.concatenate(w))


def dups_and_loops(n=2000, seed=3):
    """every (u, v) pair of a sparse random undirected graph THREE times with three different weights (the minimum must win, whichever
    entry a kernel meets first), self loops of weight 0 on the even vertices and of weight 7 on every third"""
    rng = np.random.default_rng(seed)
    a = np.concatenate([np.arange(n - 1), rng.integers(0, n, 2 * n)])
    b = np.concatenate([np.arange(1, n), rng.integers(0, n, 2 * n)])
    keep = a != b
    a, b = a[keep], b[keep]
    k = len(a)
    base = rng.integers(1, 40, k).astype(np.float32)
    perm = np.array([[0.0, 11.0, 5.0], [5.0, 0.0, 11.0], [11.0, 5.0, 0.0]], dtype=np.float32)[rng.integers(0, 3, k)]
    s = np.concatenate([np.repeat(a, 3), np.repeat(b, 3)])
    d = np.concatenate([np.repeat(b, 3), np.repeat(a, 3)])
    w = np.concatenate([(base[:, None] + perm).ravel(), (base[:, None] + perm[:, ::-1]).ravel()])
    l0, l7 = np.arange(0, n, 2), np.arange(0, n, 3)
    s = np.concatenate([s, l0, l7]); d = np.concatenate([d, l0, l7])
    w = np.concatenate([w, np.zeros(len(l0), dtype=np.float32), np.full(len(l7), 7.0, dtype=np.float32)])
    return csr_from_edges(n, s, d, w)


# directed_with_sinks: vertices by role
DWS_ROOT, DWS_DEG0_SOURCE, DWS_PAIR = 0, 1, (2, 3)


def directed_with_sinks(n=600, seed=4):
    """a directed random graph from DWS_ROOT over vertices 4 .. n - 1; DWS_DEG0_SOURCE has no out-edge (it points nowhere, some
    point to it); DWS_PAIR is a component of two vertices pointing at each other; the last 50 vertices are unreachable (they
    only point INTO the graph), every vertex whose id is a multiple of 7 is a sink (out-degree 0)"""
    rng = np.random.default_rng(seed)
    body = np.arange(4, n - 50)
    s, d = [np.full(8, DWS_ROOT)], [rng.choice(body, 8, replace=False)]
    s.append(body[:-1]); d.append(body[1:])                           # a spine, so that the body is reachable ...
    s.append(rng.choice(body, 3 * n)); d.append(rng.choice(body, 3 * n))
    s.append(rng.choice(body, 5)); d.append(np.full(5, DWS_DEG0_SOURCE))
    s.append(np.array(DWS_PAIR)); d.append(np.array(DWS_PAIR[::-1]))
    s.append(np.arange(n - 50, n)); d.append(rng.choice(body, 50))
    s, d = np.concatenate(s), np.concatenate(d)
    keep = (s % 7 != 0) | (s == DWS_ROOT)                              # ... up to the sinks on it
    return csr_from_edges(n, s[keep], d[keep])


def sized_targets(n):
    """the ids on both sides of the ends of the LDS tables (and of the vertex range)"""
    t = set()
    for end in (0, n, n & ~1, 32768, 73728):
        for k in range(-3, 3):
            if 0 <= end + k < n:
                t.add(end + k)
    return np.array(sorted(t), dtype=np.int64)


def sized(n, seed=None):
    """a sparse random directed multigraph over n vertices whose out-degrees do not increase with the id (the hub-first layout sorts
    by degree and keeps ties in order: layout ids are the ids).  The first min(n, 4) rows are long -- at least 64 entries each, at
    least 16 units of 64 together --, the others hold 4 .. 1 entries.  Half the entries point at sized_targets(n), the vertices
    whose bounds sit at the ends of the LDS tables; parallel entries (the rule for n < 64) carry whatever weights they are given."""
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    nl = min(n, 4)
    per_long = 64 * -(-16 // nl) + 1                                   # (+1: the last unit of a long row holds ONE entry)
    deg = np.empty(n, dtype=np.int64)
    deg[:nl] = per_long
    rest = np.arange(nl, n)
    deg[nl:] = np.maximum(1, 4 - (4 * (rest - nl)) // max(n - nl, 1))
    m = int(deg.sum())
    src = np.repeat(np.arange(n), deg)
    dst = rng.integers(0, n, m)
    t = sized_targets(n)
    aim = rng.random(m) < 0.5
    dst[aim] = t[rng.integers(0, len(t), int(aim.sum()))]
    # a spine v -> v + 1 in every row's first entry, so that everything is reached from vertex 0 (and the run has a long tail)
    first = np.cumsum(deg) - deg
    dst[first[:-1]] = np.arange(1, n)
    return csr_from_edges(n, src, dst)


def overflow_chain(n=12):
    """an undirected path whose every edge weighs 1e38: 0, 1e38, 2e38, 3e38, and the fourth hop's sum is +inf -- above FLT_MAX,
    what "not reached" is stored as, so it never improves anything: vertices 4 .. n - 1 stay FLT_MAX although they are connected"""
    ro, ci = path(n)
    return ro, ci, np.full(len(ci), 1e38, dtype=np.float32)


# ---- weight classes --------------------------------------------------------------------------------------------------------------
# kind -> the sweep variant a run must select on a layout with 24-bit ids whose unit blocks hold entries of the class (3: every
# unit-block weight survives the round trip through IEEE half, 2: float weights)
VARIANT = {"distinct": 3, "int2048": 3, "half_edges": 3, "negzero": 3, "one_inexact_long": 2, "one_inexact_short": 3,
           "half_inf": 2, "subnormal": 2, "huge": 2, "mixed_range": 2}
KINDS = tuple(VARIANT)
# classes whose EVERY weight is half-exact; one_inexact_short is half-exact in the unit blocks only
ALL_HALF_EXACT = ("distinct", "int2048", "half_edges", "negzero")
# classes whose path sums are exact in float32 on the small-diameter graphs (ladder, R-MAT): a float64 Dijkstra gives the same values
EXACT_SUMS = ("distinct", "int2048", "negzero", "one_inexact_long", "one_inexact_short", "subnormal")
SHORT_ROW_MAX = 16                      # a row of at most this many entries is short under every long-row threshold the sweep takes (17 .. 64)
UNIT = 64


def half_exact(w):
    """numpy's float16 is IEEE half, subnormals and round-to-nearest-even included (65520 -> inf)"""
    w = np.asarray(w, dtype=np.float32)
    with np.errstate(over="ignore"):
        return w.astype(np.float16).astype(np.float32) == w


def _pos_in_row(ro):
    deg = np.diff(ro).astype(np.int64)
    return np.arange(int(ro[-1]), dtype=np.int64) - np.repeat(ro[:-1].astype(np.int64), deg), np.repeat(np.arange(len(deg)), deg)


def weights(kind, ro, ci, rng):
    """the weights of class `kind` for the CSR (ro, ci), float32, one per entry"""
    m = len(ci)
    deg = np.diff(ro).astype(np.int64)
    pos, row = _pos_in_row(ro)
    if kind == "distinct":
        # entry k of a row weighs (1024 + k % 1024) * 2^(k / 1024 % 5 - 10): 5120 different values in [1, 32) on a grid of 2^-10, each
        # with an 11-bit significand (half-exact); entry k of ROW 0 weighs 64 (k % 30 + 1) instead.  ladder(): a leaf's distance is
        # 64 (hub + 1) + its entry's weight -- below 2048 on a grid of 2^-10: exact in float32, and no two are equal.
        w = (1024 + pos % 1024).astype(np.float64) * np.exp2((pos // 1024) % 5 - 10.0)
        w[row == 0] = 64.0 * (pos[row == 0] % 30 + 1)
        return w.astype(np.float32)
    if kind == "int2048":
        w = rng.integers(0, 2049, m).astype(np.float32)
        if m:
            w[rng.integers(0, m, 4)] = 2048.0
        return w
    if kind == "half_edges":
        vals = np.array([0.0, 2.0 ** -24, 2.0 ** -14, 1.0, 2047.0, 2048.0, 65504.0], dtype=np.float32)
        return vals[rng.integers(0, len(vals), m)]
    if kind == "negzero":
        return np.where(rng.random(m) < 0.5, np.float32(-0.0), np.float32(1.5)).astype(np.float32)
    if kind in ("one_inexact_long", "one_inexact_short"):
        w = rng.integers(0, 64, m).astype(np.float32)
        if kind == "one_inexact_long":
            rows = np.nonzero(deg >= UNIT)[0]
            if not len(rows):
                raise ValueError("one_inexact_long: no row of >= 64 entries")
            r = rows[np.argmin(deg[rows])]
            w[ro[r + 1] - 1] = 2049.0                                  # the LAST entry of the shortest such row
        else:
            rows = np.nonzero((deg >= 1) & (deg <= SHORT_ROW_MAX))[0]
            if not len(rows):
                raise ValueError("one_inexact_short: no short row")
            r = rows[np.argmax(deg[rows])]
            w[ro[r + 1] - 1] = 2049.0
        return w
    if kind == "half_inf":
        w = rng.integers(0, 64, m).astype(np.float32)
        w[rng.random(m) < 0.02] = 65520.0
        rows = np.nonzero(deg >= UNIT)[0]
        if len(rows):
            w[ro[rows[0]]] = 65520.0
        return w
    if kind == "subnormal":
        return (rng.integers(1, 1025, m).astype(np.float64) * 2.0 ** -149).astype(np.float32)
    if kind == "huge":
        return (rng.random(m) * 1e38).astype(np.float32)
    if kind == "mixed_range":
        return np.exp2(rng.integers(-60, 60, m).astype(np.float64)).astype(np.float32)
    raise KeyError(kind)


def unit_block_half_exact(ro, w, long_min):
    """does every weight of the rows of >= long_min entries (the rows the unit blocks hold) survive the round trip through half?"""
    deg = np.diff(ro)
    inside = np.repeat(deg >= long_min, deg)
    return bool(np.all(half_exact(np.asarray(w)[inside])))


def dijkstra_f64(ro, ci, w, src):
    """plain float64 Dijkstra; unreached: +inf"""
    import heapq
    n = len(ro) - 1
    dist = np.full(n, np.inf)
    dist[src] = 0.0
    w = np.asarray(w, dtype=np.float64)
    heap = [(0.0, int(src))]
    while heap:
        d, u = heapq.heappop(heap)
        if d > dist[u]:
            continue
        for e in range(ro[u], ro[u + 1]):
            v = ci[e]
            nd = d + w[e]
            if nd < dist[v]:
                dist[v] = nd
                heapq.heappush(heap, (nd, int(v)))
    return dist


def bfs_depth(ro, ci, src):
    """hops from src (-1: unreached)"""
    n = len(ro) - 1
    lab = np.full(n, -1, dtype=np.int64)
    lab[src] = 0
    front = np.array([src], dtype=np.int64)
    d = 0
    while len(front):
        d += 1
        cnt = (ro[front + 1] - ro[front]).astype(np.int64)
        if cnt.sum() == 0:
            break
        idx = np.repeat(ro[front].astype(np.int64) - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt) + np.arange(int(cnt.sum()))
        nb = np.unique(ci[idx])
        nb = nb[lab[nb] < 0]
        lab[nb] = d
        front = nb
    return lab
