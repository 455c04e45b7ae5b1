"""numpy model of the vertex similarity (include/mgx/sim_fused.hpp): the definition the fused path and the operator
path must both reproduce.

    graph:    the underlying simple undirected graph of the triangle count (tests/tc_model.py): N(v) = the distinct neighbours of v
              other than v, original ids, d(v) = |N(v)| = sdeg[v]; `symmetric` as there.  Its sorted adjacency is k-truss's
              (tests/ktruss_model.py: adjacency)
    pairs:    P pairs (u, v); None: EDGES MODE, the m_dag edges (src[e], dag_ci[e]) in the order of mgx_ktruss_edges
    common:   c = |N(u) & N(v)| (int32); u == v: c = d(u)
    scores:   float64, by the measure:
                common    c
                jaccard   c / (d(u) + d(v) - c)         overlap   c / min(d(u), d(v))
                sorensen  2 c / (d(u) + d(v))          cosine    c / sqrt(d(u) d(v))        (each 0 where its denominator is 0)
                weighted  the sum of x[w] over the common w, x float64[n]: here math.fsum, the correctly rounded sum; the device
                          sums in a fixed order of its own and stays within c 2^-52 sum |x[w]| of it
    stats:    pairs, the sum of c, pairs with c > 0, adjacency entries (2 m_dag), the longest simple row
    classes:  by la = the shorter row's length and lb = the longer's (classify): none (la == 0), lane (la <= short_max), probe
              (lb >= probe_ratio la), wave (la <= wave_max), block
"""
import math

import numpy as np

from tests import ktruss_model, tc_model

MEASURES = ("common", "jaccard", "overlap", "sorensen", "cosine", "weighted")
STAT_KEYS = ("pairs", "common", "positive", "entries", "longest_row")
NONE, LANE, PROBE, WAVE, BLOCK = range(5)
BIN_KEYS = ("none", "lane", "probe", "wave", "block")
SHORT_MAX, PROBE_RATIO, WAVE_MAX, STAGE = 16, 8, 512, 4096
WAVE_STAGE, BLOCK_STAGE = 512, 4096


def adjacency(row_offsets, col_indices, symmetric):
    """-> (src int32[m_dag], dst int32[m_dag], adj_ro int32[n + 1], adj_ci int32[2 m_dag]): the edges and the sorted simple adjacency"""
    dag_ro, dag_ci, _ = tc_model.dag(row_offsets, col_indices, symmetric)
    src, adj_ro, adj_ci, _ = ktruss_model.adjacency(dag_ro, dag_ci)
    return src, dag_ci, adj_ro, adj_ci


def degrees(row_offsets, col_indices, symmetric):
    return np.diff(adjacency(row_offsets, col_indices, symmetric)[2]).astype(np.int32)


def weights(kind, d):
    """x of Adamic-Adar (1 / ln d, 0 where d < 2) and of resource allocation (1 / d, 0 where d == 0), as SimilarityProblem builds them"""
    d = np.asarray(d).astype(np.float64)
    x = np.zeros(len(d), dtype=np.float64)
    if kind == "adamic_adar":
        x[d >= 2] = 1.0 / np.log(d[d >= 2])
    else:
        x[d > 0] = 1.0 / d[d > 0]
    return x


def classify(la, lb, short_max=SHORT_MAX, probe_ratio=PROBE_RATIO, wave_max=WAVE_MAX, stage=STAGE):
    """sim_class of every (la, lb), la <= lb"""
    la, lb = np.asarray(la, dtype=np.int64), np.asarray(lb, dtype=np.int64)
    return np.where(la == 0, NONE, np.where(la <= short_max, LANE, np.where(lb >= probe_ratio * la, PROBE, np.where(la <= wave_max, WAVE, BLOCK))))


def score(measure, c, du, dv):
    """float64 of every pair: one numpy division of exact integers each; the cosine one multiplication, one root, one division"""
    c, du, dv = (np.asarray(a, dtype=np.int64) for a in (c, du, dv))
    if measure == "common":
        return c.astype(np.float64)
    if measure == "cosine":
        den = np.sqrt(du.astype(np.float64) * dv.astype(np.float64))
        num = c
    else:
        num, den = {"jaccard": (c, du + dv - c), "overlap": (c, np.minimum(du, dv)), "sorensen": (2 * c, du + dv)}[measure]
    out = np.zeros(len(c), dtype=np.float64)
    ok = den != 0
    out[ok] = num[ok].astype(np.float64) / np.asarray(den, dtype=np.float64)[ok]
    return out


def common_of(adj_ro, adj_ci, u, v):
    """the common neighbours of one pair, ascending (the shorter row searched in the longer)"""
    a, b = adj_ci[adj_ro[u]:adj_ro[u + 1]], adj_ci[adj_ro[v]:adj_ro[v + 1]]
    if len(a) > len(b):
        a, b = b, a
    if len(a) == 0:
        return a
    pos = np.minimum(np.searchsorted(b, a), len(b) - 1)
    return a[b[pos] == a]


def similarity(row_offsets, col_indices, pairs=None, measure="jaccard", x=None, symmetric=True, **opts):
    """-> {"pairs" int32[P, 2], "common" int32[P], "scores" float64[P], "abs" float64[P] (weighted: the sum of |x[w]|, for the bound),
    "la", "lb", "classes" int64[P], "stats" {STAT_KEYS}, "bins" {BIN_KEYS}}"""
    src, dst, adj_ro, adj_ci = adjacency(row_offsets, col_indices, symmetric)
    n = len(adj_ro) - 1
    pr = np.stack([src, dst], axis=1) if pairs is None else np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(pr) and (pr.min() < 0 or pr.max() >= n):
        raise ValueError("a pair names a vertex outside [0, n)")
    d = np.diff(adj_ro.astype(np.int64))
    P = len(pr)
    c = np.zeros(P, dtype=np.int64)
    sums, mags = np.zeros(P, dtype=np.float64), np.zeros(P, dtype=np.float64)
    for p in range(P):
        w = common_of(adj_ro, adj_ci, int(pr[p, 0]), int(pr[p, 1]))
        c[p] = len(w)
        if measure == "weighted":
            sums[p] = math.fsum(x[w].tolist())
            mags[p] = math.fsum(np.abs(x[w]).tolist())
    du, dv = d[pr[:, 0]], d[pr[:, 1]]
    la, lb = np.minimum(du, dv), np.maximum(du, dv)
    cl = classify(la, lb, **opts)
    return {"pairs": pr.astype(np.int32), "common": c.astype(np.int32), "scores": sums if measure == "weighted" else score(measure, c, du, dv),
            "abs": mags, "la": la, "lb": lb, "classes": cl,
            "stats": {"pairs": P, "common": int(c.sum()), "positive": int((c > 0).sum()), "entries": int(len(adj_ci)),
                      "longest_row": int(d.max()) if n else 0},
            "bins": {k: int((cl == i).sum()) for i, k in enumerate(BIN_KEYS)}}


def weighted_bound(c, mags):
    """|device - fsum| <= c 2^-52 sum |x[w]|: the standard bound of c - 1 additions in any order, doubled"""
    return np.asarray(c, dtype=np.float64) * 2.0 ** -52 * np.asarray(mags, dtype=np.float64)


def ulps(got, want):
    """the distance of two float64 arrays in units of the last place of `want`"""
    return np.abs(np.asarray(got) - np.asarray(want)) / np.spacing(np.abs(np.asarray(want)))


def search_cap(lb):
    """loads of one binary search in a row of lb entries: floor(log2 lb) + 1 <= ceil(log2 lb) + 1"""
    return int(lb).bit_length()


def entries_read_cap(la, lb, cl, stage=STAGE):
    """the adjacency entries the pair kernels may load for one pair.  lane, probe: per entry of the short row itself and one search.
    wave, block: the short row once and the long row ONCE, plus two bound searches per chunk when the short row takes several"""
    la, lb = int(la), int(lb)
    if cl == NONE:
        return 0
    if cl in (LANE, PROBE):
        return la * (1 + search_cap(lb))
    s = min(stage, WAVE_STAGE if cl == WAVE else BLOCK_STAGE)
    chunks = (la + s - 1) // s
    return la + lb + (2 * chunks * search_cap(lb) if chunks > 1 else 0)
