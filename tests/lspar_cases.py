"""Inputs of the fused sparsification's path tests, shared by the CPU suite (tests/test_lspar_cases_cpu.py: by
tests/lspar_model.py alone, each case has the property it was built for) and the GPU suite (tests/test_gpu_lspar_paths.py: fused
path == operator path == model on them).  numpy only; everything is generated from the thresholds handed in
(include/mgx/lspar_fused.hpp: rows of at most short_max entries take the group kernels, a longer row is cut into segments of seg
entries, a wave each).

Builders return (row_offsets, col_indices) as int32; rows are read as they stand (not sorted)."""
from fractions import Fraction

import numpy as np

from tests import lspar_model as model

SHORT_MAX, SEG, K_MAX = 64, 4096, 32                      # today's constants (the GPU suite passes LsparProblem.info()'s)
SEL_ROUNDS = 4                                            # register rounds of the short rows' select: short_max / 16 entries apart
KS = (1, 2, 3, 5, 6, 7, 8, 9, 12, 17, 31, 32)             # both lspar_sim bodies, every padding 0 .. 3, partial last chunks of 8
KEEP_ES = (Fraction(1, 2), Fraction(1, 3), Fraction(1, 4), Fraction(2, 3), Fraction(3, 4))
E_GRID = tuple(i / 256.0 for i in range(1, 256))          # where cut_e() looks


def stride(k):
    """columns of the fused minhash table"""
    return k if k <= 2 else (k + 3) & ~3


def edge_lengths(short_max=SHORT_MAX, seg=SEG):
    return (0, short_max - 1, short_max, short_max + 1, seg - 1, seg, seg + 1, 2 * seg, 2 * seg + 1)


def _csr_of_lengths(deg, rng, n):
    ro = np.concatenate([[0], np.cumsum(deg)])
    return ro.astype(np.int32), rng.integers(0, n, int(ro[-1])).astype(np.int32)


def length_edges(short_max=SHORT_MAX, seg=SEG, graph_seed=2, per=2, fill=301):
    """`per` rows of every length of edge_lengths() scattered among `fill` rows of 0 .. 8 entries, random neighbours
    -> (ro, ci, {length: its vertices})"""
    rng = np.random.default_rng(graph_seed)
    lengths = edge_lengths(short_max, seg)
    n = per * len(lengths) + fill
    deg = rng.integers(0, 9, n)
    at = rng.permutation(n)[:per * len(lengths)]
    by_length = {}
    for i, d in enumerate(lengths):
        by_length[d] = [int(v) for v in at[i * per:(i + 1) * per]]
        deg[by_length[d]] = d
    ro, ci = _csr_of_lengths(deg, rng, n)
    return ro, ci, by_length


def long_items(ro, short_max=SHORT_MAX, seg=SEG):
    """what the fused run lists: the segments of the rows longer than short_max"""
    d = np.diff(np.asarray(ro, dtype=np.int64))
    return int(((d[d > short_max] + seg - 1) // seg).sum())


def graded(k, d, period, levels, seed=model.SEED):
    """Vertex 0 has the entries 1 .. d.  A[j] is the vertex where hash function j takes its minimum over that row; neighbour u with
    period | u has the row A[:s], s = (u / period) % (levels + 1), so that it shares (at least) its first s minhashes with vertex 0;
    every other neighbour (and one with s = 0) has a lone self-loop.  -> (ro, ci): sim(0, u) takes every level 0 .. levels, spread evenly over the row"""
    assert 1 <= levels <= k
    n = d + 1
    ids = np.arange(1, n, dtype=np.int64)
    A = np.array([ids[np.argmin(model.keys(n, model.salt(seed, j))[1:])] for j in range(k)], dtype=np.int32)
    s = np.where(ids % period == 0, (ids // period) % (levels + 1), 0)
    deg = np.concatenate([[d], np.maximum(s, 1)])
    ro = np.concatenate([[0], np.cumsum(deg)])
    ci = np.empty(int(ro[-1]), dtype=np.int32)
    ci[:d] = ids
    for u, su in zip(ids, s):
        ci[ro[u]:ro[u + 1]] = A[:su] if su else u
    return ro.astype(np.int32), ci


def graded_long(k, seg=SEG, seed=model.SEED):
    """a hub of three full segments and five entries, about (3 seg / 37) / (k + 1) entries at every level above 0"""
    return graded(k, 3 * seg + 5, 37, k, seed)


def graded_short(k, short_max=SHORT_MAX, seed=model.SEED):
    """a row of exactly short_max entries whose levels 0 .. min(k, 3) each recur in every register round of the short select"""
    return graded(k, short_max, 1, min(k, 3), seed)


def row_sims(ro, ci, seed, k, v=0):
    mh = model.minhashes(ro, ci, seed, k)
    row = np.asarray(ci[ro[v]:ro[v + 1]], dtype=np.int64)
    return (mh[row] == mh[v]).sum(axis=1).astype(np.int64)


def cut_of(sims, t):
    """the select's arithmetic on one row: -> (cut level c, q = entries of level c kept, positions of the level-c entries)"""
    k = int(sims.max())
    ge = np.array([(sims >= c).sum() for c in range(k + 2)])
    c = max(c for c in range(k + 1) if ge[c] >= t)
    return c, int(t - ge[c + 1]), np.nonzero(sims == c)[0]


def cut_place(sims, t, k, chunk):
    """where the cut of a row falls among its chunks (segments of a long row, register rounds of a short one): None unless the cut
    level lies strictly inside 0 .. k, strictly inside its level, and the level has entries in several chunks; else "first" / "last"
    when the q-th entry of the level is in the first / last chunk that holds entries of the level, "middle" when the level has
    entries in chunks on both sides of it"""
    c, q, at = cut_of(sims, t)
    if not (0 < c < k and 0 < q < len(at)):
        return None
    chunks = at // chunk
    mine = chunks[q - 1]
    before, after = bool((chunks < mine).any()), bool((chunks > mine).any())
    if before and after:
        return "middle"
    return "first" if after else ("last" if before else None)


def cut_e(sims, k, chunk, place):
    """the first e of E_GRID that puts the row's cut at `place` (None: there is none)"""
    d = len(sims)
    for e in E_GRID:
        t = int(model.keep_count(d, e))
        if 0 < t < d and cut_place(sims, t, k, chunk) == place:
            return e
    return None


def keep_degrees(squares=128, cubes=40, fourths=16):
    """j^p - 1, j^p, j^p + 1 for p = 2, 3, 4: where floor(pow(d, a / b)) sits on either side of an integer"""
    out = set()
    for p, top in ((2, squares), (3, cubes), (4, fourths)):
        for j in range(2, top + 1):
            out.update((j ** p - 1, j ** p, j ** p + 1))
    return np.array(sorted(out), dtype=np.int64)


def keep_count_edges(graph_seed=3, **tops):
    """one row of every degree of keep_degrees(), random neighbours -> (ro, ci)"""
    rng = np.random.default_rng(graph_seed)
    deg = keep_degrees(**tops)
    return _csr_of_lengths(deg, rng, len(deg))


def exact_keep(d, e):
    """t = the largest integer with t^b <= d^a for e = a / b <= 1 (a Fraction), by integer arithmetic alone"""
    a, b = e.numerator, e.denominator
    assert 0 < a <= b
    out = np.zeros(len(d), dtype=np.int64)
    for i, x in enumerate(int(x) for x in d):
        if x <= 0:
            continue
        target = x ** a
        lo, hi = 0, x + 1                                   # lo^b <= target < hi^b (a <= b), halved to hi == lo + 1
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if mid ** b <= target:
                lo = mid
            else:
                hi = mid
        out[i] = lo
    return out


PLACES = ("first", "middle", "last")


def graded_params(ro, ci, seed, k, chunk):
    """the (k, e) a graded case runs with: an e per place of the cut; k = 1 has no level strictly inside 0 .. k, so it runs with the
    default e only.  -> [(place or None, e)]"""
    if k < 2:
        return [(None, model.E)]
    sims = row_sims(ro, ci, seed, k)
    return [(place, cut_e(sims, k, chunk, place)) for place in PLACES]
