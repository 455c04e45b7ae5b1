"""Inputs and the exact reference of PageRank's path tests, shared by the CPU suite (tests/test_pagerank_cases_cpu.py: the builder
yields what it promises, the reference does not depend on the order of the sums, a faulty read would show) and the GPU suite
(tests/test_gpu_pagerank_paths.py).  numpy only; everything is generated.

Why one iteration can be compared bit for bit: with alpha = 1/2, n a power of two and every SOURCE's out-degree a
power of two, r_0 / d(u) is 2^-k.  A row of L such terms, the largest out-degree being dmax, sums to a multiple of r_0 / dmax below
L * r_0: at most log2(L * dmax) bits, so with L * dmax <= 2^24 every partial sum in ANY order is a float32 and no addition rounds.
The update computes base + alpha * (S + D / n) in double -- exact: D is a count times r_0, everything spans far fewer than 53 bits --
and rounds to float32 once.  pagerank_model.ranks does the same operations in float64, so the ranks must be bit-equal to its r_1
rounded to float32.  |r_1 - r_0| of float32 ranks >= (1 - alpha) / n are multiples of ulp((1 - alpha) / n) (2^-41 at n = 2^17) with
a sum below 2: e_1 is exact in double in any order as well.

The graphs are bipartite "leaves -> hubs": one hub per requested in-row length, leaves with power-of-two out-degrees that fill the
hubs' in-rows exactly, every other vertex isolated (dangling).  Directed, the in-rows come from the graph's genuine CSC and every
vertex is exact.  Symmetric (every reverse added) the hubs' terms are still powers of two, but a LEAF sums up to max(out_degrees) terms
r_0 / L of its hubs, rounded float32 quotients: leaves are compared at LEAF_RTOL."""
import functools

import numpy as np

from tests import pagerank_model as model

N = 1 << 17                         # r_0 = 2^-17; ids stay below 2^23 (the layout's 24-bit unit blocks)
ALPHA = 0.5
LANE_MAX, HUGE_MIN, HUGE_BLOCKS = 16, 8192, 64      # include/mgx/pagerank_fused.hpp: PGR_LANE_MAX, PGR_HUGE_MIN, PGR_HUGE_BLOCKS
WAVE, BLOCK = 64, 256                                # include/mgx/wave.hpp: a wave's / a workgroup's entries per step of the unrolled loops
FOLD_TIERS = (4096, 65536)                           # include/mgx/nreduce.hpp: NRS_FOLD_DEG, the tiers of k_nrs_fold above 256 entries
OUT_DEGREES = (1, 2, 4, 8)
# a leaf of a symmetric graph: 1 ulp per rounded quotient r_0 / L, at most 7 float32 additions of positive terms (8 terms), the final
# rounding; 12 * 2^-24 covers the 9 half-ulp steps with room for the second-order terms.  Derived, not measured.
LEAF_RTOL = 12 * 2.0 ** -24


def edge_lengths(layout=False, lane_max=LANE_MAX, huge_min=HUGE_MIN):
    """in-row lengths at every edge of the general reduce (k_pagerank_reduce, k_pagerank_reduce_huge):
      lane | wave                       0, 1, lane_max - 1 .. lane_max + 2
      the wave loop (two steps of 64 entries a trip, then `if (e < e1)`): every remainder class around 64, 128, 192, 256
      wave | huge                       huge_min - 1 .. huge_min + 1
      the workgroup loop (two steps of 256 a trip, the same tail): huge_min + 255 .. 257 and + 511 .. 513
      a row of three whole trips of the huge threshold and five entries
    layout=True adds the tiers of k_nrs_fold (nreduce_cases.edge_degrees): 4095 .. 4097, 65535 .. 65537"""
    out = [0, 1, lane_max - 1, lane_max, lane_max + 1, lane_max + 2]
    for k in (1, 2, 3, 4):
        out += [k * WAVE - 1, k * WAVE, k * WAVE + 1]
    out += [huge_min - 1, huge_min, huge_min + 1]
    for k in (1, 2):
        out += [huge_min + k * BLOCK - 1, huge_min + k * BLOCK, huge_min + k * BLOCK + 1]
    out.append(3 * huge_min + 5)
    if layout:
        for t in FOLD_TIERS:
            out += [t - 1, t, t + 1]
    return tuple(out)


def bipartite(lengths, n=N, out_degrees=OUT_DEGREES, seed=0):
    """(src, dst, hubs): the entries leaf -> hub.  hubs[i] has exactly lengths[i] in-entries; hub ids are drawn over the whole id
    range, leaves from the rest.  Every leaf has a power-of-two number of out-entries drawn from out_degrees; what the last drawn
    leaf would overshoot is filled by leaves of ONE entry each (fewer than max(out_degrees) of them).  The entries are dealt to the
    leaves in random order, so a leaf's hubs are random (parallel entries happen and count) and a hub's sources have mixed degrees."""
    lengths = np.asarray(lengths, dtype=np.int64)
    degs = np.asarray(sorted(out_degrees), dtype=np.int64)
    assert len(degs) >= 2 and (degs > 0).all() and ((degs & (degs - 1)) == 0).all(), "out-degrees are powers of two"
    assert n & (n - 1) == 0 and n < 1 << 23
    assert int(lengths.max()) * int(degs.max()) <= 1 << 24, "a row's sum must fit float32's 24 bits"
    rng = np.random.default_rng(seed)
    hubs = rng.choice(n, len(lengths), replace=False).astype(np.int64)
    total = int(lengths.sum())
    draw = rng.choice(degs, total // int(degs.min()) + 1)
    cum = np.cumsum(draw)
    k = int(np.searchsorted(cum, total, side="right"))              # the first k leaves fit
    rest = total - (int(cum[k - 1]) if k else 0)
    leaf_deg = np.concatenate([draw[:k], np.ones(rest, dtype=np.int64)])
    assert int(leaf_deg.sum()) == total and len(np.unique(leaf_deg)) >= 3, "at least three different out-degrees"
    others = np.setdiff1d(np.arange(n, dtype=np.int64), hubs)
    assert len(leaf_deg) <= len(others), "%d leaves do not fit beside %d hubs in %d ids" % (len(leaf_deg), len(hubs), n)
    leaves = rng.choice(others, len(leaf_deg), replace=False)
    src = np.repeat(leaves, leaf_deg)
    dst = rng.permutation(np.repeat(hubs, lengths))
    return src, dst, hubs


def csr(n, src, dst, directed):
    """(ro, ci) int32, rows sorted by neighbour, parallel entries kept.  directed: the entries src -> dst only; else every reverse too"""
    s, d = (src, dst) if directed else (np.concatenate([src, dst]), np.concatenate([dst, src]))
    order = np.lexsort((d, s))
    ro = np.concatenate([[0], np.cumsum(np.bincount(s, minlength=n))])
    assert ro[-1] == len(s) < 2 ** 31
    return ro.astype(np.int32), d[order].astype(np.int32)


def want32(ro, ci, symmetric):
    """r_1 of the float64 model at alpha = 1/2, rounded to float32 once"""
    return model.ranks(ro, ci, ALPHA, 0.0, 1, symmetric)[0].astype(np.float32)


def want_e1(r1, n):
    """e_1 = sum |r_1 - r_0| of float32 ranks r_1, exact in double in any order (the head of this file).  Of want32 it is what a run
    whose every rank is bit-equal must report; of a run's own ranks it is what that run must report whatever its leaves' last bits.
    NOT the model's own e_1: that is taken of the unrounded r_1."""
    return float(np.abs(np.asarray(r1, dtype=np.float32).astype(np.float64) - 1.0 / n).sum())


def exact_mask(n, src, symmetric):
    """vertices compared bit for bit: all of a directed graph; of a symmetric one all but the leaves (hubs and isolated vertices)"""
    mask = np.ones(n, dtype=bool)
    if symmetric:
        mask[src] = False
    return mask


class Case:
    """one graph with everything the tests compare against, computed once"""

    def __init__(self, lengths, directed, n=N, out_degrees=OUT_DEGREES, seed=0):
        self.n, self.directed, self.symmetric = n, directed, not directed
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.src, self.dst, self.hubs = bipartite(lengths, n, out_degrees, seed)
        self.ro, self.ci = csr(n, self.src, self.dst, directed)
        self.out_deg = np.diff(self.ro).astype(np.int64)
        # the rows the reduce walks: the CSC's when directed (mgx_graph_build_csc), the CSR's own when symmetric
        self.in_len = np.bincount(self.dst, minlength=n).astype(np.int64) if directed else self.out_deg
        self.dangling = int((self.out_deg == 0).sum())
        self.want = want32(self.ro, self.ci, self.symmetric)
        self.want.setflags(write=False)
        self.exact = exact_mask(n, self.src, self.symmetric)
        self.e1 = want_e1(self.want, n)

    def in_entries(self):
        """(target, source) of every in-entry, grouped by target (model order)"""
        return model.in_entries(self.ro, self.ci, self.symmetric)

    def huge_rows(self, huge_min=HUGE_MIN):
        return int((self.in_len >= huge_min).sum())

    def leaf_bound(self):
        """|got - want| allowed per vertex: 0 on the exact mask, LEAF_RTOL * want elsewhere"""
        return np.where(self.exact, 0.0, LEAF_RTOL * self.want.astype(np.float64))

    def differing(self, got):
        """(vertices outside the comparison, the in-row lengths of the hubs among them)"""
        bad = ~(np.abs(got.astype(np.float64) - self.want.astype(np.float64)) <= self.leaf_bound())     # (a NaN is outside)
        bad |= self.exact & (got.view(np.uint32) != self.want.view(np.uint32))          # (bit for bit: -0.0, NaN)
        hub_bad = sorted(int(self.in_len[h]) for h in self.hubs if bad[h])
        return np.nonzero(bad)[0], hub_bad


@functools.lru_cache(maxsize=None)
def edge_case(directed, layout=False, n=N, seed=0):
    """one hub per edge_lengths(layout) over n vertices"""
    return Case(edge_lengths(layout), directed, n=n, seed=seed)


@functools.lru_cache(maxsize=None)
def many_huge(n=N, rows=130):
    """rows hubs of huge_min + i entries -- more than two trips of k_pagerank_reduce_huge's 64-workgroup stride over its list --, leaf
    degrees 8 and 16 (and the ones that fill up); directed, about 1.1 M entries"""
    return Case([HUGE_MIN + i for i in range(rows)], True, n=n, out_degrees=(8, 16), seed=rows)


@functools.lru_cache(maxsize=None)
def capacity_case(k, n=N):
    """k hubs of exactly huge_min entries and nothing else: the huge list's capacity in_entries / huge_min + 1 is k + 1 for k rows"""
    return Case([HUGE_MIN] * k, True, n=n, out_degrees=(4, 8, 16), seed=100 + k)


def chunked_fold_lengths():
    """the edge lengths with the fold's 4096 tier and one row above 65536: a symmetric graph of under 0.5 M entries"""
    return edge_lengths(False) + (FOLD_TIERS[0] - 1, FOLD_TIERS[0], FOLD_TIERS[0] + 1, FOLD_TIERS[1] + 1)


@functools.lru_cache(maxsize=None)
def chunked_fold_case(n=1 << 20):
    return Case(chunked_fold_lengths(), False, n=n, seed=20)
