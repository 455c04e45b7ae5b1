"""CPU suite: the inputs and the reference of PageRank's path tests (tests/pagerank_cases.py) are what tests/test_gpu_pagerank_paths.py
takes them for -- the builder delivers the in-row lengths it promises, the rounded float64 model is what float32 sums give in ANY
order (bit for bit where the case says exact, within the derived leaf tolerance elsewhere), and a dropped, doubled or misindexed
entry of every special row changes that row's float32 rank: the comparison can see the faults it is there for."""
import math
import os
import re

import numpy as np
import pytest

from tests import pagerank_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {
    "directed": lambda: pc.edge_case(True),
    "symmetric": lambda: pc.edge_case(False),
    "layout": lambda: pc.edge_case(False, True),
    "many_huge": pc.many_huge,
    "capacity1": lambda: pc.capacity_case(1),
    "capacity64": lambda: pc.capacity_case(64),
    "chunked_fold": pc.chunked_fold_case,
}


def test_constants_are_the_headers():
    text = open(os.path.join(ROOT, "include", "mgx", "pagerank_fused.hpp")).read()
    for name, value in (("PGR_LANE_MAX", pc.LANE_MAX), ("PGR_HUGE_MIN", pc.HUGE_MIN), ("PGR_HUGE_BLOCKS", pc.HUGE_BLOCKS)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1)) == value, name
    text = open(os.path.join(ROOT, "include", "mgx", "nreduce.hpp")).read()
    m = re.search(r"NRS_FOLD_DEG\[3\]\s*=\s*\{\s*(\d+),\s*(\d+),\s*(\d+)\s*\}", text)
    assert m and (int(m.group(2)), int(m.group(1))) == pc.FOLD_TIERS, m and m.groups()


def test_edge_lengths_are_the_listed_ones():
    general = [0, 1, 15, 16, 17, 18, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 8191, 8192, 8193,
               8192 + 255, 8192 + 256, 8192 + 257, 8192 + 511, 8192 + 512, 8192 + 513, 3 * 8192 + 5]
    assert sorted(pc.edge_lengths()) == general and len(set(general)) == len(general)
    assert sorted(pc.edge_lengths(True)) == sorted(general + [4095, 4096, 4097, 65535, 65536, 65537])
    # every remainder class of the two unrolled loops: whole trips, one step left, a step and the tail, the tail alone
    wave = {(d % 128) for d in general if pc.LANE_MAX < d < pc.HUGE_MIN}
    assert {0, 1, 63, 64, 65, 127} <= wave
    block = {(d % 512) for d in general if d >= pc.HUGE_MIN}
    assert {0, 1, 255, 256, 257, 511} <= block
    # a retuned threshold moves the edges with it
    assert {31, 32, 33, 34, 4095, 4096, 4097} <= set(pc.edge_lengths(False, 32, 4096))
    assert set(pc.chunked_fold_lengths()) >= {4095, 4096, 4097, 65537} and sum(pc.chunked_fold_lengths()) * 2 < 500000


@pytest.mark.parametrize("name", list(CASES))
def test_builder_delivers_what_it_promises(name):
    c = CASES[name]()
    n = c.n
    assert n & (n - 1) == 0 and n < 1 << 23 and len(c.ro) == n + 1 and c.ro.dtype == np.int32 and c.ci.dtype == np.int32
    assert len(set(c.hubs.tolist())) == len(c.hubs) == len(c.lengths)
    assert np.array_equal(c.in_len[c.hubs], c.lengths)
    leaves = np.unique(c.src)
    assert not np.intersect1d(leaves, c.hubs).size
    total = int(c.lengths.sum())
    assert int(c.ro[-1]) == len(c.ci) == total * (1 if c.directed else 2)
    assert c.ci.min() >= 0 and c.ci.max() < n
    if c.symmetric:
        assert np.array_equal(c.out_deg[c.hubs], c.lengths)                  # the hub's row IS its in-row
        # every entry has its reverse, with multiplicity
        rows = np.repeat(np.arange(n), c.out_deg)
        fwd = np.sort(rows.astype(np.int64) * n + c.ci)
        rev = np.sort(c.ci.astype(np.int64) * n + rows)
        assert np.array_equal(fwd, rev)
    else:
        assert (c.out_deg[c.hubs] == 0).all()                                # hubs dangle
    d = c.out_deg[leaves]
    assert (d > 0).all() and ((d & (d - 1)) == 0).all(), "leaf out-degrees are powers of two"
    assert len(np.unique(d)) >= 3 and int(c.lengths.max()) * int(d.max()) <= 1 << 24
    # everything else is isolated
    rest = np.ones(n, dtype=bool)
    rest[c.hubs] = False
    rest[leaves] = False
    assert (c.out_deg[rest] == 0).all() and (c.in_len[rest] == 0).all()
    assert c.dangling == int(rest.sum()) + (len(c.hubs) if c.directed else int((c.lengths == 0).sum()))
    # rows sorted by neighbour
    rows = np.repeat(np.arange(n, dtype=np.int64), c.out_deg)
    key = rows * n + c.ci
    assert (np.diff(key) >= 0).all()
    # a hub's sources have mixed out-degrees: a misindexed read can change its sum
    tgt, src = c.in_entries()
    for h, L in zip(c.hubs, c.lengths):
        if L >= 64:
            assert len(np.unique(c.out_deg[src[tgt == h]])) >= 2, L


def test_case_shapes():
    c = pc.edge_case(True)
    assert c.huge_rows() == sum(1 for d in pc.edge_lengths() if d >= pc.HUGE_MIN) == 9
    m = pc.many_huge()
    assert m.huge_rows() == 130 > 2 * pc.HUGE_BLOCKS and 1000000 < len(m.ci) < 1200000
    for k in (1, 64):
        cap = pc.capacity_case(k)
        assert cap.huge_rows() == k and len(cap.ci) // pc.HUGE_MIN + 1 == k + 1 and (cap.in_len[cap.in_len > 0] == pc.HUGE_MIN).all()
    f = pc.chunked_fold_case()
    assert f.n == 1 << 20 and len(f.ci) < 500000 and f.symmetric


def _float32_run(c, rng):
    """one iteration as the kernels compute it, the in-entries accumulated in float32 in a random order"""
    n = c.n
    r0 = np.float32(1.0 / n)
    contrib = np.zeros(n, dtype=np.float32)
    np.divide(r0, c.out_deg.astype(np.float32), out=contrib, where=c.out_deg > 0)
    tgt, src = c.in_entries()
    p = rng.permutation(len(tgt))
    S = np.zeros(n, dtype=np.float32)
    np.add.at(S, tgt[p], contrib[src[p]])
    assert S.dtype == np.float32
    D = c.dangling * float(r0)
    return ((1.0 - pc.ALPHA) / n + pc.ALPHA * (S.astype(np.float64) + D / n)).astype(np.float32)


@pytest.mark.parametrize("name", list(CASES))
def test_float32_sums_in_any_order_give_the_reference(name):
    c = CASES[name]()
    rng = np.random.default_rng(5)
    seen = []
    for _ in range(3):
        got = _float32_run(c, rng)
        bad, hub_lengths = c.differing(got)
        assert not bad.size, "%d ranks differ; hubs of in-length %s" % (bad.size, hub_lengths)
        assert np.array_equal(got[c.exact].view(np.uint32), c.want[c.exact].view(np.uint32))
        seen.append(int((got != c.want).sum()))
        # e_1 of these ranks in three orders, pairwise and correctly rounded: one value
        x = np.abs(got.astype(np.float64) - 1.0 / c.n)
        sums = {float(np.add.reduce(x[rng.permutation(c.n)])) for _ in range(3)} | {float(x.sum()), math.fsum(x), pc.want_e1(got, c.n)}
        for k in range(3):                                                   # ... and strictly left to right
            sums.add(float(np.cumsum(x[rng.permutation(c.n)])[-1]))
        assert len(sums) == 1, sums
        if c.directed:
            assert sums == {c.e1}
    print(name, "ranks off the rounded model in the last bit (leaves of a symmetric graph):", seen)
    if c.directed:
        assert seen == [0, 0, 0]
    assert c.e1 == pc.want_e1(c.want, c.n) and 0.0 < c.e1 < 2.0


@pytest.mark.parametrize("name", ["directed", "symmetric", "layout", "many_huge", "chunked_fold"])
def test_a_faulty_read_of_a_special_row_changes_its_rank(name):
    """drop the last entry, double the first, read one source of another out-degree in place of one: the hub's float32 rank moves,
    at the longest hub by at least 16 ulp.  (A length that fails this has wrong inputs, not a tight tolerance.)"""
    c = CASES[name]()
    n = c.n
    r0 = float(np.float32(1.0 / n))
    contrib = np.zeros(n, dtype=np.float64)
    np.divide(r0, c.out_deg, out=contrib, where=c.out_deg > 0)
    share = c.dangling * r0 / n
    tgt, src = c.in_entries()
    order = np.argsort(tgt, kind="stable")
    first = np.concatenate([[0], np.cumsum(np.bincount(tgt, minlength=n))])
    by_degree = {int(d): int(v) for v, d in zip(c.src[::-1], c.out_deg[c.src[::-1]])}       # a leaf of every out-degree

    def rank(S):
        return np.float32((1.0 - pc.ALPHA) / n + pc.ALPHA * (S + share))

    longest = int(c.lengths.max())
    for h, L in zip(c.hubs, c.lengths):
        if L == 0:
            continue
        s = src[order[first[h]:first[h + 1]]]
        assert len(s) == L
        S = float(contrib[s].sum())
        assert rank(S) == c.want[h]
        other = next(v for d, v in sorted(by_degree.items()) if d != c.out_deg[s[L // 2]])
        faults = {"dropped": S - contrib[s[-1]], "doubled": S + contrib[s[0]], "misindexed": S - contrib[s[L // 2]] + contrib[other]}
        for what, Sf in faults.items():
            moved = abs(float(rank(Sf)) - float(c.want[h]))
            assert moved > 0.0, (what, L)
            if L == longest:
                ulp = float(np.spacing(c.want[h]))
                print("%s: longest hub %d, %s entry moves its rank by %.1f ulp (%.3g relative)" % (name, L, what, moved / ulp, moved / float(c.want[h])))
                assert moved >= 16 * ulp, (what, L, moved / ulp)
