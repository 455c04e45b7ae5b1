"""CPU suite: the inputs of tests/test_gpu_sssp_paths.py (tests/sssp_cases.py) are what they promise, and the reference the GPU is
judged by is right on them -- the oracle's float32 Dijkstra and its restatement of the reference's frontier loop agree bit for bit
on every graph x weight class, and where the path sums are exact in float32 a float64 Dijkstra written here gives the same values."""
import numpy as np
import pytest

from tests import sssp_cases as sc

FLT_MAX = sc.FLT_MAX


@pytest.fixture(scope="module")
def graphs(oracle):
    out = {"ladder": sc.ladder()}
    for scale in (10, 13):
        _, ro, ci, _ = oracle.rmat_csr(scale, 16, scale)
        out["rmat%d" % scale] = (ro, ci)
    return out


def _sources(ro):
    deg = np.diff(ro)
    short = np.nonzero((deg >= 1) & (deg <= 4))[0]
    return sorted({int(np.argmax(deg)), int(short[len(short) // 2]), 0})


def _same(a, b):
    return a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("name", ["ladder", "rmat10", "rmat13"])
def test_the_two_oracle_routines_agree_bit_for_bit(oracle, graphs, name, kind):
    ro, ci = graphs[name]
    w = sc.weights(kind, ro, ci, np.random.default_rng(sc.KINDS.index(kind)))
    assert w.dtype == np.float32 and len(w) == len(ci) and np.all(w >= 0) and np.all(np.isfinite(w))
    for src in _sources(ro):
        dj = oracle.sssp_dijkstra_f32(ro, ci, w, src)
        en, _, _ = oracle.sssp_enact(ro, ci, w, src, 8.0)
        assert _same(dj, en), (name, kind, src)
        assert dj[src] == 0 and np.all(dj <= FLT_MAX)
        if kind in sc.EXACT_SUMS:
            d64 = sc.dijkstra_f64(ro, ci, w, src)
            want = np.where(np.isinf(d64), np.float64(FLT_MAX), d64)
            assert np.array_equal(want.astype(np.float32).astype(np.float64), want), "a path sum that float32 cannot hold"
            assert np.array_equal(dj, want.astype(np.float32)), (name, kind, src)


def test_structural_graphs_oracles_agree(oracle):
    cases = []
    for shuffled in (False, True):
        ro, ci = sc.path(3000, shuffled)
        cases.append(("path", ro, ci, sc.weights("int2048", ro, ci, np.random.default_rng(1)), [0, 1500, 2999]))
    ro, ci = sc.grid(96, 96)
    cases.append(("grid", ro, ci, sc.weights("half_edges", ro, ci, np.random.default_rng(2)), [0, 96 * 48 + 48]))
    ro, ci = sc.grid(96, 96)
    cases.append(("grid", ro, ci, sc.weights("mixed_range", ro, ci, np.random.default_rng(2)), [96 * 96 - 1]))
    for centre in (0, 100000):
        ro, ci = sc.star(100000, centre)
        cases.append(("star", ro, ci, sc.weights("distinct", ro, ci, np.random.default_rng(3)), [centre, 5]))
    ro, ci, w = sc.bf_worst()
    cases.append(("bf_worst", ro, ci, w, [0, 700]))
    ro, ci, w = sc.dups_and_loops()
    cases.append(("dups", ro, ci, w, [0, 999]))
    ro, ci = sc.directed_with_sinks()
    cases.append(("dws", ro, ci, sc.weights("int2048", ro, ci, np.random.default_rng(4)), [sc.DWS_ROOT, sc.DWS_DEG0_SOURCE, sc.DWS_PAIR[0]]))
    for name, ro, ci, w, srcs in cases:
        assert np.all(np.diff(ro) >= 0) and ro[-1] == len(ci) == len(w)
        for v in range(0, len(ro) - 1, max(1, (len(ro) - 1) // 50)):
            assert np.all(np.diff(ci[ro[v]:ro[v + 1]]) >= 0), "rows are sorted"
        for src in srcs:
            dj = oracle.sssp_dijkstra_f32(ro, ci, w, src)
            en, _, _ = oracle.sssp_enact(ro, ci, w, src, 8.0)
            assert _same(dj, en), (name, src)


def test_ladder_rows_and_distinct_distances(oracle):
    ro, ci = sc.ladder()
    deg = np.diff(ro)
    h = len(sc.LADDER_DEGS)
    assert deg[0] == h and tuple(deg[1:h + 1]) == sc.LADDER_DEGS, "a hub lost its row length"
    leaves = sc.ladder_leaves(ro)
    assert np.all(deg[leaves] == 1) and len(leaves) == sum(sc.LADDER_DEGS) - h
    # every leaf is the entry of exactly one hub row
    hub_entries = ci[ro[1]:ro[h + 1]]
    assert np.array_equal(np.sort(hub_entries[hub_entries > h]), leaves)
    w = sc.weights("distinct", ro, ci, np.random.default_rng(0))
    assert np.all(sc.half_exact(w))
    dist = oracle.sssp_dijkstra_f32(ro, ci, w, 0)
    assert np.all(dist < FLT_MAX)
    assert len(np.unique(dist[leaves])) == len(leaves), "two leaves at the same distance: an entry could go missing unseen"
    assert len(np.unique(dist)) == len(dist)
    d64 = sc.dijkstra_f64(ro, ci, w, 0)
    assert np.array_equal(dist.astype(np.float64), d64), "a source-hub-leaf sum that is not exact in float32"
    # dropping any ONE hub entry changes exactly one distance (the leaf becomes unreachable): spot check around the unit boundary
    hub = 1 + sc.LADDER_DEGS.index(65)
    for e in (ro[hub] + 1, ro[hub] + 63, ro[hub + 1] - 1):
        w2 = w.copy(); ci2 = ci.copy()
        ci2[e] = hub                                                    # the entry now leads nowhere new
        d2 = oracle.sssp_dijkstra_f32(ro, ci2, w2, 0)
        assert int((d2 != dist).sum()) == 1 and d2[ci[e]] == FLT_MAX


@pytest.mark.parametrize("kind", sc.KINDS)
def test_weight_classes_are_as_half_exact_as_they_claim(graphs, kind):
    """the expected sweep variant of a class (sc.VARIANT) is 3 exactly when every weight inside the unit blocks -- the rows of at least
    long_min entries, for every long-row threshold the sweep takes -- survives numpy's float16 round trip"""
    for name, (ro, ci) in graphs.items():
        w = sc.weights(kind, ro, ci, np.random.default_rng(sc.KINDS.index(kind)))
        for long_min in (17, 32, 64):
            assert sc.unit_block_half_exact(ro, w, long_min) == (sc.VARIANT[kind] == 3), (name, kind, long_min)
        if kind in sc.ALL_HALF_EXACT:
            assert np.all(sc.half_exact(w))
        if kind in ("one_inexact_long", "one_inexact_short"):
            bad = np.nonzero(~sc.half_exact(w))[0]
            assert len(bad) == 1 and w[bad[0]] == 2049.0
            row = int(np.searchsorted(ro, bad[0], side="right") - 1)
            d = int(ro[row + 1] - ro[row])
            assert (d >= 64) if kind == "one_inexact_long" else (1 <= d <= sc.SHORT_ROW_MAX)
    # the edges of the format themselves
    assert np.all(sc.half_exact([0.0, -0.0, 2.0 ** -24, 2.0 ** -14, 1.0, 2047.0, 2048.0, 65504.0, 1.5]))
    assert not np.any(sc.half_exact([2049.0, 65520.0, 2.0 ** -25, 2.0 ** -149, 1e38, 65505.0]))
    assert sc.VARIANT["subnormal"] == 2 and np.all(sc.weights("subnormal", *graphs["rmat10"], np.random.default_rng(0)) < 2.0 ** -126)
    assert np.all(sc.weights("subnormal", *graphs["rmat10"], np.random.default_rng(0)) > 0)
    nz = sc.weights("negzero", *graphs["rmat10"], np.random.default_rng(0))
    assert np.any(np.signbit(nz)) and set(np.unique(np.abs(nz))) == {0.0, 1.5}
    assert np.any(sc.weights("half_inf", *graphs["rmat10"], np.random.default_rng(0)) == 65520.0)
    assert sc.weights("huge", *graphs["rmat10"], np.random.default_rng(0)).max() > 9e37


def test_overflow_chain_keeps_connected_vertices_at_flt_max(oracle):
    ro, ci, w = sc.overflow_chain()
    dj = oracle.sssp_dijkstra_f32(ro, ci, w, 0)
    en, _, _ = oracle.sssp_enact(ro, ci, w, 0, 8.0)
    assert _same(dj, en)
    one = np.float32(1e38)
    assert dj[0] == 0 and dj[1] == one and dj[2] == one + one and dj[3] == (one + one) + one and dj[3] < FLT_MAX
    assert np.all(dj[4:] == FLT_MAX) and np.all(sc.bfs_depth(ro, ci, 0) >= 0), "connected, and not reached"
    with np.errstate(over="ignore"):
        assert np.isinf(((one + one) + one) + one)


@pytest.mark.parametrize("n", sc.SIZED_NS)
def test_sized_graphs_hold_the_rows_and_units_they_promise(oracle, n):
    ro, ci = sc.sized(n)
    deg = np.diff(ro).astype(np.int64)
    assert len(deg) == n and ci.min() >= 0 and ci.max() < n
    assert np.all(np.diff(deg) <= 0), "out-degrees must not increase with the id (layout ids = ids)"
    long_rows = np.nonzero(deg >= 64)[0]
    assert len(long_rows) == min(n, 4)
    assert int(((deg[long_rows] + 63) // 64).sum()) >= 16, "fewer than 16 units: no sweep"
    assert np.all(deg[long_rows] % 64 == 1), "the last unit of a long row holds one entry"
    assert np.all(deg >= 1)
    # the ends of the tables receive entries, from long rows and from short ones
    t = sc.sized_targets(n)
    hit = np.bincount(ci, minlength=n)
    assert np.all(hit[t] >= 1)
    if n > 64:
        assert hit[t].sum() >= 0.45 * (len(ci) - n), "half of the entries outside the spine aim at the tables' ends"
        for end in (n, n & ~1, 32768, 73728):
            if 2 <= end <= n:
                assert hit[end - 1] and hit[end - 2] and (end >= n or hit[end])
    assert np.all(sc.bfs_depth(ro, ci, 0) >= 0), "everything is reached from vertex 0"
    w = sc.weights("int2048", ro, ci, np.random.default_rng(n))
    dj = oracle.sssp_dijkstra_f32(ro, ci, w, 0)
    en, _, _ = oracle.sssp_enact(ro, ci, w, 0, 8.0)
    assert _same(dj, en)


def test_structural_builders(oracle):
    ro, ci = sc.path(3000, True)
    order = sc.path_order(3000, True)
    lab = sc.bfs_depth(ro, ci, int(order[0]))
    assert np.array_equal(lab[order], np.arange(3000))
    ro, ci = sc.grid(96, 96)
    assert len(ci) == 2 * (2 * 96 * 95) and sc.bfs_depth(ro, ci, 0).max() == 190
    for centre in (0, 100000):
        ro, ci = sc.star(100000, centre)
        deg = np.diff(ro)
        assert deg[centre] == 100000 and deg.sum() == 200000 and np.all(np.delete(deg, centre) == 1)
    ro, ci, w = sc.bf_worst()
    en, _, st = oracle.sssp_enact(ro, ci, w, 0, 8.0)
    n = len(ro) - 1
    assert np.array_equal(en, np.arange(n, dtype=np.float32)), "the all-path route wins"
    assert st[0] >= n - 2, "... and arrives hop by hop (the last vertex has no row to expand)"
    assert st[2] >= 4 * n, "far vertices must enter the frontier many times"
    ro, ci, w = sc.dups_and_loops()
    key = np.repeat(np.arange(len(ro) - 1, dtype=np.int64), np.diff(ro)) * len(ro) + ci
    _, cnt = np.unique(key[np.repeat(np.arange(len(ro) - 1), np.diff(ro)) != ci], return_counts=True)
    assert np.all(cnt % 3 == 0)
    loops = np.repeat(np.arange(len(ro) - 1), np.diff(ro)) == ci
    assert np.any(w[loops] == 0) and np.any(w[loops] > 0)
    ro, ci = sc.directed_with_sinks()
    deg = np.diff(ro)
    lab = sc.bfs_depth(ro, ci, sc.DWS_ROOT)
    assert deg[sc.DWS_DEG0_SOURCE] == 0 and np.all(lab[-50:] < 0) and lab[sc.DWS_PAIR[0]] < 0
    assert np.any((deg == 0) & (lab > 0)) and lab[sc.DWS_DEG0_SOURCE] > 0
    assert np.array_equal(np.nonzero(sc.bfs_depth(ro, ci, sc.DWS_PAIR[0]) >= 0)[0], sc.DWS_PAIR)
