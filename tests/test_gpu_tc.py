"""GPU suite (-m gpu): triangle counting (mgx_tc_*).  The fused path (mgx_tc_run), the operator path (mgx_tc_enact)
and the numpy / scipy model (tests/tc_model.py) agree bit for bit -- tri, sdeg, the DAG arrays and stats [0] - [4] -- on the golden
fixtures, R-MAT 10 - 18 symmetric and directed, hand-made shapes, every bin and the chunked stage forced on small graphs, and, at
full size, RMAT-20 (fused == operator path), RMAT-22 (identities and a sampled CPU check), uniform-18 and grid2d-18."""
import os
from math import comb

import numpy as np
import pytest

from tests import coloring_model as cm
from tests import tc_model as model
from tests.grid_cus import one_cu_context

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["bfs_test.mtx", "kcore_test.mtx", "pr_test.mtx", "sssp_test.mtx", "synthetic_dup.mtx"]
KEYS = model.STAT_KEYS


def _graph(ctx, ro, ci, layout=False):
    import mini_amd
    g = mini_amd.Graph.from_host(ctx, ro, ci, None)
    if layout:
        g.build_layout()
    return g


def _arrays(tp):
    dro, dci = tp.dag()
    return {"tri": tp.triangles(), "sdeg": tp.simple_degrees(), "dag_ro": dro, "dag_ci": dci}


def _same(got, want, who):
    for k in ("tri", "sdeg", "dag_ro", "dag_ci"):
        assert got[k].dtype == want[k].dtype, (who, k, got[k].dtype, want[k].dtype)
        assert np.array_equal(got[k], want[k]), "%s: %s differs in %d of %d places" % (
            who, k, int((got[k] != want[k]).sum()) if got[k].shape == want[k].shape else -1, len(want[k]))


def _check(ctx, ro, ci, symmetric, layout=False, want=None, operator=True, expect=None):
    """fused == operator path == model (tri, sdeg, the DAG, stats [0] - [4]); one host wait; built once; the repeat is equal"""
    import mini_amd
    want = model.count(ro, ci, symmetric) if want is None else want
    g = _graph(ctx, ro, ci, layout)
    tp = mini_amd.TcProblem(g)
    s1 = tp.run(symmetric)
    a1 = _arrays(tp)
    print("fused", {k: s1[k] for k in mini_amd.TcProblem.KEYS})
    _same(a1, want, "fused")
    assert {k: s1[k] for k in KEYS} == want["stats"], (s1, want["stats"])
    assert s1["host_waits"] == 1 and s1["built"] == 1
    s2 = tp.run(symmetric)
    assert s2["host_waits"] == 1 and s2["built"] == 0 and s2["launches"] < s1["launches"]
    assert {k: s2[k] for k in KEYS} == want["stats"]
    _same(_arrays(tp), a1, "fused repeat")
    if operator:
        so = tp.enact(symmetric)
        _same(_arrays(tp), want, "operator path")
        assert {k: so[k] for k in KEYS} == want["stats"], (so, want["stats"])
        assert so["built"] == 0 and so["host_waits"] >= 1
        tp2 = mini_amd.TcProblem(g)                              # the operator path first: it builds the same DAG
        so = tp2.enact(symmetric)
        assert so["built"] == 1 and {k: so[k] for k in KEYS} == want["stats"]
        _same(_arrays(tp2), want, "operator path, own build")
        tp2.close()
    assert int(a1["tri"].sum()) == 3 * s1["triangles"] and int(a1["sdeg"].sum()) == 2 * s1["edges"]
    bins = tp.bins()
    d = np.diff(want["dag_ro"].astype(np.int64))
    lo, hi = bins["short_max"], bins["wave_max"]                 # the bins the switches in effect must have made
    assert bins["short_rows"] == int(((d >= 2) & (d <= lo)).sum()), bins
    assert bins["wave_rows"] == int(((d >= 2) & (d > lo) & (d <= hi)).sum()), bins
    assert bins["block_rows"] == int(((d >= 2) & (d > lo) & (d > hi)).sum()), bins
    if expect is not None:                                       # the switches a test set are the ones the handle read
        assert {k: bins[k] for k in expect} == expect, (bins, expect)
    tp.close()
    g.close()
    return want


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("undir", [True, False])
@pytest.mark.parametrize("symmetric", [True, False])
def test_fixtures(gpu_ctx, oracle, name, undir, symmetric):
    n, ro, ci, _, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=undir)
    # (a directed load declared symmetric: the caller's responsibility -- the three implementations still agree on what
    #  "keep the entries with rank(v) < rank(u)" gives)
    _check(gpu_ctx, ro, ci, symmetric)


@pytest.mark.parametrize("scale,ef", [(10, 1), (11, 2), (12, 4), (13, 8), (14, 16), (15, 1), (16, 16)])
def test_rmat_symmetric(gpu_ctx, oracle, scale, ef):
    n, ro, ci, _ = oracle.rmat_csr(scale, ef, scale)
    _check(gpu_ctx, ro, ci, True)


@pytest.mark.parametrize("scale,ef", [(10, 2), (12, 4), (14, 8), (16, 16)])
def test_rmat_directed(gpu_ctx, oracle, scale, ef):
    n, ro, ci, _ = oracle.rmat_csr(scale, ef, scale + 100, undir=False)
    _check(gpu_ctx, ro, ci, False)


def test_rmat18_against_model(gpu_ctx, oracle):
    n, ro, ci, _ = oracle.rmat_csr(18, 16, 18)
    w = _check(gpu_ctx, ro, ci, True)
    assert w["stats"]["triangles"] > 10 ** 7


@pytest.mark.parametrize("n", [1, 1000])
def test_graph_without_entries(gpu_ctx, n):
    ro, ci = np.zeros(n + 1, np.int32), np.zeros(0, np.int32)
    for symmetric in (True, False):
        w = _check(gpu_ctx, ro, ci, symmetric)
        assert w["stats"]["triangles"] == 0 and w["stats"]["edges"] == 0 and not w["tri"].any()


def test_self_loops_only(gpu_ctx):
    v = np.arange(3000)
    ro, ci = cm.csr(3000, v, v, symmetric=False)
    for symmetric in (True, False):
        w = _check(gpu_ctx, ro, ci, symmetric)
        assert w["stats"]["edges"] == 0 and not w["sdeg"].any()


def test_tripled_pairs_and_self_loops_equal_the_simple_graph(gpu_ctx):
    n = 3000
    rng = np.random.default_rng(4)
    s, d = rng.integers(0, n, 40000), rng.integers(0, n, 40000)
    v = np.arange(n)
    for symmetric in (True, False):
        simple = model.count(*cm.csr(n, s, d, symmetric=symmetric), symmetric)
        ro, ci = cm.csr(n, np.concatenate([s, s, s, v[::7]]), np.concatenate([d, d, d, v[::7]]), symmetric=symmetric)
        w = _check(gpu_ctx, ro, ci, symmetric)
        assert w["stats"]["triangles"] == simple["stats"]["triangles"] > 0
        assert np.array_equal(w["tri"], simple["tri"]) and np.array_equal(w["sdeg"], simple["sdeg"])


def test_work_list_stages_on_one_unit(gpu_ctx, torch_mod, monkeypatch):
    """k_tc_worklist where a pass covers 2048 vertices (a one-unit context: 8 workgroups): a band graph (v -- v + 1, v + 2) of
    3 * 2048 + 5 vertices, all but two of them rows of two oriented entries, so every wave's stage of 128 short rows goes out inside
    the loop in its third pass and again behind it; and the same with all of them in the second and in the third list."""
    n = 3 * 2048 + 5
    v = np.arange(n)
    ro, ci = cm.csr(n, np.concatenate([v[:-1], v[:-2]]), np.concatenate([v[:-1] + 1, v[:-2] + 2]))
    want = model.count(ro, ci, True)
    d = np.diff(want["dag_ro"])
    assert ((d[:3 * 2048 + 1] >= 2) & (d[:3 * 2048 + 1] <= 16)).all() and want["stats"]["triangles"] == n - 2
    with one_cu_context(monkeypatch, torch_mod) as one_cu:
        for ctx in (one_cu, gpu_ctx):
            _check(ctx, ro, ci, True, want=want)
        for env in (ALL_WAVE, ALL_BLOCK):
            for k, x in env.items():
                monkeypatch.setenv(k, x)
            for ctx in (one_cu, gpu_ctx):
                _check(ctx, ro, ci, True, want=want, operator=False, expect={"short_max": 0})


def test_star_long_row(gpu_ctx):
    n, centre = 100001, 77777
    leaves = np.setdiff1d(np.arange(n), [centre])
    ro, ci = cm.csr(n, np.full(len(leaves), centre), leaves)
    assert ro[centre + 1] - ro[centre] == 100000
    for symmetric in (True, False):
        w = _check(gpu_ctx, ro, ci, symmetric)
        assert w["stats"]["triangles"] == 0 and w["stats"]["max_row"] == 1 and w["stats"]["edges"] == 100000


def _clique_want(n, symmetric=True):
    """K_n with ascending rows: every degree equal, so the rank is the id and row a = a + 1 .. n - 1"""
    d = np.arange(n - 1, -1, -1, dtype=np.int64)
    dag_ro = np.concatenate([[0], np.cumsum(d)]).astype(np.int32)
    dag_ci = np.concatenate([np.arange(a + 1, n) for a in range(n)]).astype(np.int32)
    stats = {"triangles": comb(n, 3), "edges": comb(n, 2), "max_row": n - 1, "wedges": int((d * (d - 1) // 2).sum()),
             "rows_sorted": int(symmetric)}
    return {"tri": np.full(n, comb(n - 1, 2), np.int64), "sdeg": np.full(n, n - 1, np.int32), "dag_ro": dag_ro, "dag_ci": dag_ci,
            "stats": stats}


def test_clique_2000(gpu_ctx):
    n = 2000
    ro, ci = cm.clique(n)
    small = model.count(*cm.clique(50), True)
    w50 = _clique_want(50)
    assert all(np.array_equal(small[k], w50[k]) for k in ("tri", "sdeg", "dag_ro", "dag_ci")) and small["stats"] == w50["stats"]
    w = _check(gpu_ctx, ro, ci, True, want=_clique_want(n))
    assert w["stats"]["triangles"] == comb(2000, 3) and (w["tri"] == comb(1999, 2)).all() and w["stats"]["max_row"] == 1999
    _check(gpu_ctx, ro, ci, False, want=_clique_want(n, symmetric=False), operator=False)


def test_complete_bipartite_700_900(gpu_ctx):
    p, q = 700, 900
    s, d = np.meshgrid(np.arange(p), p + np.arange(q), indexing="ij")
    ro, ci = cm.csr(p + q, s.ravel(), d.ravel())
    w = _check(gpu_ctx, ro, ci, True)
    assert w["stats"]["triangles"] == 0 and w["stats"]["edges"] == p * q and w["stats"]["max_row"] == p      # (the 900 vertices of degree 700 rank lower)


def test_two_cliques_sharing_an_edge(gpu_ctx):
    k = 300
    ids = np.random.default_rng(2).permutation(2 * k - 2 + 40)
    a, b = ids[:k], np.concatenate([ids[:2], ids[k:2 * k - 2]])
    s, d = [], []
    for c in (a, b):
        x, y = np.meshgrid(c, c, indexing="ij")
        s.append(x[x != y])
        d.append(y[x != y])
    ro, ci = cm.csr(len(ids), np.concatenate(s), np.concatenate(d), symmetric=False)      # the shared pair twice in both rows
    for symmetric in (True, False):
        w = _check(gpu_ctx, ro, ci, symmetric)
        assert w["stats"]["triangles"] == 2 * comb(k, 3)
        assert w["tri"][ids[0]] == w["tri"][ids[1]] == 2 * comb(k - 1, 2)
        assert (w["tri"][ids[2:2 * k - 2]] == comb(k - 1, 2)).all() and not w["tri"][ids[2 * k - 2:]].any()


def test_ten_thousand_disjoint_triangles(gpu_ctx):
    t = 10000
    ids = np.random.default_rng(10).permutation(3 * t + 500)
    x, y, z = ids[0:3 * t:3], ids[1:3 * t:3], ids[2:3 * t:3]
    ro, ci = cm.csr(len(ids), np.concatenate([x, y, z]), np.concatenate([y, z, x]))
    for symmetric in (True, False):
        w = _check(gpu_ctx, ro, ci, symmetric)
        assert w["stats"]["triangles"] == t and (w["tri"][ids[:3 * t]] == 1).all() and not w["tri"][ids[3 * t:]].any()


def test_unsorted_rows(gpu_ctx, oracle):
    n, ro, ci, _ = oracle.rmat_csr(13, 8, 77)
    rng = np.random.default_rng(5)
    shuffled = ci.copy()
    for v in range(n):
        shuffled[ro[v]:ro[v + 1]] = rng.permutation(ci[ro[v]:ro[v + 1]])
    assert not np.array_equal(shuffled, ci)
    sorted_want = _check(gpu_ctx, ro, ci, True)
    assert sorted_want["stats"]["rows_sorted"] == 1
    w = _check(gpu_ctx, ro, shuffled, True)
    assert w["stats"]["rows_sorted"] == 0
    for k in ("tri", "sdeg", "dag_ro", "dag_ci"):
        assert np.array_equal(w[k], sorted_want[k])
    _check(gpu_ctx, ro, shuffled, False)


def test_directed_only_triangle(gpu_ctx):
    import mini_amd
    ro, ci = cm.csr(5, [1, 3, 4], [3, 4, 1], symmetric=False)             # 1 -> 3 -> 4 -> 1, no reverses
    w = _check(gpu_ctx, ro, ci, False)
    assert w["stats"]["triangles"] == 1 and w["tri"].tolist() == [0, 1, 0, 1, 1]
    g = _graph(gpu_ctx, ro, ci)
    tp = mini_amd.TcProblem(g)
    st = tp.run(True)                                                     # the caller's word is wrong: a status, no more than the truth
    assert 0 <= st["triangles"] <= 1 and (tp.triangles() <= w["tri"]).all()
    tp.close()
    g.close()


ALL_SHORT = {"MGX_TC_SHORT_MAX": "1000000000"}
ALL_WAVE = {"MGX_TC_SHORT_MAX": "0", "MGX_TC_WAVE_MAX": "1000000000"}
ALL_BLOCK = {"MGX_TC_SHORT_MAX": "0", "MGX_TC_WAVE_MAX": "0"}


@pytest.mark.parametrize("env", [ALL_SHORT, ALL_WAVE, ALL_BLOCK, {"MGX_TC_STAGE": "64"}, dict(ALL_WAVE, MGX_TC_STAGE="64"),
                                 dict(ALL_BLOCK, MGX_TC_STAGE="64"), dict(ALL_BLOCK, MGX_TC_STAGE="1")],
                         ids=["short", "wave", "block", "stage64", "wave-stage64", "block-stage64", "block-stage1"])
def test_every_bin_and_the_chunked_stage(gpu_ctx, oracle, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    stage = int(env.get("MGX_TC_STAGE", 4096))
    expect = {"short_max": int(env.get("MGX_TC_SHORT_MAX", 16)), "wave_max": int(env.get("MGX_TC_WAVE_MAX", 256)),
              "block_stage": min(stage, 4096), "wave_stage": min(stage, 512)}
    n, ro, ci, _ = oracle.rmat_csr(14, 16, 14)
    w = _check(gpu_ctx, ro, ci, True, expect=expect)
    assert w["stats"]["max_row"] > 64                                     # stage 64: several chunks a row
    d = np.diff(w["dag_ro"].astype(np.int64))
    assert ((d >= 2) & (d <= 16)).any() and ((d > 16) & (d <= 256)).any()  # (the defaults would have used two kernels at least)
    n, ro, ci, _ = oracle.rmat_csr(12, 8, 112, undir=False)
    _check(gpu_ctx, ro, ci, False, expect=expect)
    k = 300 if env == ALL_SHORT or env.get("MGX_TC_STAGE") == "1" else 2000     # (K_2000 an entry a lane: 10^10 probes)
    _check(gpu_ctx, *cm.clique(k), True, want=_clique_want(k), operator=False, expect=expect)


def test_layout_stream_and_no_run(gpu_ctx, oracle, torch_mod):
    import mini_amd
    n, ro, ci, _ = oracle.rmat_csr(14, 8, 41)
    want = model.count(ro, ci, True)
    _check(gpu_ctx, ro, ci, True, layout=True, want=want)
    s = torch_mod.cuda.Stream()
    ctx = mini_amd.Context(0, s.cuda_stream)
    try:
        _check(ctx, ro, ci, True, want=want)
        g = _graph(ctx, ro, ci)
        tp = mini_amd.TcProblem(g)
        for getter in (tp.triangles, tp.simple_degrees, tp.dag, tp.bins, tp.triangles_device_ptr, tp.simple_degrees_device_ptr,
                       tp.clustering, tp.transitivity):
            with pytest.raises(mini_amd.MgxError):
                getter()
        st = tp.run(True)
        assert tp.triangles_device_ptr() and tp.simple_degrees_device_ptr()
        # both DAGs live on the handle: the other `symmetric` value builds its own, the first is still there
        s0 = tp.run(False)
        assert s0["built"] == 1 and s0["rows_sorted"] == 0 and s0["triangles"] == st["triangles"]
        assert np.array_equal(tp.triangles(), want["tri"])
        assert tp.run(True)["built"] == 0 and tp.run(False)["built"] == 0
        tp.close()
        g.close()
    finally:
        ctx.close()


def test_clustering_and_transitivity_against_networkx(gpu_ctx, oracle):
    import mini_amd
    import networkx as nx
    n, ro, ci, _ = oracle.rmat_csr(12, 16, 12)
    g = _graph(gpu_ctx, ro, ci)
    tp = mini_amd.TcProblem(g)
    tp.run(True)
    G = model.simple_graph(ro, ci)
    cl = nx.clustering(G)
    got = tp.clustering()
    assert got.dtype == np.float64
    np.testing.assert_allclose(got, np.array([cl[v] for v in range(n)]), rtol=1e-12, atol=0)
    np.testing.assert_allclose(tp.transitivity(), nx.transitivity(G), rtol=1e-12, atol=0)
    tp.close()
    g.close()


def _device_graph(ctx, d):
    import mini_amd
    return mini_amd.Graph.from_device(ctx, d["n"], d["m"], d["row_offsets"], d["col_indices"])


def _fused_equals_operator(ctx, d):
    import mini_amd
    g = _device_graph(ctx, d)
    tp = mini_amd.TcProblem(g)
    sf = tp.run(True)
    af = _arrays(tp)
    so = tp.enact(True)
    _same(_arrays(tp), af, "operator path against fused")
    assert {k: sf[k] for k in KEYS} == {k: so[k] for k in KEYS}, (sf, so)
    assert sf["host_waits"] == 1
    assert int(af["tri"].sum()) == 3 * sf["triangles"] and int(af["sdeg"].astype(np.int64).sum()) == 2 * sf["edges"]
    print("fused", sf, "operator", so)
    tp.close()
    g.close()
    return sf, af


def test_rmat20_fused_equals_operator_path(gpu_ctx):
    from mini_amd.rmat import rmat_csr
    sf, _ = _fused_equals_operator(gpu_ctx, rmat_csr(gpu_ctx, 20, 16))
    assert sf["triangles"] > 10 ** 8


def test_rmat22_identities_and_sampled_cpu_check(gpu_ctx):
    import mini_amd
    from mini_amd.rmat import rmat_csr
    d = rmat_csr(gpu_ctx, 22, 16)
    g = _device_graph(gpu_ctx, d)
    tp = mini_amd.TcProblem(g)
    sf = tp.run(True)
    tri, sdeg = tp.triangles(), tp.simple_degrees()
    print("fused", sf)
    assert sf["host_waits"] == 1 and sf["triangles"] > 2 ** 30 and int(tri.sum()) > 2 ** 32     # (64-bit counts are needed)
    assert int(tri.sum()) == 3 * sf["triangles"] and int(sdeg.astype(np.int64).sum()) == 2 * sf["edges"]
    ro, ci = d["row_offsets"].cpu().numpy().astype(np.int64), d["col_indices"].cpu().numpy()

    def nbrs(v):
        row = np.unique(ci[ro[v]:ro[v + 1]])
        return row[row != v]
    rng = np.random.default_rng(22)
    cand = np.nonzero((sdeg >= 2) & (sdeg <= 64))[0]
    for v in rng.choice(cand, 256, replace=False):
        nv = nbrs(v)
        assert len(nv) == sdeg[v], (v, len(nv), sdeg[v])
        twice = 0
        for a in nv:
            na = nbrs(a)
            at = np.searchsorted(na, nv)
            twice += int((na[np.minimum(at, len(na) - 1)] == nv).sum())
        assert twice % 2 == 0 and twice // 2 == tri[v], (v, twice, tri[v])
    tp.close()
    g.close()


@pytest.mark.parametrize("kind", ["uniform", "grid2d"])
def test_scale18_uniform_and_grid(gpu_ctx, kind):
    from mini_amd.rmat import grid2d_csr, uniform_csr
    sf, af = _fused_equals_operator(gpu_ctx, (uniform_csr if kind == "uniform" else grid2d_csr)(gpu_ctx, 18))
    if kind == "grid2d":
        assert sf["triangles"] == 0 and not af["tri"].any()
