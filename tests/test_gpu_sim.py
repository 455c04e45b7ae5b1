"""GPU suite (-m gpu): vertex similarity (mgx_sim_*).  The fused path (mgx_sim_run), the operator path (mgx_sim_enact)
and the numpy model (tests/sim_model.py) agree on the shared cases (tests/sim_cases.py: a pair on each side of every cut of the
classification, forced stages of 64 and 1, rows that share nothing, everything or one element at a chunk's edge), every measure and
both `symmetric` values: common and stats [0] - [4] exactly, the four ratios and the cosine bit for bit (the cosine's own bound is 2 ulp), the weighted sum
within c 2^-52 sum |x| of math.fsum and bit-equal between two runs and between (u, v) and (v, u); the bins are the model's classes;
entries_read stays under the model's cap (the long row of a chunked pair is streamed once; a leaf against a hub costs la log lb)."""
import math
import os

import numpy as np
import pytest

from tests import sim_cases as cases
from tests import sim_model as model
from tests.grid_cus import one_cu_context

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["bfs_test.mtx", "kcore_test.mtx", "pr_test.mtx", "sssp_test.mtx", "synthetic_dup.mtx"]
KEYS = model.STAT_KEYS
RATIOS = ("common", "jaccard", "overlap", "sorensen")
CASES = {"cuts": cases.cuts, "contents_64": lambda: cases.contents(64), "contents_1": lambda: cases.contents(1), "stages_64": lambda: cases.stages(64),
         "stages_1": lambda: cases.stages(1), "two_hubs": cases.two_hubs, "random": cases.small_random}


def _setenv(monkeypatch, opts):
    for k, v in opts.items():
        monkeypatch.setenv(cases.ENV[k], str(v))


def _cap(want, opts):
    return sum(model.entries_read_cap(la, lb, cl, opts.get("stage", model.STAGE)) for la, lb, cl in zip(want["la"], want["lb"], want["classes"]))


def _check_scores(got, want, measure, who):
    """the scores as the definition states them: ratios bit for bit, the weighted sum within the bound.  The cosine's bound is 2 ulp
    (sqrt within 1 ulp, then one division); on the MI355X it came out bit-equal to numpy's on every case, so that is
    what is asserted"""
    assert got.dtype == np.float64 and got.shape == want["scores"].shape, who
    if measure in RATIOS:
        assert np.array_equal(got, want["scores"]), (who, measure, int((got != want["scores"]).sum()))
    elif measure == "cosine":
        worst = float(model.ulps(got, want["scores"]).max(initial=0.0))
        print(who, "cosine: worst distance", worst, "ulp")
        assert np.array_equal(got, want["scores"]), (who, worst)
    else:
        err, bound = np.abs(got - want["scores"]), model.weighted_bound(want["common"], want["abs"])
        print(who, "weighted: worst error / bound", float((err / np.maximum(bound, 1e-300)).max(initial=0.0)))
        assert np.all(err <= bound), (who, float(err.max()), float(bound[err.argmax()]))


def _wanted(ro, ci, pairs, symmetric, x, opts):
    """the model once per graph and `symmetric`: common and classes do not depend on the measure"""
    base = model.similarity(ro, ci, pairs, "common", symmetric=symmetric, **opts)
    d = model.degrees(ro, ci, symmetric).astype(np.int64)
    pr = base["pairs"].astype(np.int64)
    out = {}
    for measure in model.MEASURES:
        w = dict(base)
        if measure == "weighted":
            wt = model.similarity(ro, ci, pairs, "weighted", x=x, symmetric=symmetric, **opts)
            w["scores"], w["abs"] = wt["scores"], wt["abs"]
        else:
            w["scores"] = model.score(measure, base["common"], d[pr[:, 0]], d[pr[:, 1]]) if len(pr) else np.zeros(0)
        out[measure] = w
    return out


def _check(ctx, monkeypatch, ro, ci, pairs, opts=None, symmetrics=(True, False), measures=model.MEASURES, operator=True):
    """fused == operator path == model for every measure; the bins, the cuts as read, entries_read under the cap; the repeat run"""
    import mini_amd
    opts = opts or {}
    _setenv(monkeypatch, opts)
    n = len(ro) - 1
    x = np.random.default_rng(n).random(max(n, 1))[:n] + 0.25
    g = mini_amd.Graph.from_host(ctx, ro, ci, None)
    sp = mini_amd.SimilarityProblem(g)
    first = None
    for symmetric in symmetrics:
        wanted = _wanted(ro, ci, pairs, symmetric, x, opts)
        built = True
        for measure in measures:
            want = wanted[measure]
            who = "%s symmetric=%d" % (measure, symmetric)
            args = dict(pairs=pairs, measure=measure, weights=x if measure == "weighted" else None, symmetric=symmetric)
            s = sp.run(**args)
            first = first or s
            assert {k: s[k] for k in KEYS} == want["stats"], (who, s, want["stats"])
            assert s["built"] == int(built), (who, s)
            if not built:
                assert s["host_waits"] == 1, (who, s)
            built = False
            got = sp.common()
            assert got.dtype == np.int32 and np.array_equal(got, want["common"]), (who, int((got != want["common"]).sum()))
            assert np.array_equal(sp.pairs(), want["pairs"]), who
            _check_scores(sp.scores(), want, measure, "fused " + who)
            b = sp.bins()
            assert {k: b[k] for k in model.BIN_KEYS} == want["bins"], (who, b, want["bins"])
            assert (b["short_max"], b["probe_ratio"], b["wave_max"], b["stage"]) == tuple(
                opts.get(k, v) for k, v in (("short_max", model.SHORT_MAX), ("probe_ratio", model.PROBE_RATIO), ("wave_max", model.WAVE_MAX), ("stage", model.STAGE)))
            assert b["entries_read"] <= _cap(want, opts), (who, b["entries_read"], _cap(want, opts))
            if operator:
                so = sp.enact(**args)
                assert {k: so[k] for k in KEYS} == want["stats"], (who, so, want["stats"])
                assert np.array_equal(sp.common(), want["common"]), "operator " + who
                _check_scores(sp.scores(), want, measure, "operator " + who)
    sp.close()
    g.close()
    return first


@pytest.mark.parametrize("name", list(CASES))
def test_parity(gpu_ctx, monkeypatch, name):
    case = CASES[name]()
    _check(gpu_ctx, monkeypatch, case["ro"], case["ci"], case["pairs"], case["opts"])


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures(gpu_ctx, monkeypatch, oracle, name):
    """the golden graphs, synthetic_dup with its self-loops and duplicates among them: random pairs and every edge; small cuts so
    that their short rows reach every class they can"""
    for undir in (True, False):
        n, ro, ci, _, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=undir)
        pr = np.random.default_rng(n).integers(0, n, (257, 2))
        opts = {"short_max": 1, "probe_ratio": 2, "wave_max": 3, "stage": 2}
        symmetrics = (True, False) if undir else (False,)
        _check(gpu_ctx, monkeypatch, ro, ci, pr, opts, symmetrics=symmetrics, measures=("jaccard", "cosine", "weighted"))
        _check(gpu_ctx, monkeypatch, ro, ci, None, opts, symmetrics=symmetrics, measures=("common",))


@pytest.mark.parametrize("P", [0, 1, 63, 65])
def test_pair_counts(gpu_ctx, monkeypatch, P):
    case = cases.small_random()
    _check(gpu_ctx, monkeypatch, case["ro"], case["ci"], case["pairs"][:P], measures=("jaccard", "weighted"), symmetrics=(True,))


def test_one_cu_grid(monkeypatch, torch_mod):
    """grids of one compute unit: every kernel's later grid-stride iterations and the list stages' carry-over between them"""
    ro, ci = cases.random_symmetric(2000, 40000, 11)
    pr = np.random.default_rng(3).integers(0, 2000, (20000, 2))
    with one_cu_context(monkeypatch, torch_mod) as ctx:
        _check(ctx, monkeypatch, ro, ci, pr, {"short_max": 8, "probe_ratio": 3, "wave_max": 40, "stage": 16}, symmetrics=(True,),
               measures=("jaccard", "weighted"))


@pytest.mark.parametrize("stage", [64, 1])
def test_forced_stage_streams_the_long_row_once(gpu_ctx, monkeypatch, stage):
    """every chunked pair of the stage's case on its own: the results of the default stage, and entries_read at most la + lb plus
    the two bound searches per chunk -- a long row streamed once per chunk would read chunks x lb"""
    import mini_amd
    case = cases.stages(stage)
    ro, ci, pairs = case["ro"], case["ci"], case["pairs"]
    want = model.similarity(ro, ci, pairs, "common", **case["opts"])
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
    plain = mini_amd.SimilarityProblem(g)                        # (the default stage; the case's short_max all the same)
    monkeypatch.setenv(cases.ENV["short_max"], str(case["opts"]["short_max"]))
    plain.run(pairs=pairs, measure="common")
    assert plain.bins()["stage"] == model.STAGE and np.array_equal(plain.common(), want["common"])
    _setenv(monkeypatch, case["opts"])
    sp = mini_amd.SimilarityProblem(g)
    chunked = 0
    for p in range(0, len(pairs), 2):
        la, lb, cl = int(want["la"][p]), int(want["lb"][p]), int(want["classes"][p])
        chunks = -(-la // stage)
        if chunks < 2:
            continue
        chunked += 1
        sp.run(pairs=pairs[p:p + 1], measure="common")
        b = sp.bins()
        assert b["stage"] == stage and b[model.BIN_KEYS[cl]] == 1
        assert sp.common()[0] == want["common"][p]
        cap = la + lb + 2 * chunks * model.search_cap(lb)
        assert cap == model.entries_read_cap(la, lb, cl, stage)
        print("la", la, "lb", lb, "chunks", chunks, "entries_read", b["entries_read"], "cap", cap)
        assert la <= b["entries_read"] <= cap, (la, lb, chunks, b["entries_read"], cap)
    assert chunked >= 8
    sp.close()
    plain.close()
    g.close()


def test_weighted_is_deterministic_and_symmetric(gpu_ctx):
    """two WEIGHTED runs are bit-equal, and score(u, v) == score(v, u) bit for bit, in every class (equally long rows among them)"""
    import mini_amd
    for case in (cases.cuts(), cases.two_hubs(), cases.contents(64)):
        ro, ci, pairs = case["ro"], case["ci"], case["pairs"]
        n = len(ro) - 1
        x = np.random.default_rng(5).random(n) * np.exp(np.random.default_rng(6).normal(0, 8, n))      # (magnitudes far apart: the order shows)
        both = np.concatenate([pairs, pairs[:, ::-1]])
        g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
        sp = mini_amd.SimilarityProblem(g)
        sp.run(pairs=both, weights=x)
        one = sp.scores().copy()
        sp.run(pairs=both, weights=x)
        assert np.array_equal(one.view(np.int64), sp.scores().view(np.int64)), case["name"]
        assert np.array_equal(one[:len(pairs)].view(np.int64), one[len(pairs):].view(np.int64)), case["name"]
        for measure in ("jaccard", "cosine"):
            sp.run(pairs=both, measure=measure)
            s = sp.scores()
            assert np.array_equal(s[:len(pairs)].view(np.int64), s[len(pairs):].view(np.int64)), (case["name"], measure)
        sp.close()
        g.close()


def test_named_weights(gpu_ctx):
    """weights="adamic_adar" / "resource_allocation": x from degrees() with numpy, the sums against networkx's indices"""
    import mini_amd
    import networkx as nx
    from tests import tc_model
    case = cases.small_random()
    ro, ci = case["ro"], case["ci"]
    pr = case["pairs"][case["pairs"][:, 0] != case["pairs"][:, 1]]
    nxg = tc_model.simple_graph(ro, ci)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
    sp = mini_amd.SimilarityProblem(g)
    deg = sp.degrees()
    assert np.array_equal(deg, model.degrees(ro, ci, True))
    tuples = [(int(a), int(b)) for a, b in pr]
    for kind, index in (("adamic_adar", nx.adamic_adar_index), ("resource_allocation", nx.resource_allocation_index)):
        assert np.array_equal(sp.weights(kind), model.weights(kind, deg))
        want = model.similarity(ro, ci, pr, "weighted", x=model.weights(kind, deg))
        sp.run(pairs=pr, weights=kind)
        _check_scores(sp.scores(), want, "weighted", kind)
        theirs = np.array([s for _, _, s in index(nxg, tuples)])
        assert np.allclose(sp.scores(), theirs, rtol=1e-12, atol=0.0), kind
    sp.close()
    g.close()


@pytest.mark.parametrize("name", ["synthetic_dup.mtx", "random"])
def test_edges_mode(gpu_ctx, oracle, name):
    """pairs() are KtrussProblem's edges in its edge-id order, common() its supports"""
    import mini_amd
    if name == "random":
        ro, ci = cases.random_symmetric(500, 6000, 2)
    else:
        _, ro, ci, _, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=True)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
    for symmetric in (True, False):
        kt = mini_amd.KtrussProblem(g)
        kt.run(symmetric=symmetric)
        src, dst, _ = kt.raw_edges()
        u, v, _ = kt.edges()
        sp = mini_amd.SimilarityProblem(g)
        s = sp.run(symmetric=symmetric, measure="common")
        pr = sp.pairs()
        assert s["pairs"] == len(src) and np.array_equal(pr[:, 0], src) and np.array_equal(pr[:, 1], dst)
        lo, hi = pr.min(axis=1), pr.max(axis=1)
        perm = np.lexsort((hi, lo))
        assert np.array_equal(lo[perm], u) and np.array_equal(hi[perm], v)
        assert np.array_equal(sp.common()[perm], kt.support())
        assert s["common"] == int(kt.support().sum()) and np.array_equal(sp.scores(), sp.common().astype(np.float64))
        so = sp.enact(symmetric=symmetric, measure="common")
        assert {k: so[k] for k in KEYS} == {k: s[k] for k in KEYS} and np.array_equal(sp.common()[perm], kt.support())
        sp.close()
        kt.close()
    g.close()


def test_hub_condition(gpu_ctx):
    """1 024 pairs of rows of 16 - 20 entries against rows of 100 000: entries_read <= sum la (ceil(log2 lb) + 2).  A cap, not a
    measurement: every entry of the short row costs itself and one binary search whatever the long row's length"""
    import mini_amd
    case = cases.hub_rows()
    ro, ci, pairs = case["ro"], case["ci"], case["pairs"]
    _, _, adj_ro, adj_ci = model.adjacency(ro, ci, True)
    d = np.diff(adj_ro.astype(np.int64))
    la, lb = d[pairs[:, 0]], d[pairs[:, 1]]
    assert len(pairs) == 1024 and la.min() == 16 and la.max() == 20 and np.all(lb == 100000)
    want = np.array([len(model.common_of(adj_ro, adj_ci, int(a), int(b))) for a, b in pairs])
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
    sp = mini_amd.SimilarityProblem(g)
    s = sp.run(pairs=pairs, measure="jaccard")
    b = sp.bins()
    assert np.array_equal(sp.common(), want) and s["longest_row"] == 100000
    assert b["wave"] == b["block"] == b["none"] == 0 and b["lane"] + b["probe"] == 1024 and b["lane"] == int((la <= 16).sum())
    cap = int((la * (math.ceil(math.log2(100000)) + 2)).sum())
    print("entries_read", b["entries_read"], "cap", cap, "the long rows hold", int(lb.sum()))
    assert 0 < b["entries_read"] <= cap
    sp.run(pairs=pairs, measure="cosine")                        # (degree products of 2 000 000: roots that are not integers)
    _check_scores(sp.scores(), {"scores": model.score("cosine", want, la, lb)}, "cosine", "hub")
    sp.run(pairs=case["plain_pairs"], measure="jaccard")         # the same rows against rows of 100: fewer loads still, not 1 000 times fewer
    assert 0 < sp.bins()["entries_read"] <= b["entries_read"]
    sp.close()
    g.close()


def test_status_and_reuse(gpu_ctx):
    """an id outside [0, n) is MGX_E_INVALID and leaves no result; P = 0 succeeds; a repeat run waits once and allocates nothing; a
    larger P afterwards is right; create / free without a run"""
    import mini_amd
    case = cases.small_random()
    ro, ci, pairs = case["ro"], case["ci"], case["pairs"]
    n = len(ro) - 1
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
    mini_amd.SimilarityProblem(g).close()                        # create / free without a run
    sp = mini_amd.SimilarityProblem(g)
    with pytest.raises(mini_amd.MgxError):
        sp.common()                                              # no run yet
    want = model.similarity(ro, ci, pairs[:100], "jaccard")
    s1 = sp.run(pairs=pairs[:100])
    assert s1["built"] == 1 and np.array_equal(sp.common(), want["common"])
    before = mini_amd.lib.mgx_device_allocations()
    s2 = sp.run(pairs=pairs[:100])
    assert mini_amd.lib.mgx_device_allocations() == before
    assert s2["built"] == 0 and s2["host_waits"] == 1 and {k: s2[k] for k in KEYS} == {k: s1[k] for k in KEYS}
    s3 = sp.run(pairs=pairs[:40])                                # fewer pairs: nothing allocated either
    assert mini_amd.lib.mgx_device_allocations() == before and s3["host_waits"] == 1
    assert np.array_equal(sp.common(), want["common"][:40]) and np.array_equal(sp.scores(), want["scores"][:40])
    for bad in ([(0, n)], [(-1, 0)], [(3, 4), (n + 7, 2), (5, 6)]):
        for go in (sp.run, sp.enact):
            with pytest.raises(mini_amd.MgxError) as err:
                go(pairs=bad)
            assert err.value.status == mini_amd.MGX_E_INVALID
            with pytest.raises(mini_amd.MgxError):
                sp.common()                                      # a failed run leaves no result
    s0 = sp.run(pairs=np.zeros((0, 2), dtype=np.int32))          # P = 0
    assert s0["pairs"] == 0 and s0["common"] == 0 and len(sp.common()) == 0 and len(sp.scores()) == 0 and s0["entries"] == s1["entries"]
    assert sp.enact(pairs=np.zeros((0, 2), dtype=np.int32))["pairs"] == 0
    full = model.similarity(ro, ci, pairs, "sorensen")
    s4 = sp.run(pairs=pairs, measure="sorensen")                 # a larger P afterwards
    assert {k: s4[k] for k in KEYS} == full["stats"] and np.array_equal(sp.common(), full["common"]) and np.array_equal(sp.scores(), full["scores"])
    with pytest.raises(ValueError):
        sp.run(pairs=pairs, measure="weighted")                  # needs weights
    sp.set_timing(True)
    sp.run(pairs=pairs)
    ms = sp.phase_ms()
    assert set(ms) == {"build", "classify", "pairs"} and all(v >= 0.0 for v in ms.values())
    sp.close()
    g.close()
