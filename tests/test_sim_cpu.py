"""CPU suite for the vertex similarity (mgx_sim_*, include/mgx/sim_fused.hpp, include/gunrock/sim/): the header declares and the
library exports it, NULL handles are statuses, the switches are in the table, the kernels keep out of scratch, the model the GPU
tests compare against (tests/sim_model.py) agrees with networkx and with the closed forms, and the shared cases
(tests/sim_cases.py) hold a pair on each side of every cut of the classification."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import sim_cases as cases
from tests import sim_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["bfs_test.mtx", "kcore_test.mtx", "pr_test.mtx", "sssp_test.mtx", "synthetic_dup.mtx"]
NAMES = ["mgx_sim_create", "mgx_sim_free", "mgx_sim_prepare", "mgx_sim_run", "mgx_sim_enact", "mgx_sim_common", "mgx_sim_scores",
         "mgx_sim_common_device", "mgx_sim_scores_device", "mgx_sim_pairs", "mgx_sim_degrees", "mgx_sim_bins", "mgx_sim_set_timing",
         "mgx_sim_phase_ms"]
# (parts of the mangled names: a kernel matches when it holds all of its parts)
KERNELS = [("k_sim_%sE" % k,) for k in ("classify", "lane", "probe", "wave", "block", "score", "maxrow")] + [("3sim", "merge_functor_t")]
SWITCHES = {"MGX_SIM_SHORT_MAX", "MGX_SIM_PROBE_RATIO", "MGX_SIM_WAVE_MAX", "MGX_SIM_STAGE"}


def test_header_declares_and_library_exports_sim(built):
    import mini_amd
    header = open(os.path.join(ROOT, "include", "mgx.h")).read()
    for name in NAMES:
        assert re.search(r"MGX_API int %s\(" % name, header), name
        assert hasattr(mini_amd.lib, name), name
    for i, name in enumerate(model.MEASURES):
        assert re.search(r"#define MGX_SIM_%s %d\b" % (name.upper(), i), header), name
        assert getattr(mini_amd, "MGX_SIM_%s" % name.upper()) == i
    sp = mini_amd.SimilarityProblem
    assert sp.KEYS == model.STAT_KEYS + ("built", "host_waits", "launches")
    assert sp.BINS[:5] == model.BIN_KEYS
    assert tuple(sp.MEASURES) == model.MEASURES
    for member in ("run", "enact", "common", "scores", "pairs", "degrees", "weights", "bins", "common_device_ptr", "scores_device_ptr", "set_timing",
                   "phase_ms", "close"):
        assert hasattr(sp, member), member


def test_null_arguments_are_invalid(built):
    import mini_amd
    lib = mini_amd.lib
    h, d = C.c_void_p(), C.c_void_p()
    st = (C.c_int64 * 8)()
    bad = mini_amd.MGX_E_INVALID
    assert lib.mgx_sim_create(None, C.byref(h)) == bad
    for go in (lib.mgx_sim_run, lib.mgx_sim_enact):
        assert go(None, 1, None, None, 0, mini_amd.MGX_SIM_JACCARD, None, st) == bad
        assert b"NULL" in lib.mgx_last_error()
    assert lib.mgx_sim_prepare(None, 1) == bad
    for fn in (lib.mgx_sim_common, lib.mgx_sim_scores, lib.mgx_sim_degrees, lib.mgx_sim_bins, lib.mgx_sim_phase_ms):
        assert fn(None, None) == bad
    for fn in (lib.mgx_sim_common_device, lib.mgx_sim_scores_device):
        assert fn(None, C.byref(d)) == bad
    assert lib.mgx_sim_pairs(None, None, None) == bad
    assert lib.mgx_sim_set_timing(None, 1) == bad
    assert lib.mgx_sim_free(None) == 0


def test_sim_switches_are_in_the_table(built):
    import mini_amd
    name, what = C.c_char_p(), C.c_char_p()
    n = mini_amd.lib.mgx_env_switches(-1, None, None)
    names = set()
    for i in range(n):
        mini_amd.lib.mgx_env_switches(i, C.byref(name), C.byref(what))
        names.add(name.value.decode())
    assert SWITCHES <= names
    assert set(cases.ENV.values()) == SWITCHES


def test_sim_kernels_do_not_spill(built):
    """build() keeps the compiler's resource remarks: the seven kernels of the fused path and the operator path's functor use no
    scratch and spill nothing"""
    path = os.path.join(ROOT, "mini_amd", "kernel_resources.txt")
    assert os.path.exists(path), "build() writes the resource remarks"
    cur, res = None, {}
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        for key, pat in (("scratch", r"ScratchSize[^:]*: (\d+)"), ("vspill", r"VGPRs Spill[^:]*: (\d+)"), ("sspill", r"SGPRs Spill[^:]*: (\d+)")):
            m = re.search(pat, line)
            if m and cur:
                res.setdefault(cur, {})[key] = int(m.group(1))
    for parts in KERNELS:
        found = [k for k in res if all(x in k for x in parts)]
        assert found, parts
        for k in found:
            assert res[k] == {"scratch": 0, "vspill": 0, "sspill": 0}, (k, res[k])


# ---- the model against networkx -------------------------------------------------------------------------------------------------
def _graphs(oracle):
    for name in FIXTURES:
        for undir in (True, False):
            n, ro, ci, _, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=undir)
            yield "%s undir=%d" % (name, undir), ro, ci, undir
    for seed in (1, 2, 3):
        ro, ci = cases.random_symmetric(60, 300 * seed, seed)
        yield "random %d" % seed, ro, ci, True


def test_model_against_networkx(oracle):
    """common_neighbors, jaccard_coefficient, adamic_adar_index and resource_allocation_index on the simple graph: the integers
    exact, the ratios bit for bit (networkx divides the same two integers), the sums within the summation bound"""
    import networkx as nx
    from tests import tc_model
    for who, ro, ci, symmetric_input in _graphs(oracle):
        g = tc_model.simple_graph(ro, ci)
        n = g.number_of_nodes()
        rng = np.random.default_rng(n)
        pr = np.concatenate([rng.integers(0, n, (150, 2)), np.array(list(g.edges())[:150], dtype=np.int64).reshape(-1, 2)])
        pr = pr[pr[:, 0] != pr[:, 1]]                             # (networkx's indices are for distinct vertices)
        tuples = [(int(a), int(b)) for a, b in pr]
        for symmetric in ([True, False] if symmetric_input else [False]):
            deg = model.degrees(ro, ci, symmetric)
            assert np.array_equal(deg, [g.degree(v) for v in range(n)]), who
            r = model.similarity(ro, ci, pr, "jaccard", symmetric=symmetric)
            assert np.array_equal(r["common"], [len(list(nx.common_neighbors(g, a, b))) for a, b in tuples]), who
            assert np.array_equal(r["scores"], [s for _, _, s in nx.jaccard_coefficient(g, tuples)]), who
            for kind, index in (("adamic_adar", nx.adamic_adar_index), ("resource_allocation", nx.resource_allocation_index)):
                x = model.weights(kind, deg)
                rw = model.similarity(ro, ci, pr, "weighted", x=x, symmetric=symmetric)
                want = np.array([s for _, _, s in index(g, tuples)])
                # (networkx sums 1 / log(d) in its own order: both sides are within the bound of the exact sum, and x itself is one
                #  rounding of 1 / log d on each side)
                assert np.all(np.abs(rw["scores"] - want) <= 2 * model.weighted_bound(r["common"] + 1, rw["abs"])), (who, kind)
            stats = r["stats"]
            assert stats["entries"] == 2 * g.number_of_edges() and stats["longest_row"] == max(dict(g.degree()).values(), default=0), who
            e = model.similarity(ro, ci, None, "common", symmetric=symmetric)                       # edges mode: every edge once
            assert sorted(map(tuple, np.sort(e["pairs"], axis=1).tolist())) == sorted(tuple(sorted(x)) for x in g.edges()), who
            assert e["stats"]["common"] == 3 * sum(nx.triangles(g).values()) // 3, who


def test_every_measure_of_the_model():
    """the six scores from c and the degrees, by hand; 0 where a denominator is 0"""
    c, du, dv = np.array([0, 2, 3, 0]), np.array([0, 4, 3, 5]), np.array([0, 9, 3, 0])
    assert model.score("common", c, du, dv).tolist() == [0.0, 2.0, 3.0, 0.0]
    assert model.score("jaccard", c, du, dv).tolist() == [0.0, 2 / 11, 1.0, 0.0]
    assert model.score("overlap", c, du, dv).tolist() == [0.0, 0.5, 1.0, 0.0]
    assert model.score("sorensen", c, du, dv).tolist() == [0.0, 4 / 13, 1.0, 0.0]
    assert model.score("cosine", c, du, dv).tolist() == [0.0, 2 / 6, 1.0, 0.0]


# ---- closed forms ----------------------------------------------------------------------------------------------------------------
def test_closed_forms():
    n = 9
    ro, ci = cases.sym(n, *cases.clique(n))                       # K_n: c = n - 2, Jaccard (n - 2) / n
    pr = [(a, b) for a in range(n) for b in range(n) if a != b]
    r = model.similarity(ro, ci, pr, "jaccard")
    assert np.all(r["common"] == n - 2) and np.all(r["scores"] == (n - 2) / n)
    assert model.similarity(ro, ci, [(3, 3)], "jaccard")["common"][0] == n - 1          # u == v: c = d(u)
    ro, ci = cases.star(6)                                        # a star: leaf-leaf c = 1 and Jaccard 1, hub-leaf c = 0
    r = model.similarity(ro, ci, [(1, 2), (5, 6), (0, 1), (3, 0)], "jaccard")
    assert r["common"].tolist() == [1, 1, 0, 0] and r["scores"].tolist() == [1.0, 1.0, 0.0, 0.0]
    ro, ci = cases.path(7)                                        # a path: two apart share the one between them
    r = model.similarity(ro, ci, [(0, 2), (1, 3), (0, 1), (0, 3), (0, 6)], "sorensen")
    assert r["common"].tolist() == [1, 1, 0, 0, 0] and r["scores"].tolist() == [2 / 3, 2 / 4, 0.0, 0.0, 0.0]
    a1, b1 = cases.clique(5)                                      # two disjoint cliques: nothing in common across them
    a2, b2 = cases.clique(4, first=5)
    ro, ci = cases.sym(9, np.concatenate([a1, a2]), np.concatenate([b1, b2]))
    r = model.similarity(ro, ci, [(0, 1), (5, 6), (0, 5), (4, 8)], "overlap")
    assert r["common"].tolist() == [3, 2, 0, 0] and r["scores"].tolist() == [3 / 4, 2 / 3, 0.0, 0.0]
    x = model.weights("adamic_adar", model.degrees(ro, ci, True))
    r = model.similarity(ro, ci, [(0, 1), (5, 6)], "weighted", x=x)
    assert r["scores"].tolist() == [math.fsum([1 / math.log(4)] * 3), math.fsum([1 / math.log(3)] * 2)]


# ---- the cases cover the classification --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case_list():
    return cases.all_cases() + [cases.hub_rows(pairs=64, hub=2000)]


def test_cases_sit_on_every_cut(case_list):
    """from the model's own classifier: every (la, lb, class) a case exists for is among its pairs, so a case cannot quietly stop
    covering a class; together the cases hold every class, both sides of each cut, u == v, (u, v) beside (v, u) and a duplicate"""
    seen = set()
    for case in case_list:
        r = model.similarity(case["ro"], case["ci"], case["pairs"], "common", **case["opts"])
        have = set(zip(r["la"].tolist(), r["lb"].tolist(), r["classes"].tolist()))
        if case["name"] == "hub":
            assert {(16, 2000, model.LANE), (17, 2000, model.PROBE)} <= have
        else:
            for need in case["need"]:
                assert need in have, (case["name"], need, sorted(have))
        seen |= {cl for _, _, cl in have}
    assert seen == {model.NONE, model.LANE, model.PROBE, model.WAVE, model.BLOCK}
    cuts = next(c for c in case_list if c["name"] == "cuts")
    pr = [tuple(p) for p in cuts["pairs"].tolist()]
    assert any(a == b for a, b in pr) and any((b, a) in pr for a, b in pr if a != b) and len(set(pr)) < len(pr)


def test_cases_contents(case_list):
    """identical rows, disjoint and interleaved rows, and the single common element at the chunk's edges, at vertex 0 and at n - 1"""
    for case in case_list:
        if not case["name"].startswith("contents"):
            continue
        _, _, adj_ro, adj_ci = model.adjacency(case["ro"], case["ci"], True)
        n = len(adj_ro) - 1
        r = model.similarity(case["ro"], case["ci"], case["pairs"], "common", **case["opts"])
        only = [model.common_of(adj_ro, adj_ci, u, v) for u, v in case["pairs"]]
        assert (r["common"] == 0).any() and ((r["common"] == r["la"]) & (r["la"] == r["lb"])).any(), case["name"]
        singles = {int(w[0]) for w in only if len(w) == 1}
        assert 0 in singles and n - 1 in singles and len(singles) >= 4, (case["name"], singles)
        s = case["opts"]["stage"]
        for (u, v), w in zip(case["pairs"], only):
            if len(w) == 1 and w[0] not in (0, n - 1):
                a = adj_ci[adj_ro[u]:adj_ro[u + 1]]
                at = int(np.searchsorted(a, w[0]))
                assert at % s in (0, s - 1), (case["name"], at, s)


def test_pair_counts():
    """P in {0, 1, 63, 65}: the model takes each"""
    case = cases.small_random()
    for P in (0, 1, 63, 65):
        r = model.similarity(case["ro"], case["ci"], case["pairs"][:P], "jaccard")
        assert r["stats"]["pairs"] == P == len(r["common"]) == len(r["scores"])


def test_entries_read_cap():
    """the cap the GPU tests hold entries_read against: a lane's pair costs la (ceil(log2 lb) + 2) at most, whatever lb is; a staged
    pair reads both rows once, plus the bound searches of its chunks"""
    assert model.search_cap(100000) == 17 == math.ceil(math.log2(100000))
    assert model.search_cap(1 << 10) == 11 == math.ceil(math.log2(1 << 10)) + 1
    assert model.entries_read_cap(20, 100000, model.LANE) == 20 * 18 <= 20 * (math.ceil(math.log2(100000)) + 2)
    assert model.entries_read_cap(100, 300, model.WAVE) == 400
    assert model.entries_read_cap(129, 300, model.WAVE, stage=64) == 129 + 300 + 2 * 3 * 9
    assert model.entries_read_cap(10000, 10000, model.BLOCK) == 20000 + 2 * 3 * 14
